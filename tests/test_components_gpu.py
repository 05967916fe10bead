"""ctunet_amd.postprocess on the GPU against an exact scipy / numpy restatement of the definitions pinned in its module
docstring: components of one class = scipy.ndimage.label of (labels == class) with generate_binary_structure(3, rank),
keep-largest = the first k of np.argsort(-sizes, kind="stable"), remove-small = keep sizes >= min_size."""
import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- restatement
def _struct(conn):
    return ndi.generate_binary_structure(3, conn)


def _ref_label(mask, conn):
    """int32 labels and counts of [N, D, H, W] masks."""
    labs, nums = zip(*(ndi.label(m, _struct(conn)) for m in mask))
    return np.stack(labs).astype(np.int32), np.array(nums, dtype=np.int32)


def _classes(item, applied):
    return [int(c) for c in np.unique(item) if c != 0] if applied is None else list(applied)


def _ref_filter(labels, conn, applied=None, k=None, min_size=None):
    out = labels.copy()
    for i, item in enumerate(labels):
        for c in _classes(item, applied):
            lab, n = ndi.label(item == c, _struct(conn))
            if n == 0:
                continue
            sizes = np.bincount(lab.ravel())[1:]
            if k is not None:
                keep = np.zeros(n, bool)
                keep[np.argsort(-sizes, kind="stable")[:k]] = True
            else:
                keep = sizes >= min_size
            out[i][(lab > 0) & ~np.concatenate([[True], keep])[lab]] = 0
    return out


def _label(mask_np, conn):
    from ctunet_amd import postprocess
    m = torch.from_numpy(mask_np).cuda()
    labels, num = postprocess.label(m, connectivity=conn)
    assert labels.dtype == torch.int32 and num.dtype == torch.int32 and labels.shape == m.shape
    return labels.cpu().numpy(), num.cpu().numpy()


def _check_label(mask, conn):
    m4 = mask if mask.ndim == 4 else mask[None]
    got, num = _label(mask, conn)
    ref, rnum = _ref_label(m4, conn)
    assert np.array_equal(got.reshape(ref.shape), ref)
    assert np.array_equal(num, rnum)


# ---------------------------------------------------------------------------------------------- label()
CONNS = (1, 2, 3)


@pytest.mark.parametrize("conn", CONNS)
def test_label_random_masks_bit_equal_to_scipy(conn):
    rng = np.random.default_rng(conn)
    for dens in (0.05, 0.3, 0.5, 0.7):
        _check_label(rng.random((40, 48, 72)) < dens, conn)


@pytest.mark.parametrize("conn", CONNS)
def test_label_structured_volumes(conn):
    # serpentine: one component whose path visits every row of every plane
    d, h, w = 9, 21, 70
    s = np.zeros((d, h, w), bool)
    for z in range(0, d, 2):
        for y in range(0, h, 2):
            s[z, y, :] = True
            s[z, y + 1 if y + 1 < h else y, (w - 1) if (y // 2) % 2 == 0 else 0] = True
        s[z + 1 if z + 1 < d else z, h - 1, 0] = True
    _check_label(s, conn)
    chk = (np.indices((20, 24, 40)).sum(0) % 2).astype(bool)
    _check_label(chk, conn)
    got, num = _label(chk, conn)
    assert num[0] == (int(chk.sum()) if conn == 1 else 1)
    _check_label(np.zeros((17, 33, 65), bool), conn)
    _check_label(np.ones((17, 33, 65), bool), conn)
    corners = np.zeros((17, 33, 65), bool)
    for z in (0, 16):
        for y in (0, 32):
            for x in (0, 64):
                corners[z, y, x] = True
    _check_label(corners, conn)
    rng = np.random.default_rng(7 + conn)
    for shape in ((17, 33, 65), (1, 1, 300), (300, 1, 1)):
        _check_label(rng.random(shape) < 0.45, conn)


@pytest.mark.parametrize("conn", CONNS)
def test_label_multi_tile_grid_and_batch(conn):
    rng = np.random.default_rng(20 + conn)
    _check_label(rng.random((96, 160, 200)) < 0.3, conn)
    batch = np.stack([rng.random((20, 30, 50)) < 0.2, np.zeros((20, 30, 50), bool), rng.random((20, 30, 50)) < 0.6])
    _check_label(batch, conn)
    # uint8 masks are binarised first: values 1 and 2 side by side form one component
    from ctunet_amd import postprocess
    m = torch.zeros(4, 4, 8, dtype=torch.uint8, device="cuda")
    m[1, 1, 2:4], m[1, 1, 4:6] = 1, 2
    labels, num = postprocess.label(m)
    assert int(num[0]) == 1 and int(labels.max()) == 1


# ---------------------------------------------------------------------------------------------- filters
def _shell_labels(d, h, w, seed, dtype, islands=True):
    """a skull shell (class 1), a flap cut out of it (class 2) and islands of both classes well inside the shell."""
    zz, yy, xx = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    r = np.sqrt(((zz - d / 2) / (0.45 * d)) ** 2 + ((yy - h / 2) / (0.45 * h)) ** 2 + ((xx - w / 2) / (0.44 * w)) ** 2)
    shell = (r <= 1.0) & (r >= 0.85)
    lab = shell.astype(dtype)
    lab[shell & (zz > 0.6 * d) & (xx > 0.55 * w)] = 2
    if not islands:
        return lab
    rng = np.random.default_rng(seed)
    inside = np.argwhere(r < 0.5)
    for c, (a, b, e) in ((1, (1, 1, 3)), (1, (1, 1, 1)), (2, (1, 1, 5)), (2, (1, 2, 1)), (1, (3, 4, 5)), (2, (2, 5, 7)),
                         (1, (2, 2, 2))):
        z, y, x = inside[rng.integers(len(inside))]
        lab[z:z + a, y:y + b, x:x + e] = c
    return lab


def _filters(lab_np, conn, applied=None):
    from ctunet_amd import postprocess
    t = torch.from_numpy(lab_np).cuda()
    t0 = t.clone()
    for k in (1, 3):
        got = postprocess.keep_largest_connected_component(t, applied_labels=applied, connectivity=conn, num_components=k)
        assert got.dtype == t.dtype and got.shape == t.shape
        assert np.array_equal(got.cpu().numpy(), _ref_filter(lab_np[None] if lab_np.ndim == 3 else lab_np, conn, applied,
                                                              k=k).reshape(lab_np.shape))
    for s in (0, 1, 50):
        got = postprocess.remove_small_objects(t, s, applied_labels=applied, connectivity=conn)
        assert got.dtype == t.dtype and got.shape == t.shape
        assert np.array_equal(got.cpu().numpy(), _ref_filter(lab_np[None] if lab_np.ndim == 3 else lab_np, conn, applied,
                                                              min_size=s).reshape(lab_np.shape))
    assert torch.equal(t, t0)


@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("conn", CONNS)
def test_filters_on_multiclass_label_maps(dtype, conn):
    lab = _shell_labels(40, 56, 72, 3, dtype)
    _filters(lab, conn)
    batch = np.stack([lab, _shell_labels(40, 56, 72, 4, dtype), np.zeros_like(lab)])
    _filters(batch, conn)


def test_applied_labels_subset_leaves_other_classes_unchanged():
    from ctunet_amd import postprocess
    lab = _shell_labels(40, 56, 72, 5, np.int64)
    lab[lab == 2] = 7                                   # arbitrary int64 class values
    lab[2:4, 2:4, 2:4] = 1 << 40
    lab[30:32, 2:4, 2:4] = 1 << 40
    for applied in ([7], [1 << 40], [1, 7]):
        _filters(lab, 3, applied)
    got = postprocess.keep_largest_connected_component(torch.from_numpy(lab).cuda(), applied_labels=[7]).cpu().numpy()
    assert np.array_equal(got[lab != 7], lab[lab != 7])
    u8 = _shell_labels(40, 56, 72, 6, np.uint8)
    got = postprocess.remove_small_objects(torch.from_numpy(u8).cuda(), 50, applied_labels=[2]).cpu().numpy()
    assert np.array_equal(got[u8 != 2], u8[u8 != 2])
    assert np.array_equal(got, _ref_filter(u8[None], 3, [2], min_size=50)[0])


def test_ties_go_to_the_earlier_component():
    from ctunet_amd import postprocess
    lab = np.zeros((12, 16, 40), np.uint8)
    lab[8:10, 2:4, 30:33] = 1          # later in C order
    lab[1:3, 10:12, 5:8] = 1           # earlier, same size (12 voxels)
    lab[5, 5, 5] = 1
    got = postprocess.keep_largest_connected_component(torch.from_numpy(lab).cuda()).cpu().numpy()
    exp = np.zeros_like(lab)
    exp[1:3, 10:12, 5:8] = 1
    assert np.array_equal(got, exp)
    assert np.array_equal(got, _ref_filter(lab[None], 3, k=1)[0])
    got2 = postprocess.keep_largest_connected_component(torch.from_numpy(lab).cuda(), num_components=2).cpu().numpy()
    assert np.array_equal(got2, np.where(lab.astype(bool) & ~(np.arange(12)[:, None, None] == 5), lab, 0))


# ---------------------------------------------------------------------------------------------- determinism, graphs
def test_deterministic_and_graph_capture():
    from ctunet_amd import postprocess
    rng = np.random.default_rng(11)
    mask = torch.from_numpy(rng.random((2, 48, 64, 80)) < 0.3).cuda()
    lab = torch.from_numpy(_shell_labels(48, 64, 80, 12, np.uint8)).cuda()
    a, na = postprocess.label(mask)
    b, nb = postprocess.label(mask)
    assert torch.equal(a, b) and torch.equal(na, nb)
    ka = postprocess.keep_largest_connected_component(lab, num_components=2)
    kb = postprocess.keep_largest_connected_component(lab, num_components=2)
    assert torch.equal(ka, kb)

    # graph: capture once on a side stream, replay after copying new inputs into the static tensors
    sm, sl = mask.clone(), lab.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        postprocess.label(sm)
        postprocess.keep_largest_connected_component(sl, num_components=2)
        postprocess.remove_small_objects(sl, 20)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st_lab, st_num = postprocess.label(sm)
        st_keep = postprocess.keep_largest_connected_component(sl, num_components=2)
        st_small = postprocess.remove_small_objects(sl, 20)
    sm.copy_(torch.from_numpy(rng.random((2, 48, 64, 80)) < 0.5))
    sl.copy_(torch.from_numpy(_shell_labels(48, 64, 80, 13, np.uint8)))
    graph.replay()
    torch.cuda.synchronize()
    el, en = postprocess.label(sm.clone())
    assert torch.equal(st_lab, el) and torch.equal(st_num, en)
    assert torch.equal(st_keep, postprocess.keep_largest_connected_component(sl.clone(), num_components=2))
    assert torch.equal(st_small, postprocess.remove_small_objects(sl.clone(), 20))
    assert not torch.equal(st_lab, a)


# ---------------------------------------------------------------------------------------------- full size, the chain
def test_full_size_two_class_keep_largest():
    from ctunet_amd import postprocess
    lab = _shell_labels(224, 512, 512, 21, np.uint8)
    got = postprocess.keep_largest_connected_component(torch.from_numpy(lab).cuda()).cpu().numpy()
    assert np.array_equal(got, _ref_filter(lab[None], 3, k=1)[0])


def test_cleanup_restores_the_surface_metrics_of_a_clean_shell():
    from ctunet_amd import metrics, postprocess
    clean = _shell_labels(64, 96, 96, 0, np.uint8, islands=False)
    noisy = clean.copy()
    noisy[3:5, 3:5, 3:6] = 1                     # far islands of both classes, inside the volume corner
    noisy[58:61, 88:90, 4:6] = 2
    noisy[30, 48, 48] = 1
    c, n = torch.from_numpy(clean).cuda(), torch.from_numpy(noisy).cuda()
    kw = dict(spacing=(1.0, 0.5, 0.5), percentile=95.0, tolerance=1.0)
    ref = metrics.surface_metrics(c, c, 3, **kw)
    dirty = metrics.surface_metrics(n, c, 3, **kw)
    assert not torch.equal(dirty["hd"], ref["hd"])
    fixed = postprocess.keep_largest_connected_component(n)
    assert torch.equal(fixed, c)
    got = metrics.surface_metrics(fixed, c, 3, **kw)
    for k in ref:
        assert torch.equal(got[k], ref[k]), k


def test_predict_volume_labels_pass_through_both_filters():
    import ctunet_amd as A
    from ctunet_amd import postprocess
    torch.manual_seed(3)
    net = A.UNetSP().cuda().eval()
    vol = torch.randn(2, 48, 40, 56, generator=torch.Generator().manual_seed(4)).cuda()
    pr = A.predict_volume(net, vol, patch=32, overlap=8, batch=2)
    heads = pr.labels if isinstance(pr.labels, (tuple, list)) else (pr.labels,)
    for lab in heads:
        for out in (postprocess.keep_largest_connected_component(lab),
                    postprocess.remove_small_objects(lab, 10, connectivity=1)):
            assert out.shape == lab.shape and out.dtype == lab.dtype and out.is_cuda
            ref = _ref_filter(lab.cpu().numpy().reshape((-1,) + tuple(lab.shape[-3:])), 3, k=1)
        assert np.array_equal(postprocess.keep_largest_connected_component(lab).cpu().numpy().reshape(ref.shape), ref)
