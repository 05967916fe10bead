"""Distance transform, signed distance and ball morphology of ctunet_amd.postprocess on the GPU against scipy.ndimage
computed here on the host (distance_ref.py; the references themselves are pinned in test_distance_cpu.py).

Tolerances.  Unit sampling: the int32 squared map is exact (bit-equal); the distance is the float32 square root of an
exactly representable integer, compared at rtol 1e-6 with scipy's float64 value rounded to float32.  Other samplings: the
float32 squared distance takes three products and two sums, the distance one square root, about 3e-7 relative in all;
1e-5 leaves room for a different, equidistant-up-to-rounding winner.  Ball results are bit-equal, every case asserting
first that the radius is at least 1e-4 (relative) away from every offset length (distance_ref.ball_decidable).
"""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import distance_ref as R

pytestmark = pytest.mark.gpu

INT32_MAX = 2 ** 31 - 1
ANISO = ((0.8, 0.45, 0.45), (1.0, 2.5, 0.7))
# W not a multiple of 4 / 16 / 64, several x blocks (130 > 64 lanes), lines past 64 (one lane block) and past 256
SHAPES = ((1, 1, 1), (1, 1, 70), (3, 5, 130), (17, 33, 65), (4, 300, 20), (260, 6, 10))
BATCH = (2, 40, 48, 72)


def _pp():
    from ctunet_amd import postprocess
    return postprocess


@functools.lru_cache(maxsize=None)
def _masks(shape):
    """name -> bool mask with at least one background voxel (never modified)."""
    out = {"d%.2f" % d: R.random_mask(shape, d, 7 + i) for i, d in enumerate((0.02, 0.5, 0.98))}
    corner = np.ones(shape, bool)
    corner[-1, -1, -1] = False                                    # a single site in a corner
    out["corner"] = corner
    for m in out.values():
        m.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref(shape, name, sampling):
    d = R.edt(_masks(shape)[name], sampling)
    d.setflags(write=False)
    return d


def _dev(m, dtype=torch.bool):
    return torch.from_numpy(np.array(m)).to(dtype).cuda()               # a copy: the cached masks are read-only


def _check_dist(got, ref, rtol):
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape
    torch.testing.assert_close(got.cpu(), torch.from_numpy(ref.astype(np.float32)), rtol=rtol, atol=0)


def _check_indices(idx, dist, mask, sampling, sq=None):
    """Every triple is in range, addresses a site of `mask` (a zero voxel) and lies at the returned distance."""
    shape = mask.shape
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (3,) + shape
    i = idx.cpu().numpy().astype(np.int64)
    for a in range(3):
        assert i[a].min() >= 0 and i[a].max() < shape[a]
    assert not mask[i[0], i[1], i[2]].any()
    grid = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    s = R.triple(sampling)
    k2 = [(i[a] - grid[a]) ** 2 for a in range(3)]
    phys = np.sqrt(sum(k2[a] * s[a] ** 2 for a in range(3)))
    np.testing.assert_allclose(dist.cpu().numpy().astype(np.float64), phys, rtol=1e-6, atol=0)
    if sq is not None:
        assert np.array_equal(sq.cpu().numpy(), (k2[0] + k2[1] + k2[2]).astype(np.int32))


# ---------------------------------------------------------------------------------------------- 1. unit sampling
@pytest.mark.parametrize("shape", SHAPES)
def test_unit_sampling_is_exact(shape):
    pp = _pp()
    for name, m in _masks(shape).items():
        ref = _ref(shape, name, None)
        t = _dev(m)
        sq, idx = pp.distance_transform_edt(t, squared=True, return_indices=True)
        assert sq.dtype == torch.int32 and sq.shape == t.shape
        want = np.rint(ref ** 2).astype(np.int32)
        assert np.array_equal(sq.cpu().numpy(), want), name
        d = pp.distance_transform_edt(t)
        _check_dist(d, ref, 1e-6)
        assert torch.equal(pp.distance_transform_edt(t, sampling=1.0, squared=True), sq)     # all-1 sampling is unit
        _check_indices(idx, d, m, None, sq)
        only = pp.distance_transform_edt(t, return_distances=False, return_indices=True)
        assert torch.equal(only, idx)


# ---------------------------------------------------------------------------------------------- 2. / 3. other samplings
@pytest.mark.parametrize("sampling", ANISO)
@pytest.mark.parametrize("shape", SHAPES)
def test_anisotropic_sampling(shape, sampling):
    pp = _pp()
    for name, m in _masks(shape).items():
        ref = _ref(shape, name, sampling)
        d, idx = pp.distance_transform_edt(_dev(m, torch.uint8), sampling=sampling, return_indices=True)
        _check_dist(d, ref, 1e-5)
        _check_indices(idx, d, m, sampling)
        sq = pp.distance_transform_edt(_dev(m), sampling=sampling, squared=True)
        assert sq.dtype == torch.float32
        torch.testing.assert_close(sq.cpu(), torch.from_numpy((ref ** 2).astype(np.float32)), rtol=2e-5, atol=0)
        torch.testing.assert_close(torch.sqrt(sq), pp.distance_transform_edt(_dev(m), sampling=sampling), rtol=1e-6, atol=0)


def test_batch_with_per_item_sampling_and_labels():
    pp = _pp()
    shape = BATCH[1:]
    labels = np.stack([R.blob(shape, 1).astype(np.int64) * 2 + R.blob(shape, 2, 3.0), R.blob(shape, 3) * 2 + R.blob(shape, 4)])
    assert set(np.unique(labels)) == {0, 1, 2, 3}
    t = torch.from_numpy(labels).cuda()
    sp = [list(ANISO[0]), list(ANISO[1])]
    for lab in (None, 2):
        m = labels != 0 if lab is None else labels == lab
        d, idx = pp.distance_transform_edt(t, sampling=sp, return_indices=True, label=lab)
        assert tuple(idx.shape) == (2, 3) + shape
        for n in range(2):
            _check_dist(d[n], R.edt(m[n], sp[n]), 1e-5)
            _check_indices(idx[n], d[n], m[n], sp[n])
        sd = pp.signed_distance(t, sampling=sp, label=lab)
        for n in range(2):
            _check_dist(sd[n], R.signed(m[n], sp[n]), 1e-5)
    # an int64 label map with large and negative labels, unit sampling, uint8 too
    big = torch.from_numpy(labels[0]).cuda() * 1000003 - (1 << 40)
    m = labels[0] == 3
    sq = pp.distance_transform_edt(big, label=3 * 1000003 - (1 << 40), squared=True)
    assert np.array_equal(sq.cpu().numpy(), np.rint(R.edt(m) ** 2).astype(np.int32))
    assert torch.equal(pp.distance_transform_edt(torch.from_numpy(labels[0]).to(torch.uint8).cuda(), label=3, squared=True), sq)


# ---------------------------------------------------------------------------------------------- 4. empty site set
@pytest.mark.parametrize("sampling", (None, ANISO[0]))
def test_empty_site_set_and_all_sites(sampling):
    pp = _pp()
    shape = (3, 5, 130)
    # item 0 all foreground (no site), item 1 all background (every voxel a site), item 2 ordinary
    m = np.stack([np.ones(shape, bool), np.zeros(shape, bool), np.array(_masks(shape)["d0.50"])])
    t = _dev(m, torch.uint8)
    d, idx = pp.distance_transform_edt(t, sampling=sampling, return_indices=True)
    sq = pp.distance_transform_edt(t, sampling=sampling, squared=True)
    assert torch.isinf(d[0]).all() and (d[0] > 0).all() and (idx[0] == -1).all()
    if sampling is None:
        assert sq.dtype == torch.int32 and (sq[0] == INT32_MAX).all()
    else:
        assert torch.isinf(sq[0]).all() and (sq[0] > 0).all()
    assert (d[1] == 0).all() and (sq[1] == 0).all()
    grid = np.stack(np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")).astype(np.int32)
    assert np.array_equal(idx[1].cpu().numpy(), grid)
    _check_dist(d[2], R.edt(m[2], sampling), 1e-6 if sampling is None else 1e-5)
    _check_indices(idx[2], d[2], m[2], sampling)
    sd = pp.signed_distance(t, sampling=sampling)
    assert (sd[0] == -float("inf")).all() and (sd[1] == float("inf")).all()
    _check_dist(sd[2], R.signed(m[2], sampling), 1e-6 if sampling is None else 1e-5)


# ---------------------------------------------------------------------------------------------- 5. signed distance
@pytest.mark.parametrize("shape", SHAPES[1:])
def test_signed_distance(shape):
    pp = _pp()
    for name in ("d0.02", "d0.50", "d0.98"):
        m = np.array(_masks(shape)[name])
        if not m.any():
            m.flat[-1] = True                                     # the reference needs both kinds of voxel
        for sampling, rtol in ((None, 1e-6), (ANISO[0], 1e-5), (ANISO[1], 1e-5)):
            sd = pp.signed_distance(_dev(m), sampling=sampling)
            _check_dist(sd, R.signed(m, sampling), rtol)
            g = sd.cpu().numpy()
            assert (g[m] < 0).all() and (g[~m] > 0).all()


# ---------------------------------------------------------------------------------------------- 6. ball morphology
_SCIPY = {"erosion": ndi.binary_erosion, "dilation": ndi.binary_dilation, "opening": ndi.binary_opening,
          "closing": ndi.binary_closing}
# (shape, radius, sampling): 3.2 exceeds the smallest side of (3, 5, 130); W = 65, 70, 130 leave scalar tails
BALL_CASES = (((17, 33, 65), 1.0, None), ((17, 33, 65), 2.5, None), ((17, 33, 65), 3.2, None), ((3, 5, 130), 3.2, None),
              ((17, 33, 65), 1.0, ANISO[0]), ((17, 33, 65), 2.0, ANISO[0]), ((12, 20, 70), 3.2, ANISO[1]),
              ((3, 5, 130), 3.2, ANISO[1]), ((1, 1, 70), 1.5, None), ((1, 1, 1), 2.5, None))


def _ball_ref(op, m, st):
    if op in ("erosion", "dilation"):
        return _SCIPY[op](m, st, border_value=0)
    return _SCIPY[op](m, st)


@pytest.mark.parametrize("shape,radius,sampling", BALL_CASES)
def test_ball_ops_bit_equal_to_scipy(shape, radius, sampling):
    pp = _pp()
    assert R.ball_decidable(radius, sampling, shape)
    assert R.ball_margin(radius, sampling, shape) >= 1e-4 or (radius, sampling) == (1.0, None)
    st = R.ball(radius, sampling)
    masks = (R.blob(shape, 5), R.random_mask(shape, 0.97, 6), np.ones(shape, bool))     # the last two touch every face
    for k, m in enumerate(masks):
        dtype = (torch.bool, torch.uint8, torch.int64)[k]
        t = _dev(m, dtype) if dtype == torch.bool else _dev(m, dtype) * 5      # (bool * int would promote to int64)
        assert t.dtype == dtype
        for op in ("erosion", "dilation", "opening", "closing"):
            got = getattr(pp, "ball_" + op)(t, radius, sampling=sampling)
            assert got.dtype == (torch.bool if dtype == torch.bool else torch.uint8) and got.shape == t.shape
            g = got.cpu().numpy()
            assert g.max(initial=0) <= 1
            assert np.array_equal(g.astype(bool), _ball_ref(op, m, st)), (op, k)


def test_ball_border_label_and_batch():
    pp = _pp()
    # a solid block touching all six faces: only the virtual border erodes it
    shape = (9, 10, 70)
    ones = np.ones(shape, bool)
    for r, s in ((1.5, None), (2.0, ANISO[0])):
        assert R.ball_margin(r, s, shape) >= 1e-4
        e = pp.ball_erosion(_dev(ones), r, sampling=s).cpu().numpy()
        ref = ndi.binary_erosion(ones, R.ball(r, s), border_value=0)
        assert np.array_equal(e, ref) and 0 < ref.sum() < ones.sum()
    # label= on an int64 / uint8 map, a batch with per-item sampling
    shape = (12, 20, 70)
    labels = np.stack([R.blob(shape, 1) * 2 + R.blob(shape, 2), R.blob(shape, 3) * 2 + R.blob(shape, 4)]).astype(np.int64)
    sp = [list(ANISO[0]), list(ANISO[1])]
    r = 2.2
    for s in sp:
        assert R.ball_margin(r, s, shape) >= 1e-4
    for dtype in (torch.int64, torch.uint8):
        t = torch.from_numpy(labels).to(dtype).cuda()
        for op in ("erosion", "dilation", "opening", "closing"):
            got = getattr(pp, "ball_" + op)(t, r, sampling=sp, label=2).cpu().numpy()
            for n in range(2):
                assert np.array_equal(got[n].astype(bool), _ball_ref(op, labels[n] == 2, R.ball(r, sp[n]))), (op, n)


def _implant_scene(shape, seed):
    """(full skull prediction, defective skull prediction): a thick shell, a cut-out flap, surface noise, stray islands."""
    d, h, w = shape
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    rad = np.sqrt(((zz - d * 0.5) / (0.45 * d)) ** 2 + ((yy - h * 0.5) / (0.46 * h)) ** 2 + ((xx - w * 0.5) / (0.44 * w)) ** 2)
    skull = (rad <= 1.0) & (rad >= 0.7)
    hole = ((zz - 0.5 * d) ** 2 + (yy - 0.5 * h) ** 2 + (xx - 0.92 * w) ** 2) <= (0.22 * min(shape)) ** 2
    surface = skull & ~ndi.binary_erosion(skull)
    full = skull & ~(surface & (rng.random(shape) < 0.3))
    defective = skull & ~hole & ~(surface & (rng.random(shape) < 0.3))
    for i in range(6):
        z, y, x = (int(rng.integers(1, s - 4)) for s in shape)
        if not skull[z - 1:z + 3, y - 1:y + 3, x - 1:x + 3].any():
            full[z:z + 1 + i % 2, y:y + 2, x:x + 1 + i % 2] = True
    return full, defective


def test_extract_implant_with_a_ball_opening():
    pp = _pp()
    shape = (48, 56, 72)
    full, defective = _implant_scene(shape, 0)
    f, d = _dev(full, torch.uint8), _dev(defective)
    r, s = 1.5, ANISO[0]
    assert R.ball_margin(r, s, shape) >= 1e-4
    for fill, conn, num in ((False, 3, 1), (True, 1, 2)):
        got = pp.extract_implant(f, d, connectivity=conn, num_components=num, fill_holes=fill, opening_radius=r, sampling=s)
        assert got.dtype == torch.uint8 and got.shape == f.shape
        m = pp.ball_opening(((f != 0) & (d == 0)).to(torch.uint8), r, sampling=s)
        if fill:
            m = pp.binary_fill_holes(m, 1)
        m = pp.keep_largest_connected_component(m, connectivity=conn, num_components=num)
        assert torch.equal(got, m) and 0 < int(got.sum()) < got.numel()
        # ... and the host composition on scipy
        h = ndi.binary_opening(full & ~defective, R.ball(r, s))
        if fill:
            h = ndi.binary_fill_holes(h)
        lab, n = ndi.label(h, ndi.generate_binary_structure(3, conn))
        sizes = np.bincount(lab.ravel())[1:]
        keep = np.zeros(n + 1, bool)
        keep[1 + np.argsort(-sizes, kind="stable")[:num]] = True
        assert np.array_equal(got.cpu().numpy().astype(bool), keep[lab])
    # without the new arguments: the iterated opening, as before (the expectation of test_morphology_gpu's composition)
    h = ndi.binary_opening(full & ~defective, ndi.generate_binary_structure(3, 1), iterations=1)
    lab, n = ndi.label(h, np.ones((3, 3, 3)))
    sizes = np.bincount(lab.ravel())[1:]
    ref = (lab == 1 + np.argsort(-sizes, kind="stable")[0]).astype(np.uint8)
    assert np.array_equal(pp.extract_implant(f, d).cpu().numpy(), ref)
    assert not np.array_equal(pp.extract_implant(f, d, opening_radius=r, sampling=s).cpu().numpy(), ref)


# ---------------------------------------------------------------------------------------------- 7. determinism, capture
def _tail(pp, buf, lab):
    sp = [list(ANISO[0]), list(ANISO[1])]
    return (pp.distance_transform_edt(buf, squared=True, return_indices=True)
            + pp.distance_transform_edt(buf, sampling=sp, return_indices=True)
            + (pp.signed_distance(buf, sampling=sp), pp.signed_distance(lab, label=2), pp.ball_opening(buf, 2.2, sampling=sp),
               pp.ball_closing(lab, 2.5, label=1)))


def test_two_calls_are_bit_equal_and_a_captured_call_replays():
    pp = _pp()
    shape = BATCH[1:]
    first = np.stack([R.blob(shape, 1), R.random_mask(shape, 0.5, 2)])
    second = np.stack([R.random_mask(shape, 0.9, 3), ~R.blob(shape, 4)])
    lab1 = np.stack([R.blob(shape, 5) * 2 + R.blob(shape, 6), R.blob(shape, 7) * 1]).astype(np.int64)
    lab2 = np.stack([R.blob(shape, 8) * 1, R.blob(shape, 9) * 2 + R.blob(shape, 10)]).astype(np.int64)
    buf, lab = _dev(first, torch.uint8), torch.from_numpy(lab1).cuda()
    a, b = _tail(pp, buf, lab), _tail(pp, buf, lab)
    for x, y in zip(a, b):
        assert torch.equal(x, y)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _tail(pp, buf, lab)                                       # warm-up: library loaded, kernels resident
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                 # outputs and workspaces: the graph's private pool
        outs = _tail(pp, buf, lab)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(outs, a):
        assert torch.equal(x, y)
    buf.copy_(_dev(second, torch.uint8))
    lab.copy_(torch.from_numpy(lab2).cuda())
    graph.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in outs]
    eager = _tail(pp, buf, lab)
    for x, y, z in zip(replayed, eager, a):
        assert torch.equal(x, y)
        assert not torch.equal(x, z)
