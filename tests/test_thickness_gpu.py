"""Local thickness of ctunet_amd.postprocess on the GPU against the unpruned numpy search of thickness_ref.py (pinned on
known answers in test_thickness_cpu.py).

Every comparison of a thickness map is bit for bit.  Unit sampling: the squared distances come from scipy's transform
rounded to integers, every quantity of the rule is an integer and the final float32 square root is correctly rounded on
both sides.  Other samplings: the reference gets the device's own squared float32 map (that function has its tests in
test_distance_gpu.py) and applies the float32 offset rule product by product, so a contracted multiply-add or an unsafe
pruning margin on the device shows as a differing bit.  Summary: counts, min and max are exact; the mean is a float64 sum
of at most 33 600 float32 values, within 1e-12 relative of numpy's pairwise float64 mean.
"""
import functools

import numpy as np
import pytest
import torch

import distance_ref as DR
import thickness_ref as R

pytestmark = pytest.mark.gpu

ANISO = ((0.8, 0.45, 0.45), (1.0, 2.5, 0.7))
# one voxel; one row; W past two tiles of 8 with odd sides; sides that are no multiple of the tile; the shape of case 4
SHAPES = ((1, 1, 70), (3, 5, 130), (17, 33, 65), (20, 24, 70))
# a single background voxel in a corner: radii up to the volume's diagonal, across every tile boundary.  Its unpruned
# reference costs voxels^2, 3 s at (17, 33, 65), so the large case is (13, 21, 45): 0.4 s
CORNER_SHAPES = ((1, 1, 70), (3, 5, 130), (13, 21, 45))
ANISO_SHAPE = (20, 24, 70)


def _pp():
    from ctunet_amd import postprocess
    return postprocess


def _dev(m, dtype=torch.bool):
    return torch.from_numpy(np.array(m)).to(dtype).cuda()               # a copy: the cached masks are read-only


@functools.lru_cache(maxsize=None)
def _masks(shape):
    """name -> bool mask with at least one background voxel (never modified)."""
    out = {"blob": DR.blob(shape, 3), "sparse": DR.random_mask(shape, 0.02, 7), "dense": DR.random_mask(shape, 0.98, 9)}
    if shape in CORNER_SHAPES:
        corner = np.ones(shape, bool)
        corner[-1, -1, -1] = False
        out["corner"] = corner
    for m in out.values():
        m.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _ref_unit(shape, name):
    t = R.local_thickness(R.squared_edt(_masks(shape)[name]))
    t.setflags(write=False)
    return t


def _same(got, ref, what=None):
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape, what
    g = got.cpu().numpy()
    bad = g != ref
    print(what, "differing voxels:", int(bad.sum()), "of", ref.size, "max |got - ref|:",
          float(np.abs(np.where(bad, g - ref, 0)).max()) if bad.any() else 0.0)
    assert np.array_equal(g, ref), what


# ---------------------------------------------------------------------------------------------- 1. unit sampling
def test_one_voxel_of_foreground_is_infinitely_thick():
    pp = _pp()
    t = pp.local_thickness(torch.ones(1, 1, 1, dtype=torch.bool, device="cuda"))
    assert t.dtype == torch.float32 and t.shape == (1, 1, 1) and torch.isinf(t).all() and (t > 0).all()
    assert torch.equal(pp.local_thickness(torch.zeros(1, 1, 1, dtype=torch.uint8, device="cuda")), torch.zeros(1, 1, 1, device="cuda"))


@pytest.mark.parametrize("shape", sorted(set(SHAPES + CORNER_SHAPES)))
def test_unit_sampling_equals_the_unpruned_search(shape):
    pp = _pp()
    for name, m in _masks(shape).items():
        _same(pp.local_thickness(_dev(m)), _ref_unit(shape, name), (shape, name))


# ---------------------------------------------------------------------------------------------- 2. rod through a ball
def test_thin_rod_through_a_thick_ball():
    pp = _pp()
    shape = (19, 19, 40)
    z, y, x = np.meshgrid(np.arange(19) - 9, np.arange(19) - 9, np.arange(40) - 20, indexing="ij")
    ball = z * z + y * y + x * x <= 49
    m = ball.copy()
    m[9, 9, 1:39] = True                                                # the rod, one voxel thick, along x
    d2 = R.squared_edt(m)
    ref = R.local_thickness(d2)
    got = pp.local_thickness(_dev(m, torch.uint8))
    _same(got, ref, "rod")
    g = got.cpu().numpy()
    centre = np.float32(2) * np.sqrt(np.float32(d2[9, 9, 20]))          # the ball's value: that of its centre voxel
    assert d2[9, 9, 20] == 50 and g.max() == centre
    rod = np.zeros(shape, bool)
    rod[9, 9, 1:39] = True
    assert (g[rod & ball] == centre).all()                              # inside the ball the rod reads the ball
    assert (g[rod & ~ball] == 2).all() and (rod & ~ball).sum() == 38 - 15
    assert (g[~m] == 0).all()


# ---------------------------------------------------------------------------------------------- 3. large radius, solid body
def test_solid_cube_free_and_against_three_faces():
    pp = _pp()
    free = np.zeros((24, 24, 24), bool)
    free[2:22, 2:22, 2:22] = True
    pushed = np.zeros((24, 24, 24), bool)
    pushed[:20, 4:, :20] = True                                         # no background beyond z = 0, y = 23 and x = 0
    for name, m in (("free", free), ("pushed", pushed)):
        ref = R.local_thickness(R.squared_edt(m))
        got = pp.local_thickness(_dev(m))
        _same(got, ref, name)
    assert ref.max() > 2 * 19                                           # the volume's faces are no background


# ---------------------------------------------------------------------------------------------- 4. other samplings
@pytest.mark.parametrize("sampling", ANISO)
def test_anisotropic_sampling_equals_the_float32_rule(sampling):
    pp = _pp()
    for name, m in _masks(ANISO_SHAPE).items():
        t = _dev(m)
        d2 = pp.distance_transform_edt(t, sampling=sampling, squared=True)
        assert d2.dtype == torch.float32
        ref = R.local_thickness(d2.cpu().numpy(), sampling)
        _same(pp.local_thickness(t, sampling=sampling), ref, (sampling, name))
    # an item without background, on the float32 path
    assert torch.isinf(pp.local_thickness(torch.ones(3, 9, 17, dtype=torch.uint8, device="cuda"), sampling=sampling)).all()


# ---------------------------------------------------------------------------------------------- 5. batch and arguments
def test_batch_labels_and_dtypes():
    pp = _pp()
    shape = (12, 20, 40)
    pair = np.stack([DR.blob(shape, 11), DR.random_mask(shape, 0.9, 12)])
    t = _dev(pair)
    sp = [list(ANISO[0]), list(ANISO[1])]
    both = pp.local_thickness(t, sampling=sp)
    assert both.shape == (2,) + shape
    for i in range(2):
        assert torch.equal(both[i], pp.local_thickness(t[i], sampling=sp[i]))
    unit = pp.local_thickness(t)
    for i in range(2):
        assert torch.equal(unit[i], pp.local_thickness(t[i]))
        assert torch.equal(unit[i], pp.local_thickness(t[i], sampling=1.0))              # all-1 sampling is the exact path
    # one unit item among scaled ones takes the float32 path, whose integers are exact too
    mixed = pp.local_thickness(t, sampling=[[1.0, 1.0, 1.0], [2.0, 2.0, 2.0]])
    assert torch.equal(mixed[0], unit[0]) and torch.equal(mixed[1], unit[1] * 2)
    labels = (DR.blob(shape, 13).astype(np.int64) * 2 + DR.blob(shape, 14, 3.0))
    assert set(np.unique(labels)) == {0, 1, 2, 3}
    labels[labels == 3] = 1
    lt = torch.from_numpy(labels).cuda()
    for s in (None, ANISO[0]):
        assert torch.equal(pp.local_thickness(lt, sampling=s, label=2), pp.local_thickness(lt == 2, sampling=s))
        a = pp.local_thickness(t[0], sampling=s)
        assert torch.equal(a, pp.local_thickness(t[0].to(torch.uint8), sampling=s))
        assert torch.equal(a, pp.local_thickness(t[0].to(torch.int64) * 5, sampling=s))


# ---------------------------------------------------------------------------------------------- 6. determinism, capture
def _tail(pp, buf):
    t = pp.local_thickness(buf, sampling=ANISO[0])
    u = pp.local_thickness(buf)
    return t, pp.thickness_summary(t, 2.0), u, pp.thickness_summary(u)


def test_two_calls_agree_and_a_captured_graph_follows_its_input():
    pp = _pp()
    shape = (2, 12, 20, 40)
    first = np.stack([DR.blob(shape[1:], 1), DR.random_mask(shape[1:], 0.5, 2)])
    second = np.stack([DR.random_mask(shape[1:], 0.9, 3), ~DR.blob(shape[1:], 4)])
    buf = _dev(first, torch.uint8)
    a, b = _tail(pp, buf), _tail(pp, buf)
    for x, y in zip(a, b):
        assert torch.equal(x, y)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _tail(pp, buf)                                            # warm-up: library loaded, kernels resident
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                 # outputs and workspaces: the graph's private pool
        outs = _tail(pp, buf)
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(outs, a):
        assert torch.equal(x, y)
    buf.copy_(_dev(second, torch.uint8))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in outs]
    eager = _tail(pp, buf)
    for x, y, z in zip(replayed, eager, a):
        assert torch.equal(x, y)
        assert not torch.equal(x, z)


# ---------------------------------------------------------------------------------------------- 7. summary
def _check_summary(pp, t, min_thickness):
    got = pp.thickness_summary(t, min_thickness)
    assert got.dtype == torch.float64 and got.is_cuda
    assert tuple(got.shape) == ((5,) if t.dim() == 3 else (t.shape[0], 5))
    rows = got.cpu().numpy().reshape(-1, 5)
    maps = t.cpu().numpy().reshape((-1,) + tuple(t.shape[-3:]))
    for row, m in zip(rows, maps):
        want = R.summary(m, min_thickness)
        print("summary", row, want)
        assert row[0] == want[0] and row[1] == want[1] and row[2] == want[2] and row[4] == want[4]
        if want[0] == 0:
            assert np.isnan(row[3])
        elif np.isinf(want[3]):
            assert row[3] == want[3]
        else:
            assert abs(row[3] - want[3]) <= 1e-12 * abs(want[3])


def test_summary_equals_numpy_on_the_returned_maps():
    pp = _pp()
    for shape in SHAPES:
        for name, m in _masks(shape).items():
            t = pp.local_thickness(_dev(m))
            _check_summary(pp, t, 2.5)
            _check_summary(pp, t, None)
    for sampling in ANISO:
        t = pp.local_thickness(_dev(_masks(ANISO_SHAPE)["blob"]), sampling=sampling)
        _check_summary(pp, t, 2.0)
        _check_summary(pp, t, float("inf"))
    # a batch: a map, an empty item and an item of infinities, each row on its own
    batch = torch.stack([pp.local_thickness(_dev(_masks(ANISO_SHAPE)["dense"])), torch.zeros(ANISO_SHAPE, device="cuda"),
                         torch.full(ANISO_SHAPE, float("inf"), device="cuda")])
    _check_summary(pp, batch, 3.0)
    rows = pp.thickness_summary(batch, 3.0).cpu().numpy()
    assert rows[1, 0] == 0 and rows[1, 1] == np.inf and rows[1, 2] == 0 and np.isnan(rows[1, 3]) and rows[1, 4] == 0
    assert rows[2, 0] == np.prod(ANISO_SHAPE) and rows[2, 1] == rows[2, 2] == rows[2, 3] == np.inf and rows[2, 4] == 0
    assert pp.thickness_summary(torch.zeros(1, 1, 1, device="cuda")).cpu().numpy()[0] == 0
