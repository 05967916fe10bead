"""ctunet_amd.preprocess on the GPU: every comparison with the restated rules (tests/preprocess_ref.py) is bit-equal."""
import functools

import numpy as np
import pytest
import torch

import preprocess_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
# gauss_xy tiles are 32 rows x 64 voxels, gauss_z tiles 32 planes x 128 voxels of the flattened plane: (17, 33, 70) and the
# batch cross the first in x and y with clipped last tiles, (35, 6, 10) crosses the second in z; (3, 4, 5) lies below
# every radius
SHAPES = ((5, 7, 19), (17, 33, 70), (3, 4, 5), (2, 9, 40, 130), (35, 6, 10))
SIGMAS = ((0.8, 1.3, 2.9), (0.0, 0.5, 7.9), (2.0, 2.0, 2.0))
ALL_32 = (7.9, 7.9, 7.9)                                         # R = 32 on every axis: the tile of gauss_xy outgrows 64 KB of LDS
MODES = ("nearest", "reflect", "constant")
DTYPES = {"i2": torch.int16, "f4": torch.float32, "u1": torch.uint8}


def _values(shape, dt, seed):
    rng = np.random.default_rng(seed)
    if dt == "i2":
        return rng.integers(-1024, 3072, shape).astype(np.int16)
    if dt == "u1":
        return rng.integers(0, 256, shape).astype(np.uint8)
    return (rng.standard_normal(shape) * 1000).astype(np.float32)


def _dev(x: np.ndarray) -> torch.Tensor:
    return torch.tensor(x, device=DEV)                          # a copy: the shared references stay read-only


def _same_bits(got: torch.Tensor, want: np.ndarray):
    got, want = np.atleast_1d(got.cpu().numpy()), np.atleast_1d(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), \
        f"{np.count_nonzero(got != want)} of {want.size} elements differ"


def _capture(run):
    """`run` captured into a graph after one warm-up on a side stream."""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    return graph


@functools.lru_cache(maxsize=None)
def _three_class():
    x = R.three_class_volume(20000)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _head():
    x = R.synthetic_head()
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------ gaussian_filter
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", MODES)
def test_gaussian_is_the_rule(shape, mode):
    from ctunet_amd import preprocess as pp
    cval = -1000.0 if mode == "constant" else 0.0
    sigmas = SIGMAS + ((ALL_32,) if shape == (35, 6, 10) else ())
    for i, sig in enumerate(sigmas):
        for j, dt in enumerate(DTYPES):
            x = _values(shape, dt, 10 * i + j)
            got = pp.gaussian_filter(_dev(x), sig, mode=mode, cval=cval)
            assert got.dtype == torch.float32
            _same_bits(got, R.gaussian_filter(x, sig, mode, cval))


def test_gaussian_spacing_out_and_reproducibility():
    from ctunet_amd import preprocess as pp
    shape, spacing = (17, 33, 70), (0.8, 0.45, 0.45)
    x = _values(shape, "i2", 3)
    xd = _dev(x)
    want = R.gaussian_filter(x, tuple(1.0 / s for s in spacing))
    a = pp.gaussian_filter(xd, 1.0, spacing=spacing)
    _same_bits(a, want)
    assert torch.equal(a.view(torch.int32), pp.gaussian_filter(xd, 1.0, spacing=spacing).view(torch.int32))
    # out= 4 bytes off the 16-byte grid, guarded either side
    n = x.size
    buf = torch.full((n + 9,), 7.0, dtype=torch.float32, device=DEV)
    out = buf[5:5 + n].view(shape)
    assert out.data_ptr() % 16 == 4
    assert pp.gaussian_filter(xd, 1.0, spacing=spacing, out=out) is out
    _same_bits(out, want)
    assert bool((buf[:5] == 7.0).all()) and bool((buf[5 + n:] == 7.0).all())
    # a non-contiguous input is made contiguous
    wide = torch.from_numpy(_values((17, 33, 140), "i2", 4)).to(DEV)
    _same_bits(pp.gaussian_filter(wide[:, :, ::2], 1.0, spacing=spacing),
               R.gaussian_filter(wide[:, :, ::2].cpu().numpy(), tuple(1.0 / s for s in spacing)))


def test_gaussian_replays_on_new_input():
    from ctunet_amd import preprocess as pp
    shape, sig = (17, 33, 70), (0.8, 1.3, 2.9)
    x0, x1 = _values(shape, "i2", 5), _values(shape, "i2", 6)
    xd = _dev(x0)
    out = torch.empty(shape, dtype=torch.float32, device=DEV)
    graph = _capture(lambda: pp.gaussian_filter(xd, sig, mode="reflect", out=out))
    xd.copy_(torch.from_numpy(x1))
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _same_bits(out, R.gaussian_filter(x1, sig, "reflect"))
    xd.copy_(torch.from_numpy(x0))
    graph.replay()
    torch.cuda.synchronize()
    _same_bits(out, R.gaussian_filter(x0, sig, "reflect"))


# ------------------------------------------------------------------------------------------------ histogram
def _hist_values(shape, dt, seed):
    """Values on both sides of (-200, 3000), some equal to either end, NaN and infinities in float32."""
    x = _values(shape, dt, seed)
    flat = x.reshape(-1)
    if dt == "u1":
        return x
    flat[::7] = 3000
    flat[3::11] = -200
    if dt == "f4":
        flat[5::13] = np.nan
        flat[6::17] = np.inf
        flat[8::19] = -np.inf
    return x


@pytest.mark.parametrize("shape", ((1,), (63,), (4097,), (3, 17, 33, 70)), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("bins", (2, 256, 4096))
def test_histogram_is_the_rule(shape, bins):
    from ctunet_amd import preprocess as pp
    for j, dt in enumerate(DTYPES):
        x = _hist_values(shape, dt, j)
        xd = _dev(x)
        rng = (10, 200) if dt == "u1" else (-200, 3000)
        want = R.histogram(x, bins, rng)
        inside = x.astype(np.float64)
        assert want.sum() == np.count_nonzero((inside >= rng[0]) & (inside <= rng[1]))
        got = pp.histogram(xd, bins, rng)
        assert got.dtype == torch.int64 and tuple(got.shape) == (bins,)
        _same_bits(got, want)
        _same_bits(pp.histogram(xd, bins, rng), want)                                  # two calls agree
        _same_bits(pp.histogram(xd, bins, torch.tensor(rng, dtype=torch.float64, device=DEV)), want)
        auto = R.histogram(x, bins)                                                    # the finite minimum and maximum
        assert auto.sum() == np.count_nonzero(np.isfinite(inside))
        out = torch.full((bins,), -5, dtype=torch.int64, device=DEV)
        assert pp.histogram(xd, bins, out=out) is out
        _same_bits(out, auto)
        lo, hi = R.finite_range(x)
        _same_bits(pp.finite_range(xd), np.array([lo, hi]))


def test_histogram_corner_cases():
    from ctunet_amd import preprocess as pp
    const = np.full((5, 6, 7), -37, np.int16)
    cd = _dev(const)
    want = R.histogram(const, 256)
    assert want[128] == const.size
    _same_bits(pp.histogram(cd), want)
    _same_bits(pp.histogram(cd, 256, (-37, -37)), want)                                # hi == lo widens by 0.5
    # off the 16-byte grid at the front: a slice of a larger buffer
    x = _values((4097 + 3,), "i2", 9)
    xd = _dev(x)
    for off in (1, 3):
        assert xd[off:].data_ptr() % 16 == 2 * off
        _same_bits(pp.histogram(xd[off:], 256, (-1024, 3072)), R.histogram(x[off:], 256, (-1024, 3072)))
        _same_bits(pp.finite_range(xd[off:]), np.array(R.finite_range(x[off:])))
    nothing = torch.full((70,), float("nan"), device=DEV)
    assert int(pp.histogram(nothing, 16).sum()) == 0
    _same_bits(pp.finite_range(nothing), np.array([np.inf, -np.inf]))


# ------------------------------------------------------------------------------------------------ threshold_otsu
def test_otsu_is_the_rule():
    from ctunet_amd import preprocess as pp
    x = _three_class()
    xd = _dev(x)
    for bins, rng in ((256, (-200, 3000)), (256, (-1024, 3072)), (4096, (-1024, 3072)), (100, (-200, 2000)), (2, (-200, 3000))):
        k, t = R.otsu(R.histogram(x, bins, rng), rng)
        thr, idx = pp.threshold_otsu(xd, bins=bins, range=rng, return_index=True)
        assert thr.dtype == torch.float64 and thr.dim() == 0 and idx.dtype == torch.int64 and idx.dim() == 0
        assert int(idx) == k
        _same_bits(thr, np.float64(t))
        h = pp.histogram(xd, bins, rng)
        _same_bits(pp.threshold_otsu(hist=h, range=rng), np.float64(t))
        _same_bits(pp.threshold_otsu(hist=h, range=torch.tensor(rng, dtype=torch.float64, device=DEV)),
                   np.float64(t))
    t = float(pp.threshold_otsu(xd, range=(-200, 3000)))
    assert 30.0 < t < 900.0                                                            # between the tissue and bone means
    k, t = R.otsu(R.histogram(x, 256), R.finite_range(x))                              # range=None: found on the device
    thr, idx = pp.threshold_otsu(xd, return_index=True)
    assert int(idx) == k and float(thr) == t and -1000.0 < t < 30.0


def test_otsu_documented_indices():
    from ctunet_amd import preprocess as pp
    const = np.full(1000, 37, np.int16)
    thr, idx = pp.threshold_otsu(_dev(const), return_index=True)
    assert int(idx) == 0 and float(thr) == 36.5 + 0.5 / 256
    two = np.where(np.arange(1000) % 3 == 0, 100, -50).astype(np.int16)
    thr, idx = pp.threshold_otsu(_dev(two), bins=64, range=(-100, 156), return_index=True)
    assert (int(idx), float(thr)) == R.otsu(R.histogram(two, 64, (-100, 156)), (-100, 156)) == (12, -50.0)
    thr, idx = pp.threshold_otsu(hist=torch.zeros(16, dtype=torch.int64, device=DEV), range=(0, 1), return_index=True)
    assert int(idx) == 0 and float(thr) == 0.5 / 16


def test_otsu_feeds_binarize_inside_one_graph():
    from ctunet_amd import preprocess as pp
    rng = (-200, 3000)
    a = _head()
    b = _values(a.shape, "i2", 8)                                                      # another volume, another threshold
    ta, tb = R.otsu(R.histogram(a, 256, rng), rng)[1], R.otsu(R.histogram(b, 256, rng), rng)[1]
    assert ta != tb and not np.array_equal(R.binarize(b, ta), R.binarize(b, tb))
    xd = _dev(a)
    mask = torch.empty(a.shape, dtype=torch.uint8, device=DEV)
    graph = _capture(lambda: pp.binarize(xd, pp.threshold_otsu(xd, range=rng), out=mask))
    graph.replay()
    torch.cuda.synchronize()
    _same_bits(mask, R.binarize(a, ta))
    xd.copy_(torch.from_numpy(b))
    graph.replay()
    torch.cuda.synchronize()
    _same_bits(mask, R.binarize(b, tb))


# ------------------------------------------------------------------------------------------------ binarize
@pytest.mark.parametrize("w", (15, 16, 17, 70))
def test_binarize_is_the_rule(w):
    from ctunet_amd import preprocess as pp
    shape = (3, 5, w)
    for j, dt in enumerate(DTYPES):
        x = _hist_values(shape, dt, 20 + j)
        xd = _dev(x)
        lower, upper = (50, 200) if dt == "u1" else (-200, 3000)
        for up in (None, upper):
            want = R.binarize(x, lower, up)
            assert 0 < want.sum() < want.size
            got = pp.binarize(xd, lower, up)
            assert got.dtype == torch.uint8
            _same_bits(got, want)
            lt = torch.tensor(float(lower), dtype=torch.float64, device=DEV)
            ut = None if up is None else torch.tensor(float(up), dtype=torch.float64, device=DEV)
            _same_bits(pp.binarize(xd, lt, ut), want)
            buf = torch.full((x.size + 40,), 9, dtype=torch.uint8, device=DEV)         # out= one byte off the 16-byte grid
            out = buf[17:17 + x.size].view(shape)
            assert out.data_ptr() % 16 == 1
            assert pp.binarize(xd, lower, up, out=out) is out
            _same_bits(out, want)
            assert bool((buf[:17] == 9).all()) and bool((buf[17 + x.size:] == 9).all())
    half = _dev(np.array([0.5, 1.0, 1.5, np.nan], np.float32))
    assert pp.binarize(half, 0.5, 1.5).tolist() == [0, 1, 1, 0]                        # > lower, <= upper


# ------------------------------------------------------------------------------------------------ extract_skull
@pytest.mark.parametrize("threshold", (300, "otsu"))
def test_extract_skull_is_the_chain(threshold):
    from ctunet_amd import postprocess, preprocess as pp
    ct = _head()
    assert ct.shape == (40, 48, 56)
    xd = _dev(ct)
    spacing, sigma, rng = (0.8, 0.45, 0.45), 0.5, (-200, 3000)
    got = pp.extract_skull(xd, threshold, spacing=spacing, sigma=sigma, otsu_range=rng if threshold == "otsu" else None,
                           closing_radius=1.0)
    smooth = pp.gaussian_filter(xd, sigma, spacing=spacing)
    t = pp.threshold_otsu(smooth, range=rng) if threshold == "otsu" else threshold
    raw = pp.binarize(smooth, t)
    kept = postprocess.keep_largest_connected_component(raw)
    want = postprocess.ball_closing(kept, 1.0, sampling=spacing)
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    # and the chain against the restated rules as far as they go
    s = R.gaussian_filter(ct, tuple(sigma / q for q in spacing))
    tr = R.otsu(R.histogram(s, 256, rng), rng)[1] if threshold == "otsu" else threshold
    _same_bits(raw, R.binarize(s, tr))
    m = got.cpu().numpy()
    assert int(raw[3, 3, 3]) == 1 and not m[:8, :8, :8].any()                          # the island was there and is gone
    shell = (ct > 700)
    shell[:8, :8, :8] = False
    # the shell is present, the air is not: smoothing by a voxel takes the outermost layer of a shell 3 to 5 voxels thick
    # below either threshold, never more
    assert m[shell].mean() > 0.75 and m[ct < -500].mean() < 0.01
    # the steps can be switched off
    plain = pp.extract_skull(xd, 300, components=0)
    _same_bits(plain, R.binarize(ct, 300))
