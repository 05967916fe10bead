"""ctunet_amd.resample on the GPU: every comparison with the restated rule (tests/resample_ref.py) is bit-equal."""
import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import resample_ref as R

pytestmark = pytest.mark.gpu

# tiles are 4 planes x 4 rows x 16 chunks of 16 output bytes (32 int64 .. 256 uint8 voxels along x)
CASES = {
    "odd": ((7, 9, 11), (13, 8, 20)),
    "unit_axis": ((5, 1, 6), (9, 3, 4)),
    "up_and_down": ((40, 48, 56), (31, 64, 45)),
    "many_tiles": ((70, 70, 130), (33, 150, 67)),                # several tiles a side, odd row lengths
    "gather": ((64, 64, 256), (8, 8, 16)),                       # a factor past any staged box: the direct-gather route
    "wide": ((6, 5, 300), (5, 7, 531)),                          # more than one tile column of uint8 chunks, odd rows
    "identity": ((6, 10, 33), (6, 10, 33)),
}
LEADS = ((), (3,), (2, 2))
NEAREST_DTYPES = (torch.bool, torch.uint8, torch.int16, torch.int32, torch.int64, torch.float32)
LINEAR_DTYPES = (torch.float32, torch.int16, torch.uint8)
LABEL_DTYPES = (torch.bool, torch.uint8, torch.int64)
DEV = "cuda"


def _values(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == torch.float32:
        return torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * 1000)
    if dtype == torch.bool:
        return torch.from_numpy(rng.random(shape) < 0.5)
    lo, hi = {torch.uint8: (0, 256), torch.int16: (-1024, 3072), torch.int32: (-2 ** 31, 2 ** 31),
              torch.int64: (-2 ** 62, 2 ** 62)}[dtype]
    return torch.from_numpy(rng.integers(lo, hi, shape)).to(dtype)


def _labels(shape, dtype, k, seed, stray=False):
    """Random labels below k; with `stray` also values >= k (and negative ones in an int64 map)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, k, shape)
    if stray:
        s = rng.random(shape)
        x[s < 0.15] = k + 1 if dtype != torch.bool else 1
        if dtype == torch.int64:
            x[s > 0.93] = -1
    return torch.from_numpy(x).to(dtype)


def _blob(shape, seed, sigma=2.0):
    g = ndi.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), sigma)
    return g > np.median(g)


def _same_bits(got: torch.Tensor, want: np.ndarray):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), \
        f"{np.count_nonzero(got != want)} of {want.size} voxels differ"


@pytest.mark.parametrize("case", CASES)
def test_nearest_is_the_rule(case):
    from ctunet_amd import resample as rs
    shape, size = CASES[case]
    _, a = R.scales(shape, size)
    for i, dtype in enumerate(NEAREST_DTYPES):
        lead = LEADS[i % 3]
        x = _values(lead + shape, dtype, i)
        got = rs.resample(x.to(DEV), size, mode="nearest")
        assert got.dtype == dtype and tuple(got.shape) == lead + size
        _same_bits(got, R.nearest(x.numpy(), size, a))


@pytest.mark.parametrize("case", CASES)
def test_linear_is_the_rule(case):
    from ctunet_amd import resample as rs
    shape, size = CASES[case]
    _, a = R.scales(shape, size)
    for i, dtype in enumerate(LINEAR_DTYPES):
        for lead in (LEADS if dtype == torch.float32 else LEADS[i:i + 1]):
            x = _values(lead + shape, dtype, 10 + i)
            got = rs.resample(x.to(DEV), size, mode="linear")
            assert got.dtype == torch.float32 and tuple(got.shape) == lead + size
            _same_bits(got, R.linear(x.numpy(), size, a))


@pytest.mark.parametrize("k", (2, 3, 16))
@pytest.mark.parametrize("case", CASES)
def test_label_linear_is_the_rule(case, k):
    from ctunet_amd import resample as rs
    shape, size = CASES[case]
    _, a = R.scales(shape, size)
    for i, dtype in enumerate(LABEL_DTYPES):
        if dtype == torch.bool and k != 2:
            continue
        lead = LEADS[(i + k) % 3]
        for stray in (False, True):
            x = _labels(lead + shape, dtype, k, 20 + i, stray)
            got = rs.resample(x.to(DEV), size, mode="label_linear", num_classes=k)
            assert got.dtype == dtype and tuple(got.shape) == lead + size
            _same_bits(got, R.label_linear(x.numpy(), size, a, k))
    # smooth regions, where most voxels see one class and the rest a border between two
    x = torch.from_numpy(_blob(shape, k).astype(np.uint8) * (k - 1))
    _same_bits(rs.resample(x.to(DEV), size, mode="label_linear", num_classes=k), R.label_linear(x.numpy(), size, a, k))


def test_label_linear_int64_stray_beyond_32_bits():
    """2**32 + 1 is no class; a comparison through a 32-bit cast would read it as label 1."""
    from ctunet_amd import resample as rs
    (shape, size), k = CASES["odd"], 3
    _, a = R.scales(shape, size)
    rng = np.random.default_rng(40)
    x = rng.integers(0, k, shape)
    stray = rng.random(shape) < 0.2
    x[stray] = 2 ** 32 + 1
    want = R.label_linear(x, size, a, k)
    assert np.array_equal(want, R.label_linear(np.where(stray, -1, x), size, a, k))
    assert np.count_nonzero(want != R.label_linear(np.where(stray, 1, x), size, a, k)) > 100      # of 2080
    _same_bits(rs.resample(torch.from_numpy(x).to(DEV), size, mode="label_linear", num_classes=k), want)


def test_spacing_mode_is_the_rule():
    from ctunet_amd import resample as rs
    shape, s, t = (21, 40, 37), (0.8, 0.45, 0.45), (1.0, 0.7, 0.31)
    size, a = R.scales(shape, None, s, t)
    assert size == (17, 26, 54)
    x = _values(shape, torch.int16, 1)
    _same_bits(rs.resample(x.to(DEV), spacing=s, new_spacing=t), R.linear(x.numpy(), size, a))
    _same_bits(rs.resample(x.to(DEV), spacing=s, new_spacing=t, mode="nearest"), R.nearest(x.numpy(), size, a))
    forced, a2 = R.scales(shape, (16, 27, 54), s, t)
    assert a2 == a
    _same_bits(rs.resample(x.to(DEV), (16, 27, 54), spacing=s, new_spacing=t), R.linear(x.numpy(), forced, a))
    r = rs.Resampler(shape, in_spacing=s, out_spacing=t).to(DEV)
    assert r.out_shape == size and r.out_spacing == t
    y = r(x.to(DEV))
    _same_bits(y, R.linear(x.numpy(), size, a))
    back = r.inverse(y)
    assert tuple(back.shape) == shape
    _same_bits(back, R.linear(y.cpu().numpy(), shape, tuple(sj / tj for sj, tj in zip(s, t))))


def test_identities():
    from ctunet_amd import resample as rs
    shape = CASES["identity"][0]
    for dtype in NEAREST_DTYPES:
        x = _values((2,) + shape, dtype, 3).to(DEV)
        assert torch.equal(rs.resample(x, shape, mode="nearest"), x)
    # linear: the last voxel of an axis is lerp(in[n-2], in[n-1], 1) = p + (q - p), which is q for the integer dtypes
    # and for every float32 pair whose difference is exact, not for all of them; everywhere else the weight is 0
    for dtype in LINEAR_DTYPES:
        x = _values(shape, dtype, 4).to(DEV)
        y = rs.resample(x, shape, mode="linear")
        if dtype == torch.float32:
            assert torch.equal(y[:-1, :-1, :-1], x[:-1, :-1, :-1])
            assert torch.equal(rs.resample(x.round(), shape, mode="linear"), x.round())
        else:
            assert torch.equal(y, x.float())
    for dtype in LABEL_DTYPES:
        for k in (2, 3, 16):
            x = _labels(shape, dtype, 2 if dtype == torch.bool else k, 5).to(DEV)
            assert torch.equal(rs.resample(x, shape, mode="label_linear", num_classes=k), x)
    # nearest up by 2 then down by 2
    x = _values((3, 9, 7, 21), torch.int16, 6).to(DEV)
    up = rs.resample(x, (18, 14, 42), mode="nearest")
    assert torch.equal(up[:, ::2, ::2, ::2], x) and torch.equal(up[:, 1::2, 1::2, 1::2], x)
    assert torch.equal(rs.resample(up, (9, 7, 21), mode="nearest"), x)
    # a constant stays the constant: p + w (q - p) with q == p
    for c in (-1234.567, 3.0e38):
        x = torch.full((11, 13, 17), c, dtype=torch.float32, device=DEV)
        for size in ((23, 5, 40), (4, 30, 9)):
            y = rs.resample(x, size)
            assert torch.equal(y, torch.full(size, c, dtype=torch.float32, device=DEV))


def test_out_leaves_its_surroundings_alone_and_calls_repeat():
    from ctunet_amd import resample as rs
    shape, size = CASES["up_and_down"]
    n = size[0] * size[1] * size[2]
    for mode, dtype, k, sentinel in (("linear", torch.int16, None, -7.5), ("nearest", torch.int64, None, -77),
                                     ("label_linear", torch.uint8, 3, 255), ("nearest", torch.uint8, None, 254)):
        x = (_labels(shape, dtype, 3, 1) if k else _values(shape, dtype, 2)).to(DEV)
        first = rs.resample(x, size, mode=mode, num_classes=k)
        assert torch.equal(rs.resample(x, size, mode=mode, num_classes=k), first)          # two calls are bit-equal
        for pad in (1, 3, 16):                                   # out starts at every kind of misalignment
            buf = torch.full((n + 2 * pad,), sentinel, dtype=first.dtype, device=DEV)
            out = buf[pad:pad + n].view(size)
            ret = rs.resample(x, size, mode=mode, num_classes=k, out=out)
            assert ret is out and torch.equal(out, first)
            assert bool((buf[:pad] == sentinel).all()) and bool((buf[pad + n:] == sentinel).all())


def test_captured_call_replays_on_new_input():
    from ctunet_amd import resample as rs
    shape, size = CASES["many_tiles"]
    r = rs.Resampler(shape, size).to(DEV)
    xs = _values((2,) + shape, torch.int16, 1).to(DEV)
    ls = _labels((2,) + size, torch.uint8, 3, 2).to(DEV)
    out = torch.empty((2,) + size, dtype=torch.float32, device=DEV)
    back = torch.empty((2,) + shape, dtype=torch.uint8, device=DEV)

    def run():
        r(xs, out=out)
        r.inverse(ls, mode="label_linear", num_classes=3, out=back)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()                                                     # warm-up: library loaded, tables resident
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    x2, l2 = _values((2,) + shape, torch.int16, 7).to(DEV), _labels((2,) + size, torch.uint8, 3, 8).to(DEV)
    xs.copy_(x2)
    ls.copy_(l2)
    out.zero_()
    back.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, r(x2)) and torch.equal(back, r.inverse(l2, mode="label_linear", num_classes=3))
    _same_bits(out, R.linear(x2.cpu().numpy(), size, r.scale))


def test_round_trip_of_a_blob_beats_nearest():
    """scanner grid -> 1 mm -> scanner grid: label_linear returns in_shape and a higher Dice than nearest on the same map."""
    from ctunet_amd import resample as rs
    shape, s = (40, 88, 88), (0.8, 0.45, 0.45)
    m = torch.from_numpy(_blob(shape, 4, 4.0).astype(np.uint8)).to(DEV)
    r = rs.Resampler(shape, in_spacing=s, out_spacing=1.0).to(DEV)
    assert r.out_shape == (32, 40, 40)

    def dice(p):
        return 2.0 * float((p & m).sum()) / float(p.sum() + m.sum())

    scores = {}
    for mode, k in (("label_linear", 2), ("nearest", None)):
        back = r.inverse(r(m, mode=mode, num_classes=k), mode=mode, num_classes=k)
        assert tuple(back.shape) == shape and back.dtype == torch.uint8
        scores[mode] = dice(back)
    print(scores)
    assert scores["label_linear"] > scores["nearest"]
