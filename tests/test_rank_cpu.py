"""The rank filters of ctunet_amd.preprocess without a GPU: the restated rule (tests/rank_ref.py) against scipy.ndimage, the
total order on float32 specials, the rank arithmetic, argument validation (which must raise from the Python layer before
anything is launched) and the refusals of the C entry point."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import rank_ref as R

SHAPES = ((5, 7, 9), (2, 3, 4), (1, 1, 6), (9, 17, 33))
SIZES = ((3, 3, 3), (5, 5, 5), (1, 3, 7), (7, 1, 3))
MODES = ("nearest", "reflect", "constant")
PERCENTILES = (0, 10, 25, 50, 90, 100, -20)


def _inputs(shape, rng):
    yield (rng.random(shape) < 0.4).astype(np.uint8), 1
    yield rng.integers(-1024, 3072, shape).astype(np.int16), -1000
    yield rng.integers(-6, 7, shape).astype(np.float32) * np.float32(0.75), -1.5      # repeated values


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.dtype == np.float32:
        assert not np.isnan(want).any() and (got == want).all()
    else:
        assert np.array_equal(got, want)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", MODES)
def test_restatement_is_scipys_filter(shape, mode):
    rng = np.random.default_rng(3)
    for x, cval in _inputs(shape, rng):
        for size in SIZES:
            n = size[0] * size[1] * size[2]
            kw = dict(size=size, mode=mode, cval=cval)
            _same(R.median_filter(x, size, mode, cval), ndi.median_filter(x, **kw))
            for p in PERCENTILES:
                _same(R.percentile_filter(x, p, size, mode, cval), ndi.percentile_filter(x, p, **kw))
            for r in (1, -2):
                _same(R.rank_filter(x, R.signed_rank(r, n), size, mode, cval), ndi.rank_filter(x, r, **kw))
            _same(R.rank_filter(x, 0, size, mode, cval), ndi.minimum_filter(x, **kw))
            _same(R.rank_filter(x, n - 1, size, mode, cval), ndi.maximum_filter(x, **kw))


def test_key_order_on_float32_specials():
    ordered = np.array([0xffc00000, 0xff800001, 0xff800000, 0xc0000000, 0x80000001, 0x80000000, 0x00000000, 0x00000001,
                        0x007fffff, 0x3f800000, 0x7f800000, 0x7fc00000, 0x7fffffff], np.uint32).view(np.float32)
    k = R.key(ordered)
    assert (np.diff(k.astype(np.int64)) > 0).all()                  # -NaNs < -inf < .. < -0 < +0 < .. < +inf < +NaNs
    assert len(np.unique(R.key(np.arange(-32768, 32768).astype(np.int16)))) == 65536
    x = R.specials()
    assert np.isnan(x).any() and np.isinf(x).any() and (x.view(np.uint32) == 0x80000000).any()
    for size, mode in (((3, 3, 3), "nearest"), ((1, 3, 3), "reflect"), ((3, 1, 5), "constant")):
        n = size[0] * size[1] * size[2]
        clean = ndi.maximum_filter(np.isnan(x).astype(np.uint8), size=size, mode=mode, cval=0) == 0
        assert clean.any()
        for rank in (0, n // 2, n - 1, 1):
            got = R.rank_filter(x, rank, size, mode, 2.0)
            # the output is an element of the window with its own bits
            assert np.isin(got.view(np.uint32), np.append(x.view(np.uint32), np.float32(2.0).view(np.uint32))).all()
            want = ndi.rank_filter(x, rank, size=size, mode=mode, cval=2.0)
            assert (got[clean] == want[clean]).all()                # by value: -0.0 == +0.0


def test_percentile_rank_is_scipys():
    from ctunet_amd import preprocess as pp
    ns = sorted({a * b * c for a in (1, 3, 5, 7) for b in (1, 3, 5, 7) for c in (1, 3, 5, 7)})
    for n in ns:
        for p in (-100, -20, 0, 0.1, 25, 50, 99.9, 100):
            q = p + 100 if p < 0 else p
            want = n - 1 if q == 100 else int(float(n) * q / 100.0)
            assert pp.percentile_rank(p, n) == want == R.percentile_rank(p, n), (n, p)
    for bad in (101, -100.5, float("nan"), "50", True):
        with pytest.raises(ValueError):
            pp.percentile_rank(bad, 27)
    assert pp.path_of(3, 13) == "fast3" and pp.path_of(3, 0) == pp.path_of((5, 1, 7), 34) == "separable"
    assert pp.path_of((3, 3, 5), 22) == pp.path_of(5, 62) == "generic"
    assert set(pp.TILE) == {"fast3", "separable", "generic"}


def test_bad_arguments_raise_from_python(monkeypatch):
    from ctunet_amd import _lib, preprocess as pp

    def no_launch(*a, **k):
        raise AssertionError("validation must come before the library is touched")
    monkeypatch.setattr(_lib, "on", no_launch)
    x = torch.zeros(4, 5, 6, dtype=torch.int16)
    filters = (pp.median_filter, pp.minimum_filter, pp.maximum_filter, lambda *a, **k: pp.percentile_filter(a[0], 50, *a[1:], **k),
               lambda *a, **k: pp.rank_filter(a[0], 1, *a[1:], **k))
    for f in filters:
        for size in (2, 9, 0, -3, (3, 3), (3, 4, 3), (3, 3, 9), 3.0, np.ones((3, 3, 3)), True, None):
            with pytest.raises(ValueError):
                f(x, size)
        for kw in (dict(mode="wrap"), dict(mode=None), dict(cval=1.5), dict(cval=40000), dict(cval=float("nan")),
                   dict(cval="0")):
            with pytest.raises(ValueError):
                f(x, 3, **kw)
        with pytest.raises(ValueError):
            f(x.to(torch.int64), 3)
        with pytest.raises(ValueError):
            f(x[0], 3)
        with pytest.raises(ValueError):
            f(torch.zeros(1, 1025, 2, dtype=torch.uint8), 3)
        with pytest.raises(ValueError):
            f(x, 3, out=torch.zeros(4, 5, 6, dtype=torch.float32))
        with pytest.raises(ValueError):
            f(x, 3, out=torch.zeros(4, 5, 7, dtype=torch.int16))
        with pytest.raises(ValueError, match="shares memory"):
            f(x, 3, out=x)
        with pytest.raises(ValueError, match="no CPU fallback"):
            f(x, 3)
    with pytest.raises(ValueError):
        pp.median_filter(torch.zeros(4, 5, 6, dtype=torch.uint8), 3, mode="constant", cval=-1)
    with pytest.raises(ValueError):
        pp.median_filter(torch.zeros(4, 5, 6), 3, mode="constant", cval=1e39)
    with pytest.raises(ValueError):
        pp.median_filter(torch.zeros(4, 5, 6), 3, mode="constant", cval=float("inf"))
    for p in (101, -101, float("nan"), None):
        with pytest.raises(ValueError):
            pp.percentile_filter(x, p, 3)
    for r in (27, -28, 1.0, None):
        with pytest.raises(ValueError):
            pp.rank_filter(x, r, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        pp.rank_filter(x, -27, 3)
    for m in (2, 9, (3, 3), -1, 1.0):
        with pytest.raises(ValueError):
            pp.extract_skull(x, 300, median=m)
    with pytest.raises(ValueError, match="no CPU fallback"):
        pp.extract_skull(x, 300, median=3)
    with pytest.raises(ValueError, match="extract_skull.*no CPU fallback"):
        pp.extract_skull(x, 300, median=0)


def test_c_entry_refuses_without_launching():
    from ctunet_amd import _lib
    lib = _lib.load()
    assert len(_lib.SIGNATURES["ctu_rank_filter"][1]) == 13 and len(_lib.SIGNATURES["ctu_rank_filter_ws_bytes"][1]) == 5
    size = lambda *s: (ctypes.c_int * 3)(*s)
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below is refused before a launch
    call = lambda inp=fake, dtype=5, N=1, shape=(4, 5, 6), sz=size(3, 3, 3), rank=13, mode=0, cval=0.0, out=fake: \
        lib.ctu_rank_filter(inp, dtype, N, *shape, sz, rank, mode, cval, out, None, None)
    assert lib.ctu_rank_filter_ws_bytes(1, 4, 5, 6, size(3, 3, 3)) == 0
    assert call(inp=None) == -1 and b"null" in lib.ctu_last_error()
    assert call(out=None) == -1 and call(sz=None) == -1
    assert call(sz=size(3, 2, 3)) == -1 and b"odd" in lib.ctu_last_error()
    assert call(sz=size(9, 3, 3)) == -1 and call(sz=size(3, 3, 0)) == -1
    assert call(rank=27) == -1 and b"rank" in lib.ctu_last_error()
    assert call(rank=-1) == -1
    assert call(dtype=4) == -1 and call(mode=3) == -1 and call(mode=-1) == -1
    assert call(shape=(4, 1025, 6)) == -1 and call(shape=(0, 5, 6)) == -1 and call(N=0) == -1
    assert call(cval=0.5) == -1 and call(cval=32768.0) == -1 and call(dtype=3, cval=-1.0) == -1
    assert call(dtype=0, cval=float("inf")) == -1 and call(dtype=0, cval=1e39) == -1
