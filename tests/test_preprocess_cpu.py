"""ctunet_amd.preprocess without a GPU: the restated rules (tests/preprocess_ref.py) against scipy and numpy, Otsu's documented
cases, the C-ABI entry points in the ctypes table and the built library, and argument validation, which must raise before
anything is launched."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import preprocess_ref as R

SHAPES = ((5, 7, 19), (17, 33, 70), (3, 4, 5), (2, 9, 40, 130))
SIGMAS = ((0.8, 1.3, 2.9), (0.0, 0.5, 7.9), (2.0, 2.0, 2.0))
MODES = ("nearest", "reflect", "constant")
NEW_SYMBOLS = {"ctu_gaussian_ws_bytes": 5, "ctu_gaussian_filter": 13, "ctu_minmax_ws_bytes": 1, "ctu_finite_minmax": 6,
               "ctu_histogram": 9, "ctu_threshold_otsu": 8, "ctu_binarize": 9}


def _values(shape, dt, rng):
    if dt == "i2":
        return rng.integers(-1024, 3072, shape).astype(np.int16)
    if dt == "u1":
        return rng.integers(0, 256, shape).astype(np.uint8)
    return (rng.standard_normal(shape) * 1000).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES)
def test_gaussian_rule_is_scipys_filter(shape):
    """scipy sums each axis in float64 and stores float32 once per axis; the rule rounds each of its 3 R + 1 operations of
    an axis, but the weights fall off so that over every element |rule - scipy| <= (R_max + 3) 2^-24 max(max|x|, |cval|)."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for sig in SIGMAS:
        for mode in MODES:
            for dt in ("i2", "f4", "u1"):
                x = _values(shape, dt, rng)
                cval = -1000.0 if mode == "constant" else 0.0
                got = R.gaussian_filter(x, sig, mode, cval)
                assert got.dtype == np.float32 and got.shape == x.shape
                lead = (0.0,) * (x.ndim - 3)
                want = ndi.gaussian_filter(x.astype(np.float64), lead + sig, mode=mode, cval=cval)
                rmax = max(R.radius(s) for s in sig)
                bound = (rmax + 3) * 2.0 ** -24 * max(np.abs(x.astype(np.float64)).max(), abs(cval))
                err = np.abs(got.astype(np.float64) - want).max()
                worst = max(worst, err / bound)
                assert err <= bound, (shape, sig, mode, dt, err, bound)
    print(f"{shape}: worst |rule - scipy| / bound = {worst:.3f}")


def test_gaussian_weights_and_radius():
    from ctunet_amd import preprocess as pp
    for s in (0.0, 0.1, 0.5, 1.0 / 0.45, 1.25, 7.9, 8.1):
        w = pp.gaussian_weights(s)
        assert w.dtype == np.float32 and np.array_equal(w.view(np.int32), R.weights(s).view(np.int32))
        assert len(w) == int(4.0 * s + 0.5) + 1
        assert abs(float(w[0]) + 2.0 * float(w[1:].astype(np.float64).sum()) - 1.0) < 1e-6
    assert np.array_equal(pp.gaussian_weights(0.0), np.ones(1, np.float32))
    assert R.radius(7.9) == 32 and R.radius(0.5) == 2


@pytest.mark.parametrize("bins", (256, 4096))
def test_histogram_rule_is_numpys(bins):
    x = R.three_class_volume(20000)
    assert x.min() < -1000 and x.max() > 1500
    h = R.histogram(x, bins, (-1024, 3072))                    # (hi - lo) / bins is a power of two: no edge lies between two
    want, _ = np.histogram(x, bins=bins, range=(-1024, 3072))  # roundings of the two formulas
    assert h.dtype == np.int64 and np.array_equal(h, want) and h.sum() == x.size
    part = R.histogram(x, bins, (-200, 3000))
    assert part.sum() == np.count_nonzero((x >= -200) & (x <= 3000))
    full = R.histogram(x, bins)
    assert full.sum() == x.size and full[-1] >= 1              # v == hi lands in the last bin


def test_otsu_separates_tissue_from_bone():
    x = R.three_class_volume()
    k, t = R.otsu(R.histogram(x, 256, (-200, 3000)), (-200, 3000))
    assert 30.0 < t < 900.0 and t == -200.0 + (k + 0.5) * 12.5
    assert abs(t - 494.0) < 12.5                               # the figure the module docstring quotes
    k, t = R.otsu(R.histogram(x, 256, (-1024, 3072)), (-1024, 3072))
    assert -1000.0 < t < 30.0 and t == -904.0                  # the full range separates air from the head


def test_otsu_documented_indices():
    const = np.full(1000, 37, np.int16)
    k, t = R.otsu(R.histogram(const, 256), R.finite_range(const))
    assert k == 0 and t == 36.5 + 0.5 / 256                     # every variance is 0: the first bin; the range widened by 0.5
    assert R.histogram(const, 256)[128] == 1000
    two = np.where(np.arange(1000) % 3 == 0, 100, -50).astype(np.int16)
    h = R.histogram(two, 64, (-100, 156))
    lower_bin = int(np.flatnonzero(h)[0])
    k, t = R.otsu(h, (-100, 156))
    # the variance is the same from the lower value's bin up to the bin before the upper one's: the first of them, whose
    # centre is the threshold
    assert np.count_nonzero(h) == 2 and k == lower_bin == 12 and t == -100 + 12.5 * 4.0
    assert np.array_equal(R.binarize(two, t), (two == 100).astype(np.uint8))
    assert R.otsu(np.zeros(16, np.int64), (0, 1))[0] == 0


def test_new_entry_points_are_bound_and_exported():
    import ctunet_amd
    from ctunet_amd import _lib
    assert "preprocess" in ctunet_amd.__all__ and ctunet_amd.preprocess.__name__ == "ctunet_amd.preprocess"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, arity in NEW_SYMBOLS.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == arity, name
        assert hasattr(lib, name), name
    loaded = _lib.load()
    assert loaded.ctu_abi_version() == 8 == _lib.ABI_VERSION
    # geometry queries run without a GPU: the intermediate is one float per voxel, its plane rounded up to 4 floats
    assert loaded.ctu_gaussian_ws_bytes(1, 224, 512, 512, 5) == 224 * 512 * 512 * 4
    assert loaded.ctu_gaussian_ws_bytes(2, 3, 5, 7, 1) == 1024              # 2 * 3 * 36 * 4 = 864, rounded up to 256
    assert loaded.ctu_gaussian_ws_bytes(1, 224, 512, 512, 0) == 0           # no z pass, no workspace
    assert loaded.ctu_gaussian_ws_bytes(1, 224, 512, 1025, 5) == 0
    assert loaded.ctu_minmax_ws_bytes(1) > 0 and loaded.ctu_minmax_ws_bytes(0) == 0


def test_bad_arguments_raise_before_any_launch():
    from ctunet_amd import preprocess as pp
    x = torch.zeros((4, 5, 6), dtype=torch.int16)
    bad_gauss = (
        dict(sigma=8.2),                                        # R = 33
        dict(sigma=(1.0, 1.0, 3.7), spacing=(1.0, 1.0, 0.45)),  # 8.2 voxels along x
        dict(sigma=1.0, truncate=40.0),
        dict(sigma=-1.0), dict(sigma=(1.0, 2.0)), dict(sigma=float("nan")),
        dict(sigma=1.0, spacing=(1.0, 0.0, 1.0)),
        dict(sigma=1.0, mode="mirror"), dict(sigma=1.0, mode="constant", cval=float("inf")),
        dict(sigma=1.0, out=torch.zeros((4, 5, 12), dtype=torch.float32)[:, :, ::2]),
        dict(sigma=1.0, out=torch.zeros((4, 5, 6), dtype=torch.float64)),
    )
    for kw in bad_gauss:
        with pytest.raises(ValueError):
            pp.gaussian_filter(x, **kw)
    with pytest.raises(ValueError):
        pp.gaussian_filter(torch.zeros((1, 2, 1025), dtype=torch.uint8), 1.0)
    with pytest.raises(ValueError):
        pp.gaussian_filter(torch.zeros((5, 6)), 1.0)
    for dtype in (torch.float64, torch.int32, torch.int64, torch.bool, torch.float16):
        bad = torch.zeros((4, 5, 6), dtype=dtype)
        for call in (lambda: pp.gaussian_filter(bad, 1.0), lambda: pp.histogram(bad), lambda: pp.threshold_otsu(bad),
                     lambda: pp.binarize(bad, 0), lambda: pp.extract_skull(bad, 300)):
            with pytest.raises(ValueError):
                call()
    for bins in (1, 0, 4097, 2.5, True):
        with pytest.raises(ValueError):
            pp.histogram(x, bins=bins)
        with pytest.raises(ValueError):
            pp.threshold_otsu(x, bins=bins)
    for rng in ((3, 1), (0, float("inf")), (1,), "full", torch.zeros(2), torch.zeros(3, dtype=torch.float64)):
        with pytest.raises(ValueError):
            pp.histogram(x, range=rng)
    with pytest.raises(ValueError):
        pp.histogram(x, out=torch.zeros(512, dtype=torch.int64)[::2])
    with pytest.raises(ValueError):
        pp.threshold_otsu()
    with pytest.raises(ValueError):
        pp.threshold_otsu(x, hist=torch.zeros(256, dtype=torch.int64))
    with pytest.raises(ValueError):
        pp.threshold_otsu(hist=torch.zeros(256, dtype=torch.int64))                    # no range
    with pytest.raises(ValueError):
        pp.threshold_otsu(hist=torch.zeros(256, dtype=torch.int32), range=(0, 1))
    for lower, upper in (("a", None), (float("nan"), None), (0, torch.zeros(())), (torch.zeros(2, dtype=torch.float64), None)):
        with pytest.raises(ValueError):
            pp.binarize(x, lower, upper)
    with pytest.raises(ValueError):
        pp.binarize(x, 0, out=torch.zeros((4, 5, 12), dtype=torch.uint8)[:, :, ::2])
    bad_skull = (dict(threshold="otsu"), dict(threshold="li", otsu_range=(-200, 3000)), dict(threshold=None),
                 dict(threshold="otsu", otsu_range=(5, 1)), dict(threshold=300, components=9),
                 dict(threshold=300, components=-1), dict(threshold=300, closing_radius=-1.0),
                 dict(threshold=300, sigma=-0.5), dict(threshold=300, spacing=(1.0, 1.0)))
    for kw in bad_skull:
        with pytest.raises(ValueError):
            pp.extract_skull(x, **kw)
    with pytest.raises(ValueError):
        pp.extract_skull(torch.zeros((1, 1, 4, 5, 6), dtype=torch.int16), 300)
    with pytest.raises(TypeError):
        pp.extract_skull(x)                                     # threshold has no default
    # valid arguments on a host tensor: refused for the device, still a ValueError, still nothing launched
    for call in (lambda: pp.gaussian_filter(x, 1.0), lambda: pp.histogram(x, range=(0, 1)), lambda: pp.histogram(x),
                 lambda: pp.threshold_otsu(x), lambda: pp.binarize(x, 0), lambda: pp.extract_skull(x, 300)):
        with pytest.raises(ValueError, match="GPU"):
            call()
