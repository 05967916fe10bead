"""The rules of ctunet_amd.preprocess restated in numpy (the module docstring pins them): the Gaussian filter in float32
with every operation rounded on its own, the equal-bin histogram and Otsu's threshold in float64 on exact int64 prefixes,
and the range test.  The device results are compared with these bit for bit."""
import numpy as np

f32 = np.float32


def radius(sigma_vox, truncate=4.0):
    return int(truncate * sigma_vox + 0.5)


def weights(sigma_vox, truncate=4.0):
    r = radius(sigma_vox, truncate)
    if r == 0:
        return np.ones(1, f32)
    k = np.arange(0, r + 1, dtype=np.float64)
    p = np.exp(-0.5 / (np.float64(sigma_vox) * np.float64(sigma_vox)) * k * k)
    return (p / (p[0] + 2.0 * p[1:].sum())).astype(f32)


def _index(i, n, mode):
    if mode == "nearest":
        return np.clip(i, 0, n - 1)
    if mode == "reflect":
        m = np.mod(i, 2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    raise ValueError(mode)


def gauss_axis(v, w, axis, mode, cval):
    """One axis of the filter on a float32 array: acc = w_0 v[i]; acc = acc + w_k (v[i-k] + v[i+k]), k = 1..R."""
    assert v.dtype == f32 and w.dtype == f32
    v = np.moveaxis(v, axis, -1)
    n, r = v.shape[-1], len(w) - 1

    def tap(o):
        i = np.arange(n) + o
        if mode == "constant":
            t = v[..., np.clip(i, 0, n - 1)].copy()
            t[..., (i < 0) | (i >= n)] = f32(cval)
            return t
        return v[..., _index(i, n, mode)]

    acc = (w[0] * tap(0)).astype(f32)
    for k in range(1, r + 1):
        s = (tap(-k) + tap(k)).astype(f32)
        acc = (acc + (w[k] * s).astype(f32)).astype(f32)
    return np.moveaxis(acc, -1, axis)


def gaussian_filter(x, sigma_vox, mode="nearest", cval=0.0, truncate=4.0):
    """x [..., D, H, W] of any of the input dtypes; sigma_vox a (z, y, x) triple in voxels.  Axes go x, y, z."""
    v = x.astype(f32)
    for axis, s in ((-1, sigma_vox[2]), (-2, sigma_vox[1]), (-3, sigma_vox[0])):
        v = gauss_axis(v, weights(s, truncate), axis, mode, cval)
    return v


def finite_range(x):
    v = x.astype(np.float64).ravel()
    v = v[np.isfinite(v)]
    return (np.float64(np.inf), np.float64(-np.inf)) if v.size == 0 else (v.min(), v.max())


def _widen(lo, hi):
    lo, hi = np.float64(lo), np.float64(hi)
    return (lo - 0.5, hi + 0.5) if hi == lo else (lo, hi)


def histogram(x, bins, rng=None):
    lo, hi = _widen(*(finite_range(x) if rng is None else rng))
    v = x.astype(np.float64).ravel()
    with np.errstate(invalid="ignore"):
        v = v[(v >= lo) & (v <= hi)]
        scale = np.float64(bins) / (hi - lo)
    b = np.minimum(np.floor((v - lo) * scale), bins - 1).astype(np.int64)
    return np.bincount(b, minlength=bins).astype(np.int64)


def otsu(h, rng):
    """(k*, threshold) of the int64 counts h taken over rng = (lo, hi)."""
    lo, hi = _widen(*rng)
    h = h.astype(np.int64)
    bins = len(h)
    k = np.arange(bins, dtype=np.int64)
    w1, s1 = np.cumsum(h), np.cumsum(h * k)
    N, S = w1[-1], s1[-1]
    w1, s1 = w1[:-1], s1[:-1]
    w2 = N - w1
    ok = (w1 != 0) & (w2 != 0)
    var = np.zeros(bins - 1, np.float64)
    m1 = s1[ok].astype(np.float64) / w1[ok].astype(np.float64)
    m2 = (S - s1[ok]).astype(np.float64) / w2[ok].astype(np.float64)
    d = m1 - m2
    var[ok] = (w1[ok].astype(np.float64) * w2[ok].astype(np.float64)) * (d * d)
    kk = int(np.argmax(var))                                   # the first maximum
    width = (hi - lo) / np.float64(bins)
    return kk, lo + (np.float64(kk) + 0.5) * width


def binarize(x, lower, upper=None):
    v = x.astype(np.float64)
    upper = np.inf if upper is None else upper
    with np.errstate(invalid="ignore"):
        return ((v > np.float64(lower)) & (v <= np.float64(upper))).astype(np.uint8)


def three_class_volume(n=200000, seed=1):
    """Air, soft tissue and bone in the proportions 5 : 3 : 1, int16 Hounsfield units."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.normal(-1000, 20, n * 5), rng.normal(30, 25, n * 3), rng.normal(900, 300, n)])
    return x.clip(-1024, 3071).round().astype(np.int16)


def synthetic_head(shape=(40, 48, 56), seed=7):
    """A bone shell at 1000 HU around tissue at 40 in air at -1000, Gaussian noise (sd 15) and a stray bone-valued island
    of 5 x 5 x 5 voxels in a corner (large enough to outlast a smoothing of one voxel); int16."""
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    r = np.sqrt(((z - d / 2 + 0.5) / (0.42 * d)) ** 2 + ((y - h / 2 + 0.5) / (0.42 * h)) ** 2
                + ((x - w / 2 + 0.5) / (0.42 * w)) ** 2)
    ct = np.full(shape, -1000.0)
    ct[r <= 1.0] = 40.0
    ct[(r <= 1.0) & (r >= 0.8)] = 1000.0
    ct[1:6, 1:6, 1:6] = 1000.0
    ct += np.random.default_rng(seed).normal(0.0, 15.0, shape)
    return ct.round().astype(np.int16)
