"""The rank filters of ctunet_amd.preprocess restated in numpy: the key, the padding per mode, a stable argsort of the keys,
the rank-th element with its own bits; and scipy's rank arithmetic for the median, a percentile and a negative rank."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

PAD_MODE = {"nearest": "edge", "reflect": "symmetric", "constant": "constant"}


def key(x: np.ndarray) -> np.ndarray:
    """The unsigned key of every element: order-preserving, a bijection on the bits."""
    if x.dtype == np.uint8:
        return x.astype(np.uint32)
    if x.dtype == np.int16:
        return (x.astype(np.int32) + 32768).astype(np.uint32)
    assert x.dtype == np.float32, x.dtype
    b = np.ascontiguousarray(x).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def sizes(size):
    return (size,) * 3 if np.isscalar(size) else tuple(size)


def median_rank(n: int) -> int:
    return n // 2


def percentile_rank(p, n: int) -> int:
    if p < 0.0:
        p += 100
    assert 0 <= p <= 100
    return n - 1 if p == 100 else int(float(n) * p / 100.0)


def signed_rank(rank: int, n: int) -> int:
    assert -n <= rank < n
    return rank + n if rank < 0 else rank


def rank_filters(x: np.ndarray, ranks, size=3, mode="nearest", cval=0) -> list:
    """For every 0-based rank of ``ranks`` (not negative): the element of that rank of the box ``size`` around every voxel
    of ``x [..., D, H, W]``.  One sort serves all the ranks."""
    sz = sizes(size)
    n = sz[0] * sz[1] * sz[2]
    assert all(0 <= r < n for r in ranks) and all(s % 2 == 1 for s in sz)
    lead = x.ndim - 3
    pad = [(0, 0)] * lead + [(s // 2, s // 2) for s in sz]
    kw = {"constant_values": np.asarray(cval).astype(x.dtype)} if mode == "constant" else {}
    p = np.pad(x, pad, mode=PAD_MODE[mode], **kw)
    win = sliding_window_view(p, sz, axis=(-3, -2, -1)).reshape(x.shape + (n,))
    order = np.argsort(key(win), axis=-1, kind="stable")
    return [np.ascontiguousarray(np.take_along_axis(win, order[..., r:r + 1], axis=-1)[..., 0]) for r in ranks]


def rank_filter(x: np.ndarray, rank: int, size=3, mode="nearest", cval=0) -> np.ndarray:
    return rank_filters(x, (rank,), size, mode, cval)[0]


def median_filter(x, size=3, mode="nearest", cval=0):
    sz = sizes(size)
    return rank_filter(x, median_rank(sz[0] * sz[1] * sz[2]), sz, mode, cval)


def percentile_filter(x, p, size=3, mode="nearest", cval=0):
    sz = sizes(size)
    return rank_filter(x, percentile_rank(p, sz[0] * sz[1] * sz[2]), sz, mode, cval)


def specials() -> np.ndarray:
    """A float32 [4, 5, 6] volume of -0.0, +0.0, +-inf, denormals, NaNs of both signs and ordinary repeated values."""
    bits = np.array([0x80000000, 0x00000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001, 0x007fffff, 0x7fc00000,
                     0xffc00000, 0x7fffffff, 0xff800001, 0x3f800000, 0xbf800000, 0x3f800000, 0x40000000, 0xc0000000],
                    np.uint32)
    rng = np.random.default_rng(11)
    return bits[rng.integers(0, bits.size, (4, 5, 6))].view(np.float32)


def shell_with_flips(shape=(24, 40, 40), p=0.02, seed=5):
    """A 0 / 1 ellipsoid shell, and the same with isolated salt-and-pepper flips (each voxel with probability ``p``)."""
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    r = np.sqrt(((z - d / 2 + 0.5) / (0.45 * d)) ** 2 + ((y - h / 2 + 0.5) / (0.45 * h)) ** 2
                + ((x - w / 2 + 0.5) / (0.45 * w)) ** 2)
    clean = ((r <= 1.0) & (r >= 0.7)).astype(np.uint8)
    flips = np.random.default_rng(seed).random(shape) < p
    return clean, (clean ^ flips.astype(np.uint8))


def synthetic_head(shape=(24, 32, 40), seed=7):
    """A bone shell at 1000 HU around tissue at 40 in air at -1000 with Gaussian noise (sd 15) and single bright specks; int16."""
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    r = np.sqrt(((z - d / 2 + 0.5) / (0.42 * d)) ** 2 + ((y - h / 2 + 0.5) / (0.42 * h)) ** 2
                + ((x - w / 2 + 0.5) / (0.42 * w)) ** 2)
    ct = np.full(shape, -1000.0)
    ct[r <= 1.0] = 40.0
    ct[(r <= 1.0) & (r >= 0.75)] = 1000.0
    rng = np.random.default_rng(seed)
    ct += rng.normal(0.0, 15.0, shape)
    ct[rng.random(shape) < 0.01] = 3000.0
    return ct.round().astype(np.int16)
