"""NumPy restatement of the resampling rule that ctunet_amd/resample.py pins: the geometry, the per-axis float64 tables and
the three modes, with every float32 operation of the linear rule rounded on its own (numpy never fuses)."""
import math

import numpy as np


def scales(in_shape, size=None, spacing=None, new_spacing=None):
    """(out_shape, a): size alone a = n / m; spacings a = s_new / s and m = max(1, floor(n s / s_new + 0.5)) unless size."""
    n = tuple(int(v) for v in in_shape)
    if spacing is None:
        m = tuple(int(v) for v in size)
        return m, tuple(nj / mj for nj, mj in zip(n, m))
    s = (float(spacing),) * 3 if np.isscalar(spacing) else tuple(float(v) for v in spacing)
    t = (float(new_spacing),) * 3 if np.isscalar(new_spacing) else tuple(float(v) for v in new_spacing)
    m = tuple(int(v) for v in size) if size is not None else tuple(
        max(1, int(math.floor(nj * sj / tj + 0.5))) for nj, sj, tj in zip(n, s, t))
    return m, tuple(tj / sj for sj, tj in zip(s, t))


def axis_tables(n, m, a):
    """(i0 int32, i1 int32, w float32, near int32, src float64) of one axis with n input and m output voxels."""
    j = np.arange(m, dtype=np.float64)
    src = np.clip((j + 0.5) * np.float64(a) - 0.5, 0.0, np.float64(n - 1))
    i0 = np.minimum(np.floor(src), np.float64(max(n - 2, 0)))
    i1 = np.minimum(i0 + 1, np.float64(n - 1))
    near = np.minimum(np.floor((j + 0.5) * np.float64(a)), np.float64(n - 1))
    return i0.astype(np.int32), i1.astype(np.int32), (src - i0).astype(np.float32), near.astype(np.int32), src


def _grid(tz, ty, tx):
    return tz[:, None, None], ty[None, :, None], tx[None, None, :]


def nearest(x, out_shape, a):
    x = np.asarray(x)
    nz, ny, nx = (axis_tables(n, m, s)[3] for n, m, s in zip(x.shape[-3:], out_shape, a))
    z, y, xx = _grid(nz, ny, nx)
    return x[..., z, y, xx]


def linear(x, out_shape, a, dtype=np.float32, weights=None):
    """lerp(p, q, w) = p + w (q - p) in `dtype`: four lerps along x, two along y, one along z.  `weights`: the three weight
    tables to use in place of the float32 ones (the float64 composite of the tests passes the unrounded src - i0)."""
    x = np.asarray(x).astype(dtype)
    tabs = [axis_tables(n, m, s) for n, m, s in zip(x.shape[-3:], out_shape, a)]
    (z0, y0, x0), (z1, y1, x1) = _grid(*(t[0] for t in tabs)), _grid(*(t[1] for t in tabs))
    wz, wy, wx = _grid(*(t[2].astype(dtype) for t in tabs)) if weights is None else _grid(*(w.astype(dtype) for w in weights))

    def lerp(p, q, w):
        d = (q - p).astype(dtype)
        return (p + (w * d).astype(dtype)).astype(dtype)

    c00 = lerp(x[..., z0, y0, x0], x[..., z0, y0, x1], wx)
    c01 = lerp(x[..., z0, y1, x0], x[..., z0, y1, x1], wx)
    c10 = lerp(x[..., z1, y0, x0], x[..., z1, y0, x1], wx)
    c11 = lerp(x[..., z1, y1, x0], x[..., z1, y1, x1], wx)
    return lerp(lerp(c00, c01, wy), lerp(c10, c11, wy), wz)


def label_scores(x, out_shape, a, num_classes, dtype=np.float32, weights=None):
    """[K, ..., d, h, w]: the linear rule on the indicator x == c of every class."""
    x = np.asarray(x)
    return np.stack([linear(x == c, out_shape, a, dtype, weights) for c in range(num_classes)])


def label_linear(x, out_shape, a, num_classes):
    """The smallest class of the largest score (np.argmax keeps the first maximum), in x's dtype."""
    x = np.asarray(x)
    return np.argmax(label_scores(x, out_shape, a, num_classes), axis=0).astype(x.dtype)


def exact_weights(in_shape, out_shape, a):
    """The unrounded float64 weights src - i0 of the three axes."""
    return [t[4] - t[0] for t in (axis_tables(n, m, s) for n, m, s in zip(in_shape, out_shape, a))]
