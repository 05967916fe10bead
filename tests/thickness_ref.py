"""numpy restatement of the local-thickness rule of ctunet_amd.postprocess (host only, unpruned), shared by
test_thickness_cpu.py and test_thickness_gpu.py.  Written from the definition:

    the centre q covers p  iff  both are foreground and dd(p, q) < D2(q), strictly;
    R2(p) = max {D2(q) : q covers p};  thickness(p) = 2 sqrt(R2(p)) in float32, 0 on background;

with dd the integer dz^2 + dy^2 + dx^2 at unit sampling and otherwise the float32 expression
t_a = float32(k_a) * s_a, dd = (t_z t_z + t_y t_y) + t_x t_x, every product and sum rounded to float32 on its own.
D2 is an argument: 0 on background, int (unit) or float32; INT32_MAX / +inf everywhere in an item without background.
"""
import numpy as np

INT32_MAX = 2 ** 31 - 1


def squared_edt(mask):
    """Exact integer squared distance to the nearest zero voxel (unit sampling) from scipy's transform; the mask needs a
    background voxel."""
    from scipy import ndimage as ndi
    return np.rint(ndi.distance_transform_edt(np.asarray(mask) != 0) ** 2).astype(np.int64)


def r2_map(d2, sampling=None):
    """max {D2(q) : q covers p} for every voxel: every foreground q paints max(out, D2(q)) into the foreground voxels of its
    window with dd < D2(q).  Unit sampling (None): integers; otherwise float32."""
    d2 = np.asarray(d2)
    unit = sampling is None
    shape = d2.shape
    fg = d2 > 0
    if unit:
        d2 = d2.astype(np.int64)
        out = np.zeros(shape, np.int64)
        if fg.any() and d2[fg].max() >= INT32_MAX:
            out[fg] = INT32_MAX
            return out
        s = np.ones(3)
    else:
        assert d2.dtype == np.float32
        out = np.zeros(shape, np.float32)
        if fg.any() and np.isinf(d2[fg]).any():
            out[fg] = np.inf
            return out
        s32 = np.asarray(sampling, dtype=np.float32)
        assert s32.shape == (3,)
        s = s32.astype(np.float64)
    for z, y, x in zip(*np.nonzero(fg)):
        b = d2[z, y, x]
        r = np.sqrt(float(b))
        lo, hi, k2 = [], [], []
        for a, c in enumerate((z, y, x)):
            w = int(r / s[a]) + 1                                   # |k_a| s_a <= |p - q| < r, with room for rounding
            l, h = max(c - w, 0), min(c + w + 1, shape[a])
            k = np.arange(l, h) - c
            if unit:
                k2.append(k * k)
            else:
                t = k.astype(np.float32) * s32[a]
                k2.append(t * t)
            lo.append(l)
            hi.append(h)
        dd = (k2[0][:, None, None] + k2[1][None, :, None]) + k2[2][None, None, :]
        win = (slice(lo[0], hi[0]), slice(lo[1], hi[1]), slice(lo[2], hi[2]))
        cover = (dd < b) & fg[win]
        o = out[win]
        o[cover & (o < b)] = b
    return out


def local_thickness(d2, sampling=None):
    """float32 thickness map from the squared distance map."""
    r2 = r2_map(d2, sampling)
    if sampling is None:
        t = np.where(r2 >= INT32_MAX, np.float32(np.inf), np.sqrt(r2.astype(np.float32)))
    else:
        t = np.sqrt(r2)
    return (np.float32(2) * t.astype(np.float32)).astype(np.float32)


def summary(t, min_thickness=None):
    """(count, min, max, mean, below) of one item's thickness map in float64, as thickness_summary defines them."""
    t = np.asarray(t, dtype=np.float32)
    f = t[t > 0]
    if f.size == 0:
        return np.array([0.0, np.inf, 0.0, np.nan, 0.0])
    below = 0 if min_thickness is None else int((f < np.float32(min_thickness)).sum())
    with np.errstate(invalid="ignore"):
        mean = f.astype(np.float64).mean()
    return np.array([float(f.size), float(f.min()), float(f.max()), mean, float(below)])
