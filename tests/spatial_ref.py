"""NumPy restatement of the random spatial augmentation (ctunet_amd/transforms.py pins the rule under "RandomSpatial"):
the Philox draws (one sample at a time and a whole batch at once, two code paths that must agree bit for bit), the control
grid, the matrix M, the cubic B-spline displacement and the per-voxel rule, every float64 operation in the pinned order."""
from dataclasses import dataclass
from typing import Tuple

import numpy as np

from augment_ref import philox_seq, unif

RAD = 0.017453292519943295
F = np.float64


@dataclass
class Config:
    """RandomSpatial's parameters, triples spelled out."""
    flip_axes: Tuple[int, ...] = (0,)
    flip_p: float = 0.5
    scales: Tuple[float, float] = (0.9, 1.1)
    degrees: Tuple[float, float, float] = (15.0, 15.0, 15.0)
    translation: Tuple[float, float, float] = (10.0, 10.0, 15.0)
    affine_p: float = 0.5
    num_control_points: Tuple[int, int, int] = (7, 7, 7)
    max_displacement: Tuple[float, float, float] = (7.5, 7.5, 7.5)
    locked_borders: int = 2
    elastic_p: float = 0.5
    spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0)

    @classmethod
    def of(cls, t):
        """The Config of a transforms.RandomSpatial instance."""
        return cls(t.flip_axes, t.flip_p, t.scales, t.degrees, t.translation, t.affine_p, t.num_control_points,
                   t.max_displacement, t.locked_borders, t.elastic_p, t.spacing)


def _u(r):
    return unif(r).astype(F)                    # (r >> 8) 2^-24, exact


def _sym(r, a):
    return (F(2.0) * _u(r) - F(1.0)) * F(a)


# ------------------------------------------------------------------------------------------------------------- the draws
def scalars(cfg: Config, seed: int, seq: int):
    """Stream 0 of sample number seq: dict(flip, affine, elastic, scales, degrees, translation), Python scalars."""
    r = [philox_seq(c0, 0, seq, seed) for c0 in range(4)]
    flip = tuple(bool(a in cfg.flip_axes and _u(r[0][a]) < F(cfg.flip_p)) for a in range(3))
    lo, hi = F(cfg.scales[0]), F(cfg.scales[1])
    return dict(flip=flip, affine=bool(_u(r[0][3]) < F(cfg.affine_p)), elastic=bool(_u(r[1][0]) < F(cfg.elastic_p)),
                scales=tuple(float(lo + _u(r[1][1 + a]) * (hi - lo)) for a in range(3)),
                degrees=tuple(float(_sym(r[2][a], cfg.degrees[a])) for a in range(3)),
                translation=tuple(float(_sym(r[3][a], cfg.translation[a])) for a in range(3)))


def scalars_batch(cfg: Config, seed: int, seq0: int, n: int):
    """The same for samples seq0 .. seq0 + n - 1 in one vectorised Philox call: dict of arrays with leading axis n."""
    seq = (np.arange(n, dtype=np.int64) + np.int64(seq0))[:, None]
    w = philox_seq(np.arange(4, dtype=np.uint32)[None, :], 0, seq, seed)        # 4 words, each [n, c0]
    u = np.stack([_u(x) for x in w], -1)                                         # [n, c0, word]
    allowed = np.array([a in cfg.flip_axes for a in range(3)])
    lo, hi = F(cfg.scales[0]), F(cfg.scales[1])
    two_u = F(2.0) * u - F(1.0)
    return dict(flip=allowed[None, :] & (u[:, 0, :3] < F(cfg.flip_p)), affine=u[:, 0, 3] < F(cfg.affine_p),
                elastic=u[:, 1, 0] < F(cfg.elastic_p), scales=lo + u[:, 1, 1:4] * (hi - lo),
                degrees=two_u[:, 2, :3] * np.asarray(cfg.degrees, F)[None, :],
                translation=two_u[:, 3, :3] * np.asarray(cfg.translation, F)[None, :])


def _free(cfg: Config):
    g, lb = cfg.num_control_points, cfg.locked_borders
    ax = [(np.arange(v) >= lb) & (np.arange(v) < v - lb) for v in g]
    return ax[0][:, None, None] & ax[1][None, :, None] & ax[2][None, None, :]


def control(cfg: Config, seed: int, seq: int):
    """Stream 1 of sample seq, point by point: float64 [3, Gz, Gy, Gx] (mm), the locked layers 0."""
    gz, gy, gx = cfg.num_control_points
    lb = cfg.locked_borders
    phi = np.zeros((3, gz, gy, gx), F)
    for iz in range(lb, gz - lb):
        for iy in range(lb, gy - lb):
            for ix in range(lb, gx - lb):
                r = philox_seq((iz * gy + iy) * gx + ix, 1, seq, seed)
                for c in range(3):
                    phi[c, iz, iy, ix] = _sym(r[c], cfg.max_displacement[c])
    return phi


def control_batch(cfg: Config, seed: int, seq0: int, n: int):
    """The same for n samples at once: float64 [n, 3, Gz, Gy, Gx]."""
    g = cfg.num_control_points
    c0 = np.arange(g[0] * g[1] * g[2], dtype=np.uint32)[None, :]
    seq = (np.arange(n, dtype=np.int64) + np.int64(seq0))[:, None]
    w = philox_seq(c0, 1, seq, seed)
    phi = np.stack([_sym(w[c], cfg.max_displacement[c]) for c in range(3)], 1).reshape((n, 3) + tuple(g))
    return np.where(_free(cfg)[None, None], phi, F(0.0))


# ---------------------------------------------------------------------------------------------------------------- matrix
def matrix(shape, spacing, scales, degrees, translation):
    """NumPy's [L | c - L c + t] from angles in degrees (about z, y, x), float64 [3, 4]: the yardstick for the recorded M."""
    (cz, cy, cx), (sz, sy, sx) = [np.cos(F(d) * F(RAD)) for d in degrees], [np.sin(F(d) * F(RAD)) for d in degrees]
    rz = np.array([[1, 0, 0], [0, cz, -sz], [0, sz, cz]], F)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], F)
    rx = np.array([[cx, -sx, 0], [sx, cx, 0], [0, 0, 1]], F)
    L = rz @ ry @ rx @ np.diag(np.asarray(scales, F))
    c = (np.asarray(shape, F) - 1) / 2 * np.asarray(spacing, F)
    return np.concatenate([L, (c - L @ c + np.asarray(translation, F))[:, None]], 1)


def matrix_bound(shape, spacing, translation):
    """16 2^-52 (1 + max|c_a| + max|t_a|): a few ulp of sin / cos carried through the products."""
    c = (np.asarray(shape, F) - 1) / 2 * np.asarray(spacing, F)
    return 16 * 2.0 ** -52 * (1 + np.abs(c).max() + np.abs(np.asarray(translation, F)).max())


IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)


# ------------------------------------------------------------------------------------------------------------ the B-spline
def bspline(f):
    """The four uniform cubic B-spline weights of the fraction f, in the pinned order of operations."""
    f = np.asarray(f, F)
    h, f2 = F(1.0) - f, f * f
    f3 = f2 * f
    return [((h * h) * h) / F(6.0), ((F(3.0) * f3 - F(6.0) * f2) + F(4.0)) / F(6.0),
            ((((F(-3.0) * f3) + F(3.0) * f2) + F(3.0) * f) + F(1.0)) / F(6.0), f3 / F(6.0)]


def knot(s, n, sp, G):
    """(i, f, g) of world coordinate s along an axis of n voxels of spacing sp with G control points."""
    m = G - 3
    with np.errstate(invalid="ignore", over="ignore"):
        g = (np.asarray(s, F) / (F(n) * F(sp))) * F(m)
        g = np.where(g >= 0.0, g, F(0.0))                     # NaN -> 0
        g = np.where(g <= F(m), g, F(m))
    i = np.minimum(np.floor(g), m - 1).astype(np.int64)
    return i, g - i.astype(F), g


def displacement(s, shape, spacing, phi):
    """e(s) float64 [3, ...] for world points s [3, ...] and a control grid phi [3, Gz, Gy, Gx]: 64 terms, x innermost."""
    G = phi.shape[1:]
    idx, B = [], []
    for a in range(3):
        i, f, _ = knot(s[a], shape[a], spacing[a], G[a])
        idx.append(i)
        B.append(bspline(f))
    e = [np.zeros(np.shape(s[0]), F) for _ in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(4):
            for m in range(4):
                wzy = B[0][l] * B[1][m]
                for n in range(4):
                    wt = wzy * B[2][n]
                    for c in range(3):
                        e[c] = e[c] + wt * phi[c][idx[0] + l, idx[1] + m, idx[2] + n]
    return np.stack(e)


# ---------------------------------------------------------------------------------------------------------- the voxel rule
def coords(shape, spacing, M, phi=None, flip=(False, False, False)):
    """u float64 [3, D, H, W]: the input voxel coordinates every output voxel samples (steps 1-5 up to the rounding)."""
    sp = [F(v) for v in spacing]
    M = np.asarray(M, F)
    o = np.indices(shape).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        w = [o[a] * sp[a] for a in range(3)]
        q = [((M[a, 0] * w[0] + M[a, 1] * w[1]) + M[a, 2] * w[2]) + M[a, 3] for a in range(3)]
        if phi is not None:
            e = displacement(q, shape, spacing, np.asarray(phi, F))
            q = [q[a] + e[a] for a in range(3)]
        for a in range(3):
            if flip[a]:
                q[a] = (F(shape[a] - 1) * sp[a]) - q[a]
        return np.stack([q[a] / sp[a] for a in range(3)])


def sample(x, u):
    """x [..., D, H, W] sampled at u [3, d, h, w]: nearest (floor(u + 0.5)), 0 outside and where u is not finite."""
    n = x.shape[-3:]
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.floor(u + F(0.5))
        inside = np.ones(u.shape[1:], bool)
        for a in range(3):
            inside &= (k[a] >= 0.0) & (k[a] < F(n[a]))
    ki = np.where(inside[None], k, 0.0).astype(np.int64)
    return np.where(inside, x[..., ki[0], ki[1], ki[2]], x.dtype.type(0))


def expected(x, cfg: Config, rec, phi):
    """The warp of one sample x [C, D, H, W] from its record (a transforms.last_params entry, or scalars() plus a
    "matrix") and its control grid phi [3, Gz, Gy, Gx]."""
    shape = x.shape[-3:]
    return sample(x, coords(shape, cfg.spacing, np.asarray(rec["matrix"], F), phi if rec["elastic"] else None, rec["flip"]))
