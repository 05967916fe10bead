"""numpy restatement of ctunet_amd.mesh's point-to-mesh distance (host only), shared by test_mesh_distance_cpu.py and
test_mesh_distance_gpu.py; written from the rule in the module docstring and not from the kernel: brute force over all
faces, no grid.  float64 throughout, every operation a numpy operation of its own (numpy never contracts a product and a sum
into an fma); a dot product is (x + y) + z."""
import numpy as np

from mesh_ref import _triple
from mesh_voxelize_ref import centres

F64 = np.float64
CHUNK = 256                                                             # queries per broadcast against all faces


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1],
                     u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def segment(p, u, v):
    """(squared distance, closest point) from p to the segment u-v; t is clamped to [0, 1], a segment of zero length is u."""
    uv, up = v - u, p - u
    length = _dot(uv, uv)
    with np.errstate(all="ignore"):
        t = np.where(length > 0, _dot(up, uv) / np.where(length > 0, length, 1.0), 0.0)
    t = np.where(t >= 0, t, 0.0)
    t = np.where(t <= 1, t, 1.0)
    q = u + t[..., None] * uv
    d = p - q
    return _dot(d, d), q


def face_distance2(p, a, b, c):
    """(squared distance, closest point) from p to the faces (a, b, c); the arrays broadcast against each other."""
    best, q = segment(p, a, b)
    for u, v in ((b, c), (c, a)):
        d, r = segment(p, u, v)
        take = d < best                                                  # the first segment wins a tie
        best, q = np.where(take, d, best), np.where(take[..., None], r, q)
    n = _cross(b - a, c - a)
    nn = _dot(n, n)
    e0 = _dot(_cross(b - a, p - a), n)
    e1 = _dot(_cross(c - b, p - b), n)
    e2 = _dot(_cross(a - c, p - c), n)
    s = _dot(p - a, n)
    safe = np.where(nn > 0, nn, 1.0)
    plane = (s * s) / safe
    take = (nn > 0) & (e0 >= 0) & (e1 >= 0) & (e2 >= 0) & (plane < best)
    foot = p - (s / safe)[..., None] * n
    return np.where(take, plane, best), np.where(take[..., None], foot, q)


def _checked(vertices, faces):
    v32 = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    in_range = ((f >= 0) & (f < len(v32))).all(axis=1)
    finite = np.ones(len(f), dtype=bool)
    finite[in_range] = np.isfinite(v32[f[in_range]]).all(axis=(1, 2))
    if not (in_range & finite).all():
        raise ValueError(f"{int((~(in_range & finite)).sum())} faces hold an index outside [0, V) or a vertex that is not finite")
    return v32.astype(F64), f


def point_distance2(points, vertices, faces, max_distance=None):
    """(squared distances float64 [Q], faces int64 [Q], closest points float64 [Q,3]) of float64 points against the mesh.
    A point that is not finite: NaN, -1, NaN.  No face, or nothing within max_distance: inf, -1, NaN."""
    v, f = _checked(vertices, faces)
    p = np.asarray(points, dtype=F64).reshape(-1, 3)
    d2 = np.full(len(p), np.inf)
    face = np.full(len(p), -1, dtype=np.int64)
    close = np.full((len(p), 3), np.nan)
    ok = np.isfinite(p).all(axis=1)
    d2[~ok] = np.nan
    if len(f):
        a, b, c = (v[f[:, k]][None] for k in range(3))
        for c0 in range(0, len(p), CHUNK):
            rows = np.nonzero(ok[c0:c0 + CHUNK])[0] + c0
            if not len(rows):
                continue
            d, q = face_distance2(p[rows][:, None, :], a, b, c)          # [rows, F], [rows, F, 3]
            k = d.argmin(axis=1)                                         # the lowest index among the minima
            d2[rows], face[rows], close[rows] = d[np.arange(len(rows)), k], k, q[np.arange(len(rows)), k]
    if max_distance is not None:
        far = ok & (d2 > F64(np.float32(max_distance)) * F64(np.float32(max_distance)))
        d2[far], face[far], close[far] = np.inf, -1, np.nan
    return d2, face, close


def point_distance(points, vertices, faces, max_distance=None):
    """(distances float64 [Q] before the rounding to float32, faces, closest points float64) of float32 points."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(F64)
    d2, face, close = point_distance2(p, vertices, faces, max_distance)
    return np.sqrt(d2), face, close


def grid_centres(shape, spacing=None, origin=None):
    """float64 [D*H*W, 3]: the centres of a grid in C order, formed as voxelize forms them."""
    sp, org = _triple(spacing, 1.0), _triple(origin, 0.0)
    axes = [centres(org[a], sp[a], int(n)) for a, n in enumerate(shape)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)


def distance_field(vertices, faces, shape, spacing=None, origin=None, max_distance=None):
    """float64 [D,H,W]: the distances at the grid's centres, max_distance where the rule gives inf."""
    d2, _, _ = point_distance2(grid_centres(shape, spacing, origin), vertices, faces, max_distance)
    d = np.sqrt(d2)
    if max_distance is not None:
        d[np.isinf(d)] = F64(np.float32(max_distance))
    return d.reshape(tuple(int(s) for s in shape))


def tolerance(ref, diag):
    """The bound of the tests: one float32 rounding of the result, and 1e-12 of the scene's diagonal (10^4 times the float64
    disagreement between two formulations of the rule); exactly 0 where the reference is exactly 0."""
    ref = np.asarray(ref, dtype=F64)
    with np.errstate(all="ignore"):
        tol = np.spacing(ref.astype(np.float32)).astype(F64) + 1e-12 * F64(diag)
    return np.where(ref == 0, 0.0, tol)


def diagonal(*arrays):
    """The diagonal of the joint bounding box of the finite rows of the arrays."""
    pts = np.concatenate([np.asarray(a, dtype=F64).reshape(-1, 3) for a in arrays])
    pts = pts[np.isfinite(pts).all(axis=1)]
    return float(np.sqrt(((pts.max(axis=0) - pts.min(axis=0)) ** 2).sum())) if len(pts) else 0.0
