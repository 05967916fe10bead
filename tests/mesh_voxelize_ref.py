"""numpy restatement of ctunet_amd.mesh's voxelisation (host only), shared by test_mesh_voxelize_cpu.py and
test_mesh_voxelize_gpu.py; written from the rule in the module docstring and not from the kernel.  float64 throughout, every
operation a numpy operation of its own (numpy never contracts a product and a sum into an fma)."""
import numpy as np

from mesh_ref import _triple

F64 = np.float64
CHUNK = 2048                                                            # faces per broadcast against the rows of the grid


def centres(origin_a, spacing_a, n):
    """The float64 centres of one axis: double(origin) + k * double(spacing), the product and the sum rounded separately."""
    return F64(origin_a) + np.arange(n, dtype=F64) * F64(spacing_a)


def _tie_sign(e, d_y, d_z):
    """sign(E) as if the ray were shifted by (+eps, +eps^2) in (z, y): E, else -(b_y - a_y), else (b_z - a_z)."""
    s = np.sign(e)
    s = np.where(s == 0, np.sign(-d_y), s)
    return np.where(s == 0, np.sign(d_z), s)


def winding_number(vertices, faces, shape, spacing=None, origin=None):
    """int32 [D,H,W]: the winding number of the mesh around every voxel centre, by the module docstring's rule."""
    v32 = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    D, H, W = (int(s) for s in shape)
    sp, org = _triple(spacing, 1.0), _triple(origin, 0.0)                # rounded to float32 once
    zs, ys, xs = (centres(org[a], sp[a], n) for a, n in enumerate((D, H, W)))
    in_range = ((f >= 0) & (f < len(v32))).all(axis=1)
    finite = np.ones(len(f), dtype=bool)
    finite[in_range] = np.isfinite(v32[f[in_range]]).all(axis=(1, 2))
    if not (in_range & finite).all():
        raise ValueError(f"{int((~(in_range & finite)).sum())} faces hold an index outside [0, V) or a vertex that is not finite")
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]   # a repeated index: nothing
    v = v32.astype(F64)
    delta = np.zeros((D, H, W + 1), dtype=np.int64)                      # column W collects the crossings that are dropped
    pz, py = zs[None, :, None], ys[None, None, :]
    for c0 in range(0, len(f), CHUNK):
        idx = f[c0:c0 + CHUNK]
        P = v[idx]                                                       # [n, corner, (z, y, x)]
        col = lambda a: a[:, None, None]
        box = ((col(P[:, :, 0].min(axis=1)) <= pz) & (pz <= col(P[:, :, 0].max(axis=1)))
               & (col(P[:, :, 1].min(axis=1)) <= py) & (py <= col(P[:, :, 1].max(axis=1))))
        signs = []
        for q in range(3):
            r = (q + 1) % 3
            forward = idx[:, q] < idx[:, r]                              # the endpoint of lower vertex index comes first
            a = np.where(forward[:, None], P[:, q], P[:, r])
            b = np.where(forward[:, None], P[:, r], P[:, q])
            d_z, d_y = col(b[:, 0] - a[:, 0]), col(b[:, 1] - a[:, 1])
            e = d_z * (py - col(a[:, 1])) - d_y * (pz - col(a[:, 0]))
            s = _tie_sign(e, d_y, d_z)
            signs.append(np.where(col(forward), s, -s))
        e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        area = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]                  # the projection's doubled area, positive: entering
        n_z = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        n_y = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        hit = box & (signs[0] != 0) & (signs[0] == signs[1]) & (signs[1] == signs[2]) & col(area != 0)
        with np.errstate(all="ignore"):
            num = col(n_z) * (pz - col(P[:, 0, 0])) + col(n_y) * (py - col(P[:, 0, 1]))
            x_c = col(P[:, 0, 2]) - num / col(area)
        n, i, j = np.nonzero(hit)
        k = np.searchsorted(xs, x_c[n, i, j], side="right")              # the first centre with x_k > x_c (NaN: none)
        np.add.at(delta, (i, j, k), signs[0][n, i, j].astype(np.int64))
    out = np.cumsum(delta[:, :, :W], axis=2)
    assert np.abs(out).max(initial=0) < 1 << 31
    return out.astype(np.int32)


def voxelize(vertices, faces, shape, spacing=None, origin=None):
    return (winding_number(vertices, faces, shape, spacing, origin) != 0).astype(np.uint8)


def cube_mesh(lo=0.5, hi=4.5):
    """The 12-triangle cube with corners at lo and hi on every axis, wound outward (right-handed in (x, y, z)); vertex
    index = 4 z + 2 y + x with z, y, x in {0, 1}.  (vertices float32 [8,3] in (z, y, x), faces int32 [12,3])."""
    v = np.array([[z, y, x] for z in (lo, hi) for y in (lo, hi) for x in (lo, hi)], dtype=np.float32)
    quads = [(0, 4, 6, 2), (1, 3, 7, 5),                                 # x = lo, x = hi
             (0, 2, 3, 1), (4, 5, 7, 6),                                 # z = lo, z = hi
             (0, 1, 5, 4), (2, 6, 7, 3)]                                 # y = lo, y = hi
    f = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.array(f, dtype=np.int32)
