"""numpy restatement of ctunet_amd.mesh (host only), shared by test_mesh_cpu.py and test_mesh_gpu.py: marching tetrahedra
on the Kuhn split of the padded grid, welded and closed, written from the rule and not from the kernels.  The winding of
every (tetrahedron, case) comes from the geometry of that tetrahedron (normal . (vertex - inside centroid)), not from a
table; the topology helpers below (edge multiplicities, Euler characteristic) then check it on whole meshes."""
import itertools

import numpy as np

EDGES = np.array([(0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1)])   # owned edges, (dz, dy, dx)
SLOT = {tuple(e): k for k, e in enumerate(EDGES)}
PERMS = list(itertools.permutations((0, 1, 2)))                                                  # lexicographic
F32 = np.float32


def _triple(v, default):
    if v is None:
        return np.full(3, default, dtype=F32)
    a = np.asarray(v, dtype=np.float64)
    return (np.full(3, float(a)) if a.ndim == 0 else a).astype(F32)


def tet_corners(perm):
    """The path c0 .. c3 of one tetrahedron as (dz, dy, dx) rows."""
    c = np.zeros((4, 3), dtype=np.int64)
    for j, axis in enumerate(perm):
        c[j + 1] = c[j]
        c[j + 1, axis] += 1
    return c


def case_triangles(perm, case):
    """The triangles of one (tetrahedron, 4-bit case): a list of three (lo corner, hi corner) edges each, in the rule's
    order, wound by the tetrahedron's own geometry."""
    corners = tet_corners(perm)
    inside = [j for j in range(4) if (case >> j) & 1]
    outside = [j for j in range(4) if not (case >> j) & 1]
    if len(inside) in (0, 4):
        return []
    if len(inside) == 2:
        (i0, i1), (o0, o1) = inside, outside
        a, b, c, d = (i0, o0), (i0, o1), (i1, o1), (i1, o0)
        tris = [(a, b, c), (a, c, d)]
    else:
        lone, rest = (inside[0], outside) if len(inside) == 1 else (outside[0], inside)
        tris = [tuple((lone, o) for o in rest)]
    centroid = corners[inside].mean(axis=0)[::-1]                       # (x, y, z)
    out = []
    for tri in tris:
        edges = [(min(e), max(e)) for e in tri]
        p = [(corners[lo] + corners[hi])[::-1] / 2.0 for lo, hi in edges]
        n = np.cross(p[1] - p[0], p[2] - p[0])
        s = float(np.dot(n, p[0] - centroid))
        assert abs(s) > 1e-9
        if s < 0:
            edges = [edges[0], edges[2], edges[1]]
        out.append([(corners[lo], corners[hi]) for lo, hi in edges])
    return out


def extract(volume, level=0.5, spacing=None, origin=None, label=None, fill_value=None):
    """(vertices float32 [V,3] in (z, y, x), faces int32 [F,3]) of one [D,H,W] volume, in the pinned order."""
    v = np.asarray(volume)
    if v.dtype == np.float32:
        lev = F32(level)
        fill = F32(lev - F32(1)) if fill_value is None else F32(fill_value)
        field = v
    else:
        lev, fill = F32(0.5), F32(0)
        field = ((v == label) if label is not None else (v != 0)).astype(F32)
    assert fill <= lev
    D, H, W = v.shape
    P = np.full((D + 2, H + 2, W + 2), fill, dtype=F32)
    P[1:-1, 1:-1, 1:-1] = field
    ins = P > lev
    Dc, Hc, Wc = D + 1, H + 1, W + 1

    def at(arr, d):
        return arr[d[0]:d[0] + Dc, d[1]:d[1] + Hc, d[2]:d[2] + Wc]

    cross = np.stack([at(ins, (0, 0, 0)) != at(ins, e) for e in EDGES], axis=-1)      # [Dc,Hc,Wc,7]
    vid = (np.cumsum(cross.reshape(-1)) - 1).reshape(cross.shape)
    vid[~cross] = -1
    cz, cy, cx, k = np.nonzero(cross)                                                 # cells in C order, then slots
    d = EDGES[k]
    v0, v1 = P[cz, cy, cx], P[cz + d[:, 0], cy + d[:, 1], cx + d[:, 2]]
    t = ((lev - v0) / (v1 - v0)).astype(F32)
    f = (np.stack([cz, cy, cx], axis=1) - 1).astype(F32) + t[:, None] * d.astype(F32)
    sp, org = _triple(spacing, 1.0), _triple(origin, 0.0)
    verts = (org[None, :] + (f * sp[None, :]).astype(F32)).astype(F32)

    keys, tris = [], []
    for p, perm in enumerate(PERMS):
        corners = tet_corners(perm)
        case = sum(at(ins, corners[j]).astype(np.int64) << j for j in range(4))
        for c in range(1, 15):
            cells = np.argwhere(case == c)
            if not len(cells):
                continue
            lin = (cells[:, 0] * Hc + cells[:, 1]) * Wc + cells[:, 2]
            for j, tri in enumerate(case_triangles(perm, c)):
                ids = []
                for lo, hi in tri:
                    q = cells + lo
                    ids.append(vid[q[:, 0], q[:, 1], q[:, 2], SLOT[tuple(hi - lo)]])
                ids = np.stack(ids, axis=1)
                assert (ids >= 0).all()
                tris.append(ids)
                keys.append(np.stack([lin, np.full_like(lin, p), np.full_like(lin, j)], axis=1))
    if not tris:
        return verts.reshape(-1, 3), np.zeros((0, 3), dtype=np.int32)
    tris, keys = np.concatenate(tris), np.concatenate(keys)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return verts, tris[order].astype(np.int32)


# ---------------------------------------------------------------------------------------------------- helpers
def directed_edge_counts(faces):
    """Multiplicity of every directed edge (a -> b) that occurs in the faces."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    return np.unique(e, axis=0, return_counts=True)[1] if len(e) else np.zeros(0, dtype=np.int64)


def undirected_edge_counts(faces):
    f = np.asarray(faces, dtype=np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)[1] if len(e) else np.zeros(0, dtype=np.int64)


def euler(n_vertices, faces):
    """V - E + F."""
    return int(n_vertices) - len(undirected_edge_counts(faces)) + len(faces)


def is_closed_oriented(faces):
    """Every undirected edge in exactly 2 faces, every directed edge in exactly 1."""
    u, d = undirected_edge_counts(faces), directed_edge_counts(faces)
    return bool((u == 2).all() and (d == 1).all())


def face_geometry(vertices, faces):
    """float64 (cross products [F,3] in (x, y, z), volume terms [F]) of the float32 vertices."""
    p = np.asarray(vertices, dtype=np.float64)[:, ::-1][np.asarray(faces, dtype=np.int64)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return n, np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])) / 6.0


def area_volume(vertices, faces):
    n, terms = face_geometry(vertices, faces)
    return float(0.5 * np.sqrt((n * n).sum(axis=1)).sum()), float(terms.sum())
