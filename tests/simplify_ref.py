"""numpy restatement of ctunet_amd.simplify.decimate (vertex clustering on a uniform grid; the rule is pinned in the module's
docstring).  Written from the rule, not from the kernel: float64 on the float32 inputs widened, every operation rounded on
its own, the sums with np.add.at on int64, and no dense table of cells (a tiny cell_size works on the host)."""
import numpy as np

F64 = np.float64
MAX_CELLS = 1 << 28


def _cell_size(cell_size):
    c = np.asarray(cell_size, dtype=np.float32).reshape(-1)
    c = np.repeat(c, 3) if len(c) == 1 else c
    assert c.shape == (3,) and np.isfinite(c).all() and (c > 0).all(), cell_size
    return c.astype(F64)


def refused(vertices, faces):
    """The number of faces with an index outside [0, V) or a vertex that is not finite (never read through)."""
    v, f = np.asarray(vertices, dtype=np.float32), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    bad = ((f < 0) | (f >= len(v))).any(axis=1)
    ok = np.flatnonzero(~bad)
    bad[ok] = ~np.isfinite(v[f[ok]]).all(axis=(1, 2))
    return int(bad.sum())


def _empty(V):
    return np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32), np.full(V, -1, dtype=np.int32)


def grid(vertices, faces, cell_size):
    """(members, lo, hi, n): the sorted members, their box in float64 and the cells per axis as Python ints."""
    v, f = np.asarray(vertices, dtype=np.float32), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    cell = _cell_size(cell_size)
    members = np.unique(f)
    p = v[members].astype(F64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    n = [int(x) for x in np.floor((hi - lo) / cell) + 1.0]
    return members, lo, hi, n


def survivors(g, cancel=True):
    """bool [F]: the faces that survive steps 3 and 4 of the rule; ``g`` int64 [F,3] holds the cell ids of their corners."""
    keep = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 2] != g[:, 0])
    if not cancel or not keep.any():
        return keep
    idx = np.flatnonzero(keep)                                          # ascending input index
    k = g[idx]
    r = np.argmin(k, axis=1)
    rows = np.arange(len(k))
    s, x, y = k[rows, r], k[rows, (r + 1) % 3], k[rows, (r + 2) % 3]
    positive = x < y
    key = np.stack([s, np.minimum(x, y), np.maximum(x, y)], axis=1)
    group = np.unique(key, axis=0, return_inverse=True)[1].reshape(-1)
    p = np.bincount(group, weights=positive).astype(np.int64)[group]
    q = np.bincount(group, weights=~positive).astype(np.int64)[group]
    # the rank of a face among those of its key and orientation with a lower input index
    run = group * 2 + positive
    order = np.argsort(run, kind="stable")
    sorted_run = run[order]
    first = np.flatnonzero(np.r_[True, sorted_run[1:] != sorted_run[:-1]])
    start = np.repeat(first, np.diff(np.r_[first, len(order)]))
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order)) - start
    alive = np.where(positive, (p > q) & (rank < p - q), (q > p) & (rank < q - p))
    out = np.zeros(len(g), dtype=bool)
    out[idx[alive]] = True
    return out


def decimate(vertices, faces, cell_size, cancel=True, max_cells=MAX_CELLS):
    """(vertices float32 [V',3], faces int32 [F',3], map int32 [V]) by the rule; ValueError for refused input or too many
    cells (``max_cells=None``: any number, which the host can afford since it keeps no table of cells)."""
    v, f = np.asarray(vertices, dtype=np.float32), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(v)
    cell = _cell_size(cell_size)
    bad = refused(v, f)
    if bad:
        raise ValueError(f"{bad} of {len(f)} faces are refused")
    if len(f) == 0:
        return _empty(V)
    members, lo, hi, n = grid(v, f, cell_size)
    if max_cells is not None and n[0] * n[1] * n[2] > max_cells:
        raise ValueError(f"{n} cells exceed {max_cells}")
    p = v[members].astype(F64)
    top = np.array([x - 1 for x in n], dtype=F64)
    c = np.minimum(top, np.floor((p - lo) / cell)).astype(np.int64)
    cid = (c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2]
    vcell = np.full(V, -1, dtype=np.int64)
    vcell[members] = cid
    alive = survivors(vcell[f], cancel)
    if not alive.any():
        return _empty(V)
    kept = vcell[f[alive]]
    used = np.unique(kept)                                              # ascending cell id
    out_faces = np.searchsorted(used, kept).astype(np.int32)
    # positions: integer sums of the members' quantised offsets
    ext = float((hi - lo).max())
    e = int(np.frexp(ext)[1])
    S = float(np.ldexp(1.0, 30 - e))
    pos = np.searchsorted(used, cid)
    hit = used[np.minimum(pos, len(used) - 1)] == cid
    q = np.rint((p[hit] - lo) * S).astype(np.int64)
    sums = np.zeros((len(used), 3), dtype=np.int64)
    count = np.zeros(len(used), dtype=np.int64)
    np.add.at(sums, pos[hit], q)
    np.add.at(count, pos[hit], 1)
    out_vertices = (lo + (sums.astype(F64) / count.astype(F64)[:, None]) / S).astype(np.float32)
    vmap = np.full(V, -1, dtype=np.int32)
    vmap[members[hit]] = pos[hit]
    return out_vertices, out_faces, vmap


def edges_balanced(faces):
    """Invariant (a): every directed edge (a -> b) occurs as often as (b -> a)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if not len(f):
        return True
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    top = int(e.max()) + 1
    fwd, n_fwd = np.unique(e[:, 0] * top + e[:, 1], return_counts=True)
    back, n_back = np.unique(e[:, 1] * top + e[:, 0], return_counts=True)
    return bool(np.array_equal(fwd, back) and np.array_equal(n_fwd, n_back))
