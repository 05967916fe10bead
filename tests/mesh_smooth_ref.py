"""numpy restatement of ctunet_amd.mesh's adjacency and smoothing (host only), shared by test_mesh_smooth_cpu.py and
test_mesh_smooth_gpu.py; written from the rule in the module docstring and not from the kernels."""
import numpy as np

F32 = np.float32


def adjacency(n_vertices, faces):
    """(offsets int32 [V+1], neighbours int32 [E]): per vertex the distinct other vertices it shares a face with, ascending."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    pairs = np.concatenate([f[:, [0, 1]], f[:, [1, 0]], f[:, [1, 2]], f[:, [2, 1]], f[:, [2, 0]], f[:, [0, 2]]])
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    pairs = np.unique(pairs, axis=0) if len(pairs) else pairs            # sorted by (i, j): vertex order, then ascending j
    offsets = np.zeros(n_vertices + 1, dtype=np.int64)
    np.cumsum(np.bincount(pairs[:, 0], minlength=n_vertices), out=offsets[1:])
    return offsets.astype(np.int32), pairs[:, 1].astype(np.int32)


def step(vertices, offsets, neighbours, s, fixed=None):
    """One Jacobi step with factor s: float32, the sum in ascending neighbour order, a true division."""
    v = np.asarray(vertices, dtype=F32)
    off = np.asarray(offsets, dtype=np.int64)
    nb = np.asarray(neighbours, dtype=np.int64)
    deg = np.diff(off)
    acc = np.zeros_like(v)
    for k in range(int(deg.max()) if len(deg) else 0):
        has = (deg > k)[:, None]
        val = v[nb[np.where(deg > k, off[:-1] + k, 0)]] if len(nb) else acc
        # never acc + 0: a padding +0.0 would turn a -0.0 accumulator into +0.0
        acc = np.where(has, val if k == 0 else acc + val, acc)
    move = deg > 0
    if fixed is not None:
        move &= ~np.asarray(fixed).astype(bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = acc / deg.astype(F32)[:, None]
        new = v + F32(s) * (mean - v)
    assert new.dtype == F32
    return np.where(move[:, None], new, v)


def smooth(vertices, faces, iterations=10, lamb=0.5, mu=-0.53, fixed=None):
    v = np.array(vertices, dtype=F32)
    off, nb = adjacency(len(v), faces)
    for _ in range(iterations):
        v = step(v, off, nb, F32(lamb), fixed)
        if mu is not None:
            v = step(v, off, nb, F32(mu), fixed)
    return v
