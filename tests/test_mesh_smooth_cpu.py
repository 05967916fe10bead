"""Host-side checks of ctunet_amd.mesh's adjacency and smoothing: the numpy restatement (tests/mesh_smooth_ref.py) pinned on
facts that do not depend on it (degree sums, directed face edges, symmetry, hand-built meshes, volume / area / roughness of
the smoothed sphere), argument validation before anything is launched, the new C-ABI symbols and their workspace sizes."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_ref as R
import mesh_smooth_ref as S
from test_mesh_cpu import sphere_mask, torus_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ctu_mesh_adjacency_ws_bytes", "ctu_mesh_adjacency_build", "ctu_mesh_adjacency_emit", "ctu_mesh_smooth_ws_bytes",
           "ctu_mesh_smooth")
CENTRE = np.array([9.3, 10.6, 11.2])                                # of sphere_mask(), (z, y, x)


# ------------------------------------------------------------------------------------------------ hand-built meshes
def strip_mesh(n=7):
    """An open strip of 2n vertices in two rows: quads (i, i+1, n+i+1, n+i) split along (i+1, n+i)."""
    v = np.array([[0.0, r, 0.37 * i + 0.1 * r * i] for r in range(2) for i in range(n)], dtype=np.float32)
    f = [t for i in range(n - 1) for t in ((i, i + 1, n + i), (i + 1, n + i + 1, n + i))]
    return v, np.array(f, dtype=np.int32)


def cone_mesh(n=300):
    """n rim vertices and an apex (index n) of valence n; open at the base."""
    a = 2.0 * np.pi * np.arange(n) / n
    v = np.concatenate([np.stack([np.zeros(n), np.sin(a), np.cos(a)], axis=1), [[1.5, 0.0, 0.0]]]).astype(np.float32)
    f = np.array([(n, i, (i + 1) % n) for i in range(n)], dtype=np.int32)
    return v, f


def odd_mesh():
    """A duplicate face, the same face wound the other way, a [1, 1, 2] face, a [3, 3, 3] face and vertex 5 in no face."""
    v = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [-0.0, 2, -3], [7, 8, 9]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 1, 2], [2, 1, 0], [1, 1, 2], [3, 3, 3], [2, 4, 3]], dtype=np.int32)
    return v, f


ODD_NEIGHBOURS = [[1, 2], [0, 2], [0, 1, 3, 4], [2, 4], [2, 3], []]
HAND = {"strip": strip_mesh, "cone": cone_mesh, "odd": odd_mesh}


def neighbour_sets(n_vertices, faces):
    """The rule by set arithmetic, face by face."""
    sets = [set() for _ in range(n_vertices)]
    for a, b, c in np.asarray(faces).tolist():
        for x, y in ((a, b), (b, c), (c, a)):
            if x != y:
                sets[x].add(y)
                sets[y].add(x)
    return sets


def lists_of(offsets, neighbours):
    return [neighbours[offsets[i]:offsets[i + 1]].tolist() for i in range(len(offsets) - 1)]


@pytest.fixture(scope="module")
def meshes():
    return {"sphere": R.extract(sphere_mask()), "torus": R.extract(torus_mask()),
            "voxel": R.extract(np.ones((1, 1, 1), dtype=np.uint8))}


# ------------------------------------------------------------------------------------------------ the reference, pinned
@pytest.mark.parametrize("name,lo,hi", [("sphere", 4, 10), ("torus", 4, 10), ("voxel", 4, 6)])
def test_reference_adjacency_of_closed_meshes(meshes, name, lo, hi):
    v, f = meshes[name]
    off, nb = S.adjacency(len(v), f)
    assert off.dtype == np.int32 and nb.dtype == np.int32 and off.shape == (len(v) + 1,) and off[0] == 0
    deg = np.diff(off)
    assert deg.sum() == len(nb) == 3 * len(f)
    assert deg.min() >= lo and deg.max() <= hi
    # a closed oriented manifold: the table is the set of directed face edges
    src = np.repeat(np.arange(len(v)), deg)
    table = set(zip(src.tolist(), nb.tolist()))
    edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    assert table == set(map(tuple, edges.tolist())) and len(table) == len(nb)
    assert table == {(j, i) for i, j in table}                          # symmetric
    assert all(a < b for i in range(len(v)) for a, b in zip(nb[off[i]:off[i + 1] - 1], nb[off[i] + 1:off[i + 1]]))


@pytest.mark.parametrize("name", sorted(HAND))
def test_reference_adjacency_of_hand_built_meshes(name):
    v, f = HAND[name]()
    off, nb = S.adjacency(len(v), f)
    got = lists_of(off, nb)
    assert got == [sorted(s) for s in neighbour_sets(len(v), f)]
    if name == "odd":
        assert got == ODD_NEIGHBOURS
    if name == "cone":
        n = len(v) - 1
        assert got[n] == list(range(n)) and got[0] == [1, n - 1, n] and got[5] == [4, 6, n]
    if name == "strip":
        n = len(v) // 2
        assert got[0] == [1, n] and got[1] == [0, 2, n, n + 1] and got[n - 1] == [n - 2, 2 * n - 2, 2 * n - 1]
        assert got[2 * n - 1] == [n - 1, 2 * n - 2]
    e, fe = S.adjacency(0, np.zeros((0, 3), dtype=np.int32))
    assert e.tolist() == [0] and fe.shape == (0,)


def test_reference_step_by_hand():
    """One vertex of the odd mesh worked out operation by operation."""
    v, f = odd_mesh()
    off, nb = S.adjacency(len(v), f)
    out = S.step(v, off, nb, np.float32(0.5))
    acc = v[0].copy()                                                   # vertex 2: neighbours 0, 1, 3, 4
    for j in (1, 3, 4):
        acc = acc + v[j]
    want = v[2] + np.float32(0.5) * (acc / np.float32(4) - v[2])
    assert np.array_equal(out[2].view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert np.array_equal(out[5].view(np.uint32), v[5].view(np.uint32))  # no neighbours: the bits stay


def test_smoothing_figures_on_the_sphere_mask(meshes):
    """Taubin keeps the volume and removes the staircase; Laplacian shrinks (figures of the rule at iterations = 10)."""
    v, f = meshes["sphere"]
    area0, vol0 = R.area_volume(v, f)
    rad = lambda p: np.linalg.norm(p.astype(np.float64) - CENTRE, axis=1)
    t = S.smooth(v, f, 10)
    lap = S.smooth(v, f, 10, mu=None)
    assert t.dtype == np.float32 and t.shape == v.shape
    area_t, vol_t = R.area_volume(t, f)
    assert abs(vol_t / vol0 - 1.0) < 0.01                               # measured 1.0030
    assert R.area_volume(lap, f)[1] / vol0 < 0.96                       # measured 0.950
    assert area_t / area0 < 0.90                                        # measured 0.8525
    assert rad(v).std() == pytest.approx(0.278, abs=0.002) and rad(t).std() < 0.21      # measured 0.198
    assert np.linalg.norm(t.astype(np.float64) - v, axis=1).max() < 0.6  # measured 0.475
    assert R.euler(len(t), f) == R.euler(len(v), f) == 2
    assert np.array_equal(S.smooth(v, f, 0).view(np.uint32), v.view(np.uint32))


def test_fixed_vertices_keep_their_bits_and_still_pull(meshes):
    v, f = meshes["sphere"]
    fixed = np.random.default_rng(7).random(len(v)) < 0.3
    a, b = S.smooth(v, f, 3, fixed=fixed), S.smooth(v, f, 3)
    assert np.array_equal(a[fixed].view(np.uint32), v[fixed].view(np.uint32))
    # their free neighbours still move (a vertex stays only where the mean of its neighbours is the vertex itself, which the
    # lattice's symmetry allows at a few spots of a sphere)
    off, nb = S.adjacency(len(v), f)
    beside = np.zeros(len(v), dtype=bool)
    beside[np.repeat(np.arange(len(v)), np.diff(off))[fixed[nb]]] = True
    beside &= ~fixed
    assert beside.sum() > 1000 and (a[beside] != v[beside]).any(axis=1).mean() > 0.9
    assert (a[~fixed] != b[~fixed]).any()                               # the fixed ones entered their neighbours' sums
    assert np.array_equal(S.smooth(v, f, 3, fixed=fixed.astype(np.uint8)), a)


# ------------------------------------------------------------------------------------------------ the module's host side
def test_symbols_in_header_table_and_library():
    from ctunet_amd import _lib, mesh
    header = open(os.path.join(ROOT, "include", "ctunet_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.load().ctu_abi_version() == _lib.ABI_VERSION == 8
    assert mesh.ADJ_SCAN_CHUNK == int(re.search(r"#define CTU_MESH_ADJ_SCAN_CHUNK (\d+)", header).group(1))
    assert mesh.MAX_ITERATIONS == int(re.search(r"#define CTU_MESH_SMOOTH_MAX_ITERATIONS (\d+)", header).group(1)) == 10000
    assert mesh.Adjacency._fields == ("offsets", "neighbours")


def test_workspace_bytes_and_limits():
    from ctunet_amd import _lib, mesh
    lib = _lib.load()
    a256 = lambda n: -(-n // 256) * 256
    fmax = ((1 << 31) - 1) // 6
    for V, F in ((0, 0), (1, 0), (14, 24), (2766, 5528), (4096, 1), (4097, 1), (134748, 285704), ((1 << 31) - 1, fmax)):
        adj = 256 + 2 * a256(4 * V) + a256(8 * -(-V // mesh.ADJ_SCAN_CHUNK)) + a256(24 * F)
        assert lib.ctu_mesh_adjacency_ws_bytes(V, F) == adj
        assert lib.ctu_mesh_smooth_ws_bytes(V) == 2 * a256(16 * V)
        assert mesh.smooth_workspace_bytes(V, F) == adj + 2 * a256(16 * V) + 4 * (V + 1) + 24 * F
    for V, F in ((1 << 31, 1), (-1, 1), (4, -1), (4, fmax + 1), (4, 1 << 62)):
        assert lib.ctu_mesh_adjacency_ws_bytes(V, F) == 0
        with pytest.raises(ValueError, match="2\\^31"):
            mesh.smooth_workspace_bytes(V, F)
    assert lib.ctu_mesh_smooth_ws_bytes(1 << 31) == 0 and lib.ctu_mesh_smooth_ws_bytes(-1) == 0
    for bad in ((4.0, 1), (True, 1), ("4", 1)):
        with pytest.raises(ValueError):
            mesh.smooth_workspace_bytes(*bad)


def test_c_entry_points_refuse_bad_arguments():
    """CTU_REQUIRE fires before any launch, so these calls need no GPU; the message comes through ctu_last_error."""
    from ctunet_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    fmax = ((1 << 31) - 1) // 6

    def err(status):
        assert status == -1
        return lib.ctu_last_error().decode()

    build, emit, smooth = lib.ctu_mesh_adjacency_build, lib.ctu_mesh_adjacency_emit, lib.ctu_mesh_smooth
    assert "null" in err(build(None, 4, 2, p, p, None))
    assert "null" in err(build(p, 4, 2, None, p, None))
    assert "null" in err(build(p, 4, 2, p, None, None))
    assert "2^31" in err(build(p, 1 << 31, 2, p, p, None))
    assert "2^31" in err(build(p, 4, fmax + 1, p, p, None))
    assert "2^31" in err(build(p, -1, 2, p, p, None))
    assert "without vertices" in err(build(p, 0, 2, p, p, None))
    assert "aligned" in err(build(p, 4, 2, p, p + 4, None))
    assert build(None, 0, 0, None, None, None) == 0 and build(None, 4, 0, None, None, None) == 0      # empty: nothing to launch
    assert "2^31" in err(emit(1 << 31, 2, 6, p, p, p, None))
    assert "2^31" in err(emit(4, fmax + 1, 6, p, p, p, None))
    assert "total" in err(emit(4, 2, 13, p, p, p, None))
    assert "total" in err(emit(4, 2, -1, p, p, p, None))
    assert "null" in err(emit(4, 2, 6, None, p, p, None))
    assert "null" in err(emit(4, 2, 6, p, None, p, None))
    assert "aligned" in err(emit(4, 2, 6, p, p, p + 8, None))
    assert emit(4, 2, 0, None, None, None, None) == 0 and emit(0, 0, 0, None, None, None, None) == 0

    def sm(vert=p, V=4, off=p, nb=p, E=6, fixed=None, it=10, lam=0.5, has_mu=1, mu=-0.53, out=p, ws=p):
        return smooth(vert, V, off, nb, E, fixed, it, lam, has_mu, mu, out, ws, None)

    assert "2^31" in err(sm(V=1 << 31))
    assert "2^31" in err(sm(E=1 << 31))
    assert "2^31" in err(sm(V=-1))
    assert "iterations" in err(sm(it=-1))
    assert "iterations" in err(sm(it=10001))
    for lam in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        assert "lambda" in err(sm(lam=lam))
    for mu in (-0.5, -0.25, 0.0, 0.6, float("nan"), float("-inf")):
        assert "mu" in err(sm(mu=mu))
    assert "null" in err(sm(vert=None))
    assert "null" in err(sm(out=None))
    assert "null" in err(sm(off=None))
    assert "null" in err(sm(ws=None))
    assert "neighbours" in err(sm(nb=None))
    assert "aligned" in err(sm(ws=p + 4))
    assert sm(vert=None, V=0, off=None, nb=None, E=0, out=None, ws=None) == 0                          # empty: nothing to launch
    assert "mu" not in err(sm(has_mu=0, mu=float("nan"), out=None))                                   # mu is not read without has_mu


def test_argument_validation_raises_before_any_launch():
    from ctunet_amd import mesh
    v, f = (torch.from_numpy(a) for a in odd_mesh())
    m = mesh.Mesh(v, f)
    V = v.shape[0]
    adj = mesh.Adjacency(torch.zeros(V + 1, dtype=torch.int32), torch.zeros(4, dtype=torch.int32))
    bad = [
        (dict(iterations=-1), "iterations"), (dict(iterations=10001), "iterations"), (dict(iterations=2.0), "iterations"),
        (dict(iterations=True), "iterations"), (dict(iterations=None), "iterations"),
        (dict(lamb=0), "lamb"), (dict(lamb=-0.5), "lamb"), (dict(lamb=1.5), "lamb"), (dict(lamb=float("nan")), "lamb"),
        (dict(lamb="a"), "lamb"), (dict(lamb=True), "lamb"), (dict(lamb=1e-60), "lamb"),
        (dict(mu=-0.5), "mu"), (dict(mu=0.53), "mu"), (dict(mu=0.0), "mu"), (dict(mu=float("-inf")), "mu"),
        (dict(mu=float("nan")), "mu"), (dict(mu=-1e39), "mu"), (dict(mu="a"), "mu"), (dict(lamb=0.6, mu=-0.53), "mu"),
        (dict(mu=-0.5 - 1e-12), "mu"),                                       # equal to -lamb once rounded to float32
        (dict(fixed=np.zeros(V, dtype=bool)), "fixed"), (dict(fixed=torch.zeros(V + 1, dtype=torch.bool)), "fixed"),
        (dict(fixed=torch.zeros(V, 1, dtype=torch.bool)), "fixed"), (dict(fixed=torch.zeros(V, dtype=torch.int32)), "fixed"),
        (dict(fixed=torch.zeros(V)), "fixed"), (dict(fixed=torch.zeros(V, dtype=torch.bool, device="meta")), "device"),
        (dict(adjacency=(adj.offsets,)), "Adjacency"), (dict(adjacency="a"), "Adjacency"),
        (dict(adjacency=(adj.offsets.long(), adj.neighbours)), "int32"),
        (dict(adjacency=(adj.offsets, adj.neighbours.long())), "int32"),
        (dict(adjacency=(adj.offsets[:-1], adj.neighbours)), "V \\+ 1"),
        (dict(adjacency=(torch.zeros(V + 2, dtype=torch.int32), adj.neighbours)), "V \\+ 1"),
        (dict(adjacency=(adj.offsets.view(1, -1), adj.neighbours)), "int32 vectors"),
        (dict(adjacency=(adj.offsets.to("meta"), adj.neighbours)), "device"),
    ]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            mesh.smooth(m, **kw)
    for kw in ({}, dict(mu=None), dict(iterations=0), dict(fixed=torch.zeros(V, dtype=torch.uint8)), dict(adjacency=adj),
               dict(lamb=1.0, mu=-1.01)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            mesh.smooth(m, **kw)
    with pytest.raises(ValueError, match="no CPU fallback"):
        mesh.adjacency(m)
    for fn in (mesh.smooth, mesh.adjacency):
        for broken in ((v, f.long()), (v.double(), f), (v[:, :2], f), (torch.zeros(0, 3), f), "mesh"):
            with pytest.raises(ValueError):
                fn(broken)
        # the limits, on tensors without storage: V < 2^31 and 6F < 2^31
        big_v = mesh.Mesh(torch.empty((1 << 31, 3), device="meta"), torch.empty((1, 3), dtype=torch.int32, device="meta"))
        big_f = mesh.Mesh(torch.empty((4, 3), device="meta"), torch.empty(((1 << 31) // 6 + 1, 3), dtype=torch.int32, device="meta"))
        for big in (big_v, big_f):
            with pytest.raises(ValueError, match="2\\^31"):
                fn(big)


def test_documents_no_longer_list_smoothing_as_out_of_scope():
    from ctunet_amd import mesh
    assert "Out of scope: decimation, formats other than binary STL, marching cubes." in mesh.__doc__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Mesh smoothing" in design and not re.search(r"Out of scope:\s*smoothing", design)
