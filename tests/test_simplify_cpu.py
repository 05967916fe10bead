"""ctunet_amd.simplify without a GPU: the numpy reference (tests/simplify_ref.py) pinned on facts that do not depend on it
(the invariants of the rule, the counts of a prototype, hand-made cases), and the module's host side."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import mesh_ref as R
import simplify_ref as D
from test_mesh_cpu import sphere_mask, torus_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ctu_mesh_decimate_ws_bytes", "ctu_mesh_decimate_bounds", "ctu_mesh_decimate_build", "ctu_mesh_decimate_emit")
SPACING = (0.8, 0.45, 0.45)
R50 = (17, 33, 65)
CELLS = (0.05, 1, 1.5, 2.5, 4, 1000)
TRIPLE = (2.4, 1.35, 1.8)                                            # an anisotropic cell for the spaced sphere
MESHES = ("sphere", "sphere_spaced", "torus", "r50", "shell")


def shell_mask():
    """A spherical shell 4 voxels thick with a round opening: at cells of 2.5 its two sheets share clusters in places."""
    z, y, x = np.indices((30, 30, 30))
    r = np.sqrt((z - 14.5) ** 2 + (y - 14.5) ** 2 + (x - 14.5) ** 2)
    return (r >= 8.0) & (r <= 12.0) & ~((np.sqrt((y - 14.5) ** 2 + (x - 14.5) ** 2) <= 5.0) & (z < 15))


def sparse_mesh(n=12, side=210.0):
    """A dozen small triangles spread over a box of more than 4096 x 1024 unit cells; every one spans three cells."""
    rng = np.random.default_rng(3)
    base = rng.random((n, 3)) * (side - 4.0)
    base[0], base[-1] = 0.0, side - 4.0
    corners = np.array([[0.2, 0.3, 0.4], [2.7, 0.6, 1.9], [1.1, 3.2, 3.6]])
    v = (base[:, None, :] + corners[None]).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def fan_mesh(n):
    """n distinct faces around a hub in the lowest cell; the rim vertices lie in n + 1 different unit cells."""
    a = np.linspace(0.0, np.pi / 2, n + 1)
    rim = np.stack([np.zeros(n + 1), 5000.0 * np.sin(a) + 2.0, 5000.0 * np.cos(a) + 2.0], axis=1)
    v = np.concatenate([[[0.0, 0.0, 0.0]], rim]).astype(np.float32)
    i = np.arange(1, n + 1)
    return v, np.stack([np.zeros(n, dtype=np.int64), i, i + 1], axis=1).astype(np.int32)


def many_faces_mesh(n_vertices=150000, n_faces=2048 * 256 + 4097):
    """More faces than the 2048 blocks of 256 threads of the bounds pass, so its blocks stride; random triangles in a box
    whose extreme vertices only the last face uses."""
    rng = np.random.default_rng(7)
    v = (rng.random((n_vertices, 3)) * 96.0 + 2.0).astype(np.float32)
    v[-3:] = [[0.0, 50.0, 100.0], [100.0, 0.0, 50.0], [50.0, 100.0, 0.0]]
    f = rng.integers(0, n_vertices - 3, size=(n_faces, 3)).astype(np.int32)
    f[-1] = [n_vertices - 3, n_vertices - 2, n_vertices - 1]
    return v, f


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    """(vertices, faces) of the reference extraction, on the host."""
    if name == "sphere":
        return R.extract(sphere_mask())
    if name == "sphere_spaced":
        return R.extract(sphere_mask(), spacing=SPACING)
    if name == "torus":
        return R.extract(torus_mask())
    if name == "r50":
        return R.extract(np.random.default_rng(50).random(R50) < 0.5)
    if name == "shell":
        return R.extract(shell_mask())
    if name == "sparse":
        return sparse_mesh()
    if name == "many":
        return many_faces_mesh()
    assert name == "fan"
    return fan_mesh(4096)


@functools.lru_cache(maxsize=None)
def ref(name, cell, cancel=True):
    """The reference's (vertices, faces, map); without the cell limit, which the host does not need."""
    v, f = mesh_of(name)
    return D.decimate(v, f, cell, cancel, max_cells=None)


def cells_of(name):
    return CELLS + ((TRIPLE,) if name == "sphere_spaced" else ())


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("name", MESHES)
def test_invariants_of_the_rule(name):
    v, f = mesh_of(name)
    assert D.edges_balanced(f)
    members = np.unique(f)
    for cell in cells_of(name):
        c3 = np.broadcast_to(np.asarray(cell, dtype=np.float32).astype(np.float64), (3,))
        volumes = []
        for cancel in (True, False):
            ov, of, vmap = ref(name, cell, cancel)
            assert ov.dtype == np.float32 and of.dtype == np.int32 and vmap.dtype == np.int32 and vmap.shape == (len(v),)
            assert len(of) <= len(f) and len(ov) <= len(v)
            assert D.edges_balanced(of), (cell, cancel)                                          # (a)
            if len(of):
                assert of.min() == 0 and of.max() == len(ov) - 1 and len(np.unique(of)) == len(ov)
                assert (of[:, 0] != of[:, 1]).all() and (of[:, 1] != of[:, 2]).all() and (of[:, 2] != of[:, 0]).all()
            hit = members[vmap[members] >= 0]
            moved = np.abs(v[hit].astype(np.float64) - ov[vmap[hit]].astype(np.float64))
            bound = c3 * (1 + 1e-6) + 1e-6 * np.abs(v[members]).max()
            assert (moved <= bound).all(), (cell, cancel, moved.max(axis=0))                     # (b)
            assert (vmap[np.setdiff1d(np.arange(len(v)), members)] == -1).all()
            _, terms = R.face_geometry(ov, of)
            volumes.append((float(terms.sum()), float(np.abs(terms).sum())))
            if cell == 0.05:
                # every vertex its own cluster: the same mesh, renumbered in cell order, to within the quantum
                assert len(of) == len(f) and len(ov) == len(v) and np.array_equal(of, vmap[f])
                assert np.abs(ov[vmap] - v).max() <= np.abs(v).max() * 2.0 ** -22
            if cell == 1000:
                assert len(of) == 0 and len(ov) == 0 and (vmap == -1).all()
        (on, scale), (off, _) = volumes
        assert abs(on - off) <= 1e-9 * max(scale, 1.0), (cell, on, off)
    # cancellation does something exactly where sheets share clusters
    if name in ("shell", "r50"):
        assert len(ref(name, 2.5)[1]) < len(ref(name, 2.5, False)[1])
        assert len(ref(name, 1)[1]) == len(ref(name, 1, False)[1])


def test_counts_of_the_prototype_on_the_sphere():
    v, f = mesh_of("sphere")
    assert (len(v), len(f)) == (2766, 5528)
    for cell, nv, nf in ((1.0, 930, 1856), (1.5, 375, 746), (2.5, 135, 266), (4.0, 56, 108)):
        ov, of, _ = ref("sphere", cell)
        assert (len(ov), len(of)) == (nv, nf), cell
        if cell <= 2.5:
            assert R.euler(len(ov), of) == 2


def tri(*faces):
    return np.array(faces, dtype=np.int32).reshape(-1, 3)


SQUARE = np.array([[0, 0, 0], [0, 0, 3], [0, 3, 0], [0, 3, 3], [7, 7, 7]], dtype=np.float32)      # a planar mesh: no extent in z


def test_hand_made_cancellation():
    v = SQUARE[:4]
    a, b = [0, 1, 2], [0, 2, 1]
    ov, of, vmap = D.decimate(v, tri(a, b), 1.0)
    assert len(ov) == 0 and len(of) == 0 and (vmap == -1).all()
    ov, of, vmap = D.decimate(v, tri(a, b), 1.0, cancel=False)
    assert np.array_equal(of, tri([0, 1, 2], [0, 2, 1])) and len(ov) == 3 and vmap.tolist() == [0, 1, 2, -1]
    # three copies (in any rotation) against one reverse: the two of lowest index survive, in their own corner order
    faces = tri([1, 2, 0], b, a, [2, 0, 1])
    ov, of, vmap = D.decimate(v, faces, 1.0)
    assert np.array_equal(of, tri([1, 2, 0], [0, 1, 2])) and len(ov) == 3
    ov, of, _ = D.decimate(v, faces, 1.0, cancel=False)
    assert np.array_equal(of, faces)
    # one against three reverses
    ov, of, _ = D.decimate(v, tri(a, b, [2, 1, 0], [1, 0, 2]), 1.0)
    assert np.array_equal(of, tri([0, 2, 1], [2, 1, 0]))
    # different keys do not meet
    ov, of, _ = D.decimate(v, tri(a, [1, 3, 2], [0, 2, 1]), 1.0)
    assert np.array_equal(of, tri([0, 2, 1])) and np.array_equal(ov, v[[1, 2, 3]])


def test_hand_made_degenerate_and_refused_input():
    v = SQUARE
    # a repeated index is dropped like any face with two corners in one cell; vertex 4 is unreferenced
    ov, of, vmap = D.decimate(v, tri([0, 1, 1], [0, 1, 2]), 1.0)
    assert np.array_equal(of, tri([0, 1, 2])) and np.array_equal(ov, v[:3]) and vmap.tolist() == [0, 1, 2, -1, -1]
    for bad in (5, -1):
        assert D.refused(v, tri([0, 1, 2], [0, bad, 2])) == 1
        with pytest.raises(ValueError, match="refused"):
            D.decimate(v, tri([0, 1, 2], [0, bad, 2]), 1.0)
    w = v.copy()
    w[4] = np.nan
    assert D.refused(w, tri([0, 1, 2])) == 0 and D.refused(w, tri([0, 1, 2], [0, 1, 4])) == 1
    with pytest.raises(ValueError, match="refused"):
        D.decimate(w, tri([0, 1, 4]), 1.0)
    ov, of, _ = D.decimate(w, tri([0, 1, 2]), 1.0)                      # an unreferenced NaN vertex is harmless
    assert np.array_equal(ov, v[:3]) and np.array_equal(of, tri([0, 1, 2]))
    # all members coincide: ext == 0, one cell, nothing left
    same = np.repeat(v[3:4], 3, axis=0)
    ov, of, vmap = D.decimate(same, tri([0, 1, 2]), 0.5)
    assert len(ov) == 0 and len(of) == 0 and (vmap == -1).all()
    assert D.decimate(v, np.zeros((0, 3), dtype=np.int32), 1.0)[2].tolist() == [-1] * 5
    # a planar mesh has an axis of zero extent: one layer of cells
    assert D.grid(v[:4], tri([0, 1, 2], [1, 3, 2]), 1.0)[3] == [1, 4, 4]
    ov, of, _ = D.decimate(v[:4], tri([0, 1, 2], [1, 3, 2]), 2.0)
    assert np.array_equal(of, tri([0, 1, 2], [1, 3, 2])) and (ov[:, 0] == 0).all()
    # clusters of several members sit at their mean
    ov, of, _ = D.decimate(np.array([[0, 0, 0], [0, 0, 1], [0, 9, 0], [0, 9, 9], [0, 8, 9]], dtype=np.float32),
                           tri([0, 2, 3], [1, 2, 4]), 4.0)
    assert np.array_equal(ov, np.array([[0, 0, 0.5], [0, 9, 0], [0, 8.5, 9]], dtype=np.float32))
    assert np.array_equal(of, tri([0, 1, 2], [0, 1, 2]))
    with pytest.raises(ValueError, match="cells"):
        D.decimate(*sparse_mesh(), 0.25)


def test_shapes_of_the_shared_cases():
    v, f = mesh_of("sparse")
    assert len(f) == 12 and 2 * 4096 * 1024 < np.prod(D.grid(v, f, 1.0)[3]) < D.MAX_CELLS
    assert len(ref("sparse", 1.0)[1]) == 12
    v, f = mesh_of("many")
    assert len(f) > 2048 * 256 and D.grid(v, f, 2.0)[3] == [51, 51, 51] and D.grid(v, f[:-1], 2.0)[3] == [48, 48, 48]
    assert len(ref("many", 2.0)[1]) > len(f) // 2
    v, f = mesh_of("fan")
    ov, of, _ = ref("fan", 1.0)
    assert len(of) == len(f) == 4096 and len(ov) == 4098 and (of[:, 0] == 0).all()


# ------------------------------------------------------------------------------------------------ the module's host side
def test_symbols_in_header_table_and_library():
    import ctunet_amd
    from ctunet_amd import _lib, mesh, simplify
    header = open(os.path.join(ROOT, "include", "ctunet_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.load().ctu_abi_version() == _lib.ABI_VERSION == 8
    assert simplify.MAX_CELLS == int(re.search(r"#define CTU_MESH_DECIMATE_MAX_CELLS (\d+)", header).group(1)) == 1 << 28 == D.MAX_CELLS
    assert simplify.MAX_BUCKET == int(re.search(r"#define CTU_MESH_DECIMATE_MAX_BUCKET (\d+)", header).group(1)) == 4096
    assert "simplify" in ctunet_amd.__all__ and ctunet_amd.simplify.decimate is simplify.decimate
    assert "Out of scope: decimation, formats other than binary STL, marching cubes." in mesh.__doc__
    assert "ctunet_amd.simplify" in mesh.__doc__
    for word in ("Out of scope", "two", "MAX_BUCKET", "not bit for bit", "2-manifold"):
        assert word in simplify.__doc__ or word in simplify.decimate.__doc__, word


def test_workspace_bytes_and_limits():
    from ctunet_amd import _lib, simplify
    lib = _lib.load()
    a256 = lambda n: -(-n // 256) * 256
    top = (1 << 31) - 1
    for V, F, cells in ((1, 1, 1), (3, 1, 8), (2766, 5528, 12167), (134748, 285704, 1 << 20), (4096, 4097, 4098), (top, top, 1 << 28)):
        build = (256 + a256(V) + 6 * a256(4 * V) + a256(24 * V) + 2 * a256(4 * F) + a256(16 * F) + a256(cells) + a256(4 * cells)
                 + a256(8 * -(-max(V, F, cells) // 4096)))
        assert lib.ctu_mesh_decimate_ws_bytes(V, F, cells) == build
        assert lib.ctu_mesh_decimate_ws_bytes(V, F, 0) == 256
        assert simplify.workspace_bytes(V, F, cells) == build + 256
    for V, F, cells in ((1 << 31, 1, 1), (1, 1 << 31, 1), (-1, 1, 1), (1, -1, 1), (1, 1, (1 << 28) + 1), (1, 1, -1)):
        assert lib.ctu_mesh_decimate_ws_bytes(V, F, cells) == 0
        with pytest.raises(ValueError, match="2\\^31"):
            simplify.workspace_bytes(V, F, cells)
    for bad in ((4.0, 1, 1), (True, 1, 1), ("4", 1, 1), (4, 1, 0), (4, 1, 2.0)):
        with pytest.raises(ValueError):
            simplify.workspace_bytes(*bad)


def test_c_entry_points_refuse_bad_arguments():
    """CTU_REQUIRE fires before any launch, so these calls need no GPU; the message comes through ctu_last_error."""
    from ctunet_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    f3 = lambda *x: (ctypes.c_float * 3)(*x)
    lo, hi, cell = f3(0, 0, 0), f3(1, 2, 3), f3(1, 1, 1)

    def err(status):
        assert status == -1
        return lib.ctu_last_error().decode()

    def bounds(vert=p, V=4, faces=p, F=2, ws=p):
        return lib.ctu_mesh_decimate_bounds(vert, V, faces, F, ws, None)

    def build(vert=p, V=4, faces=p, F=2, lo=lo, hi=hi, cell=cell, cells=24, cancel=1, ws=p):
        return lib.ctu_mesh_decimate_build(vert, V, faces, F, lo, hi, cell, cells, cancel, ws, None)

    def emit(faces=p, V=4, F=2, Vp=3, Fp=1, lo=lo, hi=hi, ov=p, of=p, om=None, ws=p):
        return lib.ctu_mesh_decimate_emit(faces, V, F, Vp, Fp, lo, hi, ov, of, om, ws, None)

    for fn in (bounds, build, emit):
        assert "2^31" in err(fn(V=1 << 31))
        assert "2^31" in err(fn(F=1 << 31))
        assert "2^31" in err(fn(V=-1))
        assert "at least one" in err(fn(F=0))
        assert "at least one" in err(fn(V=0))
        assert "null" in err(fn(faces=None))
        assert "null" in err(fn(ws=None))
        assert "aligned" in err(fn(ws=p + 4))
    assert "null" in err(bounds(vert=None)) and "null" in err(build(vert=None))
    assert "null" in err(build(lo=None)) and "null" in err(build(cell=None)) and "null" in err(emit(hi=None))
    for fn in (build, emit):
        assert "lo <= hi" in err(fn(lo=f3(0, 3, 0)))
        assert "finite" in err(fn(hi=f3(1, float("nan"), 3)))
        assert "finite" in err(fn(lo=f3(float("-inf"), 0, 0)))
    for bad in (f3(1, 0, 1), f3(1, -1, 1), f3(1, 1, float("nan")), f3(float("inf"), 1, 1)):
        assert "cell_size" in err(build(cell=bad))
    assert "more than" in err(build(cell=f3(1e-3, 1e-3, 1e-3)))
    assert "more than" in err(build(cell=f3(1e-30, 1, 1)))
    assert "is not the grid" in err(build(cells=23)) and "2 x 3 x 4 = 24" in err(build(cells=25))
    assert "totals" in err(emit(Vp=5)) and "totals" in err(emit(Fp=3)) and "totals" in err(emit(Vp=-1))
    assert "null" in err(emit(ov=None)) and "null" in err(emit(of=None))


def test_argument_validation_raises_before_any_launch():
    from ctunet_amd import mesh, simplify
    v, f = torch.from_numpy(SQUARE), torch.from_numpy(tri([0, 1, 2], [1, 3, 2]))
    m = mesh.Mesh(v, f)
    bad = [
        (dict(cell_size=0), "cell_size"), (dict(cell_size=-1.0), "cell_size"), (dict(cell_size=float("nan")), "cell_size"),
        (dict(cell_size=float("inf")), "cell_size"), (dict(cell_size=1e-60), "cell_size"), (dict(cell_size=1e39), "cell_size"),
        (dict(cell_size=(1, 2)), "cell_size"), (dict(cell_size=(1, 0, 1)), "cell_size"), (dict(cell_size="a"), "cell_size"),
        (dict(cell_size=None), "cell_size"), (dict(cell_size=True), "cell_size"), (dict(cell_size=(1, "b", 1)), "cell_size"),
        (dict(cell_size=1.0, cancel=1), "booleans"), (dict(cell_size=1.0, return_map=None), "booleans"),
    ]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            simplify.decimate(m, **kw)
    for kw in (dict(cell_size=1.0), dict(cell_size=(1.0, 2.0, 0.5), cancel=False, return_map=True), dict(cell_size=torch.tensor([1.0, 2.0, 3.0]))):
        with pytest.raises(ValueError, match="no CPU fallback"):
            simplify.decimate(m, **kw)
    with pytest.raises(ValueError, match="no CPU fallback"):
        simplify.decimate(mesh.Mesh(v, f[:0]), 1.0)                    # F == 0 too: the device decides where the result lives
    for broken in ((v, f.long()), (v.double(), f), (v[:, :2], f), (torch.zeros(0, 3), f), "mesh", (v, f.to("meta"))):
        with pytest.raises(ValueError):
            simplify.decimate(broken, 1.0)
    big_v = mesh.Mesh(torch.empty((1 << 31, 3), device="meta"), torch.empty((1, 3), dtype=torch.int32, device="meta"))
    big_f = mesh.Mesh(torch.empty((4, 3), device="meta"), torch.empty((1 << 31, 3), dtype=torch.int32, device="meta"))
    for big in (big_v, big_f):
        with pytest.raises(ValueError, match="2\\^31"):
            simplify.decimate(big, 1.0)


def test_documents_point_to_the_module():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert 0 < design.index("### Mesh smoothing") < design.index("### Mesh decimation") < design.index("### Mesh voxelisation")
    assert "Out of scope on purpose: decimation" not in design and "a BVH, decimation" not in design
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "simplify.decimate(" in readme
    src = open(os.path.join(ROOT, "ct-unet_amd", "ctunet_amd", "simplify.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(scipy|oracle)", src, flags=re.M)
