"""Host-side checks of ctunet_amd.mesh's voxelisation: the numpy restatement (tests/mesh_voxelize_ref.py) pinned on ground
truth that does not depend on it (a mask's mesh voxelises back to the mask, a field's to field > level, a hand-made cube to
its block under any winding and numbering, degenerate faces change nothing), read_stl, argument validation before anything
is launched, and the new C-ABI symbols."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_ref as R
import mesh_voxelize_ref as X
from test_mesh_cpu import _two

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ctu_mesh_voxelize_ws_bytes", "ctu_mesh_voxelize")
SPACING, ORIGIN = (0.8, 0.45, 0.45), (-10, 3.5, 0.25)
LEVEL = 0.5


def random_mask(shape, seed):
    return (np.random.default_rng(seed).random(shape) < 0.45).astype(np.uint8)


def random_field(shape, seed):
    """float32 samples in [0, 1), none within 0.05 of LEVEL."""
    f = np.random.default_rng(seed).random(shape).astype(np.float32)
    near = np.abs(f - np.float32(LEVEL)) < 0.05
    f[near] = np.where(f[near] > LEVEL, np.float32(LEVEL + 0.06), np.float32(LEVEL - 0.06))
    assert (np.abs(f - np.float32(LEVEL)) >= 0.05).all()
    return f


# the four body diagonals of a 2x2x2 block: two voxels that touch only at a corner
DIAGONALS = [((1, 1, 1), (2, 2, 2)), ((1, 1, 2), (2, 2, 1)), ((1, 2, 1), (2, 1, 2)), ((1, 2, 2), (2, 1, 1))]
MASKS = {
    "voxel": lambda: np.ones((1, 1, 1), dtype=np.uint8),
    "full": lambda: np.ones((3, 4, 5), dtype=np.uint8),
    "r567": lambda: random_mask((5, 6, 7), 0),
    "r449": lambda: random_mask((4, 4, 9), 1),
    **{f"diagonal{n}": (lambda a=a, b=b: _two(a, b)) for n, (a, b) in enumerate(DIAGONALS)},
}


def cube_block():
    b = np.zeros((6, 6, 6), dtype=np.int32)
    b[1:5, 1:5, 1:5] = 1
    return b


# ------------------------------------------------------------------------------------------------ the reference, pinned
@pytest.mark.parametrize("name", sorted(MASKS))
def test_a_masks_mesh_voxelises_back_to_the_mask(name):
    m = MASKS[name]()
    v, f = R.extract(m)
    w = X.winding_number(v, f, m.shape)
    assert w.dtype == np.int32 and w.shape == m.shape
    assert set(np.unique(w).tolist()) <= {0, 1}
    assert np.array_equal(w, m.astype(np.int32))
    assert np.array_equal(X.voxelize(v, f, m.shape), m)
    # with spacing and origin on both sides
    v, f = R.extract(m, spacing=SPACING, origin=ORIGIN)
    assert np.array_equal(X.winding_number(v, f, m.shape, SPACING, ORIGIN), m.astype(np.int32))


def test_the_full_volumes_surface_lies_in_the_virtual_layer():
    v, _ = R.extract(MASKS["full"]())
    inside = ((v > -0.25) & (v < np.array([2.25, 3.25, 4.25]))).all(axis=1)
    assert not inside.any()


@pytest.mark.parametrize("shape,seed", [((5, 6, 7), 3), ((4, 4, 9), 4)])
def test_a_fields_mesh_voxelises_back_to_field_above_level(shape, seed):
    field = random_field(shape, seed)
    v, f = R.extract(field, level=LEVEL, spacing=SPACING, origin=ORIGIN)
    w = X.winding_number(v, f, shape, SPACING, ORIGIN)
    assert np.array_equal(w, (field > np.float32(LEVEL)).astype(np.int32))
    assert 0 < w.sum() < w.size


def test_hand_made_cube_under_any_winding_and_numbering():
    """Corners at 0.5 and 4.5 on a 6^3 grid: the face diagonals and edges pass exactly through row centres."""
    v, f = X.cube_mesh()
    assert R.is_closed_oriented(f) and R.area_volume(v, f) == pytest.approx((96.0, 64.0))
    block = cube_block()
    assert np.array_equal(X.winding_number(v, f, (6, 6, 6)), block)
    assert np.array_equal(X.winding_number(v, f[:, ::-1], (6, 6, 6)), -block)          # inward: -1 inside
    assert np.array_equal(X.voxelize(v, f[:, ::-1], (6, 6, 6)), block.astype(np.uint8))
    for seed in range(6):                                                            # a tie rule that depended on index order fails here
        rng = np.random.default_rng(seed)
        perm = rng.permutation(8)
        v2 = np.empty_like(v)
        v2[perm] = v
        g = perm[f][rng.permutation(12)].astype(np.int32)
        g = np.take_along_axis(g, (np.arange(3)[None, :] + rng.integers(0, 3, size=(12, 1))) % 3, axis=1)
        assert np.array_equal(X.winding_number(v2, g, (6, 6, 6)), block)


def degenerate_faces(v, f):
    """v with three more vertices and faces that must change nothing: repeated indices, no area, edge-on projections."""
    extra = np.array([[2.0, 2.0, 1.0], [2.0, 2.0, 3.0], [3.0, 3.0, 2.0]], dtype=np.float32)
    n = len(v)
    more = [[0, 0, 1], [2, 5, 2], [3, 3, 3],                                          # repeated indices
            [n, n + 1, 7],                                                           # edge-on: n and n+1 project to one point
            [0, 7, n + 2]]                                                           # collinear in projection (z = y): no area
    return np.concatenate([v, extra]), np.concatenate([f, np.array(more, dtype=np.int32)])


def test_degenerate_faces_change_nothing():
    v, f = X.cube_mesh()
    v2, f2 = degenerate_faces(v, f)
    assert np.array_equal(X.winding_number(v2, f2, (6, 6, 6)), cube_block())
    # a face that lies in a plane z = const projects edge-on
    flat = np.array([[2.0, 1.0, 1.0], [2.0, 4.0, 1.0], [2.0, 1.0, 4.0]], dtype=np.float32)
    assert not X.winding_number(flat, np.array([[0, 1, 2]], dtype=np.int32), (6, 6, 6)).any()
    # a zero-area face of a mask's own kind: a sample equal to level makes vertices coincide at a lattice point
    field = random_field((4, 5, 6), 8)
    field[1, 2, 3] = np.float32(LEVEL)
    fv, ff = R.extract(field, level=LEVEL)
    n, _ = R.face_geometry(fv, ff)
    assert ((n * n).sum(axis=1) == 0).any()
    assert np.array_equal(X.winding_number(fv, ff, field.shape), (field > np.float32(LEVEL)).astype(np.int32))


def test_open_and_far_meshes_are_bounded():
    v, f = X.cube_mesh()
    w = X.winding_number(v, f[:10], (6, 6, 6))                                        # the y = hi side is missing
    assert np.abs(w).max() <= 1
    for far in (v + np.float32(100.0), v * np.float32(1e30), v - np.float32(1e30)):
        assert not X.winding_number(far, f, (6, 6, 6)).any()
    with pytest.raises(ValueError):
        X.winding_number(v, np.array([[0, 1, 8]]), (6, 6, 6))
    bad = v.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        X.winding_number(bad, f, (6, 6, 6))
    assert not X.winding_number(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), (2, 3, 4)).any()


# ------------------------------------------------------------------------------------------------ read_stl
def test_read_stl_round_trips_through_stl_bytes(tmp_path):
    from ctunet_amd import mesh
    for v, f in (R.extract(MASKS["r567"](), spacing=SPACING, origin=ORIGIN), X.cube_mesh(), R.extract(MASKS["voxel"]())):
        # number the vertices by first appearance in the faces, as a reader must
        _, first = np.unique(f.reshape(-1), return_index=True)
        order = f.reshape(-1)[np.sort(first)]
        assert len(order) == len(v)                                                  # no unreferenced vertex
        rank = np.empty(len(v), dtype=np.int64)
        rank[order] = np.arange(len(v))
        v1, f1 = v[order], rank[f].astype(np.int32)
        got = mesh.read_stl(mesh.stl_bytes(v1, f1, header=b"round trip"))
        assert isinstance(got, mesh.Mesh) and not got.vertices.is_cuda and not got.faces.is_cuda
        assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32
        assert np.array_equal(got.vertices.numpy().view(np.uint32), v1.view(np.uint32))
        assert np.array_equal(got.faces.numpy(), f1)
        path = tmp_path / "m.stl"
        mesh.write_stl(path, mesh.Mesh(torch.from_numpy(v1), torch.from_numpy(f1)))
        again = mesh.read_stl(path)
        assert torch.equal(again.vertices, got.vertices) and torch.equal(again.faces, got.faces)
        assert torch.equal(mesh.read_stl(str(path)).faces, got.faces)


def test_read_stl_welds_the_cubes_36_corners_to_8():
    from ctunet_amd import mesh
    v, f = X.cube_mesh()
    soup = v[f.reshape(-1)]                                                          # 36 corners, nothing shared
    data = mesh.stl_bytes(soup, np.arange(36).reshape(12, 3))
    assert len(data) == 84 + 50 * 12
    got = mesh.read_stl(data)
    assert got.vertices.shape == (8, 3) and got.faces.shape == (12, 3)
    gv, gf = got.vertices.numpy(), got.faces.numpy()
    assert np.array_equal(gv[gf], v[f])                                              # the same triangles, in order and winding
    assert R.is_closed_oriented(gf)
    assert np.array_equal(X.winding_number(gv, gf, (6, 6, 6)), cube_block())
    empty = mesh.read_stl(mesh.stl_bytes(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)))
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3)
    # -0.0 and 0.0 differ in their bits and stay apart
    tri = np.array([[0.0, 0, 0], [-0.0, 0, 0], [1, 1, 1]], dtype=np.float32)
    assert mesh.read_stl(mesh.stl_bytes(tri, [[0, 1, 2]])).vertices.shape == (3, 3)


def test_read_stl_refuses_what_it_cannot_read():
    from ctunet_amd import mesh
    data = mesh.stl_bytes(*X.cube_mesh())
    for cut in (0, 10, 83, 84, 100, len(data) - 1):
        with pytest.raises(ValueError, match="truncated"):
            mesh.read_stl(data[:cut])
    with pytest.raises(ValueError, match="counts 12 triangles"):
        mesh.read_stl(data + b"\0")
    wrong = data[:80] + np.uint32(11).astype("<u4").tobytes() + data[84:]
    with pytest.raises(ValueError, match="counts 11 triangles"):
        mesh.read_stl(wrong)
    ascii_form = b"solid cube\nfacet normal 0 0 1\n outer loop\n  vertex 0 0 0\n  vertex 1 0 0\n  vertex 0 1 0\n endloop\nendfacet\nendsolid cube\n"
    for text in (ascii_form, b"solid x\nendsolid x\n"):
        with pytest.raises(ValueError, match="ASCII"):
            mesh.read_stl(text)


# ------------------------------------------------------------------------------------------------ the module's host side
def test_symbols_in_header_table_and_library():
    from ctunet_amd import _lib, mesh
    header = open(os.path.join(ROOT, "include", "ctunet_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.load().ctu_abi_version() == _lib.ABI_VERSION == 8
    for fn in ("voxelize", "winding_number", "voxelize_workspace_bytes", "read_stl"):
        assert callable(getattr(mesh, fn))


def test_workspace_bytes_and_limits():
    from ctunet_amd import _lib, mesh
    lib = _lib.load()
    a256 = lambda n: -(-n // 256) * 256
    for shape in ((1, 1, 1), (3, 5, 130), (224, 304, 304), (1024, 1024, 1024)):
        n = shape[0] * shape[1] * shape[2]
        assert lib.ctu_mesh_voxelize_ws_bytes(*shape) == mesh.voxelize_workspace_bytes(shape) == 256 + a256(4 * n)
    for shape in ((0, 4, 4), (4, 1025, 4), (4, 4, -1)):
        assert lib.ctu_mesh_voxelize_ws_bytes(*shape) == 0
        with pytest.raises(ValueError, match="every side"):
            mesh.voxelize_workspace_bytes(shape)


def test_c_entry_point_refuses_bad_arguments():
    """CTU_REQUIRE fires before any launch, so these calls need no GPU; the message comes through ctu_last_error."""
    from ctunet_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    f3 = lambda *v: (ctypes.c_float * 3)(*v)

    def call(vert=p, V=8, faces=p, F=12, shape=(6, 6, 6), sp=None, org=None, wind=0, out=p, ws=p):
        return lib.ctu_mesh_voxelize(vert, V, faces, F, *shape, sp, org, wind, out, ws, None)

    def err(status):
        assert status == -1
        return lib.ctu_last_error().decode()

    assert "bad shape" in err(call(shape=(0, 6, 6)))
    assert "bad shape" in err(call(shape=(6, 1025, 6)))
    assert "2^31" in err(call(V=1 << 31))
    assert "2^31" in err(call(F=1 << 31))
    assert "2^31" in err(call(V=-1))
    assert "without vertices" in err(call(V=0))
    for sp in (f3(0, 1, 1), f3(1, -1, 1), f3(1, 1, float("inf")), f3(float("nan"), 1, 1)):
        assert "spacing" in err(call(sp=sp))
    for org in (f3(0, float("inf"), 0), f3(0, 0, float("nan"))):
        assert "origin" in err(call(org=org))
    assert "null" in err(call(out=None))
    assert "null" in err(call(ws=None))
    assert "null" in err(call(vert=None))
    assert "null" in err(call(faces=None))
    assert "aligned" in err(call(ws=p + 4))


def test_argument_validation_raises_before_any_launch():
    from ctunet_amd import mesh
    v, f = (torch.from_numpy(a) for a in X.cube_mesh())
    m = mesh.Mesh(v, f)
    for fn in (mesh.voxelize, mesh.winding_number):
        bad = [
            (dict(shape=(6, 6)), "triple"), (dict(shape=6), "triple"), (dict(shape=(6, 6, 6.0)), "integers"),
            (dict(shape=(6, 0, 6)), "every side"), (dict(shape=(6, 6, 1025)), "every side"), (dict(shape=(True, 6, 6)), "integers"),
            (dict(shape=(6, 6, 6), spacing=0), "spacing"), (dict(shape=(6, 6, 6), spacing=(1, 1)), "spacing"),
            (dict(shape=(6, 6, 6), spacing=(1, -1, 1)), "spacing"), (dict(shape=(6, 6, 6), spacing=float("nan")), "spacing"),
            (dict(shape=(6, 6, 6), spacing=1e-60), "spacing"),
            (dict(shape=(6, 6, 6), origin=(0, 0)), "origin"), (dict(shape=(6, 6, 6), origin=float("inf")), "origin"),
            (dict(shape=(6, 6, 6), origin="a"), "origin"), (dict(shape=(6, 6, 6), origin=1e39), "origin"),
        ]
        for kw, match in bad:
            with pytest.raises(ValueError, match=match):
                fn(m, **kw)
        for kw in (dict(shape=(6, 6, 6)), dict(shape=torch.Size((2, 3, 4)), spacing=SPACING, origin=ORIGIN),
                   dict(shape=[6, 6, 6], spacing=2, origin=torch.tensor([0.5, 0.5, 0.5]))):
            with pytest.raises(ValueError, match="no CPU fallback"):
                fn(m, **kw)
        with pytest.raises(ValueError, match="no CPU fallback"):                      # an empty mesh on the host raises too
            fn(mesh.Mesh(torch.zeros(0, 3), torch.zeros((0, 3), dtype=torch.int32)), (6, 6, 6))
        for broken in ((v, f.long()), (v.double(), f), (v[:, :2], f), (torch.zeros(0, 3), f), "mesh"):
            with pytest.raises(ValueError):
                fn(broken, (6, 6, 6))
        big_v = mesh.Mesh(torch.empty((1 << 31, 3), device="meta"), torch.empty((1, 3), dtype=torch.int32, device="meta"))
        big_f = mesh.Mesh(torch.empty((4, 3), device="meta"), torch.empty((1 << 31, 3), dtype=torch.int32, device="meta"))
        for big in (big_v, big_f):
            with pytest.raises(ValueError, match="2\\^31"):
                fn(big, (6, 6, 6))


def test_documents_state_the_rule_and_the_pipeline_line():
    from ctunet_amd import mesh
    doc = mesh.__doc__
    assert "mesh.voxelize(mesh.smooth(m), scan.shape, spacing=(0.8, 0.45, 0.45))" in doc and "metrics.surface_metrics(v, truth" in doc
    for phrase in ("(+eps, +eps^2)", "endpoint of lower", "x_k > x_c", "tests/mesh_voxelize_ref.py", "read_stl"):
        assert phrase in doc, phrase
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "mesh.voxelize(" in readme and "mesh.read_stl(" in readme
