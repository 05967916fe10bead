"""Host-side checks of ctunet_amd.mesh: the numpy restatement (tests/mesh_ref.py) pinned on facts that do not depend on it
(counts, volumes, areas, Euler characteristics, closed and consistently oriented surfaces), argument validation before
anything is launched, the new C-ABI symbols, and the byte layout of binary STL."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ctu_mesh_ws_bytes", "ctu_mesh_count", "ctu_mesh_emit", "ctu_mesh_measure")


def _grid():
    return np.meshgrid(np.arange(20.0), np.arange(22.0), np.arange(24.0), indexing="ij")


def sphere_field():
    z, y, x = _grid()
    return (7.0 - np.sqrt((z - 9.3) ** 2 + (y - 10.6) ** 2 + (x - 11.2) ** 2)).astype(np.float32)


def sphere_mask():
    z, y, x = _grid()
    return np.sqrt((z - 9.3) ** 2 + (y - 10.6) ** 2 + (x - 11.2) ** 2) <= 7.0


def torus_mask():
    z, y, x = _grid()
    return np.sqrt((np.sqrt((y - 10.5) ** 2 + (x - 11.5) ** 2) - 6.5) ** 2 + (z - 9.5) ** 2) <= 2.2


def _two(a, b):
    m = np.zeros((4, 4, 4), dtype=np.uint8)
    m[a] = m[b] = 1
    return m


CASES = {
    "voxel": lambda: (np.ones((1, 1, 1), dtype=np.uint8), {}),
    "block": lambda: (np.ones((2, 3, 4), dtype=np.uint8), {}),
    "sphere_field": lambda: (sphere_field(), dict(level=0.0, fill_value=-100.0)),
    "sphere_mask": lambda: (sphere_mask(), {}),
    "torus": lambda: (torus_mask(), {}),
    "random": lambda: (np.random.default_rng(0).random((5, 6, 7)) < 0.5, {}),
    "body_diagonal": lambda: (_two((1, 1, 1), (2, 2, 2)), {}),
    "other_body_diagonal": lambda: (_two((1, 1, 2), (2, 2, 1)), {}),
    "face_diagonal": lambda: (_two((1, 1, 1), (1, 2, 2)), {}),
}


@pytest.fixture(scope="module")
def meshes():
    return {k: R.extract(v, **kw) for k, (v, kw) in ((k, f()) for k, f in CASES.items())}


def test_single_voxel(meshes):
    v, f = meshes["voxel"]
    assert (len(v), len(f)) == (14, 24) and R.euler(len(v), f) == 2
    area, vol = R.area_volume(v, f)
    assert vol == pytest.approx(0.5, rel=1e-7) and area == pytest.approx(3.6213203, rel=1e-7)


def test_block_of_ones(meshes):
    v, f = meshes["block"]
    assert (len(v), len(f)) == (174, 344) and R.euler(len(v), f) == 2
    assert R.area_volume(v, f)[1] == 22.0


def test_sphere(meshes):
    v, f = meshes["sphere_field"]
    area, vol = R.area_volume(v, f)
    assert R.euler(len(v), f) == 2
    assert vol == pytest.approx(1422.097, rel=1e-4) and area == pytest.approx(612.513, rel=1e-4)
    assert vol < 4.0 / 3.0 * np.pi * 7.0 ** 3 and area < 4.0 * np.pi * 7.0 ** 2
    v, f = meshes["sphere_mask"]
    assert (len(v), len(f)) == (2766, 5528) and R.euler(len(v), f) == 2


def test_torus(meshes):
    v, f = meshes["torus"]
    assert R.euler(len(v), f) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_closed_oriented_manifold(meshes, name):
    v, f = meshes[name]
    assert len(f) > 0
    assert (R.undirected_edge_counts(f) == 2).all()
    assert (R.directed_edge_counts(f) == 1).all()
    assert R.area_volume(v, f)[1] > 0
    assert f.dtype == np.int32 and v.dtype == np.float32 and f.min() == 0 and f.max() == len(v) - 1


def test_kuhn_split_joins_one_body_diagonal_only(meshes):
    """Two voxels across the (0,0,0)-(1,1,1) diagonal form one surface, across another body diagonal or a face diagonal of
    the same split they stay two (chi = 2 per closed surface)."""
    assert R.euler(len(meshes["body_diagonal"][0]), meshes["body_diagonal"][1]) == 2
    assert R.euler(len(meshes["other_body_diagonal"][0]), meshes["other_body_diagonal"][1]) == 4


def test_empty_inputs_give_no_mesh():
    for vol, kw in ((np.zeros((3, 4, 5), dtype=np.uint8), {}), (np.zeros((3, 4, 5), dtype=np.float32), {}),
                    (np.full((2, 2, 2), 3, dtype=np.int64), dict(label=2))):
        v, f = R.extract(vol, **kw)
        assert v.shape == (0, 3) and f.shape == (0, 3)


def test_spacing_and_origin_move_vertices_only():
    m = np.random.default_rng(1).random((4, 5, 6)) < 0.4
    v0, f0 = R.extract(m)
    v1, f1 = R.extract(m, spacing=(0.8, 0.45, 0.45), origin=(-10, 3.5, 0.25))
    assert np.array_equal(f0, f1)
    want = np.float32([-10, 3.5, 0.25]) + v0 * np.float32([0.8, 0.45, 0.45])
    assert np.array_equal(v1, want.astype(np.float32))
    assert (v0.min(axis=0) == -0.5).all()                       # the virtual layer closes the surface half a voxel outside


# ------------------------------------------------------------------------------------------------ the module's host side
def test_symbols_in_header_table_and_library():
    from ctunet_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctunet_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.load().ctu_abi_version() == _lib.ABI_VERSION == 8


def test_package_exports_the_module():
    import ctunet_amd
    assert "mesh" in ctunet_amd.__all__ and ctunet_amd.mesh.extract_surface


def test_workspace_bytes_and_limits():
    from ctunet_amd import _lib, mesh
    lib = _lib.load()
    for shape in ((1, 1, 1), (3, 5, 130), (224, 512, 512), (1024, 1024, 1024)):
        rows, wcp = (shape[0] + 1) * (shape[1] + 1), -(-(shape[2] + 1) // 16) * 16
        a256 = lambda n: -(-n // 256) * 256
        want = 256 + 3 * a256(4 * rows) + a256(rows * wcp) + a256(4 * rows * wcp)
        assert mesh.workspace_bytes(shape) == want
        # at most 8 bytes per cell + O(rows): <= 15 pad cells of 5 bytes and 12 bytes per row, six segments rounded to 256
        assert want <= 8 * (shape[0] + 1) * (shape[1] + 1) * (shape[2] + 1) + 87 * rows + 6 * 256
    assert mesh.SCAN_BLOCK == int(re.search(r"#define CTU_MESH_SCAN_BLOCK (\d+)",
                                            open(os.path.join(ROOT, "include", "ctunet_hip.h")).read()).group(1))
    for bad in ((0, 4, 4), (4, 1025, 4), (4, 4), (4, 4, 4.0), None):
        with pytest.raises(ValueError):
            mesh.workspace_bytes(bad)
    assert lib.ctu_mesh_ws_bytes(4, 1025, 4) == 0 and lib.ctu_mesh_ws_bytes(0, 1, 1) == 0
    assert lib.ctu_mesh_ws_bytes(1024, 1024, 1024) > 0


def test_c_entry_points_refuse_bad_arguments():
    """CTU_REQUIRE fires before any launch, so these calls need no GPU; the message comes through ctu_last_error."""
    from ctunet_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) // 16 * 16 + 16

    def err(status):
        assert status == -1
        return lib.ctu_last_error().decode()

    assert "null" in err(lib.ctu_mesh_count(None, 3, 2, 2, 2, 0, 0, 0.5, p, None))
    assert "bad shape" in err(lib.ctu_mesh_count(p, 3, 2, 1025, 2, 0, 0, 0.5, p, None))
    assert "bad shape" in err(lib.ctu_mesh_count(p, 3, 0, 2, 2, 0, 0, 0.5, p, None))
    assert "dtype" in err(lib.ctu_mesh_count(p, 5, 2, 2, 2, 0, 0, 0.5, p, None))
    assert "label" in err(lib.ctu_mesh_count(p, 0, 2, 2, 2, 1, 1, 0.5, p, None))
    assert "aligned" in err(lib.ctu_mesh_count(p, 3, 2, 2, 2, 0, 0, 0.5, p + 4, None))
    assert "2^31" in err(lib.ctu_mesh_emit(p, 3, 2, 2, 2, 0.5, 0.0, None, None, 1 << 31, 8, p, p, p, None))
    assert "2^31" in err(lib.ctu_mesh_emit(p, 3, 2, 2, 2, 0.5, 0.0, None, None, 8, 1 << 31, p, p, p, None))
    assert "totals" in err(lib.ctu_mesh_emit(p, 3, 2, 2, 2, 0.5, 0.0, None, None, 0, 8, p, p, p, None))
    assert "fill_value" in err(lib.ctu_mesh_emit(p, 0, 2, 2, 2, 0.5, 0.75, None, None, 8, 8, p, p, p, None))
    bad_sp = (ctypes.c_float * 3)(1.0, 0.0, 1.0)
    assert "spacing" in err(lib.ctu_mesh_emit(p, 3, 2, 2, 2, 0.5, 0.0, bad_sp, None, 8, 8, p, p, p, None))
    assert "null" in err(lib.ctu_mesh_emit(p, 3, 2, 2, 2, 0.5, 0.0, None, None, 8, 8, None, p, p, None))
    assert "null" in err(lib.ctu_mesh_measure(p, 1, p, 1, None, None, p, None))
    assert "2^31" in err(lib.ctu_mesh_measure(p, 1 << 31, p, 1, p, None, p, None))
    assert "without vertices" in err(lib.ctu_mesh_measure(None, 0, p, 1, p, None, p, None))
    assert lib.ctu_mesh_emit(p, 3, 2, 2, 2, 0.5, 0.0, None, None, 0, 0, None, None, p, None) == 0      # empty: nothing to launch


def test_argument_validation_raises_before_any_launch():
    from ctunet_amd import mesh
    u8 = torch.zeros(3, 4, 5, dtype=torch.uint8)
    f32 = torch.zeros(3, 4, 5)
    bad = [
        (dict(volume=np.zeros((3, 4, 5))), "one \\[D,H,W\\] tensor"),
        (dict(volume=torch.zeros(2, 3, 4, 5, dtype=torch.uint8)), "one \\[D,H,W\\] tensor"),
        (dict(volume=torch.zeros(3, 4, 5, dtype=torch.int32)), "must be one of"),
        (dict(volume=torch.zeros(3, 4, 5, dtype=torch.float64)), "must be one of"),
        (dict(volume=torch.zeros(2, 1025, 2, dtype=torch.uint8)), "every side"),
        (dict(volume=torch.zeros(0, 4, 5, dtype=torch.uint8)), "every side"),
        (dict(volume=u8, level=0.25), "level 0.5"),
        (dict(volume=u8, level="a"), "level"),
        (dict(volume=f32, level=float("nan")), "level"),
        (dict(volume=u8, fill_value=1), "virtual layer"),
        (dict(volume=f32, level=0.5, fill_value=0.75), "must not exceed"),
        (dict(volume=f32, fill_value=float("inf")), "fill_value"),
        (dict(volume=f32, label=1), "label belongs"),
        (dict(volume=u8, label=1.5), "label must be"),
        (dict(volume=u8, label=True), "label must be"),
        (dict(volume=u8, spacing=0), "spacing"),
        (dict(volume=u8, spacing=(1, 2)), "spacing"),
        (dict(volume=u8, spacing=(1, -2, 1)), "spacing"),
        (dict(volume=u8, spacing=1e-60), "spacing"),
        (dict(volume=u8, origin=(1, 2)), "origin"),
        (dict(volume=u8, origin="abc"), "origin"),
        (dict(volume=u8, origin=(0, float("nan"), 0)), "origin"),
        (dict(volume=u8), "must live on the GPU"),
        (dict(volume=f32, level=0.0, fill_value=-1.0, spacing=(0.8, 0.45, 0.45), origin=2.0), "must live on the GPU"),
    ]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            mesh.extract_surface(**kw)
    good = mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    for fn in (mesh.measure, mesh.face_normals):
        with pytest.raises(ValueError, match="no CPU fallback"):
            fn(good)
        for m in ((good.vertices, good.faces.long()), (good.vertices.double(), good.faces), (good.vertices[:, :2], good.faces),
                  (torch.zeros(0, 3), good.faces), "mesh"):
            with pytest.raises(ValueError):
                fn(m)


def test_product_module_imports_neither_oracle_nor_scipy():
    src = open(os.path.join(ROOT, "ct-unet_amd", "ctunet_amd", "mesh.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(scipy|oracle)", src, flags=re.M)


# ------------------------------------------------------------------------------------------------ binary STL
def test_write_stl_byte_layout(tmp_path):
    from ctunet_amd import mesh
    # (z, y, x) vertices of a tetrahedron, wound outward in (x, y, z), and one face without area
    v = torch.tensor([[0, 0, 0], [0, 0, 2], [0, 3, 0], [4, 0, 0]], dtype=torch.float32)
    f = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3], [1, 1, 2]], dtype=torch.int32)
    path = tmp_path / "t.stl"
    mesh.write_stl(path, mesh.Mesh(v, f), header=b"ctunet test")
    raw = path.read_bytes()
    assert len(raw) == 84 + 50 * 5
    assert raw[:80] == b"ctunet test".ljust(80, b"\0")
    assert int(np.frombuffer(raw, dtype="<u4", count=1, offset=80)[0]) == 5
    rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("p", "<f4", (3, 3)), ("a", "<u2")]), offset=84)
    assert rec.dtype.itemsize == 50 and (rec["a"] == 0).all()
    assert np.array_equal(rec["p"], v.numpy()[:, ::-1][f.numpy()])                    # columns (x, y, z), winding kept
    n = np.cross(rec["p"][:, 1] - rec["p"][:, 0], rec["p"][:, 2] - rec["p"][:, 0]).astype(np.float64)
    length = np.linalg.norm(n, axis=1)
    assert np.allclose(rec["n"][:4], n[:4] / length[:4, None], atol=1e-7) and (rec["n"][4] == 0).all()
    # outward: the signed volume of the written triangles is the tetrahedron's, 2 * 3 * 4 / 6
    p = rec["p"][:4].astype(np.float64)
    assert np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0 == pytest.approx(4.0)
    assert mesh.stl_bytes(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)) == b"\0" * 84
    for hdr in (b"x" * 81, b"solid abc", "text"):
        with pytest.raises(ValueError):
            mesh.write_stl(path, mesh.Mesh(v, f), header=hdr)
    with pytest.raises(ValueError, match="does not exist"):
        mesh.write_stl(path, mesh.Mesh(v, torch.tensor([[0, 1, 4]], dtype=torch.int32)))


def test_stl_of_the_reference_mesh_round_trips(tmp_path, meshes):
    from ctunet_amd import mesh
    v, f = meshes["sphere_mask"]
    path = tmp_path / "s.stl"
    mesh.write_stl(path, mesh.Mesh(torch.from_numpy(v), torch.from_numpy(f)))
    raw = path.read_bytes()
    assert len(raw) == 84 + 50 * len(f)
    rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("p", "<f4", (3, 3)), ("a", "<u2")]), offset=84)
    p = rec["p"].astype(np.float64)
    vol = np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0
    assert vol == pytest.approx(R.area_volume(v, f)[1], rel=1e-12)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (np.einsum("ij,ij->i", n, rec["n"].astype(np.float64)) > 0).all()
