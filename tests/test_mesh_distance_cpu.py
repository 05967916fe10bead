"""Host-side checks of ctunet_amd.mesh's point-to-mesh distance: the numpy restatement (tests/mesh_distance_ref.py) against an
independent formulation (the region-based closest-point algorithm, written here and shipped nowhere) and against closed
forms, the new C-ABI symbols, the CTU_REQUIRE refusals, argument validation before anything is launched, the workspace
formula and the documents."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import mesh_distance_ref as M
import mesh_ref as R
import mesh_smooth_ref as S
import mesh_voxelize_ref as X
from test_mesh_voxelize_cpu import LEVEL, random_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ctu_mesh_grid_ws_bytes", "ctu_mesh_grid_build", "ctu_mesh_grid_emit", "ctu_mesh_distance")
SPACING, ORIGIN = (0.8, 0.45, 0.45), (-10, 3.5, 0.25)


def sphere(n, radius2):
    z, y, x = np.indices((n, n, n))
    c = (n - 1) / 2
    return ((z - c) ** 2 + (y - c) ** 2 + (x - c) ** 2 <= radius2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def base_mesh(name):
    """The three meshes the rule is pinned on: a mask's, its smoothed version, a float field's.  (vertices, faces)"""
    if name == "sphere12":
        v, f = R.extract(sphere(12, 20.0), spacing=SPACING, origin=ORIGIN)
    elif name == "sphere12_smoothed":
        v, f = base_mesh("sphere12")
        v = S.smooth(v, f)
    elif name == "field678":
        v, f = R.extract(random_field((6, 7, 8), 5), level=LEVEL, spacing=SPACING, origin=ORIGIN)
    else:
        raise KeyError(name)
    v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def queries(v, f, seed, n=200):
    """float32 [*, 3]: n points in the bounding box enlarged by 20 % per side, the first 50 vertices, the midpoints of the
    edges of the first 20 faces, and three points 100 diagonals away."""
    rng = np.random.default_rng(seed)
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    ext = np.where(hi > lo, hi - lo, 1.0)
    diag = float(np.sqrt((ext ** 2).sum()))
    box = lo - 0.2 * ext + rng.random((n, 3)) * 1.4 * ext
    tri = v[f[:20]].astype(np.float64)
    mid = np.concatenate([(tri[:, k] + tri[:, (k + 1) % 3]) / 2 for k in range(3)])
    far = lo + np.array([[100.0, 0, 0], [-100.0, 100.0, 0], [30.0, -60.0, 100.0]]) * diag
    return np.concatenate([box, v[:50].astype(np.float64), mid, far]).astype(np.float32)


def region_based_distance2(p, a, b, c):
    """The textbook closest point on a triangle by Voronoi regions (vertex, edge, interior), float64, broadcasting; the
    squared distance from p.  Independent of the rule's min-over-segments form; for triangles with area."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = p - b
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = p - c
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        t_ab, t_ac = d1 / (d1 - d3), d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = 1.0 / (va + vb + vc)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    full = np.broadcast_shapes(p.shape, a.shape)
    picks = [np.broadcast_to(a, full), np.broadcast_to(b, full), a + t_ab[..., None] * ab, np.broadcast_to(c, full),
             a + t_ac[..., None] * ac, b + t_bc[..., None] * (c - b)]
    q = a + ab * (vb * denom)[..., None] + ac * (vc * denom)[..., None]
    for cond, pick in reversed(list(zip(conds, picks))):
        q = np.where(cond[..., None], pick, q)
    return ((p - q) ** 2).sum(-1)


# ------------------------------------------------------------------------------------------------ the reference, pinned
@pytest.mark.parametrize("name", ["sphere12", "sphere12_smoothed", "field678"])
def test_the_reference_agrees_with_the_region_based_algorithm(name):
    v, f = base_mesh(name)
    n, _ = R.face_geometry(v, f)
    assert ((n * n).sum(axis=1) > 0).all()                                            # the independent form needs area
    p = queries(v, f, 11)
    diag = M.diagonal(v, p[:-3])
    d, face, close = M.point_distance(p, v, f)
    assert d.shape == (len(p),) and (face >= 0).all() and np.isfinite(close).all()
    tri = v[f].astype(np.float64)
    other = np.sqrt(region_based_distance2(p.astype(np.float64)[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]).min(axis=1))
    gap = np.abs(d - other)
    print(f"{name}: largest disagreement {gap[:-3].max() / diag:.2e} of the diagonal near, {(gap[-3:] / d[-3:]).max():.2e} relative far")
    assert (gap[:-3] <= 1e-12 * diag).all()
    assert (gap[-3:] <= 1e-12 * d[-3:]).all()                                         # 100 diagonals away: relative to the distance
    # the closest point lies on the face's plane side at that distance, and a vertex is at distance 0 from its own mesh
    assert np.allclose(np.sqrt(((p.astype(np.float64) - close) ** 2).sum(axis=1)), d, rtol=1e-12, atol=1e-12 * diag)
    assert (d[200:250] == 0).all()


def test_the_reference_on_closed_forms_and_degenerate_faces():
    v, f = X.cube_mesh()                                                             # corners at 0.5 and 4.5
    rng = np.random.default_rng(3)
    p = (rng.random((500, 3)) * 12.0 - 3.5).astype(np.float32)
    d, face, close = M.point_distance(p, v, f)
    pd = p.astype(np.float64)
    gap = np.maximum(np.maximum(0.5 - pd, pd - 4.5), 0.0)
    outside = (gap > 0).any(axis=1)
    assert outside.sum() > 100 and (~outside).sum() > 10
    assert np.abs(d[outside] - np.sqrt((gap[outside] ** 2).sum(axis=1))).max() <= 1e-14
    inside = np.minimum(pd - 0.5, 4.5 - pd).min(axis=1)
    assert np.abs(d[~outside] - inside[~outside]).max() <= 1e-14
    # faces without area are their segments and change nothing where they lie on the surface or inside it is farther
    seg = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 3.0], [1.0, 1.0, 2.0], [7.0, 7.0, 7.0]], dtype=np.float32)
    for tri in ([0, 1, 1], [0, 0, 1], [0, 1, 2], [1, 0, 1]):                          # repeated indices and collinear corners
        dd, ff, cc = M.point_distance(np.array([[1.0, 2.0, 2.5], [1.0, 1.0, 5.0], [1.0, 1.0, 1.5]], np.float32), seg, [tri])
        assert np.array_equal(dd, [1.0, 2.0, 0.0]) and np.array_equal(ff, [0, 0, 0])
        assert np.array_equal(cc, [[1.0, 1.0, 2.5], [1.0, 1.0, 3.0], [1.0, 1.0, 1.5]])
    dd, _, cc = M.point_distance(np.array([[7.0, 4.0, 3.0]], np.float32), seg, [[3, 3, 3]])      # a point
    assert dd[0] == 5.0 and np.array_equal(cc[0], [7.0, 7.0, 7.0])
    # ties go to the lowest face index; max_distance cuts strictly beyond it; what is not finite stays apart
    dd, ff, _ = M.point_distance(np.array([[0.5, 0.5, 0.5], [2.5, 2.5, -1.5], [np.nan, 0, 0], [0, np.inf, 0]], np.float32), v, f, max_distance=2.0)
    assert np.array_equal(dd[:2], [0.0, 2.0]) and ff[0] == 0 and ff[1] >= 0
    assert np.isnan(dd[2:]).all() and (ff[2:] == -1).all()
    dd, ff, cc = M.point_distance(np.array([[2.5, 2.5, -1.5]], np.float32), v, f, max_distance=1.999)
    assert np.isinf(dd[0]) and ff[0] == -1 and np.isnan(cc).all()
    dd, ff, _ = M.point_distance(p[:4], np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert np.isinf(dd).all() and (ff == -1).all()
    with pytest.raises(ValueError):
        M.point_distance(p[:4], v, [[0, 1, 8]])
    bad = v.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        M.point_distance(p[:4], bad, f)
    field = M.distance_field(v, f, (6, 6, 6), max_distance=1.25)
    assert field.shape == (6, 6, 6) and field.max() == 1.25 and field[2, 2, 2] == 1.25 and field[1, 1, 1] == 0.5 and field[0, 3, 3] == 0.5


def test_smoothing_moves_the_sphere_by_less_than_a_voxel():
    """The bound of the pipeline test in test_mesh_distance_gpu.py, verified on the reference."""
    v, f = R.extract(sphere(16, 36.0), spacing=SPACING)
    d, _, _ = M.point_distance(S.smooth(v, f), v, f)
    print(f"deviation of the smoothed 16^3 sphere: max {d.max():.4f}, mean {d.mean():.4f} (largest spacing {max(SPACING)})")
    assert 0 < d.max() < max(SPACING) and np.isfinite(d).all()


# ------------------------------------------------------------------------------------------------ the module's host side
def test_symbols_in_header_table_and_library():
    from ctunet_amd import _lib, mesh, metrics
    header = open(os.path.join(ROOT, "include", "ctunet_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.load().ctu_abi_version() == _lib.ABI_VERSION == 8
    assert re.search(r"#define\s+CTU_MESH_GRID_MAX_CELLS\s+%d\b" % mesh.MAX_CELLS, header)
    for fn in ("build_face_grid", "point_distance", "distance_field", "distance_workspace_bytes"):
        assert callable(getattr(mesh, fn))
    assert callable(metrics.mesh_surface_metrics)
    assert mesh.FaceGrid._fields == ("offsets", "faces", "corners", "frame", "dims", "cell_size")


def test_workspace_bytes_match_the_documentation():
    from ctunet_amd import _lib, mesh
    lib = _lib.load()
    a256 = lambda n: -(-n // 256) * 256
    for F in (1, 12, 1000, 1024, 1025, 300000, (1 << 31) - 1):
        cap = min(1 << 24, max(65536, 64 * F))
        want = 256 + a256(64 * -(-F // 256)) + 2 * a256(4 * cap) + a256(8 * -(-cap // 4096))
        assert lib.ctu_mesh_grid_ws_bytes(F, cap) == want
        assert mesh.distance_workspace_bytes(8, F) == mesh.distance_workspace_bytes(8, F, cell_size=0.5) == want
    assert mesh.distance_workspace_bytes(0, 0) == 0
    assert lib.ctu_mesh_grid_ws_bytes(12, 0) == lib.ctu_mesh_grid_ws_bytes(12, (1 << 24) + 1) == lib.ctu_mesh_grid_ws_bytes(-1, 64) == 0
    assert lib.ctu_mesh_grid_ws_bytes(1 << 31, 64) == 0
    for V, F in ((-1, 4), (4, -1), (1 << 31, 4), (4, 1 << 31), (True, 4), (4.0, 4)):
        with pytest.raises(ValueError, match="distance_workspace_bytes"):
            mesh.distance_workspace_bytes(V, F)
    for bad in (0, -1.0, float("inf"), float("nan"), "a", 1e-60):
        with pytest.raises(ValueError, match="cell_size"):
            mesh.distance_workspace_bytes(8, 12, cell_size=bad)


def test_c_entry_points_refuse_bad_arguments():
    """CTU_REQUIRE fires before any launch, so these calls need no GPU; the message comes through ctu_last_error."""
    from ctunet_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) // 16 * 16 + 16
    f3 = lambda *v: (ctypes.c_float * 3)(*v)

    def err(status):
        assert status == -1
        return lib.ctu_last_error().decode()

    def build(vert=p, V=8, faces=p, F=12, size=0.0, cap=65536, corners=p, ws=p):
        return lib.ctu_mesh_grid_build(vert, V, faces, F, size, cap, corners, ws, None)

    assert "2^31" in err(build(V=1 << 31))
    assert "2^31" in err(build(F=1 << 31))
    assert "2^31" in err(build(F=0))
    assert "2^31" in err(build(V=-1))
    assert "without vertices" in err(build(V=0))
    assert "max_cells" in err(build(cap=0))
    assert "max_cells" in err(build(cap=(1 << 24) + 1))
    for size in (-1.0, float("inf"), float("nan")):
        assert "cell_size" in err(build(size=size))
    for kw in (dict(vert=None), dict(faces=None), dict(corners=None), dict(ws=None)):
        assert "null" in err(build(**kw))
    assert "aligned" in err(build(ws=p + 4))
    assert "aligned" in err(build(corners=p + 8))

    def emit(corners=p, F=12, cap=65536, cells=8, pairs=40, offsets=p, items=p, ws=p):
        return lib.ctu_mesh_grid_emit(corners, F, cap, cells, pairs, offsets, items, ws, None)

    assert "2^31" in err(emit(F=0))
    assert "cells" in err(emit(cells=0))
    assert "cells" in err(emit(cells=65537))
    assert "cells" in err(emit(cap=(1 << 24) + 1))
    assert "cell_size" in err(emit(pairs=1 << 31))
    assert "pairs" in err(emit(pairs=-1))
    for kw in (dict(corners=None), dict(offsets=None), dict(items=None), dict(ws=None)):
        assert "null" in err(emit(**kw))
    assert "aligned" in err(emit(ws=p + 4))

    def query(corners=p, F=12, offsets=p, items=p, pairs=40, frame=p, dims=(2, 2, 2), points=p, Q=5, shape=(0, 0, 0), sp=None,
              org=None, md=0.0, far=float("inf"), dist=p, face=None, closest=None):
        return lib.ctu_mesh_distance(corners, F, offsets, items, pairs, frame, *dims, points, Q, *shape, sp, org, md, far, dist, face,
                                     closest, None)

    assert "2^31" in err(query(F=0))
    assert "2^31" in err(query(pairs=1 << 31))
    assert "face grid" in err(query(dims=(0, 2, 2)))
    assert "face grid" in err(query(dims=(4096, 4096, 2)))
    for md in (-1.0, float("inf"), float("nan")):
        assert "max_distance" in err(query(md=md))
    assert "Q must" in err(query(Q=-1))
    assert "Q must" in err(query(Q=1 << 31))
    assert "bad shape" in err(query(points=None, shape=(0, 4, 4)))
    assert "bad shape" in err(query(points=None, shape=(4, 1025, 4)))
    for sp in (f3(0, 1, 1), f3(1, -1, 1), f3(1, 1, float("inf")), f3(float("nan"), 1, 1)):
        assert "spacing" in err(query(points=None, shape=(4, 4, 4), sp=sp))
    for org in (f3(0, float("inf"), 0), f3(0, 0, float("nan"))):
        assert "origin" in err(query(points=None, shape=(4, 4, 4), org=org))
    for kw in (dict(corners=None), dict(offsets=None), dict(items=None), dict(frame=None), dict(dist=None)):
        assert "null" in err(query(**kw))
    assert "aligned" in err(query(corners=p + 4))
    assert query(Q=0) == 0                                                           # no query: nothing to launch


def test_argument_validation_raises_before_any_launch():
    from ctunet_amd import mesh, metrics
    v, f = (torch.from_numpy(a) for a in X.cube_mesh())
    m = mesh.Mesh(v, f)
    pts = torch.zeros((5, 3))
    empty = mesh.Mesh(torch.zeros(0, 3), torch.zeros((0, 3), dtype=torch.int32))
    # point_distance
    for bad in (pts.double(), torch.zeros(5, 2), torch.zeros(5), "points", pts.to("meta")):
        with pytest.raises(ValueError, match="points"):
            mesh.point_distance(bad, m)
    for md in (0, -1.0, float("inf"), float("nan"), "a", True, 1e39, 1e-60):
        with pytest.raises(ValueError, match="max_distance"):
            mesh.point_distance(pts, m, max_distance=md)
    for cs in (0, -1.0, float("inf"), "a", True):
        with pytest.raises(ValueError, match="cell_size"):
            mesh.point_distance(pts, m, cell_size=cs)
        with pytest.raises(ValueError, match="cell_size"):
            mesh.build_face_grid(m, cell_size=cs)
    with pytest.raises(ValueError, match="FaceGrid"):
        mesh.point_distance(pts, m, grid=(v, f))
    grid = mesh.FaceGrid(torch.zeros(2, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros((12, 12)),
                         torch.zeros(6, dtype=torch.float64), (1, 1, 1), 1.0)
    with pytest.raises(ValueError, match="not both"):
        mesh.point_distance(pts, m, grid=grid, cell_size=1.0)
    for broken, match in ((grid._replace(corners=torch.zeros((11, 12))), "another mesh"), (grid._replace(dims=(1, 2, 1)), "dims"),
                          (grid._replace(dims=(1, 1)), "dims"), (grid._replace(dims=(0, 1, 1)), "dims"),
                          (grid._replace(offsets=torch.zeros(2, dtype=torch.int64)), "int32"),
                          (grid._replace(frame=torch.zeros(6)), "frame"), (grid._replace(frame=torch.zeros(5, dtype=torch.float64)), "frame"),
                          (grid._replace(faces=torch.zeros(0, dtype=torch.int32, device="meta")), "device")):
        with pytest.raises(ValueError, match=match):
            mesh.point_distance(pts, m, grid=broken)
        with pytest.raises(ValueError, match=match):
            mesh.distance_field(m, (6, 6, 6), max_distance=1.0, grid=broken)
    for kw in (dict(), dict(max_distance=2.0, return_faces=True, return_points=True), dict(grid=grid), dict(cell_size=0.5)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            mesh.point_distance(pts, m, **kw)
    with pytest.raises(ValueError, match="no CPU fallback"):
        mesh.point_distance(torch.zeros((0, 3)), empty)
    with pytest.raises(ValueError, match="no CPU fallback"):
        mesh.build_face_grid(m)
    # distance_field: voxelize's grid validation, and max_distance is required
    bad = [(dict(shape=(6, 6)), "triple"), (dict(shape=(6, 0, 6)), "every side"), (dict(shape=(6, 6, 1025)), "every side"),
           (dict(shape=(6, 6, 6), spacing=0), "spacing"), (dict(shape=(6, 6, 6), spacing=(1, -1, 1)), "spacing"),
           (dict(shape=(6, 6, 6), origin=(0, 0)), "origin"), (dict(shape=(6, 6, 6), origin=float("inf")), "origin")]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            mesh.distance_field(m, max_distance=1.0, **kw)
    with pytest.raises(ValueError, match="max_distance"):
        mesh.distance_field(m, (6, 6, 6))
    for md in (None, 0, -1.0, float("inf"), "a"):
        with pytest.raises(ValueError, match="max_distance"):
            mesh.distance_field(m, (6, 6, 6), max_distance=md)
    for kw in (dict(), dict(signed=True), dict(spacing=SPACING, origin=ORIGIN), dict(grid=grid)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            mesh.distance_field(m, (6, 6, 6), max_distance=1.0, **kw)
    # every function checks the mesh and its limits first
    big_v = mesh.Mesh(torch.empty((1 << 31, 3), device="meta"), torch.empty((1, 3), dtype=torch.int32, device="meta"))
    big_f = mesh.Mesh(torch.empty((4, 3), device="meta"), torch.empty((1 << 31, 3), dtype=torch.int32, device="meta"))
    for fn in (lambda x: mesh.point_distance(pts, x), lambda x: mesh.distance_field(x, (6, 6, 6), max_distance=1.0), mesh.build_face_grid):
        for broken in ((v, f.long()), (v.double(), f), (v[:, :2], f), (torch.zeros(0, 3), f), "mesh"):
            with pytest.raises(ValueError):
                fn(broken)
        for big in (big_v, big_f):
            with pytest.raises(ValueError, match="2\\^31"):
                fn(big)
    with pytest.raises(ValueError, match="2\\^31"):
        mesh.point_distance(torch.empty((1 << 31, 3), device="meta"), mesh.Mesh(v.to("meta"), f.to("meta")))
    # mesh_surface_metrics
    for kw, match in ((dict(percentile=101), "percentile"), (dict(tolerance=-1.0), "tolerance"), (dict(tolerance=float("nan")), "tolerance")):
        with pytest.raises(ValueError, match=match):
            metrics.mesh_surface_metrics(m, m, **kw)
    with pytest.raises(ValueError):
        metrics.mesh_surface_metrics(m, "mesh")
    with pytest.raises(ValueError, match="different devices"):
        metrics.mesh_surface_metrics(m, mesh.Mesh(v.to("meta"), f.to("meta")))
    for a, b in ((m, m), (empty, m), (empty, empty)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            metrics.mesh_surface_metrics(a, b, tolerance=1.0)


def test_documents_state_the_rule_and_the_pipeline_lines():
    from ctunet_amd import mesh, metrics
    doc = mesh.__doc__
    for phrase in ("tests/mesh_distance_ref.py", "minimum over its three edge segments", "((p-a) . n)^2 / |n|^2", "lowest face index",
                   "does not depend on the cell size", "min(2^24, max(65536, 64 F))", "mesh.point_distance(mesh.smooth(m).vertices, m)",
                   "mesh.distance_field(other, scan.shape", "Out of scope: decimation, formats other than binary STL, marching cubes."):
        assert phrase in doc, phrase
    assert not re.search(r"Out of scope of voxelisation:[^\n]*signed distance", doc)
    assert "unweighted" in metrics.mesh_surface_metrics.__doc__ and "vertices" in metrics.mesh_surface_metrics.__doc__
    assert "grows with the distance" in mesh.point_distance.__doc__ and "grows with the distance" in doc
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "mesh.point_distance(mesh.smooth(m).vertices, m)" in readme and "mesh.distance_field(" in readme and "signed=True" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Distance to a mesh" in design and "profiles/mesh_distance.md" in design
    assert os.path.exists(os.path.join(ROOT, "profiles", "mesh_distance.md"))
