"""ctunet_amd.mesh.point_distance, distance_field and build_face_grid and metrics.mesh_surface_metrics on the GPU: against the
brute-force numpy reference (tests/mesh_distance_ref.py) on small meshes, independence of the face grid (bit-equal results
under four cell sizes, no reference needed), a closed form at 100 000 points, max_distance, the truncated and signed field,
refusals, the metrics against numpy and the pipeline line.

The bound against the reference, with diag the diagonal of the joint bounding box of mesh and queries:
|dev - ref| <= np.spacing(float32(ref)) + 1e-12 diag, and exactly 0 where the reference is exactly 0 (mesh_distance_ref.tolerance).
The first term is the one float32 rounding of the result; the second is 10^4 times the float64 disagreement between two
formulations of the rule (1e-16 diag, test_mesh_distance_cpu.py).  Neither can hide a wrong face: neighbours differ by far more."""
import functools

import numpy as np
import pytest
import torch

import mesh_distance_ref as M
import mesh_ref as R
import mesh_smooth_ref as S
import mesh_voxelize_ref as X
from test_mesh_distance_cpu import SPACING, base_mesh, queries, sphere
from test_mesh_voxelize_cpu import degenerate_faces

pytestmark = pytest.mark.gpu

NOT_FINITE = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [-np.inf, np.nan, 1.0]], dtype=np.float32)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                           # a copy: the cached cases are read-only


def _spanning():
    """The sphere and one triangle across its whole box: a face listed in many cells."""
    v, f = base_mesh("sphere12")
    lo, hi = v.min(axis=0), v.max(axis=0)
    big = np.array([lo, [hi[0], hi[1], lo[2]], [lo[0], hi[1], hi[2]]], dtype=np.float32)
    return np.concatenate([v, big]), np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)


MESHES = {
    "sphere12": lambda: base_mesh("sphere12"),
    "sphere12_smoothed": lambda: base_mesh("sphere12_smoothed"),
    "field678": lambda: base_mesh("field678"),
    "cube": X.cube_mesh,
    "cube_degenerate": lambda: degenerate_faces(*X.cube_mesh()),
    "flat_triangle": lambda: (np.array([[2.0, 1.0, 1.0], [2.0, 4.0, 1.0], [2.0, 1.0, 4.0]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)),
    "coincident": lambda: (np.full((3, 3), 1.25, dtype=np.float32), np.array([[0, 1, 2], [2, 1, 0]], dtype=np.int32)),
    "sphere12_spanning": _spanning,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices, faces, queries) on the host; the queries end with the points that are not finite."""
    v, f = MESHES[name]()
    v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)
    p = np.concatenate([queries(v, f, 7 + sorted(MESHES).index(name)), NOT_FINITE])
    for a in (v, f, p):
        a.setflags(write=False)
    return v, f, p


@functools.lru_cache(maxsize=None)
def reference(name):
    v, f, p = case(name)
    out = M.point_distance(p, v, f)
    for a in out:
        a.setflags(write=False)
    return out


def device_mesh(name):
    from ctunet_amd import mesh
    v, f, _ = case(name)
    return mesh.Mesh(dev(v), dev(f))


def assert_within(got, ref, diag, what=""):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref)), what
    fin = np.isfinite(ref)
    err, tol = np.abs(got[fin] - ref[fin]), M.tolerance(ref[fin], diag)
    rounded = int((got[fin] != ref[fin].astype(np.float32)).sum())
    print(f"{what}: largest error {err.max(initial=0):.3e}, {rounded} of {int(fin.sum())} differ from float32(ref)")
    assert (err <= tol).all(), what


def bits(t):
    return t.cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.int32)


@pytest.mark.parametrize("name", sorted(MESHES))
def test_against_the_reference(name):
    from ctunet_amd import mesh
    v, f, p = case(name)
    ref, _, _ = reference(name)
    diag = M.diagonal(v, p)
    m = device_mesh(name)
    d, face, close = mesh.point_distance(dev(p), m, return_faces=True, return_points=True)
    assert d.dtype == torch.float32 and face.dtype == torch.int32 and close.dtype == torch.float32
    assert tuple(d.shape) == (len(p),) and tuple(face.shape) == (len(p),) and tuple(close.shape) == (len(p), 3) and d.is_cuda
    d, face, close = d.cpu().numpy(), face.cpu().numpy(), close.cpu().numpy()
    assert_within(d, ref, diag, name)
    # what is not finite: NaN, -1, NaN
    assert np.isnan(d[-3:]).all() and (face[-3:] == -1).all() and np.isnan(close[-3:]).all()
    ok = slice(0, len(p) - 3)
    assert ((face[ok] >= 0) & (face[ok] < len(f))).all()
    # the returned face lies at the returned distance (ties make the index itself free)
    tri = v[f[face[ok]]].astype(np.float64)
    d2, _ = M.face_distance2(p[ok].astype(np.float64), tri[:, 0], tri[:, 1], tri[:, 2])
    assert_within(d[ok], np.sqrt(d2), diag, name + ": the returned face")
    # and so does the returned closest point, up to the rounding of its three coordinates to float32
    there = np.sqrt(((p[ok].astype(np.float64) - close[ok].astype(np.float64)) ** 2).sum(axis=1))
    rounding = np.sqrt(((0.5 * np.spacing(np.abs(close[ok]))).astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(there - d[ok]) <= np.spacing(d[ok]) + 1e-12 * diag + rounding).all()
    assert np.array_equal(bits(mesh.point_distance(dev(p), m)), d.view(np.uint32))           # the plain call: one tensor


@pytest.mark.parametrize("name", sorted(MESHES))
def test_the_result_does_not_depend_on_the_grid(name):
    """The test of the search bound: the default cell size, a quarter of it, four times it and one cell (brute force)."""
    from ctunet_amd import mesh
    v, f, p = case(name)
    m, pts = device_mesh(name), dev(p)
    g = mesh.build_face_grid(m)
    assert isinstance(g, mesh.FaceGrid) and g.cell_size > 0 and g.offsets.shape[0] == g.dims[0] * g.dims[1] * g.dims[2] + 1
    assert int(g.offsets[-1]) == g.faces.shape[0] >= len(f) and g.corners.shape == (len(f), 12)
    base = mesh.point_distance(pts, m, return_faces=True, return_points=True)
    dims = {g.dims}
    for kw in (dict(cell_size=g.cell_size / 4), dict(cell_size=g.cell_size * 4), dict(cell_size=1e30), dict(grid=g), dict()):
        if "cell_size" in kw:
            dims.add(mesh.build_face_grid(m, **kw).dims)
        got = mesh.point_distance(pts, m, return_faces=True, return_points=True, **kw)
        for a, b in zip(base, got):
            assert np.array_equal(bits(a), bits(b)), kw
    assert mesh.build_face_grid(m, cell_size=1e30).dims == (1, 1, 1)
    if name.startswith(("sphere", "field")):
        assert len(dims) == 4                                                        # four different grids were searched
    # a planar mesh, a single triangle, coinciding vertices: an axis without extent has one cell
    if name == "flat_triangle":
        assert g.dims[0] == 1 and mesh.build_face_grid(m, cell_size=0.5).dims == (1, 7, 7)
    if name == "coincident":
        assert g.dims == (1, 1, 1) and mesh.build_face_grid(m, cell_size=1e-3).dims == (1, 1, 1)


@pytest.mark.parametrize("q", [0, 1, 65])
def test_few_queries(q):
    from ctunet_amd import mesh
    v, f, p = case("sphere12")
    ref, _, _ = reference("sphere12")
    m = device_mesh("sphere12")
    d, face, close = mesh.point_distance(dev(p[:q]), m, return_faces=True, return_points=True)
    assert tuple(d.shape) == (q,) and tuple(face.shape) == (q,) and tuple(close.shape) == (q, 3)
    assert_within(d.cpu().numpy(), ref[:q], M.diagonal(v, p), f"Q = {q}")
    view = dev(np.concatenate([p[:q], p[:q]], axis=1))[:, 3:]                        # a non-contiguous view is copied
    assert q <= 1 or not view.is_contiguous()                                        # one row of a wider tensor counts as contiguous
    assert np.array_equal(bits(mesh.point_distance(view, m)), bits(d))


def test_analytic_box_distance_at_size():
    """100 000 points around the cube against the closed form for points outside the box: 391 blocks, a partial last wave."""
    from ctunet_amd import mesh
    v, f = X.cube_mesh()                                                             # corners at 0.5 and 4.5
    rng = np.random.default_rng(17)
    p = (rng.random((100000, 3)) * 14.0 - 4.5).astype(np.float32)
    pd = p.astype(np.float64)
    gap = np.maximum(np.maximum(0.5 - pd, pd - 4.5), 0.0)
    outside = (gap > 0).any(axis=1)
    want = np.sqrt((gap ** 2).sum(axis=1))
    m = mesh.Mesh(dev(v), dev(f))
    d = mesh.point_distance(dev(p), m).cpu().numpy()
    assert outside.sum() > 90000 and np.isfinite(d).all()
    assert_within(d[outside], want[outside], M.diagonal(v, p), "box")
    inside = np.minimum(pd - 0.5, 4.5 - pd).min(axis=1)
    assert_within(d[~outside], inside[~outside], M.diagonal(v, p), "inside the box")
    assert np.array_equal(d.view(np.uint32), bits(mesh.point_distance(dev(p), m, cell_size=1.0)))


def test_max_distance():
    from ctunet_amd import mesh
    v, f, p = case("sphere12_smoothed")
    ref, _, _ = reference("sphere12_smoothed")
    diag = M.diagonal(v, p)
    fin = np.isfinite(ref)
    cap = float(np.float32(0.7))
    assert (np.abs(ref[fin] - cap) > 1e-9 * diag).all()                               # no query sits on the cap
    far = fin & (ref > cap)
    assert 20 < far.sum() < fin.sum() - 20
    m, pts = device_mesh("sphere12_smoothed"), dev(p)
    free = mesh.point_distance(pts, m, return_faces=True, return_points=True)
    for kw in (dict(), dict(cell_size=0.1), dict(cell_size=1e30), dict(grid=mesh.build_face_grid(m))):
        d, face, close = mesh.point_distance(pts, m, max_distance=cap, return_faces=True, return_points=True, **kw)
        dn, fn, cn = d.cpu().numpy(), face.cpu().numpy(), close.cpu().numpy()
        assert np.isposinf(dn[far]).all() and (fn[far] == -1).all() and np.isnan(cn[far]).all()
        near = fin & ~far
        for a, b in zip(free, (d, face, close)):                                     # the nearer queries: unchanged bit for bit
            assert np.array_equal(bits(a)[near], bits(b)[near])
        assert np.isnan(dn[~fin]).all() and (fn[~fin] == -1).all()


FIELD_GRID = dict(shape=(9, 10, 11), spacing=(0.7, 0.5, 0.45), origin=(-10.5, 3.2, 0.1))


def test_distance_field():
    from ctunet_amd import mesh
    v, f, _ = case("sphere12")
    m = device_mesh("sphere12")
    cap = 1.5
    ref = M.distance_field(v, f, max_distance=cap, **FIELD_GRID)
    centres = M.grid_centres(**FIELD_GRID)
    diag = M.diagonal(v, centres)
    d = mesh.distance_field(m, max_distance=cap, **FIELD_GRID)
    assert d.dtype == torch.float32 and tuple(d.shape) == FIELD_GRID["shape"] and d.is_contiguous() and d.is_cuda
    dn = d.cpu().numpy()
    assert_within(dn, ref, diag, "field")
    truncated = ref == cap
    assert 50 < truncated.sum() < ref.size - 50 and (dn[truncated] == np.float32(cap)).all() and dn.max() == np.float32(cap)
    assert np.array_equal(bits(d), bits(mesh.distance_field(m, max_distance=cap, grid=mesh.build_face_grid(m, cell_size=0.3), **FIELD_GRID)))
    # the sign: positive outside, negative inside, by the winding number
    w = X.winding_number(v, f, FIELD_GRID["shape"], FIELD_GRID["spacing"], FIELD_GRID["origin"])
    assert 20 < (w != 0).sum() < w.size - 20
    s = mesh.distance_field(m, max_distance=cap, signed=True, **FIELD_GRID).cpu().numpy()
    assert np.array_equal(s, np.where(w != 0, -dn, dn)) and (s[w != 0] <= 0).all() and (s[w == 0] >= 0).all()
    # centres that float32 represents exactly: the field is point_distance at those points, bit for bit
    grid = dict(shape=(9, 10, 11), spacing=0.5, origin=0.25)
    sm = device_mesh("cube")
    c32 = M.grid_centres(**grid).astype(np.float32)
    assert np.array_equal(c32.astype(np.float64), M.grid_centres(**grid))
    a = mesh.distance_field(sm, max_distance=1.0, **grid)
    b = mesh.point_distance(dev(c32), sm, max_distance=1.0)
    assert 0 < int(torch.isinf(b).sum()) < b.numel()                                 # the cube's core is farther than 1
    b = torch.where(torch.isinf(b), torch.full_like(b, 1.0), b)
    assert np.array_equal(bits(a).reshape(-1), bits(b))


@pytest.mark.parametrize("bad", ["minus_one", "V", "int_min", "nan", "inf"])
def test_refused_faces_raise_and_leave_no_fault_behind(bad):
    from ctunet_amd import mesh
    v, f, p = case("sphere12")
    v, f = v.copy(), f.copy()
    k = len(f) // 2
    if bad in ("nan", "inf"):
        v[f[k, 1], 2] = np.nan if bad == "nan" else np.inf
        count = int((f == f[k, 1]).any(axis=1).sum())
    else:
        f[k, 2] = {"minus_one": -1, "V": len(v), "int_min": -(1 << 31)}[bad]
        count = 1
    m = mesh.Mesh(dev(v), dev(f))
    for call in (lambda: mesh.point_distance(dev(p), m), lambda: mesh.build_face_grid(m, cell_size=2.0),
                 lambda: mesh.distance_field(m, (4, 4, 4), max_distance=1.0)):
        with pytest.raises(ValueError, match=rf"does not exist or is not finite \({count} of {len(f)} faces"):
            call()
    good = mesh.point_distance(dev(p), device_mesh("sphere12"))
    assert_within(good.cpu().numpy(), reference("sphere12")[0], M.diagonal(case("sphere12")[0], p), "after a refusal")


def test_limits_and_empty_meshes():
    from ctunet_amd import mesh
    m = device_mesh("sphere12")
    _, _, p = case("sphere12")
    with pytest.raises(ValueError, match="cell_size"):                               # more cells than the cap
        mesh.build_face_grid(m, cell_size=1e-3)
    with pytest.raises(ValueError, match="cell_size"):
        mesh.point_distance(dev(p), m, cell_size=1e-3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        mesh.point_distance(torch.from_numpy(p.copy()), mesh.Mesh(m.vertices.cpu(), m.faces.cpu()))
    with pytest.raises(ValueError, match="lives on|live on"):
        mesh.point_distance(torch.from_numpy(p.copy()), m)
    empty = mesh.Mesh(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    no_faces = mesh.Mesh(torch.ones((5, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    for e in (empty, no_faces):
        d, face, close = mesh.point_distance(dev(p), e, return_faces=True, return_points=True)
        dn = d.cpu().numpy()
        assert np.isposinf(dn[:-3]).all() and np.isnan(dn[-3:]).all() and (face == -1).all() and torch.isnan(close).all()
        field = mesh.distance_field(e, (3, 4, 5), max_distance=2.5)
        assert field.shape == (3, 4, 5) and (field == 2.5).all()
        g = mesh.build_face_grid(e)
        assert g.dims == (1, 1, 1) and g.faces.shape[0] == 0
        assert torch.isposinf(mesh.point_distance(dev(p[:5]), e, grid=g)).all()


def test_what_the_calls_allocate():
    from ctunet_amd import mesh
    v, f, p = case("sphere12")
    m, pts = device_mesh("sphere12"), dev(p)
    g = mesh.build_face_grid(m)
    mesh.point_distance(pts, m, grid=g)
    torch.cuda.synchronize()
    key = "requested_bytes.all.allocated"
    t0 = torch.cuda.memory_stats()[key]
    g2 = mesh.build_face_grid(m)
    t1 = torch.cuda.memory_stats()[key]
    d = mesh.point_distance(pts, m, grid=g)
    t2 = torch.cuda.memory_stats()[key]
    out = mesh.point_distance(pts, m, grid=g, return_faces=True, return_points=True)
    t3 = torch.cuda.memory_stats()[key]
    cells = g.dims[0] * g.dims[1] * g.dims[2]
    assert g2.dims == g.dims and g2.faces.shape == g.faces.shape
    assert t1 - t0 == mesh.distance_workspace_bytes(len(v), len(f)) + 48 * len(f) + 4 * (cells + 1) + 4 * g.faces.shape[0] + 48
    assert t2 - t1 == 4 * len(p) and t3 - t2 == 20 * len(p)
    assert np.array_equal(bits(d), bits(out[0]))


def test_mesh_surface_metrics():
    from ctunet_amd import mesh, metrics
    va, fa = base_mesh("sphere12")
    vb, fb = base_mesh("sphere12_smoothed")
    vb = (vb + np.float32(0.15)).astype(np.float32)                                  # moved, so that the two directions differ
    a, b = mesh.Mesh(dev(va), dev(fa)), mesh.Mesh(dev(vb), dev(fb))
    dab = M.point_distance(va, vb, fb)[0].astype(np.float32).astype(np.float64)      # the rule rounds to float32 once
    dba = M.point_distance(vb, va, fa)[0].astype(np.float32).astype(np.float64)
    both = np.concatenate([dab, dba])
    diag = M.diagonal(va, vb)
    tau = 0.2
    assert (np.abs(both - tau) > 1e-6).all() and 0.1 < (both <= tau).mean() < 0.9
    got = metrics.mesh_surface_metrics(a, b, percentile=95.0, tolerance=tau)
    assert set(got) == {"hd", "hd_p", "assd", "nsd"}
    assert all(t.dtype == torch.float32 and t.is_cuda and t.dim() == 0 for t in got.values())
    want = {"hd": max(dab.max(), dba.max()), "hd_p": max(np.percentile(dab, 95.0), np.percentile(dba, 95.0)), "assd": both.mean()}
    for key, w in want.items():
        print(f"{key}: {got[key].item():.7f} against {w:.7f}")
        # every distance within the bound of the reference, so is a maximum, an order statistic or a mean of them; then one rounding
        assert abs(got[key].item() - w) <= 2 * np.spacing(np.float32(w)) + 1e-12 * diag, key
    assert got["nsd"].item() == np.float32((both <= tau).mean())
    assert want["hd_p"] < want["hd"] and metrics.mesh_surface_metrics(a, b, percentile=100.0)["hd_p"].item() == got["hd"].item()
    assert "nsd" not in metrics.mesh_surface_metrics(a, b) and torch.isnan(metrics.mesh_surface_metrics(a, b, percentile=None)["hd_p"])
    again = metrics.mesh_surface_metrics(a, b, tolerance=tau, grid_a=mesh.build_face_grid(a), grid_b=mesh.build_face_grid(b, cell_size=0.5))
    assert all(got[k].item() == again[k].item() for k in got)
    same = metrics.mesh_surface_metrics(a, a, tolerance=0.0)
    assert same["hd"].item() == 0 and same["hd_p"].item() == 0 and same["assd"].item() == 0 and same["nsd"].item() == 1
    empty = mesh.Mesh(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    for x, y, nsd in ((a, empty, 0.0), (empty, a, 0.0), (empty, empty, float("nan"))):
        r = metrics.mesh_surface_metrics(x, y, tolerance=tau)
        assert all(torch.isnan(r[k]) for k in ("hd", "hd_p", "assd"))
        assert torch.isnan(r["nsd"]) if nsd != nsd else r["nsd"].item() == nsd


def test_smoothing_moves_the_surface_by_less_than_a_voxel():
    """The pipeline line: the deviation of mesh.smooth(m) from m for the 16^3 sphere is finite, positive and below the largest
    voxel spacing (the reference gives 0.123 at most against a spacing of 0.8: test_mesh_distance_cpu.py)."""
    from ctunet_amd import mesh
    m = mesh.extract_surface(dev(sphere(16, 36.0)), spacing=SPACING)
    d = mesh.point_distance(mesh.smooth(m).vertices, m)
    print(f"deviation of the smoothed sphere: max {d.max().item():.4f}, mean {d.mean().item():.4f}")
    assert torch.isfinite(d).all() and 0 < d.max().item() < max(SPACING)
