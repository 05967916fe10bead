"""ctunet_amd.mesh on the GPU against tests/mesh_ref.py: faces bit for bit (same order), vertices bit for bit for masks, the
topology of the device result itself, measure / face_normals, hygiene (repeatability, streams, views, workspace) and the
pipeline's last step end to end (implant -> mesh -> STL)."""
import functools

import numpy as np
import pytest
import torch

import mesh_ref as R
from test_mesh_cpu import sphere_field, torus_mask, _grid

pytestmark = pytest.mark.gpu

SPACING, ORIGIN = (0.8, 0.45, 0.45), (-10, 3.5, 0.25)
# (31, 33, 3): (D+1)(H+1) = 1088 cell rows exceed mesh.SCAN_BLOCK = CTU_MESH_SCAN_BLOCK = 1024 threads of the scan, so
# a thread scans more than one row (the second scan level; (40, 48, 72) has 2009 rows and does too).
# (9, 10, 48): W is a multiple of 16, the only shape whose uint8 rows take the 16-byte loads.
SHAPES = [(1, 1, 1), (1, 1, 70), (3, 5, 130), (17, 33, 65), (40, 48, 72), (31, 33, 3), (9, 10, 48)]
KINDS = ["r02", "r50", "r98", "zeros", "ones", "checker", "border"]


@functools.lru_cache(maxsize=None)
def make_mask(shape, kind):
    if kind[0] == "r":
        seed = SHAPES.index(shape) * 10 + KINDS.index(kind)
        return (np.random.default_rng(seed).random(shape) < int(kind[1:]) / 100.0).astype(np.uint8)
    if kind == "zeros":
        return np.zeros(shape, dtype=np.uint8)
    if kind == "ones":
        return np.ones(shape, dtype=np.uint8)
    if kind == "checker":
        z, y, x = np.indices(shape)
        return ((z + y + x) % 2).astype(np.uint8)
    m = np.zeros(shape, dtype=np.uint8)                           # border: the six faces only
    m[[0, -1]] = 1
    m[:, [0, -1]] = 1
    m[:, :, [0, -1]] = 1
    return m


@functools.lru_cache(maxsize=None)
def ref_mask(shape, kind, spaced):
    kw = dict(spacing=SPACING, origin=ORIGIN) if spaced else {}
    return R.extract(make_mask(shape, kind), **kw)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(m):
    return m.vertices.cpu().numpy(), m.faces.cpu().numpy()


def test_scan_second_level_shape_is_what_the_comment_says():
    from ctunet_amd import mesh
    assert 32 * 34 > mesh.SCAN_BLOCK >= 2 * 2 and 41 * 49 > mesh.SCAN_BLOCK


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_masks_bit_equal(shape, kind):
    """Faces and vertices are bit-equal to the reference, with unit spacing and with spacing and origin: mesh.hip is built
    with contraction off (#pragma clang fp contract(off)), so origin + (index + t d) spacing rounds after every operation
    as numpy does, and t is exactly 0.5 for a mask."""
    from ctunet_amd import mesh
    vol = dev(make_mask(shape, kind))
    for spaced in (False, True):
        rv, rf = ref_mask(shape, kind, spaced)
        m = mesh.extract_surface(vol, **(dict(spacing=SPACING, origin=ORIGIN) if spaced else {}))
        v, f = host(m)
        assert v.dtype == np.float32 and f.dtype == np.int32 and m.vertices.device == vol.device
        assert v.shape == rv.shape and f.shape == rf.shape
        assert np.array_equal(f, rf)
        assert np.array_equal(v.view(np.uint32), rv.view(np.uint32))
    if kind in ("zeros",):
        assert v.shape == (0, 3) and f.shape == (0, 3)


def _fields():
    z, y, x = _grid()
    torus = (2.2 - np.sqrt((np.sqrt((y - 10.5) ** 2 + (x - 11.5) ** 2) - 6.5) ** 2 + (z - 9.5) ** 2)).astype(np.float32)
    rnd = torch.rand((17, 33, 65), generator=torch.Generator().manual_seed(5)).numpy()
    rnd4 = torch.rand((6, 7, 36), generator=torch.Generator().manual_seed(6)).numpy()
    return {"sphere": (sphere_field(), 0.0, -100.0), "sphere_default_fill": (sphere_field(), 0.0, None),
            "torus": (torus, 0.0, -100.0), "rand": (rnd, 0.37, None), "rand_fill": (rnd, 0.37, 0.37),
            "rand_aligned": (rnd4, 0.37, -3.0)}


@pytest.mark.parametrize("name", ["sphere", "sphere_default_fill", "torus", "rand", "rand_fill", "rand_aligned"])
def test_float_fields(name):
    """Faces bit-equal; vertices within atol = 1e-6 max|coordinate| (about 8 float32 ulp for the three rounded operations
    after t), with and without spacing."""
    from ctunet_amd import mesh
    field, level, fill = _fields()[name]
    assert not (field == np.float32(level)).any()
    for kw in ({}, dict(spacing=SPACING, origin=ORIGIN)):
        rv, rf = R.extract(field, level=level, fill_value=fill, **kw)
        v, f = host(mesh.extract_surface(dev(field), level=level, fill_value=fill, **kw))
        assert len(rf) > 0 and np.array_equal(f, rf) and v.shape == rv.shape
        assert np.abs(v.astype(np.float64) - rv).max() <= 1e-6 * np.abs(rv).max()
    if name == "torus":
        assert R.euler(len(v), f) == 0 and np.array_equal(f, R.extract(torus_mask())[1])


@pytest.mark.parametrize("shape", [(17, 33, 65), (8, 8, 16)], ids=["odd", "aligned"])
def test_dtypes_and_label(shape):
    from ctunet_amd import mesh
    lab = np.random.default_rng(3).integers(0, 3, size=shape)
    rv, rf = R.extract(lab == 2)
    got = [mesh.extract_surface(dev(lab == 2)),
           mesh.extract_surface(dev(lab.astype(np.uint8)), label=2),
           mesh.extract_surface(dev(lab.astype(np.int64)), label=2),
           mesh.extract_surface(dev((lab == 2).astype(np.int64) * -7))]
    for m in got:
        v, f = host(m)
        assert np.array_equal(f, rf) and np.array_equal(v, rv)
    v, f = host(mesh.extract_surface(dev(lab.astype(np.uint8))))
    rv, rf = R.extract(lab != 0)
    assert np.array_equal(f, rf) and np.array_equal(v, rv)
    v, f = host(mesh.extract_surface(dev(lab.astype(np.int64)), label=5))
    assert v.shape == (0, 3) and f.shape == (0, 3)


@pytest.mark.parametrize("kind", ["r50", "checker"])
def test_topology_of_the_device_result(kind):
    from ctunet_amd import mesh
    shape = (17, 33, 65)
    v, f = host(mesh.extract_surface(dev(make_mask(shape, kind))))
    assert (R.undirected_edge_counts(f) == 2).all()
    assert (R.directed_edge_counts(f) == 1).all()
    rv, rf = ref_mask(shape, kind, False)
    assert R.euler(len(v), f) == R.euler(len(rv), rf)


@pytest.mark.parametrize("case", ["sphere", "r50", "checker_big"])
def test_measure_and_normals(case):
    """float64 sums of at most 10^6 terms: area within rtol 1e-10 and volume within atol 1e-10 sum|terms| of numpy's float64
    values from the same float32 vertices (N * 1.1e-16 bounds either)."""
    from ctunet_amd import mesh
    if case == "sphere":
        m = mesh.extract_surface(dev(sphere_field()), level=0.0, fill_value=-100.0, spacing=SPACING)
    elif case == "r50":
        m = mesh.extract_surface(dev(make_mask((17, 33, 65), "r50")), spacing=SPACING, origin=ORIGIN)
    else:
        m = mesh.extract_surface(dev(make_mask((40, 48, 72), "checker")))          # more faces than 1024 measure blocks hold
    v, f = host(m)
    assert len(f) > 0
    n, terms = R.face_geometry(v, f)
    area = 0.5 * np.sqrt((n * n).sum(axis=1)).sum()
    out = mesh.measure(m)
    assert out.dtype == torch.float64 and out.shape == (2,) and out.device == m.vertices.device
    got = out.tolist()
    assert abs(got[0] - area) <= 1e-10 * area * max(1.0, len(f) / 1e6)
    assert abs(got[1] - terms.sum()) <= 1e-10 * np.abs(terms).sum() * max(1.0, len(f) / 1e6)
    assert got[1] > 0
    assert torch.equal(mesh.measure(m), out)                                       # fixed order: bit-equal
    nrm = mesh.face_normals(m)
    assert nrm.dtype == torch.float32 and tuple(nrm.shape) == f.shape
    nn = nrm.cpu().numpy().astype(np.float64)[:, ::-1]                              # (x, y, z)
    assert np.abs(np.linalg.norm(nn, axis=1) - 1.0).max() <= 1e-6
    unit = n / np.linalg.norm(n, axis=1, keepdims=True)
    assert np.abs(nn - unit).max() <= 1e-6
    if case == "sphere":                                                            # outward: away from the centre
        c = (v.astype(np.float64)[:, ::-1][f].mean(axis=1) - np.array([11.2, 10.6, 9.3]) * np.array(SPACING)[::-1])
        assert (np.einsum("ij,ij->i", nn, c) > 0).all()


def test_normals_of_a_face_without_area_and_empty_mesh():
    from ctunet_amd import mesh
    v = torch.tensor([[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 0, 2]], dtype=torch.float32, device="cuda")
    f = torch.tensor([[0, 1, 2], [0, 1, 1], [0, 1, 3]], dtype=torch.int32, device="cuda")
    n = mesh.face_normals(mesh.Mesh(v, f)).cpu().numpy()
    assert np.array_equal(n, np.float32([[1, 0, 0], [0, 0, 0], [0, 0, 0]]))           # (z, y, x): x cross y = z
    assert mesh.measure(mesh.Mesh(v, f)).tolist() == [0.5, 0.0]
    e = mesh.extract_surface(torch.zeros(3, 4, 5, dtype=torch.uint8, device="cuda"))
    assert mesh.measure(e).tolist() == [0.0, 0.0] and tuple(mesh.face_normals(e).shape) == (0, 3)


def test_two_calls_and_streams_agree():
    from ctunet_amd import mesh
    vol = dev(make_mask((17, 33, 65), "r50"))
    field = dev(_fields()["rand"][0])
    a, b = mesh.extract_surface(vol, spacing=SPACING), mesh.extract_surface(vol, spacing=SPACING)
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)
    assert torch.equal(mesh.measure(a), mesh.measure(b))
    fa = mesh.extract_surface(field, level=0.37)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = mesh.extract_surface(vol, spacing=SPACING)
        fc = mesh.extract_surface(field, level=0.37)
        mc = mesh.measure(c)
    s.synchronize()
    assert torch.equal(a.vertices, c.vertices) and torch.equal(a.faces, c.faces) and torch.equal(mc, mesh.measure(a))
    assert torch.equal(fa.vertices, fc.vertices) and torch.equal(fa.faces, fc.faces)


def test_non_contiguous_view_is_handled():
    """A view is copied to a contiguous tensor first: the mesh is that of the view's values."""
    from ctunet_amd import mesh
    big = dev(make_mask((17, 33, 65), "r50"))
    view = big.permute(2, 0, 1)[::2, 1:, :]
    assert not view.is_contiguous()
    a, b = mesh.extract_surface(view), mesh.extract_surface(view.contiguous())
    rv, rf = R.extract(view.cpu().numpy())
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces)
    assert np.array_equal(a.faces.cpu().numpy(), rf) and np.array_equal(a.vertices.cpu().numpy(), rv)


def test_workspace_bytes_is_what_the_call_allocates():
    from ctunet_amd import mesh
    shape = (17, 33, 65)
    vol = dev(make_mask(shape, "r50"))
    mesh.extract_surface(vol)                                                       # library and context loaded
    torch.cuda.synchronize()
    key = "requested_bytes.all.allocated"
    before = torch.cuda.memory_stats()[key]
    m = mesh.extract_surface(vol)
    after = torch.cuda.memory_stats()[key]
    assert after - before == mesh.workspace_bytes(shape) + 12 * m.vertices.shape[0] + 12 * m.faces.shape[0]


def test_implant_to_stl_end_to_end(tmp_path):
    from ctunet_amd import mesh, postprocess
    z, y, x = np.indices((48, 48, 48))
    r = np.sqrt((z - 23.5) ** 2 + (y - 23.5) ** 2 + (x - 23.5) ** 2)
    full = ((r >= 14) & (r <= 20)).astype(np.uint8)
    hole = (np.sqrt((y - 23.5) ** 2 + (x - 23.5) ** 2) <= 7) & (z < 24)
    defective = full * ~hole
    implant = postprocess.extract_implant(dev(full), dev(defective))
    assert int(implant.sum()) > 100
    m = mesh.extract_surface(implant, spacing=SPACING)
    rv, rf = R.extract(implant.cpu().numpy(), spacing=SPACING)
    assert np.array_equal(m.faces.cpu().numpy(), rf) and np.array_equal(m.vertices.cpu().numpy(), rv)
    path = tmp_path / "implant.stl"
    mesh.write_stl(path, m, header=b"implant")
    raw = path.read_bytes()
    nf = int(np.frombuffer(raw, dtype="<u4", count=1, offset=80)[0])
    assert nf == m.faces.shape[0] and len(raw) == 84 + 50 * nf
    rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("p", "<f4", (3, 3)), ("a", "<u2")]), offset=84)
    p = rec["p"].astype(np.float64)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    unit = n / np.linalg.norm(n, axis=1, keepdims=True)
    assert np.abs(rec["n"] - unit).max() <= 1e-6
    vol = np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0
    area, volume = mesh.measure(m).tolist()
    assert vol == pytest.approx(volume, rel=1e-5) and volume > 0 and area > 0
