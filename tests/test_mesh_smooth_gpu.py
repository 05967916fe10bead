"""ctunet_amd.mesh.adjacency and mesh.smooth on the GPU against tests/mesh_smooth_ref.py, bit for bit throughout: the table
for extracted and hand-built meshes (any face order), the smoothed positions (Taubin and Laplacian, fixed vertices, a prebuilt
table), hygiene (repeatability, streams, views, workspace), refusal of bad face indices, and the pipeline end to end."""
import functools

import numpy as np
import pytest
import torch

import mesh_ref as R
import mesh_smooth_ref as S
from test_mesh_cpu import sphere_mask
from test_mesh_gpu import SPACING, ORIGIN, dev, ref_mask
from test_mesh_smooth_cpu import HAND

pytestmark = pytest.mark.gpu

R50 = (17, 33, 65)                      # V = 134748 vertices: 33 chunks of the adjacency scan (the second level)
BIG_V = 4096 * 1024 + 4097              # more chunks than the 1024 threads that scan the chunk sums: several chunks per thread
CASES = ["voxel", "sphere", "sphere_spaced", "r50", "r50_spaced", "strip", "cone", "odd", "empty", "big_v"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices, faces) on the host; the extracted ones are the reference's (test_mesh_gpu.py checks the device's against
    them bit for bit)."""
    if name in HAND:
        return HAND[name]()
    if name == "voxel":
        return R.extract(np.ones((1, 1, 1), dtype=np.uint8))
    if name == "sphere":
        return R.extract(sphere_mask())
    if name == "sphere_spaced":
        return R.extract(sphere_mask(), spacing=SPACING, origin=ORIGIN)
    if name in ("r50", "r50_spaced"):
        return ref_mask(R50, "r50", name == "r50_spaced")
    if name == "empty":
        return np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32)
    assert name == "big_v"
    # mostly unreferenced vertices; faces at both ends, across chunk borders and across the thread border of the chunk scan
    v = (np.arange(3 * BIG_V, dtype=np.int64) % 1021).astype(np.float32).reshape(BIG_V, 3)
    ids = np.array([0, 1, 4095, 4096, 4097, 8191, 8192, 5 * 4096 - 1, 5 * 4096, 4096 * 1024 - 1, 4096 * 1024, BIG_V - 2, BIG_V - 1])
    f = np.stack([ids[:-2], ids[1:-1], ids[2:]], axis=1)
    return v, np.concatenate([f, [[BIG_V - 1, 0, 4096 * 1024]]]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def ref_adjacency(name):
    v, f = case(name)
    return S.adjacency(len(v), f)


@functools.lru_cache(maxsize=None)
def ref_smooth(name, iterations, mu, fixed_seed=None):
    v, f = case(name)
    return S.smooth(v, f, iterations, 0.5, mu, fixed_mask(name, fixed_seed))


def fixed_mask(name, seed):
    return None if seed is None else np.random.default_rng(seed).random(len(case(name)[0])) < 0.3


def device_mesh(name):
    from ctunet_amd import mesh
    v, f = case(name)
    return mesh.Mesh(dev(v), dev(f))


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def test_shapes_reach_the_scan_levels_the_comments_name():
    from ctunet_amd import mesh
    assert len(case("sphere")[0]) == 2766 < mesh.ADJ_SCAN_CHUNK < 1024 * 128 < len(case("r50")[0]) == 134748
    assert len(case("r50")[1]) == 285704 and len(case("voxel")[0]) == 14
    assert -(-BIG_V // mesh.ADJ_SCAN_CHUNK) > 1024


@pytest.mark.parametrize("name", CASES)
def test_adjacency_equals_the_reference(name):
    from ctunet_amd import mesh
    m = device_mesh(name)
    a = mesh.adjacency(m)
    off, nb = ref_adjacency(name)
    assert a.offsets.dtype == torch.int32 and a.neighbours.dtype == torch.int32
    assert a.offsets.device == m.vertices.device == a.neighbours.device
    assert np.array_equal(a.offsets.cpu().numpy(), off) and np.array_equal(a.neighbours.cpu().numpy(), nb)
    if name in ("voxel", "sphere", "r50"):
        assert len(nb) == 3 * len(case(name)[1])                       # closed and oriented: E = 3F
    b = mesh.adjacency(m)
    assert torch.equal(a.offsets, b.offsets) and torch.equal(a.neighbours, b.neighbours)


@pytest.mark.parametrize("name", ["sphere", "r50", "cone", "odd"])
def test_face_order_and_corner_order_do_not_matter(name):
    from ctunet_amd import mesh
    v, f = case(name)
    rng = np.random.default_rng(11)
    g = f[rng.permutation(len(f))]
    g = np.take_along_axis(g, (np.arange(3)[None, :] + rng.integers(0, 3, size=(len(g), 1))) % 3, axis=1)
    a = mesh.adjacency(mesh.Mesh(dev(v), dev(g)))
    off, nb = ref_adjacency(name)
    assert np.array_equal(a.offsets.cpu().numpy(), off) and np.array_equal(a.neighbours.cpu().numpy(), nb)


@pytest.mark.parametrize("mu", [-0.53, None], ids=["taubin", "laplacian"])
@pytest.mark.parametrize("iterations", [0, 1, 10])
@pytest.mark.parametrize("name", ["voxel", "sphere", "sphere_spaced", "strip", "cone", "odd", "empty"])
def test_smooth_bit_equal(name, iterations, mu):
    from ctunet_amd import mesh
    m = device_mesh(name)
    out = mesh.smooth(m, iterations, mu=mu)
    want = ref_smooth(name, iterations, mu)
    assert out.vertices.dtype == torch.float32 and out.vertices.shape == m.vertices.shape
    assert out.faces is m.faces
    assert np.array_equal(bits(out.vertices), want.view(np.uint32))
    assert np.array_equal(bits(m.vertices), case(name)[0].view(np.uint32))      # the input is untouched


@pytest.mark.parametrize("name,iterations,mu", [("r50", 0, -0.53), ("r50", 1, -0.53), ("r50", 10, -0.53), ("r50_spaced", 3, None),
                                                ("r50_spaced", 1, -0.53), ("big_v", 1, None)])
def test_smooth_bit_equal_large(name, iterations, mu):
    from ctunet_amd import mesh
    out = mesh.smooth(device_mesh(name), iterations, mu=mu)
    assert np.array_equal(bits(out.vertices), ref_smooth(name, iterations, mu).view(np.uint32))


def test_smooth_of_a_device_extracted_mesh():
    """The pipeline's own order of calls, with and without spacing and origin."""
    from ctunet_amd import mesh
    vol = dev(sphere_mask().astype(np.uint8))
    for name, kw in (("sphere", {}), ("sphere_spaced", dict(spacing=SPACING, origin=ORIGIN))):
        out = mesh.smooth(mesh.extract_surface(vol, **kw))
        assert np.array_equal(bits(out.vertices), ref_smooth(name, 10, -0.53).view(np.uint32))


@pytest.mark.parametrize("name,iterations", [("sphere", 10), ("r50", 1), ("odd", 10)])
def test_fixed_vertices(name, iterations):
    from ctunet_amd import mesh
    m = device_mesh(name)
    fixed = fixed_mask(name, 5)
    want = ref_smooth(name, iterations, -0.53, 5)
    assert np.array_equal(want[fixed].view(np.uint32), case(name)[0][fixed].view(np.uint32))
    assert not np.array_equal(want, ref_smooth(name, iterations, -0.53))
    for fx in (dev(fixed), dev(fixed.astype(np.uint8))):
        out = mesh.smooth(m, iterations, fixed=fx)
        assert np.array_equal(bits(out.vertices), want.view(np.uint32))


@pytest.mark.parametrize("name", ["sphere", "r50", "cone"])
def test_prebuilt_adjacency(name):
    from ctunet_amd import mesh
    m = device_mesh(name)
    a = mesh.adjacency(m)
    for kw in ({}, dict(mu=None, iterations=3), dict(iterations=0)):
        x, y = mesh.smooth(m, adjacency=a, **kw), mesh.smooth(m, **kw)
        assert torch.equal(x.vertices.view(torch.int32), y.vertices.view(torch.int32))
    assert np.array_equal(bits(mesh.smooth(m, adjacency=a).vertices), ref_smooth(name, 10, -0.53).view(np.uint32))


def test_two_calls_streams_and_views_agree():
    from ctunet_amd import mesh
    m = device_mesh("r50_spaced")
    a, b = mesh.smooth(m), mesh.smooth(m)
    assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = mesh.smooth(m)
        adj = mesh.adjacency(m)
    s.synchronize()
    ref = mesh.adjacency(m)
    assert torch.equal(a.vertices.view(torch.int32), c.vertices.view(torch.int32))
    assert torch.equal(adj.offsets, ref.offsets) and torch.equal(adj.neighbours, ref.neighbours)
    wide = torch.zeros((m.vertices.shape[0], 6), device="cuda")
    wide[:, ::2] = m.vertices
    view = wide[:, ::2]
    faces_t = m.faces.t().contiguous().t()
    assert not view.is_contiguous() and not faces_t.is_contiguous()
    d = mesh.smooth(mesh.Mesh(view, faces_t))
    assert torch.equal(a.vertices.view(torch.int32), d.vertices.view(torch.int32)) and d.faces is faces_t
    assert torch.equal(view, m.vertices)


def test_workspace_bytes_is_what_the_call_allocates():
    from ctunet_amd import _lib, mesh
    lib = _lib.load()
    m = device_mesh("r50")
    V, F = m.vertices.shape[0], m.faces.shape[0]
    a = mesh.adjacency(m)
    E = a.neighbours.shape[0]
    mesh.smooth(m, adjacency=a)
    torch.cuda.synchronize()
    key = "requested_bytes.all.allocated"
    before = torch.cuda.memory_stats()[key]
    out = mesh.smooth(m, adjacency=a)
    mid = torch.cuda.memory_stats()[key]
    out2 = mesh.smooth(m)
    after = torch.cuda.memory_stats()[key]
    assert mid - before == lib.ctu_mesh_smooth_ws_bytes(V) + 12 * V
    assert after - mid == lib.ctu_mesh_smooth_ws_bytes(V) + 12 * V + lib.ctu_mesh_adjacency_ws_bytes(V, F) + 4 * (V + 1) + 4 * E
    assert after - mid <= mesh.smooth_workspace_bytes(V, F) + 12 * V
    assert torch.equal(out.vertices, out2.vertices)


@pytest.mark.parametrize("index", ["V", -1, -(1 << 31), (1 << 31) - 1])
def test_bad_face_index_is_refused(index):
    """The build kernels skip a face with an index outside [0, V) and count it; the host raises.  Nothing is read through the
    index, so the call is safe by construction; only the exception is asserted."""
    from ctunet_amd import mesh
    v, f = case("sphere")
    g = f.copy()
    g[len(g) // 2, 1] = len(v) if index == "V" else index
    m = mesh.Mesh(dev(v), dev(g))
    with pytest.raises(ValueError, match="refers to a vertex that does not exist"):
        mesh.adjacency(m)
    with pytest.raises(ValueError, match="refers to a vertex that does not exist"):
        mesh.smooth(m)


def test_implant_to_smooth_stl_end_to_end(tmp_path):
    from ctunet_amd import mesh, postprocess
    z, y, x = np.indices((48, 48, 48))
    r = np.sqrt((z - 23.5) ** 2 + (y - 23.5) ** 2 + (x - 23.5) ** 2)
    full = ((r >= 14) & (r <= 20)).astype(np.uint8)
    hole = (np.sqrt((y - 23.5) ** 2 + (x - 23.5) ** 2) <= 7) & (z < 24)
    implant = postprocess.extract_implant(dev(full), dev(full * ~hole))
    # the reference alone, from the same mask: Taubin keeps the volume within 1 % and reduces the area
    rv, rf = R.extract(implant.cpu().numpy(), spacing=SPACING)
    rs = S.smooth(rv, rf)
    (area0, vol0), (area1, vol1) = R.area_volume(rv, rf), R.area_volume(rs, rf)
    assert len(rf) > 1000 and abs(vol1 / vol0 - 1.0) < 0.01 and area1 < area0
    m = mesh.extract_surface(implant, spacing=SPACING)
    s = mesh.smooth(m)
    assert np.array_equal(bits(s.vertices), rs.view(np.uint32))
    (a0, v0), (a1, v1) = mesh.measure(m).tolist(), mesh.measure(s).tolist()
    assert abs(v1 / v0 - 1.0) < 0.01 and a1 < a0
    assert v1 == pytest.approx(vol1, rel=1e-9) and a1 == pytest.approx(area1, rel=1e-9)
    path = tmp_path / "implant.stl"
    mesh.write_stl(path, s, header=b"smoothed implant")
    raw = path.read_bytes()
    nf = int(np.frombuffer(raw, dtype="<u4", count=1, offset=80)[0])
    assert nf == m.faces.shape[0] == len(rf) and len(raw) == 84 + 50 * nf
