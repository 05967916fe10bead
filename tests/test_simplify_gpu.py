"""ctunet_amd.simplify.decimate on the GPU against tests/simplify_ref.py: vertices, faces and map bit for bit throughout; the
scan levels and the bucket bound, refusals, hygiene (repeatability, streams, views, workspace) and the pipeline end to end."""
import numpy as np
import pytest
import torch

import mesh_ref as R
import mesh_smooth_ref as S
import mesh_voxelize_ref as X
import simplify_ref as D
from test_mesh_cpu import sphere_mask
from test_simplify_cpu import SPACING, TRIPLE, fan_mesh, mesh_of, ref

pytestmark = pytest.mark.gpu

SMALL = ("sphere", "torus", "shell")
CASES = ([(name, cell, cancel) for name in SMALL for cell in (0.05, 1.5, 2.5, 1000) for cancel in (True, False)]
         + [("sphere_spaced", 2.5, True), ("sphere_spaced", TRIPLE, True), ("sphere_spaced", TRIPLE, False),
            ("r50", 1.5, True), ("r50", 2.5, True), ("r50", 2.5, False), ("sparse", 1.0, True), ("sparse", 1.0, False), ("many", 2.0, True),
            ("fan", 1.0, True), ("fan", 1.0, False)])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_mesh(name):
    from ctunet_amd import mesh
    v, f = mesh_of(name)
    return mesh.Mesh(dev(v), dev(f))


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def assert_equals_reference(got, index, want):
    ov, of, vmap = want
    assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32 and index.dtype == torch.int32
    assert tuple(got.vertices.shape) == ov.shape and tuple(got.faces.shape) == of.shape and tuple(index.shape) == vmap.shape
    assert np.array_equal(got.faces.cpu().numpy(), of)
    assert np.array_equal(index.cpu().numpy(), vmap)
    assert np.array_equal(bits(got.vertices), ov.view(np.uint32))


def test_shapes_reach_the_scan_levels_the_comments_name():
    from ctunet_amd import mesh, simplify
    chunk = mesh.ADJ_SCAN_CHUNK
    for name in SMALL:                                                  # the smallest cell of the small cases fits the grid
        v, f = mesh_of(name)
        assert chunk < np.prod(D.grid(v, f, 0.05)[3]) <= simplify.MAX_CELLS
    v, f = mesh_of("r50")                                               # the V- and F-sized scans take their second level
    assert len(v) > 1024 * 128 > chunk and len(f) > 2 * len(v) - 8192
    assert np.prod(D.grid(v, f, 0.05)[3]) > simplify.MAX_CELLS
    v, f = mesh_of("sparse")                                            # several chunks per thread of the chunk scan
    assert -(-int(np.prod(D.grid(v, f, 1.0)[3])) // chunk) > 2 * 1024
    assert len(mesh_of("fan")[1]) == simplify.MAX_BUCKET               # the largest bucket that is walked
    assert len(mesh_of("many")[1]) > 2048 * 256                         # the blocks of the bounds pass stride over the faces


@pytest.mark.parametrize("name,cell,cancel", CASES)
def test_bit_equal_to_the_reference(name, cell, cancel):
    from ctunet_amd import simplify
    m = device_mesh(name)
    got, index = simplify.decimate(m, cell, cancel=cancel, return_map=True)
    assert got.vertices.device == got.faces.device == index.device == m.vertices.device
    assert_equals_reference(got, index, ref(name, cell, cancel))
    alone = simplify.decimate(m, cell, cancel=cancel)
    assert torch.equal(alone.faces, got.faces) and torch.equal(alone.vertices.view(torch.int32), got.vertices.view(torch.int32))
    v, f = mesh_of(name)
    assert np.array_equal(bits(m.vertices), v.view(np.uint32)) and np.array_equal(m.faces.cpu().numpy(), f)    # untouched


def test_hand_made_cases():
    from ctunet_amd import mesh, simplify
    square = np.array([[0, 0, 0], [0, 0, 3], [0, 3, 0], [0, 3, 3], [np.nan, 7, 7]], dtype=np.float32)
    a, b = [0, 1, 2], [0, 2, 1]
    for faces, cell in (([a, b], 1.0), ([[1, 2, 0], b, a, [2, 0, 1]], 1.0), ([a, b, [2, 1, 0], [1, 0, 2]], 1.0),
                        ([a, [1, 3, 2], b], 1.0), ([[0, 1, 1], a], 1.0), ([a, [1, 3, 2]], 2.0), ([a, [1, 3, 2]], (5.0, 0.5, 2.0))):
        f = np.array(faces, dtype=np.int32)
        for cancel in (True, False):
            got, index = simplify.decimate(mesh.Mesh(dev(square), dev(f)), cell, cancel=cancel, return_map=True)
            assert_equals_reference(got, index, D.decimate(square, f, cell, cancel))
    # all members coincide, and no faces at all
    same = np.repeat(square[3:4], 3, axis=0)
    got, index = simplify.decimate(mesh.Mesh(dev(same), dev(np.array([a], dtype=np.int32))), 0.5, return_map=True)
    assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and index.tolist() == [-1, -1, -1]
    got, index = simplify.decimate(mesh.Mesh(dev(square), dev(np.zeros((0, 3), dtype=np.int32))), 0.5, return_map=True)
    assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and index.tolist() == [-1] * 5
    assert got.faces.dtype == torch.int32 and got.vertices.is_cuda


@pytest.mark.parametrize("bad", ["V", -1, -(1 << 31), "nan", "inf"])
def test_refused_faces_raise(bad):
    """Such a face is skipped on the device, never read through, and counted; only the exception is asserted."""
    from ctunet_amd import mesh, simplify
    v, f = (a.copy() for a in mesh_of("sphere"))
    if isinstance(bad, str) and bad != "V":
        v[f[len(f) // 2, 1], 2] = float(bad)
    else:
        f[len(f) // 2, 1] = len(v) if bad == "V" else bad
    with pytest.raises(ValueError, match="does not exist or is not finite"):
        simplify.decimate(mesh.Mesh(dev(v), dev(f)), 1.5)


def test_too_many_cells_and_too_large_a_bucket_raise():
    from ctunet_amd import mesh, simplify
    with pytest.raises(ValueError, match=r"more than 268435456; cell_size=\(0\.1.*fits"):
        simplify.decimate(device_mesh("r50"), 0.05)
    with pytest.raises(ValueError, match="needs .* cells"):
        simplify.decimate(device_mesh("sphere"), (1.0, 1e-6, 1.0))
    # one face more than the bucket bound around one hub: the guard answers, promptly, and no lane walks the bucket
    v, f = fan_mesh(simplify.MAX_BUCKET + 1)
    m = mesh.Mesh(dev(v), dev(f))
    with pytest.raises(ValueError, match="more than 4096 surviving faces share their lowest cluster"):
        simplify.decimate(m, 1.0)
    got, index = simplify.decimate(m, 1.0, cancel=False, return_map=True)            # without cancellation nothing is walked
    assert_equals_reference(got, index, D.decimate(v, f, 1.0, cancel=False))


def test_two_calls_streams_and_views_agree():
    from ctunet_amd import mesh, simplify
    m = device_mesh("r50")
    want = ref("r50", 2.5)
    a, ia = simplify.decimate(m, 2.5, return_map=True)
    b, ib = simplify.decimate(m, 2.5, return_map=True)
    assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32)) and torch.equal(a.faces, b.faces) and torch.equal(ia, ib)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c, ic = simplify.decimate(m, 2.5, return_map=True)
    s.synchronize()
    assert_equals_reference(c, ic, want)
    wide = torch.zeros((m.vertices.shape[0], 6), device="cuda")
    wide[:, ::2] = m.vertices
    view = wide[:, ::2]
    faces_t = m.faces.t().contiguous().t()
    assert not view.is_contiguous() and not faces_t.is_contiguous()
    d, idx = simplify.decimate(mesh.Mesh(view, faces_t), 2.5, return_map=True)
    assert_equals_reference(d, idx, want)
    assert torch.equal(view, m.vertices) and torch.equal(faces_t, m.faces)


def test_workspace_bytes_is_what_the_call_allocates():
    from ctunet_amd import simplify
    m = device_mesh("r50")
    v, f = mesh_of("r50")
    V, F = len(v), len(f)
    cells = int(np.prod(D.grid(v, f, 1.5)[3]))
    simplify.decimate(m, 1.5)
    torch.cuda.synchronize()
    key = "requested_bytes.all.allocated"
    before = torch.cuda.memory_stats()[key]
    out = simplify.decimate(m, 1.5)
    mid = torch.cuda.memory_stats()[key]
    out2, index = simplify.decimate(m, 1.5, return_map=True)
    after = torch.cuda.memory_stats()[key]
    result = 12 * out.vertices.shape[0] + 12 * out.faces.shape[0]
    assert mid - before == simplify.workspace_bytes(V, F, cells) + result
    assert after - mid == simplify.workspace_bytes(V, F, cells) + result + 4 * V
    assert torch.equal(out.faces, out2.faces)


def test_extract_smooth_decimate_measure_voxelize_end_to_end():
    from ctunet_amd import mesh, simplify
    mask = sphere_mask()
    rv, rf = R.extract(mask, spacing=SPACING)
    rs = S.smooth(rv, rf)
    dv, df, _ = D.decimate(rs, rf, 1.0)
    assert 0 < len(df) < len(rf) / 2 and D.edges_balanced(df)
    m = simplify.decimate(mesh.smooth(mesh.extract_surface(dev(mask.astype(np.uint8)), spacing=SPACING)), 1.0)
    assert np.array_equal(bits(m.vertices), dv.view(np.uint32)) and np.array_equal(m.faces.cpu().numpy(), df)
    n, terms = R.face_geometry(dv, df)
    area = 0.5 * np.sqrt((n * n).sum(axis=1)).sum()
    got = mesh.measure(m).tolist()
    assert abs(got[0] - area) <= 1e-10 * area * max(1.0, len(df) / 1e6)
    assert abs(got[1] - terms.sum()) <= 1e-10 * np.abs(terms).sum() * max(1.0, len(df) / 1e6)
    assert got[1] > 0                                                    # still wound outward
    vox = mesh.voxelize(m, mask.shape, spacing=SPACING)
    want = X.voxelize(dv, df, mask.shape, spacing=SPACING)
    assert want.any() and np.array_equal(vox.cpu().numpy(), want)
