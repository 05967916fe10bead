"""ctunet_amd.mesh.voxelize and mesh.winding_number on the GPU: bit-equal to tests/mesh_voxelize_ref.py on small grids, the
round trip voxelize(extract_surface(M)) == M at the shapes where the kernels change path (no reference needed), both scatter
paths in one wave, hygiene (repeatability, streams, views, workspace, far and refused meshes) and the pipeline end to end."""
import functools

import numpy as np
import pytest
import torch

import mesh_ref as R
import mesh_smooth_ref as S
import mesh_voxelize_ref as X
from test_mesh_voxelize_cpu import LEVEL, MASKS, ORIGIN, SPACING, cube_block, degenerate_faces, random_field, random_mask

pytestmark = pytest.mark.gpu

# The scan gives a lane 4 voxels where W % 4 == 0 and 1 otherwise, and a wave 64 / SEG rows, SEG = the lanes of a row rounded
# up to a power of two.  W = 130: three 64-lane steps, the last one partial; 65: one step plus one voxel; 64: 4 rows of 16
# lanes; (2, 3, 260): two steps of 4 voxels per lane; (1, 1, 1): a one-lane segment; (2, 300, 3): 16 rows of 4 lanes in a wave
ROUND_TRIP_SHAPES = [(3, 5, 130), (9, 7, 64), (9, 7, 65), (1, 1, 1), (2, 300, 3), (2, 3, 260)]
OTHER_GRID = dict(shape=(11, 13, 15), spacing=0.5, origin=(-0.3, 0.17, -0.41))      # half the spacing of the mesh's grid
BIG_GRID = (44, 44, 70)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sphere16():
    z, y, x = np.indices((16, 16, 16))
    return ((z - 7.5) ** 2 + (y - 7.5) ** 2 + (x - 7.5) ** 2 <= 36.0).astype(np.uint8)


def renumbered_cube(seed=2):
    v, f = X.cube_mesh()
    perm = np.random.default_rng(seed).permutation(8)
    v2 = np.empty_like(v)
    v2[perm] = v
    return v2, perm[f].astype(np.int32)


def _mask_case(name, spaced):
    m = MASKS[name]()
    kw = dict(spacing=SPACING, origin=ORIGIN) if spaced else {}
    return R.extract(m, **kw) + (dict(shape=m.shape, **kw),)


def _field_case(shape, seed):
    return R.extract(random_field(shape, seed), level=LEVEL, spacing=SPACING, origin=ORIGIN) + (dict(shape=shape, spacing=SPACING, origin=ORIGIN),)


# name -> (vertices, faces, grid keywords), all on the host
CASES = {
    **{name: functools.partial(_mask_case, name, False) for name in MASKS},
    **{name + "_spaced": functools.partial(_mask_case, name, True) for name in ("r567", "r449", "full")},
    "field567": functools.partial(_field_case, (5, 6, 7), 3),
    "field449": functools.partial(_field_case, (4, 4, 9), 4),
    "cube": lambda: X.cube_mesh() + (dict(shape=(6, 6, 6)),),
    "cube_reversed": lambda: (X.cube_mesh()[0], X.cube_mesh()[1][:, ::-1], dict(shape=(6, 6, 6))),
    "cube_renumbered": lambda: renumbered_cube() + (dict(shape=(6, 6, 6)),),
    "cube_degenerate": lambda: degenerate_faces(*X.cube_mesh()) + (dict(shape=(6, 6, 6)),),
    "cube_open": lambda: (X.cube_mesh()[0], X.cube_mesh()[1][:10], dict(shape=(6, 6, 6))),
    "mask_on_another_grid": lambda: R.extract(MASKS["r567"]()) + (OTHER_GRID,),
    "smoothed_sphere": lambda: (S.smooth(*R.extract(sphere16())), R.extract(sphere16())[1], dict(shape=(16, 16, 16))),
    "smoothed_sphere_on_another_grid": lambda: (S.smooth(*R.extract(sphere16())), R.extract(sphere16())[1],
                                                dict(shape=(16, 16, 20), spacing=(1.0, 1.0, 0.8), origin=(0.1, 0.2, -0.3))),
}


@functools.lru_cache(maxsize=None)
def case(name):
    v, f, grid = CASES[name]()
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32), grid


@functools.lru_cache(maxsize=None)
def ref_winding(name):
    v, f, grid = case(name)
    w = X.winding_number(v, f, grid["shape"], grid.get("spacing"), grid.get("origin"))
    w.setflags(write=False)
    return w


def device_mesh(name):
    from ctunet_amd import mesh
    v, f, _ = case(name)
    return mesh.Mesh(dev(v), dev(f))


def test_the_reference_grids_stay_small():
    for name in CASES:
        d, h, w = case(name)[2]["shape"]
        assert d <= 16 and h <= 16 and w <= 20, name


@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_equal_to_the_reference(name):
    from ctunet_amd import mesh
    m = device_mesh(name)
    grid = case(name)[2]
    want = ref_winding(name)
    w = mesh.winding_number(m, **grid)
    assert w.dtype == torch.int32 and tuple(w.shape) == tuple(grid["shape"]) and w.device == m.vertices.device
    assert np.array_equal(w.cpu().numpy(), want)
    v = mesh.voxelize(m, **grid)
    assert v.dtype == torch.uint8 and tuple(v.shape) == tuple(grid["shape"]) and v.is_contiguous()
    assert np.array_equal(v.cpu().numpy(), (want != 0).astype(np.uint8))
    if name == "cube_reversed":
        assert np.array_equal(want, -cube_block())
    if name in ("cube", "cube_renumbered", "cube_degenerate"):
        assert np.array_equal(want, cube_block())
    if name.startswith("smoothed_sphere"):
        assert set(np.unique(want).tolist()) == {0, 1}                               # this mesh does not intersect itself


@pytest.mark.parametrize("spaced", [False, True], ids=["unit", "spaced"])
@pytest.mark.parametrize("shape", ROUND_TRIP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_round_trip_of_masks_and_fields(shape, spaced):
    """voxelize(extract_surface(M)) == M, and a field cut at its level comes back as field > level; both meshes are the
    device's own (test_mesh_gpu.py checks them against the reference)."""
    from ctunet_amd import mesh
    kw = dict(spacing=SPACING, origin=ORIGIN) if spaced else {}
    seed = ROUND_TRIP_SHAPES.index(shape)
    mask = np.ones(shape, dtype=np.uint8) if shape == (1, 1, 1) else random_mask(shape, 20 + seed)
    vol = dev(mask)
    m = mesh.extract_surface(vol, **kw)
    assert torch.equal(mesh.voxelize(m, shape, **kw), vol)
    assert torch.equal(mesh.winding_number(m, vol.shape, **kw), vol.to(torch.int32))
    field = random_field(shape, 30 + seed)
    fm = mesh.extract_surface(dev(field), level=LEVEL, **kw)
    assert np.array_equal(mesh.voxelize(fm, shape, **kw).cpu().numpy(), (field > np.float32(LEVEL)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def two_path_mesh(mask_shape):
    """The 12-triangle cube over 40 x 40 rows of BIG_GRID (every face's box holds far more rows than a lane walks: the wave's
    cooperative path) and, behind it in x, the mesh of a random mask (faces of 0-2 rows: the per-lane path), in one mesh: the
    first wave holds the 12 cube faces and 52 of the others.  (vertices, faces, the expected volume)."""
    cv, cf = X.cube_mesh(1.5, 41.5)
    mask = random_mask(mask_shape, 40)
    mv, mf = R.extract(mask, origin=(5, 7, 46))
    want = np.zeros(BIG_GRID, dtype=np.uint8)
    want[2:42, 2:42, 2:42] = 1
    box = tuple(slice(o, o + n) for o, n in zip((5, 7, 46), mask_shape))
    assert not want[box].any() and mv[:, 2].min() > 41.5                             # disjoint: the union is the sum
    want[box] = mask
    return np.concatenate([cv, mv]), np.concatenate([cf, mf + len(cv)]).astype(np.int32), want


# the scatter kernel is launched in 65536 // F slices (at least 1, SLICE_FACES of mesh_voxelize.hip) that share the rows of
# the large faces: a mesh of few faces takes many, one of more than 32768 faces takes one
@pytest.mark.parametrize("mask_shape,slices", [((4, 5, 6), 57), ((10, 12, 20), 3), ((16, 18, 22), 1)], ids=["57_slices", "3_slices", "1_slice"])
def test_both_scatter_paths_in_one_wave(mask_shape, slices):
    from ctunet_amd import mesh
    v, f, want = two_path_mesh(mask_shape)
    assert max(1, min(256, 65536 // len(f))) == slices
    a = mesh.winding_number(mesh.Mesh(dev(v), dev(f)), BIG_GRID)
    assert np.array_equal(a.cpu().numpy(), want.astype(np.int32))
    g = f[np.random.default_rng(41).permutation(len(f))]                             # large faces now sit in many waves
    b = mesh.winding_number(mesh.Mesh(dev(v), dev(g)), BIG_GRID)
    assert torch.equal(a, b)
    assert np.array_equal(mesh.voxelize(mesh.Mesh(dev(v), dev(g)), BIG_GRID).cpu().numpy(), want)


def test_two_calls_streams_and_views_agree():
    from ctunet_amd import mesh
    m = device_mesh("smoothed_sphere_on_another_grid")
    grid = case("smoothed_sphere_on_another_grid")[2]
    want = ref_winding("smoothed_sphere_on_another_grid")
    a, b = mesh.winding_number(m, **grid), mesh.winding_number(m, **grid)
    assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = mesh.winding_number(m, **grid)
        d = mesh.voxelize(m, **grid)
    s.synchronize()
    assert torch.equal(a, c) and torch.equal(d, (a != 0).to(torch.uint8))
    wide = torch.zeros((m.vertices.shape[0], 6), device="cuda")
    wide[:, ::2] = m.vertices
    view = wide[:, ::2]
    faces_t = m.faces.t().contiguous().t()
    assert not view.is_contiguous() and not faces_t.is_contiguous()
    e = mesh.winding_number(mesh.Mesh(view, faces_t), **grid)
    assert torch.equal(a, e) and np.array_equal(e.cpu().numpy(), want)


def test_workspace_bytes_is_what_the_call_allocates():
    from ctunet_amd import mesh
    m = device_mesh("smoothed_sphere")
    shape = (16, 16, 16)
    mesh.voxelize(m, shape)
    torch.cuda.synchronize()
    key = "requested_bytes.all.allocated"
    before = torch.cuda.memory_stats()[key]
    v = mesh.voxelize(m, shape)
    mid = torch.cuda.memory_stats()[key]
    w = mesh.winding_number(m, shape)
    after = torch.cuda.memory_stats()[key]
    ws = mesh.voxelize_workspace_bytes(shape)
    assert ws == 256 + 4 * 16 ** 3
    assert mid - before == ws + 16 ** 3 and after - mid == ws + 4 * 16 ** 3
    assert torch.equal(v, (w != 0).to(torch.uint8))


def test_meshes_outside_the_grid_give_zeros():
    from ctunet_amd import mesh
    v, f = X.cube_mesh()
    for far in (v + np.float32(100.0), v - np.float32(100.0), v * np.float32(1e30), v - np.float32(1e30), v * np.float32(-1e30)):
        m = mesh.Mesh(dev(far), dev(f))
        assert not mesh.winding_number(m, (6, 6, 6)).any()
        assert not mesh.voxelize(m, (5, 4, 70), spacing=SPACING, origin=ORIGIN).any()
    # a grid far from the mesh, and one so coarse or so fine that every centre but the first lies outside
    m = mesh.Mesh(dev(v), dev(f))
    assert not mesh.voxelize(m, (6, 6, 6), origin=1e30).any()
    assert not mesh.voxelize(m, (6, 6, 6), spacing=1e-30, origin=-1.0).any()
    one = mesh.voxelize(m, (6, 6, 6), spacing=1e30, origin=1.0)
    assert one[0, 0, 0] == 1 and one.sum() == 1


@pytest.mark.parametrize("bad", ["minus_one", "V", "int_min", "nan", "inf"])
def test_refused_faces_raise_and_leave_no_fault_behind(bad):
    """The scatter kernel skips a face with an index outside [0, V) or a vertex that is not finite, counts it and never reads
    through it; the host raises.  A valid call afterwards is correct."""
    from ctunet_amd import mesh
    v, f, grid = case("smoothed_sphere")
    v, f = v.copy(), f.copy()
    k = len(f) // 2
    if bad in ("nan", "inf"):
        v[f[k, 1], 2] = np.nan if bad == "nan" else np.inf
    else:
        f[k, 2] = {"minus_one": -1, "V": len(v), "int_min": -(1 << 31)}[bad]
    m = mesh.Mesh(dev(v), dev(f))
    for fn in (mesh.voxelize, mesh.winding_number):
        with pytest.raises(ValueError, match="does not exist or is not finite"):
            fn(m, **grid)
    good = mesh.winding_number(device_mesh("smoothed_sphere"), **grid)
    assert np.array_equal(good.cpu().numpy(), ref_winding("smoothed_sphere"))


def test_an_empty_mesh_gives_zeros():
    from ctunet_amd import mesh
    empty = mesh.Mesh(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    no_faces = mesh.Mesh(torch.ones((5, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"))
    for m in (empty, no_faces):
        v, w = mesh.voxelize(m, (3, 4, 5)), mesh.winding_number(m, (3, 4, 5), spacing=SPACING)
        assert v.dtype == torch.uint8 and w.dtype == torch.int32 and v.shape == w.shape == (3, 4, 5)
        assert v.is_cuda and not v.any() and not w.any()


def test_read_stl_to_the_device_and_voxelise():
    from ctunet_amd import mesh
    v, f = X.cube_mesh()
    got = mesh.read_stl(mesh.stl_bytes(v[f.reshape(-1)], np.arange(36).reshape(12, 3)))
    m = mesh.Mesh(got.vertices.to("cuda"), got.faces.to("cuda"))
    assert np.array_equal(mesh.winding_number(m, (6, 6, 6)).cpu().numpy(), cube_block())


def test_extract_smooth_voxelize_end_to_end():
    """The voxelised smoothed sphere against the smoothed mesh's own enclosed volume and against the source mask, at unit
    spacing on the source grid.

    The bound: the voxel count times the voxel volume is a midpoint rule for the enclosed volume, exact on every voxel the
    surface does not cut; a cut voxel contributes an error below one voxel volume.  Taubin smoothing moves a vertex of a
    sphere's staircase by less than half a voxel (test_mesh_smooth_cpu.py: at most 0.475 on the radius-7 sphere), so the
    surface stays within a voxel of the mask's boundary and the voxels it cuts are no more than the one-voxel shell of the
    source mask: the mask's voxels with a 6-neighbour outside it.  The shell's volume bounds the difference."""
    from ctunet_amd import mesh, metrics
    mask = sphere16()
    padded = np.pad(mask, 1)
    core = mask.copy()
    for axis in range(3):
        for shift in (-1, 1):
            core &= np.roll(padded, shift, axis=axis)[1:-1, 1:-1, 1:-1]
    shell_volume = float((mask & ~core & 1).sum())                                    # voxel volume 1
    assert 0 < shell_volume < 0.5 * mask.sum()
    vol = dev(mask)
    m = mesh.smooth(mesh.extract_surface(vol))
    out = mesh.voxelize(m, vol.shape)
    assert torch.equal(mesh.winding_number(m, vol.shape), out.to(torch.int32))        # every winding in {0, 1}
    enclosed = mesh.measure(m)[1].item()
    counted = float(out.sum().item())
    print(f"voxel count x voxel volume {counted:.3f}, enclosed volume {enclosed:.3f}, bound {shell_volume:.3f}")
    assert abs(counted - enclosed) <= shell_volume
    dice = metrics.surface_metrics(out, vol, 2)["dice"]
    o = out.cpu().numpy()
    want = 2.0 * (o & mask).sum() / (o.sum() + mask.sum())
    assert dice.shape == (1, 1) and dice.item() == pytest.approx(want, rel=1e-6)
