"""ctunet_amd.postprocess.region_properties / bounding_box / crop_to_box and registration.register(init="moments") on the GPU
against the restated rule (tests/regionprops_ref.py).

The shapes are chosen against the kernel's constants (csrc/regionprops.hip): a lane reads 16 x-consecutive voxels, a tile is
256 lanes, the LDS table has 128 slots and gives up after 8 probes, a wave sums for a label that at least 8 of its lanes
end with, and at most 2048 blocks are launched over all items, so a block walks several tiles only above 2048 tiles."""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import regionprops_ref as P
import registration_ref as G
from test_regionprops_cpu import check_axes

pytestmark = pytest.mark.gpu
DEV = "cuda"
TORCH = {"bool": torch.bool, "uint8": torch.uint8, "int32": torch.int32, "int64": torch.int64}
# below, at and just above the lane's 16 voxels and the tile's 256 lanes; rows that start off a 16-byte boundary (13, 70, 17)
SHAPES = [(5, 7, 13), (9, 21, 70), (40, 48, 72), (3, 4, 1024), (1, 1, 1), (2, 3, 16), (4, 8, 17), (16, 16, 16), (1, 257, 16),
          (7, 5, 33)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(t):
    return t.cpu().numpy()


def check(got, lab, R, sampling=None, origin=None):
    """Every field of a RegionProperties against the restatement of the host label map `lab`."""
    mom, boxes, ovf, cen, cov, ext, axes = P.region_properties(lab, R, sampling, origin)
    assert got.moments.dtype == torch.int64 and got.boxes.dtype == torch.int32 and got.overflow.dtype == torch.int64
    assert np.array_equal(_host(got.moments), mom)
    assert np.array_equal(_host(got.boxes), boxes)
    assert np.array_equal(_host(got.overflow), ovf)
    # float64 division is correctly rounded on both sides and nothing is contracted: bit for bit
    assert np.array_equal(_host(got.centroid), cen, equal_nan=True)
    assert np.array_equal(_host(got.covariance), cov, equal_nan=True)
    gext, gaxes = _host(got.extent), _host(got.axes)
    assert np.array_equal(np.isnan(gext), np.isnan(ext)) and np.array_equal(np.isnan(gaxes), np.isnan(axes))
    check_axes(cov, gext, gaxes, mom[..., 0])
    return mom


@functools.lru_cache(maxsize=None)
def random_case(shape, seed, R, top):
    """Labels 0..top in runs along x (labels change rarely along x, but do change inside a lane)."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, top + 1, size=shape)
    keep = rng.random(shape) < 0.35                              # a voxel keeps its own label, else repeats its left neighbour's
    keep[..., 0] = True
    idx = np.maximum.accumulate(np.where(keep, np.arange(shape[-1]), 0), axis=-1)
    return np.take_along_axis(lab, idx, axis=-1).astype(np.int64)


@pytest.mark.parametrize("dtype", ["uint8", "int32", "int64"])
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_and_dtypes(shape, dtype):
    from ctunet_amd import postprocess
    R = 5
    lab = random_case(shape, sum(shape), R, R + 2)                # labels 6 and 7 overflow
    got = postprocess.region_properties(_dev(lab).to(TORCH[dtype]), R)
    mom = check(got, lab, R)
    assert mom[..., 0].sum() + _host(got.overflow).sum() == (lab != 0).sum()


@pytest.mark.parametrize("shape", [(5, 7, 13), (9, 21, 70), (3, 4, 1024)])
def test_bool_masks(shape):
    from ctunet_amd import postprocess
    lab = random_case(shape, 3, 1, 1)
    check(postprocess.region_properties(_dev(lab != 0), 1), lab, 1)
    check(postprocess.region_properties(_dev(lab != 0), 4), lab, 4)


@pytest.mark.parametrize("dtype", ["uint8", "int32", "int64"])
def test_views_and_unaligned_storage(dtype):
    """A non-contiguous view (made contiguous by the wrapper) and a contiguous tensor whose storage starts one element off a
    16-byte boundary, so that no lane can take a 16-byte load."""
    from ctunet_amd import postprocess
    lab = random_case((12, 20, 96), 8, 6, 6)
    t = _dev(lab).to(TORCH[dtype])
    view = t[:, ::2, 5:85]
    assert not view.is_contiguous()
    check(postprocess.region_properties(view, 6), lab[:, ::2, 5:85], 6)
    flat = torch.empty(lab.size + 1, dtype=TORCH[dtype], device=DEV)
    off = flat[1:].view(lab.shape)
    off.copy_(t)
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    check(postprocess.region_properties(off, 6), lab, 6)


@pytest.mark.parametrize("N", [1, 3])
def test_batches_sampling_and_origin(N):
    from ctunet_amd import postprocess
    lab = np.stack([random_case((9, 21, 70), 20 + n, 7, 7) for n in range(N)])
    if N == 3:
        lab[1] = 0                                               # one item all background
    sampling = [(0.8, 0.45, 0.5), (1.0, 1.0, 1.0), (2.0, 0.25, 1.5)][:N]
    origin = [(-12.0, 3.5, 100.0), (0.0, 0.0, 0.0), (1e3, -1e3, 0.125)][:N]
    got = postprocess.region_properties(_dev(lab).to(torch.int32), 7, sampling=sampling, origin=origin)
    assert tuple(got.moments.shape) == (N, 7, 10) and tuple(got.axes.shape) == (N, 7, 3, 3)
    check(got, lab, 7, np.array(sampling), np.array(origin))
    got = postprocess.region_properties(_dev(lab[0]).to(torch.int32), 7, sampling=0.5, origin=(1.0, 2.0, 3.0))
    assert tuple(got.moments.shape) == (1, 7, 10)
    check(got, lab[0], 7, 0.5, (1.0, 2.0, 3.0))


def test_one_region_fills_the_volume_and_touches_all_faces():
    from ctunet_amd import postprocess
    shape = (17, 33, 130)
    full = np.ones(shape, dtype=np.int64)
    got = postprocess.region_properties(_dev(full).to(torch.uint8), 1)
    check(got, full, 1)
    assert _host(got.boxes)[0, 0].tolist() == [0, 0, 0, 17, 33, 130]
    cross = np.zeros(shape, dtype=np.int64)                      # three bars through the centre: region 2 touches six faces
    cross[8, 16, :] = cross[8, :, 65] = cross[:, 16, 65] = 2
    cross[0, 0, 0] = 1
    got = postprocess.region_properties(_dev(cross), 2)
    check(got, cross, 2)
    assert _host(got.boxes)[0, 1].tolist() == [0, 0, 0, 17, 33, 130]


@pytest.mark.parametrize("density", [0.05, 0.3, 0.7])
def test_labelled_components_with_room_and_without(density):
    """label() of a random mask: hundreds of labels per tile at the low densities (slots fill up, flushes between tiles, labels
    that find no slot), a few large ones at 0.7.  With R below the number of components the overflow is the voxel count of
    the regions left out."""
    from ctunet_amd import postprocess
    rng = np.random.default_rng(int(density * 100))
    mask = rng.random((24, 40, 72)) < density
    labels, num = postprocess.label(_dev(mask), connectivity=1)
    lab = _host(labels)
    k = int(num.item())
    assert k == ndi.label(mask)[1] and k > 8
    check(postprocess.region_properties(labels, k + 5), lab, k + 5)
    small = k // 2
    got = postprocess.region_properties(labels, small)
    check(got, lab, small)
    assert int(got.overflow.item()) == int((lab > small).sum()) > 0


def test_negative_and_large_int64_labels():
    from ctunet_amd import postprocess
    lab = random_case((9, 21, 70), 41, 5, 5).copy()
    rng = np.random.default_rng(41)
    lab[rng.random(lab.shape) < 0.1] = -3
    lab[rng.random(lab.shape) < 0.05] = np.iinfo(np.int64).min
    lab[rng.random(lab.shape) < 0.05] = (1 << 40) + 2            # its low 32 bits are a valid label
    got = postprocess.region_properties(_dev(lab), 5)
    check(got, lab, 5)
    assert int(got.overflow.item()) == int(((lab < 0) | (lab > 5)).sum())
    neg32 = np.where(lab < 0, -7, np.minimum(lab, 9))
    check(postprocess.region_properties(_dev(neg32).to(torch.int32), 5), neg32, 5)


@pytest.mark.parametrize("dtype,R", [("int32", 5000), ("int64", 65536), ("uint8", 255)])
def test_noise_map_takes_the_spill_path(dtype, R):
    """Independent labels per voxel: every lane ends a run at every voxel, and a tile of 4096 voxels holds far more distinct
    labels than the 128 slots of the block's table, so most updates go straight to the global accumulators."""
    from ctunet_amd import postprocess
    lab = np.random.default_rng(R).integers(0, R + 1, size=(8, 32, 48)).astype(np.int64)
    assert len(np.unique(lab[0, :, :])) > 128
    check(postprocess.region_properties(_dev(lab).to(TORCH[dtype]), R), lab, R)


def test_blocks_that_walk_several_tiles():
    """16 items of 136 tiles each: the grid holds 128 blocks per item, so blocks take two tiles and keep their table between
    them.  Every item holds the same map: one restatement serves all."""
    from ctunet_amd import postprocess
    lab = random_case((32, 64, 272), 77, 3, 3)
    got = postprocess.region_properties(_dev(lab).to(torch.uint8).expand(16, -1, -1, -1), 3)
    mom, boxes, ovf = P.integer_tables(lab, 3)
    assert np.array_equal(_host(got.moments), np.broadcast_to(mom, (16, 3, 10)))
    assert np.array_equal(_host(got.boxes), np.broadcast_to(boxes, (16, 3, 6)))
    assert not _host(got.overflow).any()


def test_two_calls_are_bit_equal():
    from ctunet_amd import postprocess
    lab = _dev(np.random.default_rng(5).integers(0, 301, size=(16, 40, 100))).to(torch.int32)
    a = postprocess.region_properties(lab, 300, sampling=(0.7, 0.9, 1.1))
    b = postprocess.region_properties(lab, 300, sampling=(0.7, 0.9, 1.1))
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                           y.view(torch.int64) if y.dtype == torch.float64 else y)


def test_graph_capture_and_replay_on_changed_input():
    from ctunet_amd import postprocess
    first = random_case((9, 21, 70), 50, 6, 6)
    second = random_case((9, 21, 70), 51, 6, 6)
    static = _dev(first).to(torch.int32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        postprocess.region_properties(static, 6)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = postprocess.region_properties(static, 6, sampling=(0.8, 0.45, 0.5))
    graph.replay()
    check(got, first, 6, (0.8, 0.45, 0.5))
    static.copy_(_dev(second).to(torch.int32))
    graph.replay()
    check(got, second, 6, (0.8, 0.45, 0.5))


@pytest.mark.parametrize("margin,multiple", [(0, 1), (2, 16), ((1, 0, 4), 8), (0, 48)])
def test_bounding_box(margin, multiple):
    from ctunet_amd import postprocess
    shape = (40, 64, 50)
    lab = np.zeros((4,) + shape, dtype=np.int64)
    lab[0, 0, 0, 0] = 2                                          # a voxel in the corner
    lab[1, 5:22, 6:39, 7:48] = 2
    lab[1, 0:3, 0:3, 0:3] = 1
    lab[2, :, 10:30, 20:29] = 2                                  # spans z: 16 and 48 cannot be reached without clipping
    lab[3, 3, 3, 3] = 1                                          # region 2 is empty: the whole volume
    got = postprocess.bounding_box(_dev(lab).to(torch.uint8), region=2, margin=margin, multiple_of=multiple)
    assert got.dtype == torch.int32 and tuple(got.shape) == (4, 6)
    mom, boxes, _ = P.integer_tables(lab, 2)
    assert np.array_equal(_host(got), P.bounding_box(boxes[:, 1], mom[:, 1, 0], shape, margin, multiple))
    assert _host(got)[3].tolist() == [0, 0, 0, 40, 64, 50]
    one = postprocess.bounding_box(_dev(lab[1] == 2), margin=margin, multiple_of=multiple)
    assert np.array_equal(_host(one), _host(got)[1:2])


def test_crop_to_box_is_a_view_and_round_trips():
    from ctunet_amd import postprocess
    mask = np.zeros((20, 30, 40), dtype=bool)
    mask[4:9, 11:20, 13:33] = True
    x = torch.arange(2 * 20 * 30 * 40, dtype=torch.float32, device=DEV).reshape(2, 20, 30, 40)
    box = postprocess.bounding_box(_dev(mask), margin=1, multiple_of=4)
    view, slices = postprocess.crop_to_box(x, box)
    assert all((s.stop - s.start) % 4 == 0 for s in slices) and tuple(view.shape[1:]) == tuple(s.stop - s.start for s in slices)
    lo, hi = x.data_ptr(), x.data_ptr() + x.numel() * 4
    assert lo <= view.data_ptr() < hi and view._base is not None
    assert view.data_ptr() == x[0, slices[0].start, slices[1].start, slices[2].start:].data_ptr()
    assert bool(_dev(mask)[slices].sum() == int(mask.sum()))     # the region lies inside the crop
    out = torch.zeros_like(x)
    out[(..., *slices)] = view + 1
    assert torch.equal(out[(..., *slices)], x[(..., *slices)] + 1) and float(out.sum()) == float((view + 1).sum())


# ---- register(init="moments") -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def turned():
    fixed, moving, truth = P.turned_fixture()
    return fixed, moving, truth, P.surface_voxels(moving)


def test_principal_frame_is_the_restatement():
    from ctunet_amd import registration as reg
    fixed, moving, _, _ = turned()
    for mask, sp, org in ((fixed, None, None), (moving, (0.8, 0.45, 0.5), (3.0, -2.0, 1.0))):
        c, a, e = reg.principal_frame(_dev(mask), sp, org)
        _, _, _, cen, cov, ext, axes = P.region_properties(mask, 1, sp, org)
        assert tuple(c.shape) == (3,) and tuple(a.shape) == (3, 3) and tuple(e.shape) == (3,)
        assert np.array_equal(_host(c), cen[0, 0])
        check_axes(cov, _host(e)[None], _host(a)[None], np.array([mask.sum()]))
        c8, a8, e8 = reg.principal_frame(_dev(mask.astype(np.uint8) * 7), sp, org)      # any nonzero value is foreground
        assert torch.equal(c8, c) and torch.equal(a8, a) and torch.equal(e8, e)


def test_moments_start_recovers_the_turned_skull():
    """candidate is the start the restatement picks (3, the sign choice (-,-,+)), and the largest point error is below 0.5
    voxel (0.20 in the restatement); the centroid start ends above 10 voxels (50.9) on the same input."""
    from ctunet_amd import registration as reg
    fixed, moving, truth, points = turned()
    field = ndi.distance_transform_edt(~fixed).astype(np.float32)
    pm, pf = P.region_properties(moving, 1), P.region_properties(fixed, 1)
    starts = P.moment_starts(pm[3][0, 0], pm[6][0, 0], pf[3][0, 0], pf[6][0, 0])
    want = P.select_start([G.register(points, field, init=s, iterations=30)[2][-1] for s in starts])
    r = reg.register(_dev(moving), _dev(fixed), init="moments")
    assert r.candidate.dtype == torch.int64 and r.candidate.dim() == 0 and r.candidate.is_cuda
    assert int(r.candidate) == want
    assert P.largest_point_error(_host(r.matrix), points, truth) < 0.5
    assert tuple(r.history.shape) == (31, 4) and r.num_points == len(points)
    assert np.allclose(_host(r.matrix) @ _host(r.inverse), np.eye(4), atol=1e-12)


def test_centroid_start_is_untouched_and_fails_on_the_turned_skull():
    """The default takes the parent commit's code path, restated here from its operations, bit for bit; candidate is None."""
    from ctunet_amd import postprocess, registration as reg
    fixed, moving, truth, points = turned()
    mv, fx = _dev(moving), _dev(fixed)
    r = reg.register(mv, fx)
    assert r.candidate is None and len(r) == 6
    pts = reg.surface_points(mv)
    field = postprocess.distance_transform_edt(~fx)
    init = torch.eye(4, dtype=torch.float64, device=DEV)
    init[:3, 3] = torch.nonzero(fx).to(torch.float64).mean(0) - torch.nonzero(mv).to(torch.float64).mean(0)
    old = reg.register_points(pts, field, init=init, iterations=30)
    for a, b in ((r.matrix, old.matrix), (r.inverse, old.inverse), (r.history, old.history)):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert P.largest_point_error(_host(r.matrix), points, truth) > 10.0
    matrix, inverse, history, num_points, num_fixed = reg.RegistrationResult(r.matrix, r.inverse, r.history, 3, 4)[:5]
    assert (num_points, num_fixed) == (3, 4)                     # existing constructions and unpackings keep working


def test_moments_start_with_the_similarity_model():
    """The symmetric similarity fit from the five starts.  tests/similarity_ref.py ends at 0.21 voxel from start 3 on this
    fixture (cost / (P + Q) 0.088 against 0.34 and more for the others), so the cap of 0.5 voxel holds here as well."""
    import similarity_ref as S
    from ctunet_amd import registration as reg
    fixed, moving, truth, points = turned()
    field = ndi.distance_transform_edt(~fixed).astype(np.float32)
    mfield = ndi.distance_transform_edt(~moving).astype(np.float32)
    fpoints = P.surface_voxels(fixed)
    pm, pf = P.region_properties(moving, 1), P.region_properties(fixed, 1)
    starts = P.moment_starts(pm[3][0, 0], pm[6][0, 0], pf[3][0, 0], pf[6][0, 0])
    refs = [S.register(points, field, fixed_points=fpoints, moving_field=mfield, init=s, iterations=30, dof=7) for s in starts]
    want = P.select_start([h[-1] for _, _, h in refs])
    assert P.largest_point_error(refs[want][0], points, truth) < 0.5
    r = reg.register(_dev(moving), _dev(fixed), init="moments", model="similarity")
    assert int(r.candidate) == want
    assert P.largest_point_error(_host(r.matrix), points, truth) < 0.5
    assert tuple(r.history.shape) == (31, 6) and r.num_fixed_points == len(fpoints)
