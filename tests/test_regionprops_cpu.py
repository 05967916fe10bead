"""The region-properties rule without a GPU: the numpy restatement (tests/regionprops_ref.py) against scipy.ndimage and
numpy.linalg, the argument checks of the wrappers, the box arithmetic of bounding_box, and the claim behind
register(init="moments") on the restated optimiser (tests/registration_ref.py)."""
import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import regionprops_ref as P
import registration_ref as G

EPS = np.finfo(np.float64).eps


def random_labels(shape, R, seed, density=0.6):
    rng = np.random.default_rng(seed)
    lab = rng.integers(1, R + 1, size=shape)
    return np.where(rng.random(shape) < density, lab, 0).astype(np.int64)


def blob_labels(shape, seed, density=0.35):
    """scipy's labelling of a smoothed random mask: connected regions of many voxels with distinct shapes."""
    rng = np.random.default_rng(seed)
    m = ndi.gaussian_filter(rng.random(shape), 1.5) > np.quantile(ndi.gaussian_filter(rng.random(shape), 1.5), 1 - density)
    return ndi.label(m)


@pytest.mark.parametrize("shape,R,seed", [((5, 7, 13), 6, 0), ((9, 21, 18), 40, 1), ((1, 1, 1), 3, 2), ((12, 10, 33), 300, 3)])
def test_integer_tables_are_scipys_sums_and_boxes(shape, R, seed):
    lab = random_labels(shape, R + 2, seed)                      # labels R + 1, R + 2 overflow
    lab[0, 0, 0] = -4
    mom, boxes, ovf = P.integer_tables(lab, R)
    assert mom.dtype == np.int64 and boxes.dtype == np.int32 and mom.shape == (1, R, 10) and boxes.shape == (1, R, 6)
    idx = np.arange(1, R + 1)
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
    terms = (np.ones(shape), z, y, x, z * z, z * y, z * x, y * y, y * x, x * x)
    for k, t in enumerate(terms):
        want = ndi.sum_labels(t, lab, idx)                       # float64, exact at these sizes
        assert np.array_equal(mom[0, :, k], want.astype(np.int64)), k
    assert ovf[0] == ((lab < 0) | (lab > R)).sum()
    found = ndi.find_objects(np.where((lab >= 1) & (lab <= R), lab, 0).astype(np.int32), max_label=R)
    for r, sl in enumerate(found):
        want = [0] * 6 if sl is None else [s.start for s in sl] + [s.stop for s in sl]
        assert boxes[0, r].tolist() == want, r


def test_batches_and_bool_masks():
    lab = np.stack([random_labels((6, 9, 20), 5, 10), np.zeros((6, 9, 20), dtype=np.int64), random_labels((6, 9, 20), 5, 11)])
    mom, boxes, ovf = P.integer_tables(lab, 5)
    for n in range(3):
        m1, b1, o1 = P.integer_tables(lab[n], 5)
        assert np.array_equal(mom[n], m1[0]) and np.array_equal(boxes[n], b1[0]) and ovf[n] == o1[0]
    assert not mom[1].any() and not boxes[1].any()
    mask = lab[0] > 2
    mb, bb, ob = P.integer_tables(mask, 1)
    assert mb[0, 0, 0] == mask.sum() and ob[0] == 0


@pytest.mark.parametrize("sampling,origin", [(None, None), ((0.8, 0.45, 0.5), (-12.0, 3.5, 100.0))])
def test_centroids_are_scipys_centres_of_mass(sampling, origin):
    lab, num = blob_labels((20, 24, 28), 5)
    R = num + 2                                                  # two empty regions
    _, _, _, centroid, _, _, _ = P.region_properties(lab, R, sampling, origin)
    com = np.array(ndi.center_of_mass(np.ones(lab.shape), lab, np.arange(1, num + 1)))
    sp = np.ones(3) if sampling is None else np.array(sampling)
    org = np.zeros(3) if origin is None else np.array(origin)
    want = org + sp * com
    assert np.all(np.abs(centroid[0, :num] - want) <= 1e-12 * np.maximum(np.abs(want), 1.0))
    assert np.isnan(centroid[0, num:]).all()


def check_axes(covariance, extent, axes, counts):
    """extent / axes against numpy.linalg.eigh of the same covariance on the regions whose eigenvalue gaps are at least 1 % of
    the largest eigenvalue, within 1e3 eps ||C|| / gap (float64 perturbation theory with a margin of 10^3), up to the sign
    rule, which is asserted separately, as is right-handedness.  Returns the number of regions checked."""
    checked = 0
    for C, w, A, n in zip(covariance.reshape(-1, 3, 3), extent.reshape(-1, 3), axes.reshape(-1, 3, 3), counts.reshape(-1)):
        if n < 2:
            assert np.isnan(A).all()
            continue
        assert np.array_equal(C, C.T)
        assert w[0] >= w[1] >= w[2]
        ew, ev = np.linalg.eigh(C)
        ew, ev = ew[::-1], ev[:, ::-1]
        norm = np.abs(C).sum(1).max()
        gap = min(ew[0] - ew[1], ew[1] - ew[2])
        assert np.all(np.abs(w - ew) <= 1e3 * EPS * norm)
        if norm == 0.0 or gap < 0.01 * ew[0]:
            continue
        checked += 1
        tol = 1e3 * EPS * norm / gap
        for j in range(3):
            assert abs(np.linalg.norm(A[:, j]) - 1.0) <= 16 * EPS
            s = 1.0 if np.dot(A[:, j], ev[:, j]) >= 0 else -1.0
            assert np.abs(A[:, j] - s * ev[:, j]).max() <= tol, (j, tol)
        for j in range(2):                                       # the sign rule: the first component of largest magnitude
            k = int(np.argmax(np.abs(A[:, j])))
            assert A[k, j] > 0
        assert np.array_equal(A[:, 2], np.cross(A[:, 0], A[:, 1]))
        assert abs(np.linalg.det(A) - 1.0) <= 64 * EPS           # right-handed in (z, y, x) index order
    return checked


@pytest.mark.parametrize("sampling", [None, (0.8, 0.45, 0.5)])
def test_extent_and_axes_agree_with_eigh(sampling):
    lab, num = blob_labels((24, 30, 36), 7)
    mom, _, _, _, cov, ext, axes = P.region_properties(lab, num + 1, sampling)
    assert check_axes(cov, ext, axes, mom[..., 0]) >= 5
    # an elongated box along y: the first axis is +y, the second +x (17 > 5 voxels), the third their cross product
    box = np.zeros((9, 40, 21), dtype=np.uint8)
    box[2:7, 3:37, 2:19] = 1
    _, _, _, c, _, e, a = P.region_properties(box, 1)
    assert np.array_equal(c[0, 0], [4.0, 19.5, 10.0])
    assert np.allclose(e[0, 0], [(34 ** 2 - 1) / 12, (17 ** 2 - 1) / 12, (5 ** 2 - 1) / 12], rtol=1e-14)
    assert np.array_equal(a[0, 0], np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))


def test_small_regions():
    lab = np.zeros((3, 4, 5), dtype=np.int64)
    lab[1, 2, 3] = 1                                             # one voxel
    lab[0, 0, 0] = lab[0, 0, 1] = 2                              # two voxels along x
    mom, boxes, _, c, cov, e, a = P.region_properties(lab, 3)
    assert np.array_equal(c[0, 0], [1.0, 2.0, 3.0]) and not cov[0, 0].any() and not e[0, 0].any() and np.isnan(a[0, 0]).all()
    assert np.array_equal(e[0, 1], [0.25, 0.0, 0.0]) and np.array_equal(a[0, 1][:, 0], [0.0, 0.0, 1.0])
    assert all(np.isnan(t[0, 2]).all() for t in (c, cov, e, a)) and boxes[0, 2].tolist() == [0] * 6


def test_arguments_are_checked_before_the_device():
    from ctunet_amd import postprocess
    ok = torch.zeros(4, 5, 6, dtype=torch.uint8)
    with pytest.raises(ValueError, match="must be one of"):
        postprocess.region_properties(torch.zeros(4, 5, 6, dtype=torch.int16), 3)
    with pytest.raises(ValueError, match="must be one of"):
        postprocess.region_properties(torch.zeros(4, 5, 6), 3)
    for bad in (0, -1, 65537, 2.0, True, None):
        with pytest.raises(ValueError, match="num_regions"):
            postprocess.region_properties(ok, bad)
    with pytest.raises(ValueError, match="sides up to 1024"):
        postprocess.region_properties(torch.zeros(1, 1, 1025, dtype=torch.uint8), 1)
    for bad in ((1.0, 2.0), -1.0, (1.0, 0.0, 1.0), "x", [(1.0, 1.0, 1.0)] * 2):
        with pytest.raises(ValueError, match="sampling"):
            postprocess.region_properties(ok, 1, sampling=bad)
    for bad in ((1.0, 2.0), float("nan"), (0.0, float("inf"), 0.0)):
        with pytest.raises(ValueError, match="origin"):
            postprocess.region_properties(ok, 1, origin=bad)
    with pytest.raises(ValueError, match="live on the GPU"):      # everything valid: only now the device is looked at
        postprocess.region_properties(ok, 65536, sampling=(0.5, 1.0, 2.0), origin=-3.0)
    with pytest.raises(ValueError, match="region must be"):
        postprocess.bounding_box(ok, region=3, num_regions=2)
    with pytest.raises(ValueError, match="margin"):
        postprocess.bounding_box(ok, margin=(1, 2))
    with pytest.raises(ValueError, match="multiple_of"):
        postprocess.bounding_box(ok, multiple_of=0)
    with pytest.raises(ValueError, match="live on the GPU"):
        postprocess.bounding_box(ok, margin=2, multiple_of=16)


SHAPE = (40, 64, 50)
BOXES = np.array([[0, 0, 0, 1, 1, 1],                            # a voxel in the corner
                  [39, 63, 49, 40, 64, 50],                      # in the opposite corner
                  [0, 10, 20, 40, 30, 29],                       # touching both z faces
                  [3, 0, 0, 37, 64, 50],                         # touching all y and x faces
                  [5, 6, 7, 22, 39, 48],
                  [0, 0, 0, 40, 64, 50],                         # the whole volume
                  [0, 0, 0, 0, 0, 0]], dtype=np.int32)          # empty
COUNTS = np.array([1, 1, 9, 9, 9, 9, 0])


@pytest.mark.parametrize("margin,multiple", [(0, 1), (3, 1), (0, 16), (2, 16), ((1, 0, 4), 8), (0, 48), (5, 7)])
def test_box_arithmetic(margin, multiple):
    """multiple_of = 16 cannot be reached along z = 40 by the z-spanning boxes without clipping (48 > 40), 48 by no axis but
    y; the wrapper's torch arithmetic equals the restatement, which is checked for its properties."""
    from ctunet_amd import postprocess
    want = P.bounding_box(BOXES, COUNTS, SHAPE, margin, multiple)
    mg = (margin,) * 3 if isinstance(margin, int) else margin
    got = postprocess._grow_boxes(torch.from_numpy(BOXES), torch.from_numpy(COUNTS != 0), SHAPE, mg, multiple)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    clipped = 0
    for b, n, w in zip(BOXES, COUNTS, want):
        for a in range(3):
            lo, hi, S = int(w[a]), int(w[3 + a]), SHAPE[a]
            assert 0 <= lo < hi <= S
            if n == 0:
                assert (lo, hi) == (0, S)
                continue
            grown = (max(b[a] - mg[a], 0), min(b[3 + a] + mg[a], S))
            assert lo <= grown[0] and grown[1] <= hi               # the grown box, clipped to the volume, is covered
            need = -(-(b[3 + a] - b[a] + 2 * mg[a]) // multiple) * multiple
            if need <= S:
                assert hi - lo == need
            else:
                assert (lo, hi) == (0, S)
                clipped += 1
    if multiple in (16, 48):
        assert clipped > 0


def test_crop_to_box_is_a_view_and_round_trips():
    from ctunet_amd import postprocess
    x = torch.arange(2 * 6 * 7 * 8, dtype=torch.float32).reshape(2, 6, 7, 8)
    view, slices = postprocess.crop_to_box(x, torch.tensor([[1, 2, 3, 5, 6, 8]], dtype=torch.int32))
    assert slices == (slice(1, 5), slice(2, 6), slice(3, 8)) and tuple(view.shape) == (2, 4, 4, 5)
    assert view.data_ptr() == x[0, 1, 2, 3:].data_ptr() and view._base is not None
    out = torch.zeros_like(x)
    out[(..., *slices)] = view * 2
    assert torch.equal(out[:, 1:5, 2:6, 3:8], x[:, 1:5, 2:6, 3:8] * 2) and out.sum() == (view * 2).sum()
    for bad in ([0, 0, 0, 7, 1, 1], [2, 0, 0, 2, 1, 1], [0, 0, 0, 1, 1], torch.zeros(2, 6, dtype=torch.int32)):
        with pytest.raises(ValueError):
            postprocess.crop_to_box(x, bad)


def test_moments_start_recovers_a_turned_skull_where_the_centroid_start_fails():
    """The restated optimiser on the turned fixture: from the centroid start it ends in a wrong basin (largest point error
    50.9 voxels measured, asserted > 10); the best of the five starts ends at 0.20 voxel (asserted < 0.5), and the selection
    rule picks it (final cost / P 0.109 against 0.376, 10.1 and 10.3)."""
    fixed, moving, truth = P.turned_fixture()
    points = P.surface_voxels(moving)
    field = ndi.distance_transform_edt(~fixed).astype(np.float32)
    cm = np.argwhere(moving).astype(np.float64).mean(0)
    cf = np.argwhere(fixed).astype(np.float64).mean(0)
    init = np.eye(4)
    init[:3, 3] = cf - cm
    M, _, _ = G.register(points, field, init=init, iterations=30)
    assert P.largest_point_error(M, points, truth) > 10.0
    pm = P.region_properties(moving, 1)
    pf = P.region_properties(fixed, 1)
    assert np.array_equal(pm[3][0, 0], cm) or np.abs(pm[3][0, 0] - cm).max() < 1e-12
    starts = P.moment_starts(pm[3][0, 0], pm[6][0, 0], pf[3][0, 0], pf[6][0, 0])
    assert len(starts) == 5
    for k, s in enumerate(starts):
        assert abs(np.linalg.det(s[:3, :3]) - 1.0) < 1e-12, k     # proper rotations
    results = [G.register(points, field, init=s, iterations=30) for s in starts]
    errors = [P.largest_point_error(r[0], points, truth) for r in results]
    best = int(np.argmin(errors))
    assert errors[best] < 0.5
    assert P.select_start([r[2][-1] for r in results]) == best


def test_selection_rule():
    rows = np.array([[0.5, 100.0], [0.1, 40.0], [0.3, 90.0], [0.3, 100.0], [np.nan, 100.0]])
    assert P.select_start(rows) == 2                             # 0.1 has fewer than half the inliers; the first 0.3 wins
    assert P.select_start(rows[:1]) == 0
    assert P.select_start(np.array([[0.0, 0.0], [0.0, 0.0]])) == 0
