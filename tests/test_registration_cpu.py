"""Rigid registration of ctunet_amd.registration without a GPU: the restated rule (tests/registration_ref.py) against scipy
and on the analytic skull fixture, argument validation, and the C-ABI entry points in the header, the ctypes table and the
built library."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import registration_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the analytic fixture: a cut ellipsoid shell with two bumps that break every symmetry -------------------------------
CENTRE = np.array((30.0, 34.0, 36.0))
FIXED_SHAPE, FIXED_SPACING, FIXED_ORIGIN = (60, 68, 72), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
MOVING_SHAPE, MOVING_SPACING, MOVING_ORIGIN = (52, 60, 50), (1.2, 1.1, 1.5), (-2.0, 1.5, -1.0)
HOLE_CENTRE, HOLE_RADIUS = np.array((45.0, 30.0, 20.0)), 12.0
# (w, t, hole, max_distance)
CASES = {
    1: ((0.10, -0.07, 0.12), (3.0, -2.0, 4.0), False, None),
    2: ((0.10, -0.07, 0.12), (3.0, -2.0, 4.0), True, None),
    3: ((0.20, 0.15, -0.25), (-5.0, 4.0, 3.0), True, None),
    4: ((0.20, 0.15, -0.25), (-5.0, 4.0, 3.0), True, 6.0),
    5: ((0.35, -0.30, 0.30), (6.0, -6.0, 5.0), True, None),
}


def _ellipsoid(p, centre, axes):
    return np.sqrt((((p - np.asarray(centre)) / np.asarray(axes)) ** 2).sum(-1))


def shape(p):
    """The object at world points p [..., 3] in (z, y, x)."""
    rho = _ellipsoid(p, CENTRE, (22.0, 26.0, 30.0))
    shell = (rho >= 0.86) & (rho <= 1.0) & (p[..., 0] > 14.0)
    return shell | (_ellipsoid(p, (34.0, 34.0, 66.0), (5.0, 9.0, 5.0)) <= 1.0) | \
        (_ellipsoid(p, (40.0, 14.0, 30.0), (4.0, 4.0, 7.0)) <= 1.0)


def world(shape_, spacing, origin):
    idx = np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape_), indexing="ij"), axis=-1)
    return np.asarray(origin) + idx * np.asarray(spacing)


def surface_points(mask, spacing, origin):
    """float32 world coordinates of mask & ~binary_erosion(mask), in C order of the voxels."""
    surf = mask & ~ndi.binary_erosion(mask)
    return (np.asarray(origin) + np.argwhere(surf).astype(np.float64) * np.asarray(spacing)).astype(np.float32)


def centroid_init(moving, fixed):
    M = np.eye(4)
    cm = (np.asarray(MOVING_ORIGIN) + np.argwhere(moving).astype(np.float64) * np.asarray(MOVING_SPACING)).mean(0)
    cf = (np.asarray(FIXED_ORIGIN) + np.argwhere(fixed).astype(np.float64) * np.asarray(FIXED_SPACING)).mean(0)
    M[:3, 3] = cf - cm
    return M


@functools.lru_cache(maxsize=None)
def fixed_side():
    """(fixed mask, float32 distance field in mm to the fixed object)."""
    fixed = shape(world(FIXED_SHAPE, FIXED_SPACING, FIXED_ORIGIN))
    field = ndi.distance_transform_edt(~fixed, sampling=FIXED_SPACING).astype(np.float32)
    return fixed, field


@functools.lru_cache(maxsize=None)
def fixture_case(case):
    """dict: T [4,4] (moving world -> fixed world), moving mask, hole-free region of the fixed grid, points, init, bound."""
    w, t, hole, bound = CASES[case]
    T = G.rigid(w, t, CENTRE)
    pw = world(MOVING_SHAPE, MOVING_SPACING, MOVING_ORIGIN)
    tp = pw @ T[:3, :3].T + T[:3, 3]
    moving = shape(tp)
    if hole:
        moving &= np.sqrt(((tp - HOLE_CENTRE) ** 2).sum(-1)) >= HOLE_RADIUS
    fixed, _ = fixed_side()
    fw = world(FIXED_SHAPE, FIXED_SPACING, FIXED_ORIGIN)
    clear = np.sqrt(((fw - HOLE_CENTRE) ** 2).sum(-1)) >= HOLE_RADIUS + 2.0 if hole else np.ones(FIXED_SHAPE, bool)
    return dict(T=T, moving=moving, clear=clear, points=surface_points(moving, MOVING_SPACING, MOVING_ORIGIN),
                init=centroid_init(moving, fixed), bound=bound)


def tre(M, T, points):
    p = points.astype(np.float64)
    return np.sqrt((((p @ M[:3, :3].T + M[:3, 3]) - (p @ T[:3, :3].T + T[:3, 3])) ** 2).sum(1))


@functools.lru_cache(maxsize=None)
def reference_result(case):
    """The restatement's (matrix, inverse, history) on a case: 30 iterations from the centroid start."""
    c = fixture_case(case)
    return G.register(c["points"], fixed_side()[1], FIXED_SPACING, FIXED_ORIGIN, c["init"], 30, c["bound"])


# ---- 1. the sample against scipy ---------------------------------------------------------------------------------------
def test_sample_is_scipys_map_coordinates_and_its_gradient_a_finite_difference():
    rng = np.random.default_rng(5)
    field = rng.standard_normal((9, 11, 13)).astype(np.float32)
    n = np.array(field.shape, dtype=np.float64)
    u = rng.random((4000, 3)) * (n - 1.0)
    u[:8] = np.array([[0, 0, 0], [8, 10, 12], [8, 0, 12], [3, 10, 5], [7.5, 10, 12], [8, 9.25, 0], [0, 0, 12], [4, 5, 6]])
    v, g, inside = G.sample(field, u)
    assert inside.all()
    want = ndi.map_coordinates(field.astype(np.float64), u.T, order=1, mode="nearest")
    # seven lerps of three float64 roundings each on values of magnitude max|field|
    assert np.abs(v - want).max() <= 32 * 2.0 ** -52 * np.abs(field).max()
    # the interpolant is trilinear inside one cell: a central difference along one axis is exact up to rounding
    u = np.floor(rng.random((2000, 3)) * (n - 1.0)) + 0.25 + 0.5 * rng.random((2000, 3))
    _, g, _ = G.sample(field, u)
    h = 0.125
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        fd = (G.sample(field, u + e)[0] - G.sample(field, u - e)[0]) / (2 * h)
        assert np.abs(fd - g[:, a]).max() <= 2.0 ** -44 * np.abs(field).max(), a
    # outside, on the far faces and non-finite
    u = np.array([[-1e-9, 1, 1], [8.0000001, 1, 1], [1, np.nan, 1], [np.inf, 1, 1], [8, 10, 12]])
    v, g, inside = G.sample(field, u)
    assert inside.tolist() == [False, False, False, False, True] and not v[:4].any() and not g[:4].any()
    assert v[4] == field[8, 10, 12]


def test_the_fixture_is_the_issues():
    fixed, field = fixed_side()
    assert fixed.shape == FIXED_SHAPE and field.dtype == np.float32
    for case in CASES:
        c = fixture_case(case)
        assert c["moving"].shape == MOVING_SHAPE
        assert 6000 <= len(c["points"]) <= 7500, (case, len(c["points"]))
        start = tre(c["init"], c["T"], c["points"]).mean()
        assert 3.0 <= start <= 11.5, (case, start)


# ---- 2. the restatement on the five cases -------------------------------------------------------------------------------
# measured (points, mean TRE, max TRE in mm) of the restatement, 30 iterations from the centroid start; every iteration was
# accepted and the final rms distance is 0.283-0.286 mm (the voxelisation of the two surfaces, not the fit)
#   case 1: 6982 points, 0.1719, 0.2980
#   case 2: 6563 points, 0.1505, 0.2897
#   case 3: 6565 points, 0.1054, 0.1308
#   case 4: 6565 points, 0.1054, 0.1308  (6550 inliers at the start, all 6565 from the second iteration on)
#   case 5: 6674 points, 0.1258, 0.2121


@pytest.mark.parametrize("case", sorted(CASES))
def test_reference_registers_the_fixture_below_half_a_voxel(case):
    c = fixture_case(case)
    M, inv, hist = reference_result(case)
    err = tre(M, c["T"], c["points"])
    print(f"case {case}: P {len(c['points'])}, mean TRE {err.mean():.4f}, max TRE {err.max():.4f}, "
          f"accepted {int((hist[:, 3] == 1).sum())}, rms {np.sqrt(hist[-1, 0]):.4f}")
    assert err.max() < 0.5
    assert (np.diff(hist[:, 0]) <= 0).all()                    # the cost never increases
    assert (hist[:, 3] >= 0).all() and hist[0, 3] == 1
    if c["bound"] is None:
        assert (hist[:, 1] == len(c["points"])).all()
    assert np.abs(inv @ M - np.eye(4)).max() < 1e-12
    assert np.abs(M[:3, :3] @ M[:3, :3].T - np.eye(3)).max() < 1e-13 and M[3].tolist() == [0, 0, 0, 1]


def test_reference_refuses_a_step_without_enough_inliers():
    _, field = fixed_side()
    c = fixture_case(1)
    for pts in (c["points"][:2], c["points"] + np.float32(500.0)):
        M, inv, hist = G.register(pts, field, FIXED_SPACING, FIXED_ORIGIN, c["init"], 5, None)
        assert np.array_equal(M, c["init"]) and (hist[:, 3] == -1).all() and np.isfinite(M).all()


# ---- 5. the entry points ------------------------------------------------------------------------------------------------
def test_entry_points_declared_bound_and_exported():
    import ctunet_amd
    from ctunet_amd import _lib, mesh, registration
    assert ctunet_amd.registration is registration and "registration" in ctunet_amd.__all__
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctunet_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("ctu_registration_ws_bytes", 1), ("ctu_registration_init", 5), ("ctu_registration_accumulate", 11),
                        ("ctu_registration_update", 8)):
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+CTU_REG_MAX_BLOCKS\s+%d\b" % registration.MAX_BLOCKS, src)
    assert re.search(r"#define\s+CTU_REG_MIN_INLIERS\s+%d\b" % G.MIN_INLIERS, src)
    assert callable(registration.register) and callable(registration.register_points) and callable(mesh.transform)
    assert _lib.load().ctu_abi_version() == _lib.ABI_VERSION
    ws = registration.workspace_bytes
    assert ws(1) > 0 and ws(257) > ws(1) and ws(10 ** 6) == ws(10 ** 7) and ws(0) == 0


def test_bad_arguments_raise_before_any_launch():
    from ctunet_amd import mesh, registration as reg
    pts, field = torch.zeros(8, 3), torch.zeros(4, 5, 6)
    with pytest.raises(ValueError, match="registration.*GPU"):
        reg.register_points(pts, field)
    with pytest.raises(TypeError, match="registration.*float32"):
        reg.register_points(pts.double(), field)
    with pytest.raises(TypeError, match="registration.*float32"):
        reg.register_points(pts, field.double())
    with pytest.raises(ValueError, match=r"registration.*\[P,3\]"):
        reg.register_points(torch.zeros(8, 2), field)
    with pytest.raises(ValueError, match="registration.*side"):
        reg.register_points(pts, torch.zeros(4, 1, 6))
    with pytest.raises(ValueError, match="registration.*iterations"):
        reg.register_points(pts, field, iterations=-1)
    with pytest.raises(ValueError, match="registration.*max_distance"):
        reg.register_points(pts, field, max_distance=-1.0)
    with pytest.raises(ValueError, match="registration.*spacing"):
        reg.register_points(pts, field, spacing=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="registration.*init"):
        reg.register(torch.zeros(4, 5, 6, dtype=torch.uint8), torch.zeros(4, 5, 6, dtype=torch.uint8), init="axes")
    with pytest.raises(ValueError, match="mesh.*matrix"):
        mesh.transform(mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)), torch.eye(3))
    m = mesh.transform(mesh.Mesh(torch.tensor([[1.0, 2.0, 3.0]]), torch.zeros(0, 3, dtype=torch.int32)),
                       torch.tensor(G.rigid((0.0, 0.0, 0.0), (1.0, -1.0, 0.5))))
    assert m.vertices.dtype == torch.float32 and m.vertices.tolist() == [[2.0, 1.0, 3.5]]
