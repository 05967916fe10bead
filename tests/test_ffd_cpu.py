"""The free-form deformation of ctunet_amd.registration without a GPU: the restated rule (tests/ffd_ref.py) against finite
differences and a dense Laplacian, on the warped analytic skull (test_registration_cpu's fixture under a smooth bump and an
anisotropic stretch), argument validation, and the C-ABI entry points in the header, the ctypes table and the built library."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import ffd_ref as R
import registration_ref as G
from test_registration_cpu import (CASES, CENTRE, FIXED_ORIGIN, FIXED_SHAPE, FIXED_SPACING, HOLE_CENTRE, HOLE_RADIUS, MOVING_ORIGIN,
                                   MOVING_SHAPE, MOVING_SPACING, centroid_init, fixed_side, shape, surface_points, world)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTROL_SPACING, STIFFNESS, ITERATIONS = 10.0, 0.1, 60
STRETCH = np.array((1.04, 0.97, 1.03))
BUMP, BUMP_CENTRE, BUMP_SIGMA = np.array((3.0, -2.0, 2.5)), np.array((44.0, 40.0, 44.0)), 12.0
# scene -> (case of test_registration_cpu, max_distance): 1 without the hole, 2 with it and the 6 mm bound
SCENES = {1: (1, None), 2: (2, 6.0)}


def phi(q):
    """The deformation of the head at fixed-frame points q [..., 3]: a 3-4 % anisotropic stretch and a 3 mm smooth bump."""
    d = q - BUMP_CENTRE
    return CENTRE + STRETCH * (q - CENTRE) + BUMP * np.exp(-(d * d).sum(-1, keepdims=True) / (2.0 * BUMP_SIGMA ** 2))


@functools.lru_cache(maxsize=None)
def scene(k):
    """dict: moving mask (with the hole in scene 2), full (the hole-free moving mask), points, bound and the restated rigid
    fit `affine` (30 iterations from the centroid start)."""
    case, bound = SCENES[k]
    w, t, hole, _ = CASES[case]
    T = G.rigid(w, t, CENTRE)
    pw = world(MOVING_SHAPE, MOVING_SPACING, MOVING_ORIGIN)
    tp = pw @ T[:3, :3].T + T[:3, 3]
    full = shape(phi(tp))
    moving = full & (np.sqrt(((tp - HOLE_CENTRE) ** 2).sum(-1)) >= HOLE_RADIUS) if hole else full
    points = surface_points(moving, MOVING_SPACING, MOVING_ORIGIN)
    fixed, field = fixed_side()
    affine, _, hist = G.register(points, field, FIXED_SPACING, FIXED_ORIGIN, centroid_init(moving, fixed), 30, bound)
    return dict(moving=moving, full=full, points=points, bound=bound, affine=affine, rigid_rms=float(np.sqrt(hist[-1, 0])))


@functools.lru_cache(maxsize=None)
def reference_fit(k):
    """The restatement's (control, history, lattice) on a scene: 60 iterations at h = 10 mm, stiffness 0.1."""
    c = scene(k)
    return R.fit(c["points"], fixed_side()[1], c["affine"], FIXED_SPACING, FIXED_ORIGIN, CONTROL_SPACING, STIFFNESS, ITERATIONS,
                 c["bound"])


def dice(a, b):
    return 2.0 * (a & b).sum() / (a.sum() + b.sum())


def _random_control(lat, amplitude, seed):
    return np.random.default_rng(seed).uniform(-amplitude, amplitude, (3, *lat[0]))


# ---- 1. weights, the transform, the regulariser --------------------------------------------------------------------------
def test_weights_sum_to_one_and_derivative_weights_are_finite_differences():
    f = np.linspace(0.0, 1.0, 257)
    B, dB = np.array(R.bspline(f)), np.array(R.dbspline(f))
    assert (B >= 0).all() and np.abs(B.sum(0) - 1.0).max() <= 4 * 2.0 ** -52
    assert np.abs(dB.sum(0)).max() <= 8 * 2.0 ** -52
    fm = np.linspace(0.01, 0.99, 99)
    e = 2.0 ** -12
    fd = (np.array(R.bspline(fm + e)) - np.array(R.bspline(fm - e))) / (2 * e)
    # a cubic's central difference is off by e^2 f''' / 6 with |f'''| <= 3, plus the rounding of the weights over 2 e
    assert np.abs(fd - np.array(R.dbspline(fm))).max() <= e * e / 2 + 8 * 2.0 ** -52 / e
    # continuity across a knot: the weights at f = 1 are those at f = 0 shifted by one control
    assert np.abs(B[1:, -1] - B[:3, 0]).max() <= 2.0 ** -52 and B[3, 0] == 0.0 and B[0, -1] == 0.0


def test_lattice_knot_and_jacobian():
    lat = R.lattice(FIXED_SHAPE, FIXED_SPACING, FIXED_ORIGIN, CONTROL_SPACING)
    assert lat[0] == (9, 10, 11)                                       # ceil(59 / 10) + 3, ceil(67 / 10) + 3, ceil(71 / 10) + 3
    assert R.lattice((4, 4, 4), 1.0, None, (50.0, 3.0, 1.5))[0] == (4, 4, 5)
    cell, f, free = R.knot(np.array([-3.0, 0.0, 9.99, 10.0, 59.0, 60.0, 75.0, np.nan, np.inf]), 0.0, 10.0, 6)
    assert cell.tolist() == [0, 0, 0, 1, 5, 5, 5, 0, 5]
    assert f[[0, 1, 3, 5, 6, 7, 8]].tolist() == [0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0]
    assert free.tolist() == [False, True, True, True, True, True, False, False, False]
    # the Jacobian determinant against central differences of the transform itself (float64 path of the restatement)
    rng = np.random.default_rng(3)
    ctl = _random_control(lat, 2.0, 4)
    M = G.rigid((0.02, -0.03, 0.01), (0.5, -0.25, 0.75), CENTRE)
    q = np.floor(rng.uniform(5.0, 50.0, (500, 3))) + rng.uniform(0.3, 0.7, (500, 3))     # q0 stays off the knots below
    p = (q - M[:3, 3]) @ M[:3, :3]                                                         # M^-1 q for a rotation

    def T(pp):
        q0 = G.apply(M, pp)
        cells, B, _ = R.weights([q0[:, a] for a in range(3)], lat)
        e = R.displacement(cells, B, ctl)
        return q0 + np.stack(e, 1)

    eps = 2.0 ** -10
    J = np.stack([(T(p + eps * M[:3, :3].T[b]) - T(p - eps * M[:3, :3].T[b])) / (2 * eps) for b in range(3)], axis=2)
    _, det = R.transform(p.astype(np.float32), M, lat, ctl, True)
    # float32 rounding moved the points by < 1e-5 mm; the determinant's slope is bounded by |c| / h^2 per mm
    assert np.abs(np.linalg.det(J) - det).max() < 1e-5
    # outside the box the displacement is constant along the clamped axis and the determinant ignores it
    far = np.array([[-40.0, 30.0, 30.0], [30.0, 30.0, 200.0]], np.float32)
    _, det = R.transform(far, np.eye(4), lat, ctl, True)
    moved = R.transform(far + np.array([[-5.0, 0, 0], [0, 0, 7.0]], np.float32), np.eye(4), lat, ctl)
    base = R.transform(far, np.eye(4), lat, ctl)
    assert np.abs((moved - base) - np.array([[-5.0, 0, 0], [0, 0, 7.0]])).max() < 1e-4 and np.isfinite(det).all()


def test_regulariser_is_the_graph_laplacian():
    lat = R.lattice((12, 9, 15), 1.0, None, (4.0, 3.0, 5.0))
    Gs = lat[0]
    c = _random_control(lat, 1.0, 6)
    n = int(np.prod(Gs))
    L = np.zeros((n, n))
    idx = np.arange(n).reshape(Gs)
    for ax in range(3):
        a, b = np.moveaxis(idx, ax, 0)[:-1].ravel(), np.moveaxis(idx, ax, 0)[1:].ravel()
        L[a, a] += 1; L[b, b] += 1; L[a, b] -= 1; L[b, a] -= 1
    w = 0.37
    rg, rd, _ = R.regulariser_gradient(c, w)
    flat = c.reshape(3, n)
    assert np.abs(rg.reshape(3, n) - w * flat @ L).max() <= 64 * 2.0 ** -52
    assert np.array_equal(rd.ravel(), 2.0 * w * np.diag(L))
    energy = sum(float(flat[a] @ L @ flat[a]) for a in range(3))
    assert abs(R.edges(c) - energy) <= 1e-12 * energy


def test_gradient_is_a_finite_difference_of_the_cost():
    c1 = scene(1)
    _, field = fixed_side()
    pts = c1["points"][::3]
    lat = R.lattice(FIXED_SHAPE, FIXED_SPACING, FIXED_ORIGIN, CONTROL_SPACING)
    ctl = _random_control(lat, 0.5, 8)
    w = 0.05
    acc = R.accumulate(pts, field, c1["affine"], lat, ctl, FIXED_SPACING, FIXED_ORIGIN, None, w)
    assert acc["count"] == len(pts) and (acc["diag"] > 0).all()
    rng = np.random.default_rng(9)
    d = rng.standard_normal(ctl.shape)
    d /= np.sqrt((d * d).sum())
    eps = 1e-4
    cp = R.accumulate(pts, field, c1["affine"], lat, ctl + eps * d, FIXED_SPACING, FIXED_ORIGIN, None, w)["cost"]
    cm = R.accumulate(pts, field, c1["affine"], lat, ctl - eps * d, FIXED_SPACING, FIXED_ORIGIN, None, w)["cost"]
    fd, an = (cp - cm) / (2 * eps), float((acc["grad"] * d).sum())
    print(f"directional derivative: finite difference {fd:.6f}, analytic {an:.6f}")
    # the cost is piecewise smooth (the trilinear cells): a few of 2300 points cross a voxel face within 1e-4 mm
    assert abs(fd - an) <= 2e-3 * max(abs(an), 1.0)


# ---- 2. the restatement on both scenes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sorted(SCENES))
def test_reference_halves_the_rigid_residual_without_folding(k):
    """Measured (restatement, 60 iterations, h = 10 mm, stiffness 0.1): scene 1, 6756 points, rms 0.6289 -> 0.2066 mm
    (0.329 x), 61 of 61 steps accepted, max |c| 3.04 mm, min det 0.881; scene 2 (hole, bound 6 mm), 6331 points, rms
    0.6408 -> 0.2071 mm (0.323 x), 61 of 61 accepted, max |c| 3.06 mm, min det 0.874.  The pulled atlas (next test): Dice
    0.788 rigid, 0.938 free-form."""
    c = scene(k)
    ctl, hist, lat = reference_fit(k)
    rms = float(hist[-1, 1])
    _, det = R.transform(c["points"], c["affine"], lat, ctl, True)
    print(f"scene {k}: P {len(c['points'])}, rigid rms {c['rigid_rms']:.4f}, start rms {hist[0, 1]:.4f}, final rms {rms:.4f} "
          f"({rms / c['rigid_rms']:.3f} x), accepted {int((hist[:, 5] == 1).sum())} of {len(hist)}, "
          f"max |c| {np.sqrt((ctl * ctl).sum(0)).max():.3f}, min det {det.min():.4f}, inliers {int(hist[-1, 3])}")
    assert 6000 <= len(c["points"]) <= 7500
    assert np.isfinite(hist).all() and (np.diff(hist[:, 0]) <= 0).all() and (hist[:, 5] >= 0).all() and hist[0, 5] == 1
    assert abs(hist[0, 1] - c["rigid_rms"]) < 1e-12                   # zero controls: the affine residual exactly
    assert rms <= 0.5 * c["rigid_rms"]
    assert det.min() > 0


def test_reference_pull_of_the_atlas_improves_dice():
    c = scene(1)
    ctl, _, lat = reference_fit(1)
    fixed = fixed_side()[0].astype(np.uint8)
    kw = dict(spacing=FIXED_SPACING, origin=FIXED_ORIGIN, out_spacing=MOVING_SPACING, out_origin=MOVING_ORIGIN,
              mode="label_linear", num_classes=2)
    before = R.deformable_resample(fixed, c["affine"], lat, np.zeros_like(ctl), MOVING_SHAPE, **kw)
    after = R.deformable_resample(fixed, c["affine"], lat, ctl, MOVING_SHAPE, **kw)
    import affine_ref as A
    assert np.array_equal(before, A.affine_resample(fixed, c["affine"], MOVING_SHAPE, **kw))
    d0, d1 = dice(before != 0, c["full"]), dice(after != 0, c["full"])
    print(f"Dice of the pulled atlas against the moving skull: rigid {d0:.4f}, free-form {d1:.4f}")
    assert d1 >= d0 + 0.05


def test_zero_iterations_and_zero_controls_are_the_affine_result():
    c = scene(1)
    _, field = fixed_side()
    ctl, hist, lat = R.fit(c["points"], field, c["affine"], FIXED_SPACING, FIXED_ORIGIN, CONTROL_SPACING, STIFFNESS, 0, None)
    assert not ctl.any() and hist.shape == (1, 6) and hist[0, 5] == 1
    acc = G.accumulate(c["points"], field, c["affine"], np.zeros(3), FIXED_SPACING, FIXED_ORIGIN, None)
    assert hist[0, 1] == np.sqrt(acc["cost"] / len(c["points"])) and hist[0, 3] == acc["count"] and hist[0, 2] == 0.0
    want = G.apply(c["affine"], c["points"].astype(np.float64)).astype(np.float32)
    got, det = R.transform(c["points"], c["affine"], lat, ctl, True)
    assert np.array_equal(got, want) and (det == 1.0).all()
    # a warm start of zero steps returns its controls
    warm = _random_control(lat, 1.0, 2)
    ctl, hist, _ = R.fit(c["points"], field, c["affine"], FIXED_SPACING, FIXED_ORIGIN, CONTROL_SPACING, STIFFNESS, 0, None, warm)
    assert np.array_equal(ctl, warm) and hist[0, 2] > 0


def test_reference_refuses_a_step_without_inliers():
    c = scene(1)
    _, field = fixed_side()
    ctl, hist, _ = R.fit(c["points"] + np.float32(500.0), field, np.eye(4), FIXED_SPACING, FIXED_ORIGIN, CONTROL_SPACING,
                         STIFFNESS, 3, None)
    assert not ctl.any() and (hist[:, 5] == -1).all() and np.isfinite(hist).all()


# ---- 3. the package without a GPU ----------------------------------------------------------------------------------------
def test_entry_points_declared_bound_and_exported():
    from ctunet_amd import _lib, mesh, registration, resample
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctunet_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("ctu_ffd_ws_bytes", 2), ("ctu_ffd_cells", 8), ("ctu_ffd_init", 7), ("ctu_ffd_accumulate", 20),
                        ("ctu_ffd_update", 12), ("ctu_ffd_transform_points", 10), ("ctu_ffd_resample", 23)):
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+CTU_FFD_SEGMENT\s+%d\b" % registration.FFD_SEGMENT, src)
    assert re.search(r"#define\s+CTU_FFD_MAX_G\s+%d\b" % registration.FFD_MAX_G, src) and registration.FFD_MAX_G == R.MAX_G
    for fn in (registration.register_ffd_points, registration.accumulate_ffd, registration.transform_points,
               registration.register_deformable, resample.deformable_resample, mesh.transform):
        assert callable(fn)
    assert _lib.load().ctu_abi_version() == _lib.ABI_VERSION
    ws = _lib.load().ctu_ffd_ws_bytes
    G4, G9 = (ctypes.c_int * 3)(4, 4, 4), (ctypes.c_int * 3)(9, 10, 11)
    assert ws(G4, 1) == 1024 + 8 * (13 * 64 + 2 + 256) and ws(G9, 7) == 1024 + 8 * (13 * 990 + 7 * 258)
    assert ws(G4, 0) == 0 and ws((ctypes.c_int * 3)(3, 4, 4), 1) == 0 and ws((ctypes.c_int * 3)(4, 65, 4), 1) == 0
    assert registration.ffd_lattice(FIXED_SHAPE, FIXED_SPACING, FIXED_ORIGIN, CONTROL_SPACING)[0] == (9, 10, 11)


def test_bad_arguments_raise_before_any_launch():
    from ctunet_amd import mesh, registration as reg, resample
    pts, field, eye = torch.zeros(8, 3), torch.zeros(40, 50, 60), torch.eye(4, dtype=torch.float64)
    with pytest.raises(ValueError, match="registration.*GPU"):
        reg.register_ffd_points(pts, field, eye)
    with pytest.raises(TypeError, match="registration.*float32"):
        reg.register_ffd_points(pts.double(), field, eye)
    with pytest.raises(ValueError, match=r"registration.*\[P,3\]"):
        reg.register_ffd_points(torch.zeros(8, 2), field, eye)
    with pytest.raises(ValueError, match="registration.*iterations"):
        reg.register_ffd_points(pts, field, eye, iterations=-1)
    with pytest.raises(ValueError, match="registration.*stiffness"):
        reg.register_ffd_points(pts, field, eye, stiffness=-0.1)
    with pytest.raises(ValueError, match="registration.*max_distance"):
        reg.register_ffd_points(pts, field, eye, max_distance=-1.0)
    with pytest.raises(ValueError, match="registration.*control_spacing"):
        reg.register_ffd_points(pts, field, eye, control_spacing=0.0)
    with pytest.raises(ValueError, match="registration.*more than 64"):
        reg.register_ffd_points(pts, field, eye, control_spacing=(10.0, 10.0, 0.9))
    with pytest.raises(ValueError, match="registration.*matrix"):
        reg.register_ffd_points(pts, field, None)
    with pytest.raises(ValueError, match="registration.*more than 64"):
        reg.register_deformable(torch.zeros(4, 5, 6, dtype=torch.uint8), torch.zeros(40, 50, 200, dtype=torch.uint8),
                                control_spacing=3.0)
    good = reg.DeformableResult(eye, torch.zeros(3, 4, 4, 4, dtype=torch.float64), (10.0, 10.0, 10.0), (0.0, 0.0, 0.0),
                                (9.0, 9.0, 9.0))
    with pytest.raises(TypeError, match="registration.*DeformableResult"):
        reg.transform_points(pts, eye)
    with pytest.raises(ValueError, match="registration.*control"):
        reg.transform_points(pts, good._replace(control=torch.zeros(3, 4, 4, 3, dtype=torch.float64)))
    with pytest.raises(ValueError, match="registration.*control"):
        reg.transform_points(pts, good._replace(control=torch.zeros(3, 4, 4, 4)))
    with pytest.raises(ValueError, match="registration.*control_spacing"):
        reg.transform_points(pts, good._replace(control_spacing=(1.0, -1.0, 1.0)))
    with pytest.raises(ValueError, match="registration.*GPU"):
        reg.transform_points(pts, good)
    with pytest.raises(ValueError, match="registration.*GPU"):
        mesh.transform(mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)), good)
    vol = torch.zeros(4, 5, 6, dtype=torch.uint8)
    with pytest.raises(ValueError, match="deformable_resample.*GPU"):
        resample.deformable_resample(vol, good, (4, 5, 6), mode="nearest")
    with pytest.raises(TypeError, match="registration.*DeformableResult"):
        resample.deformable_resample(vol, eye, (4, 5, 6), mode="nearest")
    with pytest.raises(ValueError, match="deformable_resample.*fill"):
        resample.deformable_resample(vol, good, (4, 5, 6), mode="nearest", fill=300)
    assert good.report()["max_displacement"] == 0.0
