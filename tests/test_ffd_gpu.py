"""ctunet_amd.registration's free-form deformation kernels on the GPU against the restated rule (tests/ffd_ref.py) on the
warped analytic skull of tests/test_ffd_cpu.py: one accumulation term by term, both scenes end to end, determinism and graph
replay, the transform of points with its Jacobian determinant, deformable_resample, and the pipeline
register_deformable -> deformable_resample."""
import numpy as np
import pytest
import torch

import ffd_ref as R
from test_ffd_cpu import (CONTROL_SPACING, ITERATIONS, SCENES, STIFFNESS, dice, reference_fit, scene)
from test_registration_cpu import (FIXED_ORIGIN, FIXED_SHAPE, FIXED_SPACING, MOVING_ORIGIN, MOVING_SHAPE, MOVING_SPACING, fixed_side)
from test_similarity_gpu import _tiled

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRAME = dict(spacing=FIXED_SPACING, origin=FIXED_ORIGIN)
LATTICE = dict(control_spacing=CONTROL_SPACING, stiffness=STIFFNESS)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _result(M, ctl, lat):
    from ctunet_amd import registration as reg
    extent = tuple((n - 1) * s for n, s in zip(FIXED_SHAPE, FIXED_SPACING))
    return reg.DeformableResult(_dev(np.asarray(M, np.float64)), _dev(np.asarray(ctl, np.float64)), tuple(lat[1]), tuple(lat[2]), extent)


# ---- 1. one accumulation -------------------------------------------------------------------------------------------------
# dyadic, scale 0.5: M p is exact for the planted points below
DYADIC = np.array([[0.5, 0, 0, 14.0], [0, 0.5, 0, 13.0], [0, 0, 0.5, 11.0], [0, 0, 0, 1.0]])
SIZES = (1, 63, 64, 65, 257, 100000)


def _points(P):
    """Scene 1's points tiled with jitter; from 63 on a NaN, an infinite and two far points (as test_similarity_gpu plants
    them), point 0 onto the last voxel centre (59, 67, 71) of the field, and from 63 on point 1 onto the knots t = (2, 3, 4)
    and point 2 onto t = ncell = (6, 7, 8)."""
    pts = _tiled(scene(1)["points"], P, P, True)
    pts[0] = (90.0, 108.0, 120.0)
    if P >= 63:
        pts[1] = (12.0, 34.0, 58.0)
        pts[2] = (92.0, 114.0, 138.0)
    return pts


@pytest.mark.parametrize("P", SIZES)
def test_one_accumulation_is_the_rule_term_by_term(P):
    """Both sides evaluate the same float64 expression per point, so only the order of summation differs: every entry of the
    gradient, the diagonal and the cost lies within P 2^-52 sum|term| of the restatement's and the inlier counts are equal.
    At 100 000 points every occupied cell spans several segments of 256.  Measured on the MI355X: exact at P = 1, at most
    0.022 of the bound up to P = 257, 0.00022 of it at 100 000 (411 segments over 38 cells, 472 over 134)."""
    from ctunet_amd import registration as reg
    c = scene(1)
    _, field = fixed_side()
    fd = _dev(field)
    pts = _points(P)
    pd = _dev(pts)
    lat = R.lattice(FIXED_SHAPE, FIXED_SPACING, FIXED_ORIGIN, CONTROL_SPACING)
    Gs = lat[0]
    assert Gs == (9, 10, 11)
    q0 = R.G.apply(DYADIC, pts[:3].astype(np.float64))
    assert (q0[0] == (59.0, 67.0, 71.0)).all()
    if P >= 63:
        assert (q0[1] == (20.0, 30.0, 40.0)).all() and (q0[2] == (60.0, 70.0, 80.0)).all()
    w = STIFFNESS * P / (Gs[0] * Gs[1] * Gs[2])
    random = np.random.default_rng(P).uniform(-2.0, 2.0, (3, *Gs))
    zero = np.zeros_like(random)
    combos = [("dyadic", DYADIC, "zero", zero, None), ("dyadic", DYADIC, "zero", zero, 3.0),
              ("dyadic", DYADIC, "random", random, None), ("dyadic", DYADIC, "random", random, 3.0),
              ("affine", c["affine"], "random", random, None)]
    for mname, M, cname, ctl, bound in combos:
        got = reg.accumulate_ffd(pd, fd, _dev(M), _dev(ctl), max_distance=bound, **FRAME, **LATTICE)
        want = R.accumulate(pts, field, M, lat, ctl, FIXED_SPACING, FIXED_ORIGIN, bound, w)
        assert got["count"] == want["count"], (mname, cname, bound)
        tol = P * 2.0 ** -52
        worst = 0.0
        for key, ab in (("grad", "absgrad"), ("diag", "absdiag"), ("cost", "cost"), ("sum2", "sum2")):
            err = np.abs(np.asarray(got[key]) - want[key])
            lim = tol * np.asarray(want[ab])
            worst = max(worst, float(np.max(err / np.maximum(lim, 1e-300))))
            assert (err <= lim).all(), (mname, cname, bound, key, float(err.max()))
        cells = np.unique(np.stack(R.weights([R.G.apply(M, pts.astype(np.float64))[:, a] for a in range(3)], lat)[0]), axis=1).shape[1]
        print(f"P {P} {mname} {cname} bound {bound}: {want['count']} inliers, {got['segments']} segments over {cells} cells, "
              f"worst error / bound {worst:.3g}")
        assert cells <= got["segments"] <= cells + P // reg.FFD_SEGMENT
        if P == 100000:
            assert got["segments"] > cells                              # cells that span segments
        if P == 1:
            assert got["segments"] == 1 and (np.asarray(got["grad"]) == want["grad"]).all()


# ---- 2. both scenes end to end -------------------------------------------------------------------------------------------
def _fit(k, **kw):
    from ctunet_amd import registration as reg
    c = scene(k)
    kw.setdefault("iterations", ITERATIONS)
    return reg.register_ffd_points(_dev(c["points"]), _dev(fixed_side()[1]), _dev(c["affine"]), max_distance=c["bound"], **FRAME,
                                   **LATTICE, **kw)


@pytest.mark.parametrize("k", sorted(SCENES))
def test_scene_end_to_end(k):
    """Measured on the MI355X: final rms 0.206607 mm (scene 1) and 0.207063 mm (scene 2), the restatement's to the digits
    printed; controls within 6.7e-16 mm of the restatement's; 61 of 61 steps accepted."""
    c = scene(k)
    ctl, hist, lat = reference_fit(k)
    r = _fit(k)
    got, h = r.control.cpu().numpy(), r.history.cpu().numpy()
    print(f"scene {k}: device rms {h[-1, 1]:.6f}, restatement {hist[-1, 1]:.6f}, max control difference "
          f"{np.abs(got - ctl).max():.3g} mm, accepted {int((h[:, 5] == 1).sum())}")
    assert h.shape == hist.shape and np.isfinite(h).all()
    assert (np.diff(h[:, 0]) <= 0).all() and (h[:, 5] >= 0).all()
    assert h[-1, 1] <= hist[-1, 1] + 0.01
    assert np.abs(got - ctl).max() <= 1e-6
    assert np.array_equal(h[:, 3:], hist[:, 3:])                        # inliers, lambda and flags step by step
    rep = r.report()
    assert rep["rms"] == h[-1, 1] and rep["rms_before"] == h[0, 1] and rep["accepted"] == int((h[:, 5] == 1).sum())
    assert rep["status"] == 0 and rep["iterations"] == ITERATIONS and rep["inlier_fraction"] == h[-1, 3] / len(c["points"])
    assert rep["max_displacement"] == float(np.sqrt((got * got).sum(0)).max())
    _, det = R.transform(c["points"], c["affine"], lat, got, True)
    assert rep["min_jacobian"] == det.min() > 0 and rep["folded"] == 0
    assert abs(h[0, 1] - c["rigid_rms"]) < 1e-9                         # zero controls: the affine residual


def test_zero_iterations_warm_start_and_refusal():
    from ctunet_amd import registration as reg
    c = scene(1)
    r = _fit(1, iterations=0)
    assert not r.control.cpu().numpy().any() and r.history.shape == (1, 6) and (r.jacobian.cpu().numpy() == 1.0).all()
    lat = R.lattice(FIXED_SHAPE, FIXED_SPACING, FIXED_ORIGIN, CONTROL_SPACING)
    warm = np.random.default_rng(2).uniform(-1.0, 1.0, (3, *lat[0]))
    r = _fit(1, iterations=0, init_control=_dev(warm))
    assert np.array_equal(r.control.cpu().numpy(), warm)
    ctl, hist, _ = R.fit(c["points"], fixed_side()[1], c["affine"], FIXED_SPACING, FIXED_ORIGIN, CONTROL_SPACING, STIFFNESS, 3,
                         None, warm)
    r = _fit(1, iterations=3, init_control=_dev(warm))
    assert np.abs(r.control.cpu().numpy() - ctl).max() <= 1e-9 and np.array_equal(r.history.cpu().numpy()[:, 3:], hist[:, 3:])
    # no inlier: every step is refused and nothing moves
    far = reg.register_ffd_points(_dev(c["points"] + np.float32(500.0)), _dev(fixed_side()[1]),
                                  torch.eye(4, dtype=torch.float64, device=DEV), iterations=3, **FRAME, **LATTICE)
    h = far.history.cpu().numpy()
    assert (h[:, 5] == -1).all() and np.isfinite(h).all() and not far.control.cpu().numpy().any()
    assert far.report()["status"] == -1


# ---- 3. determinism ------------------------------------------------------------------------------------------------------
def test_two_calls_and_a_graph_replay_are_bit_equal():
    from ctunet_amd import registration as reg
    c = scene(2)
    args = (_dev(c["points"]), _dev(fixed_side()[1]), _dev(c["affine"]))
    kw = dict(max_distance=c["bound"], iterations=12, **FRAME, **LATTICE)
    a = reg.register_ffd_points(*args, **kw)
    b = reg.register_ffd_points(*args, **kw)
    torch.cuda.synchronize()
    keep = [t.clone() for t in (a.control, a.history, a.jacobian)]
    for x, y in zip(keep, (b.control, b.history, b.jacobian)):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64))
    assert (a.history[:, 5] == 1).sum() > 5
    plan = reg.FFDPlan(*args, **kw)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        plan.run()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = plan.run()
    for t in (g.control, g.history, g.jacobian):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(keep, (g.control, g.history, g.jacobian)):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64))


# ---- 4. transform_points -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", (10.0, (7.0, 12.5, 9.0), (100.0, 34.0, 71.0)))
def test_transform_points_and_jacobian_are_the_rule_bit_for_bit(h):
    from ctunet_amd import mesh, registration as reg
    c = scene(1)
    lat = R.lattice(FIXED_SHAPE, FIXED_SPACING, FIXED_ORIGIN, h)
    if h == (100.0, 34.0, 71.0):
        assert lat[0] == (4, 5, 4)                                      # G at its minimum
    ctl = np.random.default_rng(11).uniform(-3.0, 3.0, (3, *lat[0]))
    pts = _points(6000)
    r = _result(c["affine"], ctl, lat)
    want, wdet = R.transform(pts, c["affine"], lat, ctl, True)
    got, det = reg.transform_points(_dev(pts), r, return_jacobian=True)
    assert got.dtype == torch.float32 and det.dtype == torch.float64
    assert _bits(got.cpu().numpy(), want) and _bits(det.cpu().numpy(), wdet)
    assert torch.equal(reg.transform_points(_dev(pts), r).view(torch.int32), got.view(torch.int32))
    assert np.isfinite(wdet).all() and np.isnan(want[7]).all() and (wdet != 1.0).sum() > 5000
    # the dyadic matrix puts points on the knots and the far face of the lattice
    want, wdet = R.transform(pts, DYADIC, lat, ctl, True)
    got, det = reg.transform_points(_dev(pts), r._replace(matrix=_dev(DYADIC)), return_jacobian=True)
    assert _bits(got.cpu().numpy(), want) and _bits(det.cpu().numpy(), wdet)
    # a mesh goes through the same kernel; a matrix as before
    m = mesh.Mesh(_dev(pts[:300]), torch.zeros((1, 3), dtype=torch.int32, device=DEV))
    assert _bits(mesh.transform(m, r).vertices.cpu().numpy(), R.transform(pts[:300], c["affine"], lat, ctl))
    plain = mesh.transform(m, r.matrix).vertices
    want = (m.vertices.to(torch.float64) @ r.matrix[:3, :3].T + r.matrix[:3, 3]).to(torch.float32)
    assert _bits(plain.cpu().numpy(), want.cpu().numpy())


# ---- 5. deformable_resample ----------------------------------------------------------------------------------------------
OUT_SHAPE, OUT_SPACING, OUT_ORIGIN = (21, 27, 37), (2.9, 2.4, 1.9), (-2.0, 1.5, -1.0)
OUT = dict(out_spacing=OUT_SPACING, out_origin=OUT_ORIGIN)
MODES = (("nearest", np.uint8, None), ("linear", np.float32, None), ("linear", np.uint8, None), ("label_linear", np.uint8, 2))


def _volume(dtype):
    fixed, field = fixed_side()
    return fixed.astype(np.uint8) if dtype == np.uint8 else field


def test_deformable_resample_with_zero_controls_is_affine_resample():
    from ctunet_amd import resample
    c = scene(1)
    lat = R.lattice(FIXED_SHAPE, FIXED_SPACING, FIXED_ORIGIN, CONTROL_SPACING)
    r = _result(c["affine"], np.zeros((3, *lat[0])), lat)
    for mode, dtype, K in MODES:
        x = _dev(_volume(dtype))
        kw = dict(mode=mode, num_classes=K, fill=1 if dtype == np.uint8 else 7.5, **FRAME, **OUT)
        got = resample.deformable_resample(x, r, OUT_SHAPE, **kw)
        want = resample.affine_resample(x, r.matrix, OUT_SHAPE, **kw)
        assert got.dtype == want.dtype and torch.equal(got, want), (mode, dtype)
        assert len(torch.unique(got)) > 1


@pytest.mark.parametrize("mode,dtype,K", MODES)
def test_deformable_resample_is_the_rule_bit_for_bit(mode, dtype, K):
    from ctunet_amd import resample
    c = scene(1)
    lat = R.lattice(FIXED_SHAPE, FIXED_SPACING, FIXED_ORIGIN, CONTROL_SPACING)
    ctl = np.random.default_rng(13).uniform(-4.0, 4.0, (3, *lat[0]))
    vol = _volume(dtype)
    x = _dev(vol)
    fill = 7.5 if mode == "linear" else 1
    kw = dict(mode=mode, num_classes=K, fill=fill)
    r = _result(c["affine"], ctl, lat)
    want = R.deformable_resample(vol, c["affine"], lat, ctl, OUT_SHAPE, FIXED_SPACING, FIXED_ORIGIN, OUT_SPACING, OUT_ORIGIN, **kw)
    got = resample.deformable_resample(x, r, OUT_SHAPE, **kw, **FRAME, **OUT)
    assert _bits(got.cpu().numpy(), want), (mode, dtype, int((got.cpu().numpy() != want).sum()))
    base = want
    plain = R.deformable_resample(vol, c["affine"], lat, np.zeros_like(ctl), OUT_SHAPE, FIXED_SPACING, FIXED_ORIGIN, OUT_SPACING,
                                  OUT_ORIGIN, **kw)
    assert (want != plain).mean() > 0.02                                # the controls matter
    # an out= off the 16-byte grid, with guard bytes around it
    n = int(np.prod(OUT_SHAPE))
    odt = torch.float32 if mode == "linear" else torch.uint8
    lead = 3 if odt == torch.float32 else 5
    buf = torch.full((n + 64,), 113, dtype=odt, device=DEV)
    out = buf[lead:lead + n].view(OUT_SHAPE)
    assert out.data_ptr() % 16 != 0
    assert resample.deformable_resample(x, r, OUT_SHAPE, out=out, **kw, **FRAME, **OUT) is out
    assert _bits(out.cpu().numpy(), want) and (buf[:lead] == 113).all() and (buf[lead + n:] == 113).all()
    # a NaN in the matrix: the fill everywhere; a NaN control: the fill wherever the rule says so
    bad = np.array(c["affine"])
    bad[1, 2] = np.nan
    got = resample.deformable_resample(x, r._replace(matrix=_dev(bad)), OUT_SHAPE, **kw, **FRAME, **OUT)
    assert (got == fill).all()
    holed = ctl.copy()
    holed[1, 4, 5, 5] = np.nan
    want = R.deformable_resample(vol, c["affine"], lat, holed, OUT_SHAPE, FIXED_SPACING, FIXED_ORIGIN, OUT_SPACING, OUT_ORIGIN, **kw)
    got = resample.deformable_resample(x, r._replace(control=_dev(holed)), OUT_SHAPE, **kw, **FRAME, **OUT).cpu().numpy()
    assert _bits(got, want) and (want != base).any()                   # the control at (30, 40, 40) mm lies inside the head


# ---- 6. the pipeline -----------------------------------------------------------------------------------------------------
def test_register_deformable_then_pull_the_atlas_onto_the_patient():
    """Scene 2 (the skull with the hole, bound 6 mm): the atlas pulled onto the moving grid through the similarity matrix
    alone, and through the free-form result; Dice against the hole-free moving skull.  Measured on the MI355X: 0.8105 and
    0.9466 (rms 0.647 -> 0.219 mm, min det 0.852, no folded point)."""
    from ctunet_amd import registration as reg, resample
    c = scene(2)
    fixed = _dev(fixed_side()[0].astype(np.uint8))
    d = reg.register_deformable(_dev(c["moving"]), fixed, moving_spacing=MOVING_SPACING, moving_origin=MOVING_ORIGIN,
                                fixed_spacing=FIXED_SPACING, fixed_origin=FIXED_ORIGIN, max_distance=c["bound"])
    kw = dict(out_spacing=MOVING_SPACING, out_origin=MOVING_ORIGIN, mode="label_linear", num_classes=2, **FRAME)
    before = resample.affine_resample(fixed, d.matrix, MOVING_SHAPE, **kw).cpu().numpy() != 0
    after = resample.deformable_resample(fixed, d, MOVING_SHAPE, **kw).cpu().numpy() != 0
    d0, d1 = dice(before, c["full"]), dice(after, c["full"])
    rep = d.report()
    print(f"Dice against the hole-free skull: similarity {d0:.4f}, free-form {d1:.4f}; {rep}")
    assert d1 >= d0 + 0.05
    assert rep["status"] == 0 and rep["rms"] < rep["rms_before"] and rep["min_jacobian"] > 0 and rep["folded"] == 0
