"""Random spatial augmentation on the MI355X (csrc/spatial.hip): bit equality with the NumPy restatement
(tests/spatial_ref.py) driven by the recorded matrix and control grid, the recorded matrix against NumPy's, cross-checks
against torch.flip and resample.affine_resample, graph replay, state-dict resume, the fused flap transform and the datasets
with a spatial step, and guards against non-finite coordinates."""
import numpy as np
import pytest
import torch

import augment_ref as R
import spatial_ref as S

pytestmark = pytest.mark.gpu

ON = dict(flip_p=1.0, affine_p=1.0, elastic_p=1.0)
OFF = dict(flip_p=0.0, affine_p=0.0, elastic_p=0.0)
# ranges sized for volumes a few voxels across, so that most voxels still sample inside
SMALL = dict(translation=(1.0, 1.0, 2.0), max_displacement=(1.0, 1.5, 2.0), degrees=(20.0, 10.0, 15.0), scales=(0.85, 1.2))


def _volume(n, c, dims, dtype, seed):
    g = np.random.default_rng(seed)
    if dtype == "uint8":
        return g.integers(1, 256, (n, c) + dims).astype(np.uint8)          # no zeros: 0 is the fill
    return (g.standard_normal((n, c) + dims) + 3.0).astype(np.float32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _spatial(seed, **kw):
    from ctunet_amd.transforms import RandomSpatial
    return RandomSpatial(seed=seed, **kw)


def _check_call(t, x, got, seq0):
    """One call of t on the host copy x [N,C,D,H,W] -> got: the records equal the restated draws of samples seq0 .. and
    the output equals the restatement driven by the recorded M and control grid.  Returns the records."""
    cfg = S.Config.of(t)
    n = x.shape[0]
    recs, ctl = t.last_params, t.last_control.numpy()
    assert ctl.shape == (n, 3) + cfg.num_control_points and ctl.dtype == np.float64
    assert np.array_equal(ctl.view(np.uint64), S.control_batch(cfg, t.seed, seq0, n).view(np.uint64))
    for i, rec in enumerate(recs):
        want = S.scalars(cfg, t.seed, seq0 + i)
        for k in ("flip", "affine", "elastic", "scales", "degrees", "translation"):
            assert rec[k] == want[k], (i, k, rec[k], want[k])
        M = rec["matrix"].numpy()
        if not rec["affine"]:
            assert np.array_equal(M, S.IDENTITY) and not np.signbit(M).any()
        exp = S.expected(x[i], cfg, dict(rec, matrix=M), ctl[i])
        assert exp.dtype == got.dtype and np.array_equal(_bits(got[i]), _bits(exp)), i
    return recs


STEPS = [dict(flip_p=1.0), dict(affine_p=1.0), dict(elastic_p=1.0), dict(flip_p=1.0, affine_p=1.0),
         dict(flip_p=1.0, elastic_p=1.0), dict(affine_p=1.0, elastic_p=1.0), dict(ON)]


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("steps", STEPS, ids=lambda s: "+".join(k[:-2] for k in s))
def test_each_step_alone_in_pairs_and_together(steps, dtype):
    dims = (5, 6, 19)                                          # uint8 rows end inside a 16-byte chunk
    x = _volume(2, 1, dims, dtype, 1)
    t = _spatial(100 + len(steps), flip_axes=(0, 1, 2), **dict(OFF, **steps), **SMALL, spacing=(1.0, 0.5, 0.75))
    got = t.apply(_t(x)).cpu().numpy()
    recs = _check_call(t, x, got, 0)
    for rec in recs:
        assert rec["flip"] == (("flip_p" in steps),) * 3 and rec["affine"] == ("affine_p" in steps)
        assert rec["elastic"] == ("elastic_p" in steps)
    assert (got != 0).mean() > 0.3


# below one tile in every axis; >= 2 tiles and a remainder along every axis (a tile: 4 planes x 4 rows x 64 float32 / 256 uint8)
SHAPES = [("uint8", (3, 5, 7), 1, 1, {}), ("float32", (3, 5, 7), 1, 1, {}),
          ("float32", (9, 10, 70), 1, 1, dict(degrees=(4.0, 4.0, 20.0))), ("uint8", (6, 9, 300), 1, 1, dict(degrees=(1.0, 1.0, 20.0))),
          ("uint8", (7, 9, 21), 3, 2, dict(num_control_points=(5, 7, 4), locked_borders=1, spacing=(1.25, 0.6, 0.8))),
          ("float32", (7, 9, 21), 3, 2, dict(num_control_points=(5, 7, 4), locked_borders=1, spacing=(1.25, 0.6, 0.8))),
          ("uint8", (5, 6, 40), 2, 3, dict(num_control_points=12, locked_borders=0))]


@pytest.mark.parametrize("dtype,dims,n,c,kw", SHAPES, ids=lambda v: None if isinstance(v, dict) else str(v).replace(" ", ""))
def test_bit_equal_on_tile_edges_batches_and_channels(dtype, dims, n, c, kw):
    x = _volume(n, c, dims, dtype, 2)
    # random steps: over two calls of a batch the samples take different step combinations
    t = _spatial(7, flip_axes=(0, 2), flip_p=0.5, affine_p=0.6, elastic_p=0.6, **dict(SMALL, **kw))
    xd = _t(x)
    for call in range(2):
        got = t.apply(xd).cpu().numpy()
        _check_call(t, x, got, call * n)
    assert t.state_dict() == {"seed": 7, "counter": 2 * n}
    t2 = _spatial(7, flip_axes=(0, 2), **ON, **dict(SMALL, **kw))
    _check_call(t2, x, t2.apply(xd).cpu().numpy(), 0)


@pytest.mark.parametrize("dtype,offsets", [("uint8", (1, 4, 12)), ("float32", (4, 12))])
def test_out_off_the_16_byte_grid(dtype, offsets):
    dims = (5, 6, 37)
    x = _volume(2, 2, dims, dtype, 3)
    xd = _t(x)
    td = xd.dtype
    for off in offsets:
        assert off % xd.element_size() == 0
        buf = torch.full((x.size + 64,), 0xAA if dtype == "uint8" else -7.0, dtype=td, device="cuda")
        base = (-buf.data_ptr()) % 16 // xd.element_size() + 16 // xd.element_size() + off // xd.element_size()
        out = buf[base:base + x.size].view(x.shape)
        assert out.data_ptr() % 16 == off
        t = _spatial(9, flip_axes=(1,), **ON, **SMALL)
        res = t.apply(xd, out=out)
        assert res.data_ptr() == out.data_ptr()
        _check_call(t, x, out.cpu().numpy(), 0)
        guard = torch.cat([buf[:base], buf[base + x.size:]])
        assert (guard == (0xAA if dtype == "uint8" else -7.0)).all()     # nothing written around out


def test_recorded_matrix_against_numpy():
    """M == NumPy's [L | c - L c + t] from the recorded angles, scales and translation, within
    16 2^-52 (1 + max|c| + max|t|) per entry, over 256 draws on two grids."""
    worst = 0.0
    for dims, sp in (((3, 5, 7), (40.0, 30.0, 25.0)), ((4, 4, 8), (0.8, 0.45, 0.45))):
        t = _spatial(21, **dict(OFF, affine_p=1.0), degrees=(15.0, 45.0, 180.0), spacing=sp)
        t.apply(torch.zeros((128, 1) + dims, dtype=torch.uint8, device="cuda"))
        for rec in t.last_params:
            want = S.matrix(dims, sp, rec["scales"], rec["degrees"], rec["translation"])
            ratio = np.abs(rec["matrix"].numpy() - want).max() / S.matrix_bound(dims, sp, rec["translation"])
            worst = max(worst, ratio)
    print(f"largest |M - numpy| / bound = {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_cross_checks_against_trusted_code(dtype):
    from ctunet_amd import resample
    dims, sp = (9, 10, 70), (1.5, 0.9, 0.7)
    x = _volume(2, 2, dims, dtype, 4)
    xd = _t(x)
    ident = _spatial(1, **OFF, spacing=sp)
    assert torch.equal(ident.apply(xd), xd)
    flip = _spatial(2, flip_axes=(0, 2), **dict(OFF, flip_p=1.0), spacing=sp)
    assert torch.equal(flip.apply(xd), torch.flip(xd, (2, 4)))
    aff = _spatial(3, **dict(OFF, affine_p=1.0), **SMALL, spacing=sp)
    got = aff.apply(xd)
    assert (got != 0).float().mean() > 0.3
    for i, rec in enumerate(aff.last_params):
        want = resample.affine_resample(xd[i], rec["matrix"].cuda(), dims, spacing=sp, out_spacing=sp, mode="nearest")
        assert torch.equal(got[i], want), i


def test_graph_replay():
    dims = (6, 9, 40)
    x = _volume(2, 1, dims, "uint8", 5)
    xd = _t(x)
    t = _spatial(31, flip_axes=(0, 1), flip_p=0.5, affine_p=0.7, elastic_p=0.7, **SMALL)
    out = torch.empty_like(xd)
    t.apply(xd, out=out)                                       # the warm call: allocates the record and the grid
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                  # a host synchronisation would fail the capture
        t.apply(xd, out=out)
    assert t.state_dict()["counter"] == 2                      # capturing runs nothing
    for k in (1, 2):
        g.replay()
        _check_call(t, x, out.cpu().numpy(), 2 * k)
    assert t.state_dict()["counter"] == 6


def test_preset_feeds_preallocated_buffers_in_a_graph():
    from ctunet_amd.transforms import FlapRecTransform, SaltAndPepper, SkullRandomHole

    def make():
        return FlapRecTransform(SkullRandomHole(p=0.9, double_output=True, seed=1), SaltAndPepper(p=1, noise_density=.05, seed=2),
                                spatial=_spatial(3, **SMALL))
    dims = (16, 16, 16)
    sk = _t((np.random.default_rng(6).random((2, 1) + dims) < 0.3).astype(np.uint8))
    t, twin = make(), make()
    x = torch.empty((2, 1) + dims, device="cuda")
    tg = [torch.empty((2, 2) + dims, device="cuda") for _ in range(2)]
    t.apply(sk, x=x, targets=tg)
    twin.apply(sk)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t.apply(sk, x=x, targets=tg)
    for _ in range(2):
        g.replay()
        xe, te = twin.apply(sk)
        assert torch.equal(x, xe) and all(torch.equal(u, v) for u, v in zip(tg, te))
    assert t.state_dict() == twin.state_dict() and t.state_dict()["spatial"]["counter"] == 6


def test_state_dict_resume():
    dims = (5, 6, 19)
    xd = _t(_volume(3, 1, dims, "float32", 7))
    a = _spatial(51, **SMALL)
    a.apply(xd)
    a.apply(xd)
    b = _spatial(1, **SMALL)
    b.load_state_dict(a.state_dict())
    assert b.seed == 51 and b.state_dict() == {"seed": 51, "counter": 6}
    assert torch.equal(a.apply(xd), b.apply(xd))
    c = _spatial(51, **SMALL).to("cuda")
    c.load_state_dict({"seed": 51, "counter": 9})             # loaded into a counter that is already on the device
    assert torch.equal(a.apply(xd), c.apply(xd))


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_flap_transform_with_a_spatial_step(dtype):
    from ctunet_amd.transforms import FlapRecTransform, SaltAndPepper, SkullRandomHole
    dims = (12, 14, 18)
    g = np.random.default_rng(8)
    sk = (g.random((3, 1) + dims) < 0.35).astype(np.float32)
    if dtype == "float32":
        sk = sk * (1.0 + 0.7 * (g.random(sk.shape) < 0.3)) + 0.6 * (g.random(sk.shape) < 0.1)   # the uint8 cast decides
    sk = sk.astype(dtype)
    skd = _t(sk)
    atlas = torch.rand(dims, device="cuda")
    fused = FlapRecTransform(SkullRandomHole(double_output=True, seed=61), SaltAndPepper(p=1, noise_density=.3, seed=62), atlas,
                             spatial=_spatial(63, **SMALL))
    sp = _spatial(63, **SMALL)
    plain = FlapRecTransform(SkullRandomHole(double_output=True, seed=61), SaltAndPepper(p=1, noise_density=.3, seed=62), atlas)
    for _ in range(2):
        xf, tf = fused.apply(skd)
        warped = sp.apply(skd)
        xp, tp = plain.apply(warped)
        assert torch.equal(xf, xp) and all(torch.equal(u, v) for u, v in zip(tf, tp))
        assert torch.equal(xf[:, 1], atlas.expand(3, *dims))                                # the atlas is not warped
        assert torch.equal(tf[0][:, 1], (warped[:, 0].to(torch.uint8) != 0).float())        # full skull = the warped skull
    assert fused.state_dict() == dict(plain.state_dict(), spatial=sp.state_dict())
    assert fused.last_params == plain.last_params
    # spatial=None: what the transform gave before it had the step (the restatement of tests/augment_ref.py)
    none = FlapRecTransform(SkullRandomHole(double_output=True, seed=61), SaltAndPepper(p=1, noise_density=.3, seed=62),
                            spatial=None)
    xn, (full, flap) = none.apply(skd)
    for i, rec in enumerate(none.last_params):
        img, full_e, flap_e = R.expected(sk[i, 0], rec, noise_seed=62)
        assert np.array_equal(xn[i, 0].cpu().numpy(), img)
        assert np.array_equal(full[i].cpu().numpy(), R.one_hot(full_e)) and np.array_equal(flap[i].cpu().numpy(), R.one_hot(flap_e))


def test_sample_dicts_share_one_draw():
    dims = (5, 6, 19)
    img = torch.from_numpy(_volume(1, 1, dims, "uint8", 9)[0, 0])
    t, twin = _spatial(71, **ON, **SMALL), _spatial(71, **ON, **SMALL)
    s = t({"image": img, "target": (img.flip(0), img.float()), "filepath": "a"})
    want = twin.apply(torch.stack([img, img.flip(0), img]).cuda().unsqueeze(0).float())[0]
    assert s["filepath"] == "a" and s["image"].dtype == torch.uint8 and s["target"][1].dtype == torch.float32
    assert torch.equal(s["image"].float(), want[0]) and torch.equal(s["target"][0].float(), want[1])
    assert torch.equal(s["target"][1], want[2])
    s2 = t({"image": img})
    assert set(s2) == {"image"} and t.state_dict()["counter"] == 2


def test_dataset_item_through_the_preset():
    from ctunet_amd.datasets import FlapRec2OTrainDataset, FlapRecWShapePrior2OTrainDataset
    from ctunet_amd.transforms import FlapRecTransform, SaltAndPepper, SkullRandomHole
    dims = (16, 16, 16)
    skulls = torch.from_numpy((np.random.default_rng(10).random((2,) + dims) < 0.4).astype(np.uint8))
    atlas = torch.rand(dims)
    tr = FlapRecTransform(SkullRandomHole(p=0.9, double_output=True, seed=81), SaltAndPepper(p=1, noise_density=.05, seed=82),
                          spatial=_spatial(83, flip_axes=(0,), **ON, **SMALL))
    ds = FlapRecWShapePrior2OTrainDataset(skulls, atlas, transform=tr)
    assert ds.transform.spatial is tr.spatial
    s = ds[1]
    full, flap = s["target"]
    assert s["image"].shape == (2,) + dims and full.shape == flap.shape == (2,) + dims
    warped = _spatial(83, flip_axes=(0,), **ON, **SMALL).apply(skulls[1].cuda().view(1, 1, *dims))[0, 0]
    assert not torch.equal(warped.cpu(), skulls[1]) and warped.any()
    assert torch.equal(full.cpu(), torch.from_numpy(R.one_hot(warped.cpu().numpy() != 0)))
    rec = tr.last_params[0]
    img_before_noise, _, _ = R.expected(warped.cpu().numpy(), rec)
    assert torch.equal(torch.from_numpy(img_before_noise) + flap[1].cpu(), warped.cpu().float())   # image + flap = skull
    u1, u2 = R.noise_fields(82, rec["noise_seq"], dims)
    t0, t1 = rec["thresholds"]
    quiet = ~((u1 <= np.float32(t0)) | (u2 <= np.float32(t1))) if rec["noise_applied"] else np.ones(dims, bool)
    rebuilt = (s["image"][0] + flap[1]).cpu().numpy()
    assert quiet.mean() > 0.9 and np.array_equal(rebuilt[quiet], warped.cpu().numpy().astype(np.float32)[quiet])
    assert torch.equal(s["image"][1].cpu(), atlas)
    assert FlapRec2OTrainDataset(list(skulls), transform=tr)[0]["image"].shape == (1,) + dims


def test_non_finite_coordinates_give_the_fill():
    dims = (5, 6, 19)
    x = _volume(2, 1, dims, "uint8", 11)
    xd = _t(x)
    huge_t = _spatial(91, **dict(OFF, affine_p=1.0), translation=1e300)
    got = huge_t.apply(xd)
    assert not got.any()
    huge_e = _spatial(92, **dict(OFF, elastic_p=1.0), max_displacement=1.7e308, locked_borders=0)
    got = huge_e.apply(xd).cpu().numpy()
    _check_call(huge_e, x, got, 0)
    assert not got.any()
    # a spacing at which o * spacing overflows for o >= 2: inf and NaN coordinates read nothing; the rule still holds
    for kw in (dict(OFF), dict(ON)):
        t = _spatial(93, flip_axes=(0, 1, 2), **kw, spacing=1e308)
        got = t.apply(xd).cpu().numpy()
        _check_call(t, x, got, 0)
    assert (got == 0).mean() > 0.5
    xf = _t(_volume(1, 1, dims, "float32", 12))
    assert not _spatial(94, **dict(OFF, affine_p=1.0), translation=1e300).apply(xf).any()
