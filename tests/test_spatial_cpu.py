"""Random spatial augmentation without a GPU: the restated rule (tests/spatial_ref.py) against scipy, the B-spline's
partition of unity and linear precision, the draws through two code paths, and argument validation (which must raise before
anything is launched)."""
import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import spatial_ref as S

CFG = S.Config(flip_axes=(0, 2), flip_p=1.0, affine_p=1.0, elastic_p=1.0, translation=(2.0, 1.5, 2.0),
               max_displacement=(1.5, 1.0, 1.0), locked_borders=1, spacing=(0.8, 0.45, 0.45))
SHAPE = (21, 26, 35)


def test_restatement_against_scipy():
    """All three steps on, anisotropic spacing: scipy's order-0 sampling of the same coordinates agrees on every voxel
    whose coordinates are not within 1e-9 of a rounding tie (at most 0.1 % may be left out), and most voxels sample inside."""
    rng = np.random.default_rng(3)
    x = rng.integers(1, 256, SHAPE).astype(np.uint8)          # no zeros: a voxel is 0 iff it is filled
    sc = S.scalars(CFG, seed=77, seq=5)
    assert sc["flip"] == (True, False, True) and sc["affine"] and sc["elastic"]
    M = S.matrix(SHAPE, CFG.spacing, sc["scales"], sc["degrees"], sc["translation"])
    phi = S.control(CFG, 77, 5)
    u = S.coords(SHAPE, CFG.spacing, M, phi, sc["flip"])
    got = S.sample(x, u)
    want = ndi.map_coordinates(x, u, order=0, mode="grid-constant", cval=0)
    tie = (np.abs(u - np.floor(u) - 0.5) < 1e-9).any(0)
    print(f"ties {tie.sum()} of {tie.size}, inside {np.mean(got != 0):.3f}")
    assert tie.mean() <= 1e-3
    assert np.array_equal(got[~tie], want[~tie])
    assert (got != 0).mean() >= 0.5
    # a second channel shares the warp
    x2 = np.stack([x, x[::-1]])
    g2 = S.expected(x2, CFG, dict(sc, matrix=M), phi)
    assert np.array_equal(g2[0], got) and np.array_equal(g2[1], S.sample(x[::-1], u))


def test_each_step_alone_against_its_closed_form():
    x = np.random.default_rng(4).integers(1, 256, (5, 6, 7)).astype(np.uint8)
    sp = (1.0, 2.0, 0.5)
    assert np.array_equal(S.sample(x, S.coords(x.shape, sp, S.IDENTITY)), x)
    assert np.array_equal(S.sample(x, S.coords(x.shape, sp, S.IDENTITY, flip=(True, False, True))), x[::-1, :, ::-1])
    shift = S.IDENTITY.copy()
    shift[1, 3] = 2.0                                          # one voxel along y: out[y] = x[y + 1]
    got = S.sample(x, S.coords(x.shape, sp, shift))
    assert np.array_equal(got[:, :-1], x[:, 1:]) and not got[:, -1].any()
    bad = S.IDENTITY.copy()
    bad[0, 3], bad[2, 2] = np.inf, np.nan
    assert not S.sample(x, S.coords(x.shape, sp, bad)).any()


def test_bspline_weights():
    f = np.concatenate([np.linspace(0, 1, 4001), np.random.default_rng(0).random(4000)])
    B = S.bspline(f)
    assert all((b >= 0).all() for b in B)
    assert np.abs(((B[0] + B[1]) + B[2]) + B[3] - 1.0).max() <= 4 * 2.0 ** -52
    assert [float(b) for b in S.bspline(0.0)] == [1 / 6, 4 / 6, 1 / 6, 0.0]


@pytest.mark.parametrize("G", [(7, 7, 7), (5, 7, 4), (12, 4, 9)])
def test_bspline_field_reproduces_linear_and_constant_control_values(G):
    shape, sp = (9, 14, 11), (1.5, 0.7, 1.0)
    rng = np.random.default_rng(5)
    ext = np.asarray(shape) * np.asarray(sp)
    s = rng.random((3, 500)) * ext[:, None] * 1.2 - 0.1 * ext[:, None]      # some points beyond both ends: g clamps
    a, b = 0.37, -2.25
    iz, iy, ix = np.indices(G).astype(np.float64)
    phi = np.stack([a * iz + b, a * iy + b, a * ix + b])
    e = S.displacement(s, shape, sp, phi)
    for c in range(3):
        i, f, g = S.knot(s[c], shape[c], sp[c], G[c])
        assert i.min() >= 0 and i.max() <= G[c] - 4 and (f >= 0).all() and (f <= 1).all()
        want = a * (g + 1) + b
        assert np.abs(e[c] - want).max() <= 1e-13 * np.abs(want).max()
    const = S.displacement(s, shape, sp, np.full((3,) + G, 3.25))
    assert np.abs(const - 3.25).max() <= 4 * 2.0 ** -52 * 3.25
    assert not S.displacement(s, shape, sp, np.zeros((3,) + G)).any()


def test_no_free_displacement_is_exactly_zero():
    """max_displacement = 0 draws a grid of exact zeros, and e = 0 exactly, so q = s bit for bit."""
    cfg = S.Config(max_displacement=(0.0, 0.0, 0.0), locked_borders=0)
    phi = S.control(cfg, 9, 0)
    assert phi.shape == (3, 7, 7, 7) and not phi.any()        # (2u - 1) 0 is +0 or -0; the sum starts from +0 either way
    M = S.matrix(SHAPE, cfg.spacing, (1.05, 0.95, 1.0), (5.0, -7.0, 11.0), (1.0, -2.0, 0.5))
    assert np.array_equal(S.coords(SHAPE, cfg.spacing, M, phi), S.coords(SHAPE, cfg.spacing, M))


@pytest.mark.parametrize("cfg", [S.Config(), S.Config(flip_axes=(0, 1, 2), num_control_points=(5, 7, 4), locked_borders=1,
                                                      max_displacement=(1.0, 2.0, 3.0), scales=(0.5, 2.0),
                                                      degrees=(0.0, 30.0, 5.0), flip_p=0.3, affine_p=0.7, elastic_p=0.2)])
def test_draws_agree_between_the_single_and_the_batch_path(cfg):
    seed, seq0, n = 0xFEDCBA9876543210, 2 ** 32 - 3, 7            # the sequence number crosses 2^32 inside the batch
    sb, cb = S.scalars_batch(cfg, seed, seq0, n), S.control_batch(cfg, seed, seq0, n)
    for i in range(n):
        s1 = S.scalars(cfg, seed, seq0 + i)
        assert s1["flip"] == tuple(sb["flip"][i]) and s1["affine"] == sb["affine"][i] and s1["elastic"] == sb["elastic"][i]
        for k in ("scales", "degrees", "translation"):
            assert np.array_equal(np.asarray(s1[k]).view(np.uint64), sb[k][i].view(np.uint64)), k
        assert np.array_equal(S.control(cfg, seed, seq0 + i).view(np.uint64), cb[i].view(np.uint64))
        # sample i of a batch == a single call at counter + i
        assert np.array_equal(S.control_batch(cfg, seed, seq0 + i, 1)[0], cb[i])
    lb, g = cfg.locked_borders, cfg.num_control_points
    free = np.zeros(g, bool)
    free[lb:g[0] - lb, lb:g[1] - lb, lb:g[2] - lb] = True
    assert not cb[:, :, ~free].any() and (cb[:, :, free] != 0).all()
    for c in range(3):
        assert np.abs(cb[:, c]).max() <= cfg.max_displacement[c]
    assert (sb["scales"] >= cfg.scales[0]).all() and (sb["scales"] < cfg.scales[1]).all()
    assert (np.abs(sb["degrees"]) <= np.asarray(cfg.degrees)).all()
    assert not sb["flip"][:, [a for a in range(3) if a not in cfg.flip_axes]].any()


def test_draw_frequencies():
    cfg = S.Config(flip_axes=(0, 1, 2), flip_p=0.25, affine_p=0.5, elastic_p=0.75)
    n = 4000
    sb = S.scalars_batch(cfg, 123, 0, n)
    for got, p in ((sb["flip"][:, 0], .25), (sb["flip"][:, 2], .25), (sb["affine"], .5), (sb["elastic"], .75)):
        assert abs(got.mean() - p) < 5 * np.sqrt(p * (1 - p) / n)
    assert abs(sb["translation"].mean(0) / np.asarray(cfg.translation)).max() < 5 / np.sqrt(3 * n)


def test_matrix_centre_is_fixed_without_translation():
    shape, sp = (21, 26, 35), (0.8, 0.45, 0.45)
    M = S.matrix(shape, sp, (1.1, 0.9, 1.0), (10.0, -15.0, 7.0), (0.0, 0.0, 0.0))
    c = (np.asarray(shape) - 1) / 2 * np.asarray(sp)
    assert np.abs(M[:, :3] @ c + M[:, 3] - c).max() < 1e-12
    R = M[:, :3] / np.array([1.1, 0.9, 1.0])
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and np.linalg.det(R) > 0
    assert np.array_equal(S.matrix(shape, sp, (1, 1, 1), (0, 0, 0), (0, 0, 0)), S.IDENTITY)


def test_constructor_validation():
    from ctunet_amd.transforms import FlapRecTransform, RandomSpatial, SkullRandomHole
    t = RandomSpatial(seed=3)
    assert t.flip_axes == (0,) and t.scales == (0.9, 1.1) and t.degrees == (15.0,) * 3 and t.translation == (10.0, 10.0, 15.0)
    assert t.num_control_points == (7, 7, 7) and t.max_displacement == (7.5,) * 3 and t.locked_borders == 2
    assert t.spacing == (1.0, 1.0, 1.0) and t.seed == 3 and (t.flip_p, t.affine_p, t.elastic_p) == (0.5, 0.5, 0.5)
    assert RandomSpatial(flip_axes=1, num_control_points=(5, 7, 4), locked_borders=1).flip_axes == (1,)
    for kw in (dict(flip_axes=(3,)), dict(flip_axes=(0, 0)), dict(flip_axes=(True,)), dict(flip_p=1.5), dict(affine_p=-0.1),
               dict(elastic_p="1"), dict(scales=(0.0, 1.0)), dict(scales=(1.2, 0.8)), dict(scales=(1.0, float("inf"))),
               dict(degrees=-1), dict(degrees=float("nan")), dict(translation=(1, -2, 3)), dict(max_displacement=float("inf")),
               dict(num_control_points=3), dict(num_control_points=13), dict(num_control_points=(7, 7, 2)),
               dict(locked_borders=3), dict(locked_borders=-1), dict(locked_borders=True),
               dict(num_control_points=4, locked_borders=2), dict(num_control_points=(7, 7, 4), locked_borders=2),
               dict(num_control_points=(5, 2 * 1, 6), locked_borders=1), dict(spacing=0), dict(spacing=(1, 1, -1)),
               dict(spacing=float("inf")), dict(seed=-1), dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            RandomSpatial(**kw)
    for kw in (dict(scales=1.0), dict(scales=("a", "b")), dict(degrees="15"), dict(translation=(1, 2)),
               dict(num_control_points=7.0), dict(num_control_points=(7, 7)), dict(num_control_points=(7, 7, 7.5)),
               dict(spacing=(1, 1)), dict(spacing="1")):
        with pytest.raises(TypeError):
            RandomSpatial(**kw)
    with pytest.raises(TypeError):
        FlapRecTransform(SkullRandomHole(), spatial=SkullRandomHole())
    assert FlapRecTransform(SkullRandomHole()).spatial is None


def test_apply_validation_needs_no_device():
    from ctunet_amd.transforms import RandomSpatial
    t = RandomSpatial(seed=1)
    x = torch.zeros(1, 2, 4, 5, 6, dtype=torch.uint8)
    with pytest.raises(TypeError):
        t.apply(np.zeros((1, 1, 4, 4, 4), np.uint8))
    with pytest.raises(ValueError):
        t.apply(x)                                              # a host tensor: no CPU fallback
    with pytest.raises(ValueError):
        t.apply(x[0])                                           # wrong rank
    with pytest.raises(ValueError):
        t.apply(torch.zeros(0, 1, 4, 4, 4, dtype=torch.uint8))
    for dt in (torch.int16, torch.float64, torch.bool, torch.float16):
        with pytest.raises(TypeError):
            t.apply(x.to(dt))
    with pytest.raises(TypeError):
        t.apply(x, out=[1])
    for out in (torch.zeros(1, 2, 4, 5, 7, dtype=torch.uint8), torch.zeros(1, 2, 4, 5, 6), torch.zeros(2, 2, 4, 5, 6, dtype=torch.uint8),
                torch.zeros(1, 2, 4, 6, 5, dtype=torch.uint8).transpose(3, 4)):
        with pytest.raises(ValueError, match="out must be"):
            t.apply(x, out=out)
    with pytest.raises(TypeError):
        t({"image": np.zeros((4, 4, 4))})
    with pytest.raises(RuntimeError):
        t.last_params
    with pytest.raises(RuntimeError):
        t.last_control
    assert t.state_dict() == {"seed": 1, "counter": 0}          # nothing was drawn


def test_state_dicts_and_the_preset():
    import ctunet_amd
    from ctunet_amd.transforms import FlapRecTransform, RandomSpatial, SaltAndPepper, SkullRandomHole
    t = RandomSpatial(seed=11)
    t.load_state_dict({"seed": 12, "counter": 40})
    assert t.state_dict() == {"seed": 12, "counter": 40}
    assert RandomSpatial().seed != RandomSpatial().seed
    f = FlapRecTransform(SkullRandomHole(seed=1), SaltAndPepper(seed=2), spatial=RandomSpatial(seed=3))
    sd = f.state_dict()
    assert sd["spatial"] == {"seed": 3, "counter": 0} and sd["hole"] == {"seed": 1, "counter": 0}
    f.load_state_dict({"hole": {"seed": 5, "counter": 6}, "noise": sd["noise"]})          # a dict from before the step
    assert f.spatial.state_dict() == {"seed": 3, "counter": 0} and f.hole.state_dict() == {"seed": 5, "counter": 6}
    f.load_state_dict(dict(sd, spatial={"seed": 8, "counter": 9}))
    assert f.spatial.state_dict() == {"seed": 8, "counter": 9}
    assert "spatial" not in FlapRecTransform(SkullRandomHole(seed=1)).state_dict()
    for name in ("RandomSpatial", "cranioplasty_transform"):
        assert hasattr(ctunet_amd, name) and name in ctunet_amd.__all__, name
    p = ctunet_amd.cranioplasty_transform
    assert isinstance(p, FlapRecTransform) and p.hole.p == 0.9 and p.hole.double_output
    assert p.noise.p == 1.0 and p.noise.noise_density == float(np.float32(0.05))
    assert S.Config.of(p.spatial) == S.Config()                 # the reference function's numbers
    assert ctunet_amd.flap_rec_transform.spatial is None


def test_datasets_pass_the_spatial_step_through():
    from ctunet_amd import datasets
    from ctunet_amd.transforms import FlapRecTransform, RandomSpatial, SkullRandomHole
    sp = RandomSpatial(seed=4)
    base = FlapRecTransform(SkullRandomHole(double_output=True, seed=1), spatial=sp)
    ds = datasets.FlapRec2OTrainDataset([torch.zeros(4, 4, 4)], transform=base, device="cpu")
    assert ds.transform.spatial is sp and ds.transform.hole is base.hole
    ds = datasets.FlapRecWShapePrior2OTrainDataset([torch.zeros(4, 4, 4)], torch.zeros(4, 4, 4), transform=base, device="cpu")
    assert ds.transform.spatial is sp and ds.transform.atlas is not None
    assert datasets.FlapRec2OTrainDataset([torch.zeros(4, 4, 4)], device="cpu").transform.spatial is None
