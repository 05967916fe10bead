"""SkullRandomDefect and RandomDilate on the MI355X (csrc/defect.hip): the records and the roughness lattice bit-equal to the
NumPy restatement's draws (tests/defect_ref.py), the fused pass equal to the restated voxel rule tested on every voxel,
border clamping, the maximum ball count, samples that are not cut, fused / sequential / batch / resume equivalence, graph
replay of the whole chain (warp, dilate, defect, noise), the in-memory dataset, RandomDilate against scipy and the
``realistic_cranioplasty_transform`` preset.  All comparisons are exact."""
import numpy as np
import pytest
import torch

import augment_ref as A
import defect_ref as R
import spatial_ref as S
from test_augment_gpu import _skulls

pytestmark = pytest.mark.gpu

CASES = [((37, 45, 53), 2, (1.0, 1.0, 1.0)),          # W % 4 != 0: the scalar path
         ((40, 48, 56), 3, (1.6, 0.9, 0.9)),          # the 16-byte path
         ((64, 128, 128), 1, (0.8, 0.45, 0.45))]      # a larger grid


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _shells(n, dims, dtype, seed):
    """n ellipsoidal shells [n,1,D,H,W]; float32 carries non-binary values (0.6 -> no bone, 1.7 -> bone), uint8 ones and twos."""
    g = np.random.RandomState(seed)
    s = np.repeat(R.shell(dims)[None, None], n, 0).astype(np.float32)
    if dtype == "float32":
        return s + np.where(g.rand(*s.shape) < 0.1, 0.6, 0.0).astype(np.float32) + s * 0.7 * (g.rand(*s.shape) < 0.2)
    return (s * (1 + (g.rand(*s.shape) < 0.1))).astype(np.uint8)


def _defect(seed, spacing=(1, 1, 1), **kw):
    from ctunet_amd.transforms import SkullRandomDefect
    return SkullRandomDefect(double_output=True, spacing=spacing, seed=seed, **kw)


def _noise(seed, p=1.0, nd=0.3):
    from ctunet_amd.transforms import SaltAndPepper
    return SaltAndPepper(p=p, noise_density=nd, seed=seed)


def _geo(d, dims):
    return R.geometry(dims, d.spacing, d.radius, d.roughness, d.roughness_scale)


def _check_defect(d, sk, seq0, x, full, flap, noise=None, atlas=None, need_cut=False):
    """After one call of defect d (alone or fused) on the host skulls sk [N,1,D,H,W] -> x, full, flap (host arrays): the
    records and the lattice equal the restated draws of samples seq0 .., the outputs the restated rule on every voxel."""
    n, dims = sk.shape[0], sk.shape[2:]
    geo = _geo(d, dims)
    recs, lat = d.last_params, d.last_lattice.numpy()
    raw = d._record.cpu().numpy()
    assert lat.shape == (n,) + geo["G"] and lat.dtype == np.float64 and raw.dtype == np.float64
    for i, rec in enumerate(recs):
        bone = A.value_of(sk[i, 0]) >= 1
        want = R.draw(d.seed, seq0 + i, bone, geo, d.spacing, d.p, d.balls, d.spread, d.shrink)
        assert np.array_equal(raw[i], want["record"]), (i, raw[i], want["record"])
        assert np.array_equal(lat[i], want["lattice"]), i
        for k in ("apply", "cut", "count", "k", "centre", "n_balls", "balls", "box"):
            assert rec[k] == want[k], (i, k, rec[k], want[k])
        img, full_e, flap_e = R.expected(sk[i, 0], rec, lat[i], geo, d.spacing, None if noise is None else noise.seed,
                                         0.1 if noise is None else noise.salt_ratio)
        assert np.array_equal(x[i, 0], img), i
        if atlas is not None:
            assert np.array_equal(x[i, 1], atlas), i
        assert np.array_equal(full[i], A.one_hot(full_e)) and np.array_equal(flap[i], A.one_hot(flap_e)), i
        if need_cut:
            assert rec["cut"] and 0 < flap_e.sum() < full_e.sum(), (i, flap_e.sum(), full_e.sum())
    return recs


@pytest.mark.parametrize("dims,n,spacing", CASES)
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("noisy", [False, True])
def test_records_and_fused_pass(noisy, dtype, dims, n, spacing):
    from ctunet_amd.transforms import FlapRecTransform
    sk = _shells(n, dims, dtype, 7 * n + (dtype == "uint8"))
    atlas = np.random.RandomState(5).rand(*dims).astype(np.float32)
    noise = _noise(99) if noisy else None
    t = FlapRecTransform(_defect(2024 + n, spacing), noise, _t(atlas))
    x, (full, flap) = t.apply(_t(sk))
    recs = _check_defect(t.hole, sk, 0, x.cpu().numpy(), full.cpu().numpy(), flap.cpu().numpy(), noise, atlas, need_cut=True)
    if noisy:
        nds = A.noise_scalars(99, 0, n, np.float32(0.3))
        assert [(r["noise_applied"], r["nd"], r["noise_seq"]) for r in recs] == [(a, nd, i) for i, (a, nd) in enumerate(nds)]
        assert t.noise.noise_density == nds[-1][1]
    assert t.state_dict()["hole"]["counter"] == n


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_random_skulls(dtype):
    dims, n = (37, 45, 53), 2
    sk = _skulls(n, dims, dtype, 13)
    d = _defect(31, (1.1, 0.7, 0.9))
    x, (full, flap) = d.apply(_t(sk))
    _check_defect(d, sk, 0, x.cpu().numpy(), full.cpu().numpy(), flap.cpu().numpy())


@pytest.mark.parametrize("dims,spacing", [((37, 45, 53), (1.0, 1.0, 1.0)), ((40, 48, 56), (1.6, 0.9, 0.9))])
def test_border_clamping(dims, spacing):
    sk = np.zeros((2, 1) + dims, np.uint8)
    sk[0, 0, 0, 0, 0] = sk[1, 0, -1, -1, -1] = 1
    d = _defect(5, spacing)
    x, (full, flap) = d.apply(_t(sk))
    recs = _check_defect(d, sk, 0, x.cpu().numpy(), full.cpu().numpy(), flap.cpu().numpy())
    assert recs[0]["centre"] == (0, 0, 0) and recs[0]["box"][0] == (0, 0, 0)
    assert recs[1]["centre"] == tuple(v - 1 for v in dims) and recs[1]["box"][1] == tuple(v - 1 for v in dims)
    assert flap[:, 1].sum().item() == 2 and x.sum().item() == 0          # the one bone voxel is the centre of ball 0


def test_maximum_ball_count():
    dims, spacing = (40, 48, 56), (1.6, 0.9, 0.9)
    sk = _shells(2, dims, "uint8", 3)
    d = _defect(77, spacing, balls=(12, 12), spread=1.2)
    x, (full, flap) = d.apply(_t(sk))
    recs = _check_defect(d, sk, 0, x.cpu().numpy(), full.cpu().numpy(), flap.cpu().numpy(), need_cut=True)
    assert all(r["n_balls"] == 12 and len(r["balls"]) == 12 for r in recs)


def test_no_cut():
    dims = (37, 45, 53)
    sk = _shells(3, dims, "float32", 9)
    sk[1] = 0
    sk[1, 0, 3, 4, 5] = 0.6                                                  # a value, but no bone
    d = _defect(8)
    x, (full, flap) = d.apply(_t(sk))
    recs = _check_defect(d, sk, 0, x.cpu().numpy(), full.cpu().numpy(), flap.cpu().numpy())
    assert [r["cut"] for r in recs] == [True, False, True] and recs[1]["apply"] and recs[1]["count"] == 0
    assert torch.equal(x[1, 0].cpu(), torch.zeros(dims)) and flap[1, 1].sum() == 0 and flap[1, 0].min() == 1
    d0 = _defect(8, p=0)
    x, (full, flap) = d0.apply(_t(sk))
    _check_defect(d0, sk, 0, x.cpu().numpy(), full.cpu().numpy(), flap.cpu().numpy())
    assert not any(r["apply"] or r["cut"] for r in d0.last_params)
    assert np.array_equal(x[:, 0].cpu().numpy(), A.value_of(sk[:, 0])) and flap[:, 1].sum() == 0
    assert torch.equal(full[:, 1].cpu(), torch.from_numpy((A.value_of(sk[:, 0]) >= 1).astype(np.float32)))


def test_equivalences_and_resume():
    from ctunet_amd.transforms import FlapRecTransform
    dims, spacing = (24, 28, 36), (1.0, 0.8, 0.8)
    sk = _t(_shells(4, dims, "float32", 11))
    atlas = torch.rand(dims, device="cuda")

    def fused(with_atlas=True):
        return FlapRecTransform(_defect(31, spacing), _noise(32, p=0.5), atlas if with_atlas else None)

    a, b = fused(), fused()
    xa, ta = a.apply(sk)
    for i in range(4):                                                       # a batch of N = N single calls
        xb, tb = b.apply(sk[i:i + 1])
        assert torch.equal(xa[i:i + 1], xb) and all(torch.equal(u[i:i + 1], v) for u, v in zip(ta, tb))
    assert a.state_dict() == b.state_dict()
    h, s, c = _defect(31, spacing), _noise(32, p=0.5), fused(False)
    for _ in range(2):                                                       # fused = defect, then noise
        xc, tc = c.apply(sk)
        xh, th = h.apply(sk)
        xs = s.apply(xh)
        assert torch.equal(xc, xs) and all(torch.equal(u, v) for u, v in zip(tc, th))
    assert s.noise_density == c.noise.noise_density
    r = FlapRecTransform(_defect(1, spacing), _noise(2, p=0.5))              # resume from a state dict
    r.load_state_dict(c.state_dict())
    assert r.hole.seed == 31 and r.state_dict() == c.state_dict()
    xc, tc = c.apply(sk)
    xr, tr = r.apply(sk)
    assert torch.equal(xc, xr) and all(torch.equal(u, v) for u, v in zip(tc, tr))
    from ctunet_amd.transforms import SkullRandomDefect
    both, single = _defect(31, spacing), SkullRandomDefect(spacing=spacing, seed=31)     # double_output=False: the flap alone
    xb, tb = both.apply(sk)
    x1, t1 = single.apply(sk)
    assert len(t1) == 1 and torch.equal(t1[0], tb[1]) and torch.equal(x1, xb)


def _check_chain(t, sk, before, x, full, flap, atlas=None):
    """One call of FlapRecTransform t (spatial, dilate, defect, noise) on the host uint8 skulls sk, whose members' counters
    were ``before`` (its state_dict): every stage equals its restatement, fed with the stage before."""
    n = sk.shape[0]
    cur = sk
    if t.spatial is not None:
        cfg = S.Config.of(t.spatial)
        ctl = t.spatial.last_control.numpy()
        assert np.array_equal(ctl, S.control_batch(cfg, t.spatial.seed, before["spatial"]["counter"], n))
        cur = np.stack([S.expected(cur[i], cfg, dict(rec, matrix=rec["matrix"].numpy()), ctl[i])
                        for i, rec in enumerate(t.spatial.last_params)])
    if t.dilate is not None:
        cur = R.random_dilate(cur, t.dilate.seed, before["dilate"]["counter"], t.dilate.p, t.dilate.iterations)
    _check_defect(t.hole, cur, before["hole"]["counter"], x, full, flap, t.noise, atlas)
    return cur


def test_graph_replay_of_the_whole_chain():
    from ctunet_amd.transforms import FlapRecTransform, RandomDilate, RandomSpatial
    dims, n = (40, 48, 56), 2
    sk = _shells(n, dims, "uint8", 21)
    atlas = torch.rand(dims, device="cuda")
    small = dict(translation=(1.0, 1.0, 2.0), max_displacement=(1.0, 1.5, 2.0), degrees=5.0)
    t = FlapRecTransform(_defect(41), _noise(42), atlas, RandomSpatial(seed=43, **small), RandomDilate(p=0.5, iterations=2, seed=44))
    skd = _t(sk)
    x = torch.empty((n, 2) + dims, device="cuda")
    tg = [torch.empty((n, 2) + dims, device="cuda") for _ in range(2)]
    t.apply(skd, x=x, targets=tg)                                            # the warm call allocates the kept buffers
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t.apply(skd, x=x, targets=tg)
    assert t.state_dict()["hole"]["counter"] == n                           # capturing runs nothing
    dilated = []
    for rep in range(3):
        before = t.state_dict()
        assert before["hole"]["counter"] == before["dilate"]["counter"] == before["spatial"]["counter"] == n * (1 + rep)
        g.replay()
        cur = _check_chain(t, sk, before, x.cpu().numpy(), tg[0].cpu().numpy(), tg[1].cpu().numpy(), atlas.cpu().numpy())
        dilated += [R.dilate_applied(44, before["dilate"]["counter"] + i, 0.5) for i in range(n)]
        assert np.array_equal(tg[0][:, 1].cpu().numpy(), cur[:, 0].astype(np.float32))   # full = the warped, dilated skull
    assert any(dilated) and not all(dilated)
    assert t.state_dict()["noise"]["counter"] == 4 * n


def test_dataset_yields_the_refs_items():
    from ctunet_amd.datasets import FlapRecWShapePrior2OTrainDataset
    from ctunet_amd.transforms import FlapRecTransform
    dims = (32, 32, 32)
    skulls = torch.from_numpy(_shells(3, dims, "float32", 8)[:, 0])          # [M,D,H,W] on the host
    atlas = torch.rand(dims)
    tr = FlapRecTransform(_defect(61), _noise(62))
    ds = FlapRecWShapePrior2OTrainDataset(skulls, atlas, transform=tr)
    for seq, idx in enumerate((1, 0)):
        s = ds[idx]
        assert set(s) == {"image", "target", "filepath"} and s["image"].shape == (2,) + dims and s["image"].is_cuda
        full, flap = s["target"]
        _check_defect(tr.hole, skulls[idx].numpy()[None, None], seq, s["image"][None].cpu().numpy(),
                      full[None].cpu().numpy(), flap[None].cpu().numpy(), tr.noise, atlas.numpy(), need_cut=True)


@pytest.mark.parametrize("iterations", [1, 2, 3])
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_random_dilate(dtype, iterations):
    from scipy import ndimage
    from ctunet_amd.transforms import RandomDilate
    seed = 5
    for dims in ((9, 10, 11), (20, 33, 70)):
        sk = _skulls(4, dims, dtype, 17, density=0.03)
        sk[0, 0, 0, 0, 0] = sk[1, 0, -1, -1, -1] = 1
        t = RandomDilate(p=0.5, iterations=iterations, seed=seed)
        for call in range(2):
            applied = [R.dilate_applied(seed, 4 * call + i, 0.5) for i in range(4)]
            assert any(applied) and not all(applied)
            out = t.apply(_t(sk)).cpu().numpy()
            assert out.dtype == np.uint8 and out.shape == sk.shape
            assert np.array_equal(out, R.random_dilate(sk, seed, 4 * call, 0.5, iterations))
            for i in range(4):
                bone = A.value_of(sk[i, 0]) >= 1
                want = ndimage.binary_dilation(bone, ndimage.generate_binary_structure(3, 1), iterations=iterations,
                                               border_value=0) if applied[i] else bone
                assert np.array_equal(out[i, 0], want.astype(np.uint8)), (i, applied[i])
        assert t.state_dict() == {"seed": seed, "counter": 8}
    with pytest.raises(ValueError):
        x = torch.zeros(1, 1, 4, 4, 4, dtype=torch.uint8, device="cuda")
        RandomDilate().apply(x, out=x)


def test_realistic_preset():
    from ctunet_amd import transforms as T
    t = T.realistic_cranioplasty_transform
    assert isinstance(t.hole, T.SkullRandomDefect) and t.hole.p == 0.9 and t.hole.double_output and t.noise.p == 1.0
    assert t.dilate.p == 0.3 and t.dilate.iterations == 1 and t.spatial.flip_axes == (0,) and t.atlas is None
    assert isinstance(T.cranioplasty_transform.hole, T.SkullRandomHole) and T.cranioplasty_transform.dilate is None
    dims, n = (40, 48, 56), 4
    sk = _shells(n, dims, "uint8", 2)
    t.to("cuda")
    for _ in range(2):
        before = t.state_dict()
        x, (full, flap) = t.apply(_t(sk))
        _check_chain(t, sk, before, x.cpu().numpy(), full.cpu().numpy(), flap.cpu().numpy())
        assert t.state_dict()["hole"]["counter"] == before["hole"]["counter"] + n
    s = t({"image": torch.from_numpy(sk[0, 0])})                            # the sample-dict form
    assert s["image"].dtype == torch.float32 and s["image"].shape == dims and len(s["target"]) == 2
    assert all(v.dtype == torch.uint8 and v.shape == dims for v in s["target"])
