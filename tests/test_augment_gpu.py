"""Flap-reconstruction augmentation on the MI355X (csrc/augment.hip): bit-equality with the NumPy restatement
(tests/augment_ref.py) driven by the per-sample records, the centre rule, the distributions of the draws, the density
decay, batch / fused / sequential equivalence, graph replay (alone and feeding a GraphedTrainStep), state-dict resume and
the in-memory training datasets through StepRunner."""
import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu


def _skulls(n, dims, dtype, seed, density=0.3):
    g = np.random.RandomState(seed)
    s = (g.rand(n, 1, *dims) < density).astype(np.float32)
    if dtype == "float32":          # non-binary values: the uint8 cast decides (0.6 -> 0, 1.7 -> 1)
        s += np.where(g.rand(*s.shape) < 0.1, 0.6, 0.0).astype(np.float32) + s * 0.7 * (g.rand(*s.shape) < 0.2)
        return s
    return (s * (1 + (g.rand(*s.shape) < 0.1))).astype(np.uint8)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fused(hole_seed, noise_seed, atlas=None, p_noise=1.0, nd=0.3, shapes=None, decay=True):
    from ctunet_amd.transforms import FlapRecTransform, SaltAndPepper, SkullRandomHole
    return FlapRecTransform(SkullRandomHole(double_output=True, shapes=shapes, seed=hole_seed),
                            SaltAndPepper(p=p_noise, noise_density=nd, decay=decay, seed=noise_seed), atlas)


@pytest.mark.parametrize("dims,n", [((37, 45, 53), 2), ((64, 128, 128), 1)])
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
@pytest.mark.parametrize("shape", ["sphere", "box", "flap"])
def test_bit_equal_to_numpy(shape, dtype, dims, n):
    from ctunet_amd.transforms import size_range
    sk = _skulls(n, dims, dtype, 10 * R.SHAPES.index(shape) + 2 * (dtype == "uint8") + n)
    atlas = np.random.RandomState(5).rand(*dims).astype(np.float32)
    t = _fused(1234 + n, 99, _t(atlas), shapes=(shape,))
    x, (full, flap) = t.apply(_t(sk))
    recs = t.last_params
    x, full, flap = x.cpu().numpy(), full.cpu().numpy(), flap.cpu().numpy()
    lo, hi = size_range(dims)
    nds = R.noise_scalars(99, 0, n, np.float32(0.3))
    for i, rec in enumerate(recs):
        bone = R.value_of(sk[i, 0]) >= 1
        hs = R.hole_scalars(1234 + n, i, int(bone.sum()), lo, hi, (shape,))
        assert rec["count"] == bone.sum() and rec["k"] == hs["k"] and rec["size"] == hs["size"]
        assert rec["shape"] == shape and rec["c_diam"] == hs["c_diam"] and rec["apply"] and rec["cut"]
        assert rec["centre"] == tuple(np.argwhere(bone)[hs["k"]])
        assert rec["noise_applied"] == nds[i][0] and rec["nd"] == nds[i][1] and rec["noise_seq"] == i
        img, full_e, flap_e = R.expected(sk[i, 0], rec, noise_seed=99)
        assert np.array_equal(x[i, 0], img), i
        assert np.array_equal(x[i, 1], atlas)
        assert np.array_equal(full[i], R.one_hot(full_e)) and np.array_equal(flap[i], R.one_hot(flap_e))
        assert 0 < flap_e.sum() < full_e.sum() or shape == "flap"
    assert t.noise.noise_density == nds[-1][1]


def test_centre_empty_and_probability_edges():
    from ctunet_amd.transforms import SkullRandomHole
    dims = (9, 10, 11)
    sk = _skulls(6, dims, "float32", 3, density=0.05)
    sk[2] = 0
    h = SkullRandomHole(p=1, double_output=True, seed=7)
    x, (full, flap) = h.apply(_t(sk))
    recs = h.last_params
    for i, rec in enumerate(recs):
        bone = R.value_of(sk[i, 0]) >= 1
        if i == 2:
            assert rec["count"] == 0 and not rec["cut"] and rec["centre"] == (-1, -1, -1)
            assert torch.equal(x[i, 0].cpu(), torch.zeros(dims)) and flap[i, 1].sum() == 0
        else:
            assert rec["cut"] and rec["centre"] == tuple(np.argwhere(bone)[rec["k"]])
    h0 = SkullRandomHole(p=0, double_output=True, seed=8)
    x, (full, flap) = h0.apply(_t(sk))
    assert not any(r["apply"] or r["cut"] for r in h0.last_params)
    assert np.array_equal(x[:, 0].cpu().numpy(), R.value_of(sk[:, 0])) and flap[:, 1].sum() == 0
    assert torch.equal(full[:, 1].cpu(), torch.from_numpy((R.value_of(sk[:, 0]) >= 1).astype(np.float32)))


def test_distributions():
    from ctunet_amd.transforms import SaltAndPepper, SkullRandomHole, size_range
    dims = (20, 24, 30)
    n = 3000
    sk = np.zeros((1, 1) + dims, np.uint8)
    pos = np.random.RandomState(1).choice(np.prod(dims), 25, replace=False)
    sk.reshape(-1)[pos] = 1
    h = SkullRandomHole(p=1, seed=2024)
    h.apply(_t(np.repeat(sk, n, 0)))
    recs = h.last_params
    bone = np.argwhere(sk[0, 0])
    idx = {tuple(b): j for j, b in enumerate(bone)}
    hist = np.bincount([idx[r["centre"]] for r in recs], minlength=len(bone))
    e = n / len(bone)
    assert ((hist - e) ** 2 / e).sum() < 60                     # chi-square, 24 dof: p < 1e-4
    lo, hi = size_range(dims)
    sizes = np.array([r["size"] for r in recs])
    assert set(sizes.tolist()) == set(range(lo, hi))
    for s in R.SHAPES:
        c = sum(r["shape"] == s for r in recs)
        assert abs(c - n / 3) < 5 * np.sqrt(n * 2 / 9), (s, c)
    # noise fractions, one nd' per sample: ones -> zero with P = t0 (1 - t1); zeros -> one with P = t1
    sp = SaltAndPepper(p=1, noise_density=0.5, salt_ratio=0.3, decay=False, seed=77)
    m = 400
    for fill in (1, 0):
        out = sp.apply(torch.full((m, 1) + dims, float(fill), device="cuda")).cpu().numpy()
        rs = sp.last_params
        t0 = np.array([r["thresholds"][0] for r in rs], np.float64)
        t1 = np.array([r["thresholds"][1] for r in rs], np.float64)
        p = t0 * (1 - t1) if fill else t1
        got = (out.reshape(m, -1) != fill).sum(1)
        v = np.prod(dims)
        assert abs(got.sum() - (v * p).sum()) < 5 * np.sqrt((v * p * (1 - p)).sum()), fill
        assert np.allclose(t0, np.array([r["nd"] for r in rs]) * 0.7, rtol=1e-6)


def test_density_decay():
    from ctunet_amd.transforms import SaltAndPepper
    img = torch.ones(4, 1, 8, 8, 8, device="cuda")
    s = SaltAndPepper(noise_density=0.4, seed=5)
    s.apply(img)
    s.apply(img[:3])
    chain = R.noise_scalars(5, 0, 7, np.float32(0.4))
    got = [r["nd"] for r in s.last_params]
    assert got == [c[1] for c in chain[4:]]
    assert s.noise_density == chain[-1][1] < 0.4
    f = SaltAndPepper(noise_density=0.4, decay=False, seed=5)
    f.apply(img)
    f.apply(img[:3])
    assert f.noise_density == float(np.float32(0.4))
    assert [r["nd"] for r in f.last_params] == [c[1] for c in R.noise_scalars(5, 4, 3, np.float32(0.4), decay=False)]


def test_batch_equals_single_calls_and_fused_equals_sequence():
    from ctunet_amd.transforms import SaltAndPepper, SkullRandomHole
    dims = (16, 20, 26)
    sk = _t(_skulls(4, dims, "float32", 11))
    atlas = torch.rand(dims, device="cuda")
    a, b = _fused(31, 32, atlas, p_noise=0.5), _fused(31, 32, atlas, p_noise=0.5)
    xa, ta = a.apply(sk)
    for i in range(4):
        xb, tb = b.apply(sk[i:i + 1])
        assert torch.equal(xa[i:i + 1], xb) and all(torch.equal(u[i:i + 1], v) for u, v in zip(ta, tb))
    assert a.state_dict() == b.state_dict()
    h, s = SkullRandomHole(double_output=True, seed=31), SaltAndPepper(p=0.5, noise_density=0.3, seed=32)
    c = _fused(31, 32, p_noise=0.5)
    for _ in range(2):
        xc, tc = c.apply(sk)
        xh, th = h.apply(sk)
        xs = s.apply(xh)
        assert torch.equal(xc, xs) and all(torch.equal(u, v) for u, v in zip(tc, th))
    assert s.noise_density == c.noise.noise_density


def test_graph_replay_and_graphed_train_step():
    from ctunet_amd import optim
    from ctunet_amd.graph import GraphedTrainStep
    from ctunet_amd.models import UNetSP
    dims = (32, 32, 32)
    sk = _t(_skulls(2, dims, "uint8", 21, density=0.2))
    atlas = torch.rand(dims, device="cuda")
    t, twin = _fused(41, 42, atlas), _fused(41, 42, atlas)
    t.to("cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x, tg = t.apply(sk)
    assert t.state_dict()["hole"]["counter"] == 0              # capturing runs nothing
    for _ in range(3):
        g.replay()
        xe, te = twin.apply(sk)
        assert torch.equal(x, xe) and all(torch.equal(u, v) for u, v in zip(tg, te))
    assert t.state_dict() == twin.state_dict() and t.state_dict()["hole"]["counter"] == 6
    # the transform writes straight into a captured train step's input / target buffers
    torch.manual_seed(0)
    net = UNetSP().cuda()
    opt = optim.Adam(net.parameters(), lr=1e-4, amsgrad=True)
    x0, t0 = twin.apply(sk)
    gs = GraphedTrainStep(net, opt, x0, t0, 1.0, 1.0, warmup=2)
    seen = []
    for _ in range(2):
        twin.apply(sk, x=gs.x, targets=gs.targets)
        seen.append(gs.x.clone())
        vals = gs().tolist()
        assert all(np.isfinite(vals)), vals
    assert not torch.equal(seen[0], seen[1])


def test_state_dict_resume():
    dims = (12, 14, 18)
    sk = _t(_skulls(3, dims, "float32", 4))
    a = _fused(51, 52)
    a.apply(sk)
    a.apply(sk)
    b = _fused(1, 2)
    b.load_state_dict(a.state_dict())
    assert b.hole.seed == 51 and b.noise.noise_density == a.noise.noise_density
    xa, ta = a.apply(sk)
    xb, tb = b.apply(sk)
    assert torch.equal(xa, xb) and all(torch.equal(u, v) for u, v in zip(ta, tb))


def test_dataset_drives_step_runner():
    from torch.utils.data import DataLoader
    from ctunet_amd.datasets import FlapRec2OTrainDataset, FlapRecWShapePrior2OTrainDataset
    from ctunet_amd.trainer import StepRunner
    dims = (32, 32, 32)
    skulls = torch.from_numpy(_skulls(4, dims, "float32", 8, density=0.2)[:, 0])     # [M,D,H,W] on the host
    atlas = torch.rand(dims)
    tr = _fused(61, 62)
    ds = FlapRecWShapePrior2OTrainDataset(skulls, atlas, transform=tr)
    s = ds[1]
    assert set(s) == {"image", "target", "filepath"} and s["image"].shape == (2,) + dims and s["image"].is_cuda
    full, flap = s["target"]
    assert full.shape == flap.shape == (2,) + dims and full.dtype == flap.dtype == torch.float32
    rec = tr.last_params[0]
    img_before_noise, _, _ = R.expected(skulls[1].numpy(), rec)
    assert torch.equal(full[1].cpu(), torch.from_numpy(img_before_noise) + flap[1].cpu())   # datasets.py:228
    assert torch.equal(s["image"][1].cpu(), atlas)
    d2 = FlapRec2OTrainDataset(list(skulls), transform=tr)
    assert d2[0]["image"].shape == (1,) + dims
    runner = StepRunner({"problem_handler": "FlapRecWithShapePriorDoubleOut", "model_class": "UNetSP",
                         "learning_rate": 1e-4, "ce_lambda": 1.0, "dice_lambda": 1.0})
    before = [p.detach().clone() for p in runner.models["main"].parameters()]
    runner.forward_pass("train", DataLoader(ds, batch_size=2))
    assert any(not torch.equal(a, b) for a, b in zip(before, runner.models["main"].parameters()))
    avg = runner.epoch_averages()
    assert avg and all(np.isfinite(v) for v in avg.values())
