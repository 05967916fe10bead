"""Sliding-window inference on the MI355X: the accumulation / finalize kernels against a float64 restatement, the whole
predict_volume path against the existing tiler and against the CPU oracle, batching, graph replay, 16-bit, side effects,
memory and one full-size volume.

Blend rule restated here (the docstring of ctunet_amd/inference.py pins it):
    w(i,j,k) = max(g_z(i) g_y(j) g_x(k), 1e-3),  g_a(i) = exp(-(i-(P_a-1)/2)^2 / (2 (s P_a)^2))   ("constant": w = 1)
    out(v)   = sum_p w_p y_p / sum_p w_p over the patches covering v, in z-major tile order."""
import numpy as np
import pytest
import torch

from oracle import unet_oracle as O
from util import gen, rel_err

pytestmark = pytest.mark.gpu


def _tables64(patch, blend, s=0.125):
    out = []
    for p in patch:
        i = np.arange(p, dtype=np.float64)
        out.append(np.ones(p) if blend == "constant" else np.exp(-(i - (p - 1) / 2) ** 2 / (2 * (s * p) ** 2)))
    return out


def _weight64(patch, blend, s=0.125):
    gz, gy, gx = _tables64(patch, blend, s)
    return np.maximum(gz[:, None, None] * gy[None, :, None] * gx[None, None, :], 1e-3)


def _tiles(shape, patch, overlap):
    from ctunet_amd.tiling import tile_starts
    zs, ys, xs = (tile_starts(s, p, o) for s, p, o in zip(shape, patch, overlap))
    return [(z, y, x) for z in zs for y in ys for x in xs]


def _blend64(ys, tiles, shape, patch, blend):
    """ys: float64 [T,K,pd,ph,pw] patch outputs in tile order -> (num [K,D,H,W], wsum [D,H,W]) in float64."""
    k = ys.shape[1]
    w = _weight64(patch, blend)
    num = np.zeros((k,) + tuple(shape))
    ws = np.zeros(tuple(shape))
    for y, (z0, y0, x0) in zip(ys, tiles):
        dz, dy, dx = (min(p, s - a) for p, s, a in zip(patch, shape, (z0, y0, x0)))
        ww = w[:dz, :dy, :dx]
        num[:, z0:z0 + dz, y0:y0 + dy, x0:x0 + dx] += ww * y[:, :dz, :dy, :dx]
        ws[z0:z0 + dz, y0:y0 + dy, x0:x0 + dx] += ww
    return num, ws


def _extract64(vol, tiles, patch):
    c = vol.shape[0]
    out = np.zeros((len(tiles), c) + tuple(patch))
    for t, (z0, y0, x0) in enumerate(tiles):
        src = vol[:, z0:z0 + patch[0], y0:y0 + patch[1], x0:x0 + patch[2]]
        out[t, :, :src.shape[1], :src.shape[2], :src.shape[3]] = src
    return out


def _argmax_first(p):
    return np.argmax(p, axis=0).astype(np.uint8)          # numpy: the first maximum wins


def _labels_agree(lab, ref_probs, margin):
    """labels equal wherever the top two classes of the reference differ by more than margin (one class: everywhere)."""
    if ref_probs.shape[0] == 1:
        clear = np.ones(ref_probs.shape[1:], bool)
    else:
        srt = np.sort(ref_probs, axis=0)
        clear = (srt[-1] - srt[-2]) > margin
    return bool((lab[clear] == _argmax_first(ref_probs)[clear]).all()), float(clear.mean())


def _perturb_bn(net, seed):
    """Non-trivial running statistics, so the eval forward's BatchNorm does something."""
    g = gen(seed)
    for name, b in net.named_buffers():
        if name.endswith("running_mean"):
            b.copy_(0.1 * torch.randn(b.shape, generator=g))
        elif name.endswith("running_var"):
            b.copy_(0.5 + torch.rand(b.shape, generator=g))
    return net


# ------------------------------------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("shape,patch,overlap,batch,k", [((20, 45, 70), (32, 16, 32), (8, 4, 12), 5, 3),
                                                         ((40, 37, 64), (16, 32, 16), (4, 0, 6), 5, 2),
                                                         ((18, 20, 22), (32, 32, 32), (8, 8, 8), 2, 1)])
@pytest.mark.parametrize("blend", ["gaussian", "constant"])
def test_accumulate_and_finalize_kernels_against_float64(shape, patch, overlap, batch, k, blend):
    from ctunet_amd import ops
    from ctunet_amd.inference import WEIGHT_FLOOR, plan_batches, tile_grid, window_tables
    tiles = tile_grid(shape, patch, overlap)
    bp = plan_batches(tiles, batch, shape, patch)
    assert not bp.valid.all()                      # every case ends on a partial batch
    ys = torch.rand((tiles.shape[0], k) + patch, generator=gen(5), dtype=torch.float64)
    dev = "cuda"
    tabs = tuple(torch.from_numpy(t).to(dev) for t in window_tables(patch, blend, 0.125))
    num = torch.zeros((k,) + shape, device=dev)
    ws = torch.zeros(shape, device=dev)
    for b in range(bp.coords.shape[0]):
        sel = [i for i in range(b * batch, (b + 1) * batch)]
        yb = torch.stack([ys[min(i, tiles.shape[0] - 1)] for i in sel]).float().to(dev)   # padding slots: real data
        meta = torch.from_numpy(bp.meta()[b]).to(dev)
        ops.window_accumulate(yb, meta[:3 * batch].view(batch, 3), meta[3 * batch:4 * batch], meta[4 * batch:], tabs,
                              WEIGHT_FLOOR, bp.extent, num, ws)
    rnum, rws = _blend64(ys.numpy(), [tuple(t) for t in tiles], shape, patch, blend)
    assert rel_err(num, torch.from_numpy(rnum)) <= 1e-6
    assert rel_err(ws, torch.from_numpy(rws)) <= 1e-6
    assert (rws > 0).all()
    probs = torch.empty_like(num)
    lab = torch.empty(shape, dtype=torch.uint8, device=dev)
    ops.window_finalize(num, ws, probs, lab)
    rp = rnum / rws
    assert rel_err(probs, torch.from_numpy(rp)) <= 1e-6
    # labels: exactly the first-argmax rule on the kernel's own probabilities, and the reference's where it is clear
    assert torch.equal(lab.cpu(), torch.argmax(probs, 0).to(torch.uint8).cpu())
    assert _labels_agree(lab.cpu().numpy(), rp, 1e-5)[0]
    # in place (probs = num) gives the same bits; an uncovered voxel gives 0 / label 0
    ws2 = ws.clone()
    ws2[0, 0, 0] = 0
    n2 = num.clone()
    ops.window_finalize(n2, ws2, n2, None)
    assert torch.equal(n2.view(k, -1)[:, 1:], probs.view(k, -1)[:, 1:])
    assert (n2[:, 0, 0, 0] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. the existing path
def test_constant_blend_equals_extract_model_stitch():
    import ctunet_amd as A
    from ctunet_amd.tiling import VolumeTiler
    torch.manual_seed(11)
    net = _perturb_bn(A.UNet(), 12).cuda().eval()
    vol = torch.randn((1, 56, 72, 88), generator=gen(13)).cuda()
    pred = A.predict_volume(net, vol, patch=32, overlap=8, batch=2, blend="constant")
    t = VolumeTiler(32, 8)
    patches, coords = t.extract(vol)
    with torch.no_grad():
        ref = t.stitch(net(patches), coords, vol.shape[1:])
    assert pred.probs.shape == (2, 56, 72, 88) and pred.probs.dtype == torch.float32
    assert rel_err(pred.probs, ref) <= 1e-6
    assert pred.labels.dtype == torch.uint8 and torch.equal(pred.labels, torch.argmax(pred.probs, 0).to(torch.uint8))


# ------------------------------------------------------------------------------------------------ 3. the oracle
@pytest.mark.parametrize("name", ["UNet", "UNetSP", "recAE_v2_fixed"])
def test_end_to_end_against_the_cpu_oracle(name):
    import ctunet_amd as A
    torch.manual_seed(21)
    net = _perturb_bn(getattr(A, name)(), 22)
    sd = {k: v.clone().double() if v.is_floating_point() else v.clone() for k, v in net.state_dict().items()}
    spec = O.SPECS[name]
    shape, patch, overlap = (40, 52, 70), (32, 32, 32), (8, 8, 8)
    vol = torch.randn((spec.in_ch,) + shape, generator=gen(23))
    net = net.cuda()
    pred = A.predict_volume(net, vol, patch=32, overlap=8, batch=3)        # a CPU volume: copied once
    tiles = _tiles(shape, patch, overlap)
    xs = torch.from_numpy(_extract64(vol.double().numpy(), tiles, patch))
    with torch.no_grad():
        out = O.forward(spec, sd, xs, training=False)
    outs = out if isinstance(out, tuple) else (out,)
    probs = pred.probs if isinstance(pred.probs, tuple) else (pred.probs,)
    labs = pred.labels if isinstance(pred.labels, tuple) else (pred.labels,)
    assert len(outs) == len(probs) == len(labs) == (2 if name == "UNetSP" else 1)
    for o, p, lab in zip(outs, probs, labs):
        num, ws = _blend64(o.numpy(), tiles, shape, patch, "gaussian")
        rp = num / ws
        assert p.shape == rp.shape
        e = rel_err(p, torch.from_numpy(rp))
        assert e <= 1e-5, (name, e)
        ok, frac = _labels_agree(lab.cpu().numpy(), rp, 1e-5)
        assert ok and frac > 0.9, (name, frac)


# ------------------------------------------------------------------------------------------------ 4. batching / graph
def test_batch_size_and_graph_replay():
    import ctunet_amd as A
    torch.manual_seed(31)
    net = _perturb_bn(A.UNet(), 32).cuda()
    shape = (40, 52, 70)                      # 2 x 2 x 3 = 12 tiles: batch 5 ends on a partial batch of 2
    vol = torch.randn((1,) + shape, generator=gen(33)).cuda()
    p1 = A.predict_volume(net, vol, patch=32, overlap=8, batch=1)
    p3 = A.predict_volume(net, vol, patch=32, overlap=8, batch=3)
    assert rel_err(p1.probs, p3.probs) <= 1e-6
    e5 = A.predict_volume(net, vol, patch=32, overlap=8, batch=5)
    g5 = A.predict_volume(net, vol, patch=32, overlap=8, batch=5, graph=True)
    assert torch.equal(g5.probs, e5.probs) and torch.equal(g5.labels, e5.labels)
    cap = net.__dict__["_window_graph"]
    # a second volume of the same shape replays the same capture (every batch from the graph) and is still bit-equal
    vol2 = torch.randn((1, 1) + shape, generator=gen(34)).cuda()
    g5b = A.predict_volume(net, vol2, patch=32, overlap=8, batch=5, graph=True)
    assert net.__dict__["_window_graph"][3] is cap[3]
    e5b = A.predict_volume(net, vol2, patch=32, overlap=8, batch=5)
    assert torch.equal(g5b.probs, e5b.probs) and torch.equal(g5b.labels, e5b.labels)
    assert not torch.equal(g5b.probs, g5.probs)
    # the first result is not overwritten by the second call
    assert torch.equal(g5.probs, e5.probs)
    # two-output head, graphed, labels off
    torch.manual_seed(35)
    sp = A.UNetSP().cuda()
    v3 = torch.randn((2,) + shape, generator=gen(36)).cuda()
    a = A.predict_volume(sp, v3, patch=32, overlap=8, batch=5, labels=False)
    b = A.predict_volume(sp, v3, patch=32, overlap=8, batch=5, labels=False, graph=True)
    assert a.labels is None and b.labels is None
    assert all(torch.equal(x, y) for x, y in zip(a.probs, b.probs))


# ------------------------------------------------------------------------------------------------ 5. 16-bit
# First measurement on an MI355X (UNetSP, 40x52x70, patch 32, overlap 8): max relative probability error against the fp32
# prediction of the same weights, and the share of clear voxels (top-two margin > 1e-2) whose label differs.
#   bf16: 6.97e-4, 0        fp16: 8.50e-5, 0
# Gates: about 4-6x the measured error; at most 0.1 % of the clear voxels may change label.
GATES_16 = {"bf16": (3e-3, 1e-3), "fp16": (5e-4, 1e-3)}


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_16bit_against_fp32(prec):
    import ctunet_amd as A
    torch.manual_seed(41)
    net = _perturb_bn(A.UNetSP(), 42).cuda()
    vol = torch.randn((2, 40, 52, 70), generator=gen(43)).cuda()
    ref = A.predict_volume(net, vol, patch=32, overlap=8, batch=2)
    net.set_precision(prec)
    got = A.predict_volume(net, vol, patch=32, overlap=8, batch=2)
    gotg = A.predict_volume(net, vol, patch=32, overlap=8, batch=2, graph=True)
    net.set_precision("fp32")
    err = max(rel_err(g, r) for g, r in zip(got.probs, ref.probs))
    bad = 0.0
    for g, r, lab in zip(got.probs, ref.probs, got.labels):
        rs = torch.sort(r, 0).values
        clear = (rs[-1] - rs[-2]) > 1e-2
        bad = max(bad, (lab != torch.argmax(r, 0).to(torch.uint8))[clear].float().mean().item())
    print(f"16-bit {prec}: max rel prob err {err:.3e}, label mismatch on clear voxels {bad:.3e}")
    tol_err, tol_bad = GATES_16[prec]
    assert err <= tol_err and bad <= tol_bad, (prec, err, bad)
    assert all(torch.equal(a, b) for a, b in zip(got.probs, gotg.probs))


# ------------------------------------------------------------------------------------------------ 6. side effects
@pytest.mark.parametrize("graph", [False, True])
def test_no_side_effects_on_the_model(graph):
    import ctunet_amd as A
    torch.manual_seed(51)
    net = _perturb_bn(A.UNet(), 52).cuda().train()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    vol = torch.randn((1, 40, 40, 40), generator=gen(53)).cuda()
    A.predict_volume(net, vol, patch=32, overlap=8, batch=2, graph=graph)
    assert net.training
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k
    net.eval()
    A.predict_volume(net, vol, patch=32, overlap=8, batch=2, graph=graph)
    assert not net.training


# ------------------------------------------------------------------------------------------------ 7. memory
def test_capture_runs_with_the_collector_paused(monkeypatch):
    """predict_volume(graph=True) captures with cyclic garbage collection off -- a dead model cycle holding an earlier
    capture must not be torn down inside this one -- and turns it back on afterwards."""
    import gc
    import ctunet_amd as A
    seen = []

    class Spy(torch.cuda.graph):
        def __enter__(self):
            seen.append(gc.isenabled())
            return super().__enter__()

    monkeypatch.setattr(torch.cuda, "graph", Spy)
    net = A.UNet().cuda()
    vol = torch.randn((1, 40, 40, 40), generator=gen(61)).cuda()
    A.predict_volume(net, vol, patch=32, overlap=8, batch=2, graph=True)
    assert seen == [False] and gc.isenabled()


def test_peak_memory_is_one_batch_plus_the_volume_buffers():
    import ctunet_amd as A
    torch.manual_seed(61)
    net = A.UNet().cuda()
    shape, batch = (80, 80, 80), 2                 # 3 x 3 x 3 = 27 tiles
    vol = torch.randn((1,) + shape, generator=gen(62)).cuda()
    A.predict_volume(net, vol, patch=32, overlap=8, batch=batch)        # warm: the engine's packed weights exist
    x = torch.randn(batch, 1, 32, 32, 32, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        y = net.eval()(x)
    torch.cuda.synchronize()
    fwd_peak = torch.cuda.max_memory_allocated() - base + x.numel() * 4
    del y
    v = int(np.prod(shape))
    buffers = 2 * v * 4 + v * 4 + v                # num (K = 2), wsum, labels
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    pred = A.predict_volume(net, vol, patch=32, overlap=8, batch=batch)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"memory: predict peak {peak / 1e6:.2f} MB, one-batch forward {fwd_peak / 1e6:.2f} MB, buffers {buffers / 1e6:.2f} MB")
    assert peak <= 1.1 * (fwd_peak + buffers), (peak, fwd_peak, buffers)
    all_patches = 27 * 32 ** 3 * 4 * 3             # inputs + 2-channel outputs of every patch at once
    assert peak < fwd_peak + buffers + all_patches
    assert pred.probs.shape == (2,) + shape


# ------------------------------------------------------------------------------------------------ 8. full size
def test_large_volume_unetsp_bf16():
    import ctunet_amd as A
    from ctunet_amd.tiling import VolumeTiler
    torch.manual_seed(71)
    net = _perturb_bn(A.UNetSP(), 72).cuda().set_precision("bf16")
    shape = (224, 304, 304)                        # 2 x 2 x 2 tiles of 192^3
    vol = torch.randn((2,) + shape, generator=gen(73)).cuda()
    g = A.predict_volume(net, vol, patch=192, overlap=48, batch=2)
    for p in g.probs:
        assert p.shape == (2,) + shape and torch.isfinite(p).all()
    # second head = (1 - flap, flap): sums to 1 wherever the weight sum is positive, 0 where it would be 0
    assert ((g.probs[1].sum(0) - 1).abs() < 1e-2).all()
    c = A.predict_volume(net, vol, patch=192, overlap=48, batch=2, blend="constant")
    t = VolumeTiler(192, 48)
    patches, coords = t.extract(vol)
    outs = [[], []]
    with torch.no_grad():
        for i in range(0, patches.shape[0], 2):          # the same forward batches as predict_volume
            o = net.eval()(patches[i:i + 2].contiguous())
            outs[0].append(o[0])
            outs[1].append(o[1])
    del patches
    for j in range(2):
        ref = t.stitch(torch.cat(outs[j]), coords, shape)
        assert rel_err(c.probs[j], ref) <= 1e-6
    net.set_precision("fp32")
