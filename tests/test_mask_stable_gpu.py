"""The shipped classes on mask-stable states (tests/mask_stable.py) against the fp64 oracle: the tight whole-net gate.

Every other whole-net training test of a shipped class runs at default initialisation -- gamma = 1, beta = 0, running
statistics 0 / 1, ReLU masks on zero -- where handing a layer the gamma, beta or coefficient row of a sibling of equal
width changes nothing, and where one mask flip costs percents, so those gates are 6e-2 of scale.  Here every BatchNorm
carries its own random gamma (both signs), beta, mean and variance, every third channel is off, and no mask can flip
(tests/test_mask_stable_cpu.py holds the cases to that in the oracle alone), so every output, gradient and buffer of the
engine -- which vector feeds which launch, which slice of which concat buffer, which count, which reduction is deferred
to where -- is held to max(5 x ATen's fp32 error, 1e-4 of the tensor's largest entry) + 1e-7 and a cosine of 0.99999
against fp64, at the shipped widths (fused up-convolutions, 16- to 128-channel tiles, split concat levels, 2-channel first
layers) and under every engine switch.  On these states the gradients fall by about 1e-2 per level (largest entry 1e-3 at
the head, 1e-8 and less at the deepest level), so the 1e-4 term binds at the head and the top level only; below, the
absolute 1e-7 is the wider one and the cosine (0.99999, about 4.5e-3 in relative L2; measured 1 - 1e-9) is the gate that
binds.  Measured figures: profiles/mask_stable_gates.md.

A miss here with a positive margin is a bug in the engine or in a kernel's handling of negative gamma, off channels or
non-zero beta, not a tolerance question."""
import pytest
import torch

import mask_stable as MS
from oracle import unet_oracle as O
from util import fp64_rule_misses, rel_err

pytestmark = pytest.mark.gpu


class Holder:
    verbose = False

    def __init__(self):
        self.params = dict(ce_lambda=1.0, dice_lambda=1.0, save_dice_plots=False, save_hd_plots=False)
        self.losses_and_metrics = {}
        self.pt_loss = None


def hip_net(cid, precision="fp32"):
    """A fresh module of the case's class on the GPU, in train mode, carrying the case's stable state."""
    name, kw = MS.BY_ID[cid][:2]
    net = MS.build(name, **kw)
    net.load_state_dict(MS.state(cid))
    net = net.cuda().train()
    return net if precision == "fp32" else net.set_precision(precision)


def hip_step(cid, precision="fp32"):
    """load_state_dict(stable), .cuda().train(), the handler's loss (MSE for the 3-channel plain classes, as
    test_models_gpu.oracle_train_check), backward.  Everything the step produced, on the host."""
    from ctunet_amd import ProblemHandler as PH
    net = hip_net(cid, precision)
    x, tg = MS.case_inputs(MS.BY_ID[cid])
    xi = x.cuda().requires_grad_(True)
    out = net(xi)
    kind, h = MS.loss_kind(MS.BY_ID[cid][0]), Holder()
    if kind == "double":
        PH.FlapRecWithShapePriorDoubleOut.comp_losses_metrics(h, out, [t.cuda() for t in tg], 0, 1)
        loss = h.pt_loss
    elif kind == "single":
        PH.ProblemHandler.comp_losses_metrics(h, out, tg[0].cuda(), 0, 1)
        loss = h.pt_loss
    else:
        loss = (out ** 2).mean()
    loss.backward()
    torch.cuda.synchronize()
    outs = out if isinstance(out, tuple) else (out,)
    return {"outs": [o.detach().cpu() for o in outs], "loss": loss.item(), "dx": xi.grad.cpu(),
            "grads": {n_: (None if p.grad is None else p.grad.cpu()) for n_, p in net.named_parameters()},
            "buffers": {n_: b.cpu() for n_, b in net.named_buffers()}}


def gate_a(cid, got, tag):
    """One fp32 train step against the fp64 oracle: outputs 1e-5 of max |ref|, loss 1e-5, dx and every parameter gradient
    max(5 x the ATen-CPU fp32 error of that tensor, 1e-4 of its largest fp64 entry) + 1e-7 (util.fp64_rule_misses with the
    tiny fixtures' floor), per-tensor cosine >= 0.99999, exact zeros of the fp64 gradient (off channels) <= 1e-7, BatchNorm
    buffers after the step rtol 1e-5 / atol 1e-6."""
    r64, r32 = MS.reference(cid, "fp64"), MS.reference(cid, "fp32")
    assert r64["margin"][0] > 0 and r32["margin"][0] > 0
    for o, r in zip(got["outs"], r64["outs"]):
        assert o.shape == r.shape and rel_err(o, r) < 1e-5, (tag, rel_err(o, r))
    assert abs(got["loss"] - r64["loss"]) < 1e-5, (tag, got["loss"], r64["loss"])
    g64 = r64["grads"]
    assert set(got["grads"]) == set(g64)
    for n_, r in g64.items():
        assert (got["grads"][n_] is None) == (r is None), n_           # (the dead centre block of the generic nets)
    names = [n_ for n_, r in g64.items() if r is not None]
    checks = [("dx", got["dx"], r32["dx"], r64["dx"])] + [(n_, got["grads"][n_], r32["grads"][n_], g64[n_]) for n_ in names]
    misses = fp64_rule_misses(checks, g64, False, floor=1e-4)
    live = set(MS.live(r64)) | {"dx"}
    worst_cos = (1.0, None)
    for n_, g, _, r in checks:
        a, b = g.double().flatten(), r.flatten()
        if bool((b == 0).any()):                       # an off channel's gamma, beta and weights: nothing reaches them
            z = float(a[b == 0].abs().max())
            if z > 1e-7:
                misses.append((n_, "exact zero of the fp64 gradient", z))
        if n_ not in live or float(b.norm()) == 0:
            continue
        cos = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300))
        worst_cos = min(worst_cos, (cos, n_))
        if cos < 0.99999:
            misses.append((n_, "cosine", cos))
    e, where = MS.worst_error(got["grads"], got["dx"], r64)
    e32 = MS.worst_error(r32["grads"], r32["dx"], r64)
    print(f"[{tag}] margin {r64['margin'][0]:.3f}; out {max(rel_err(o, r) for o, r in zip(got['outs'], r64['outs'])):.1e}; loss "
          f"{abs(got['loss'] - r64['loss']):.1e}; worst gradient {e:.2e} of its largest entry ({where}), ATen fp32 worst "
          f"{e32[0]:.2e} ({e32[1]}); lowest cosine 1 - {1 - worst_cos[0]:.1e} ({worst_cos[1]})")
    assert not misses, (tag, misses)
    assert set(got["buffers"]) == set(r64["buffers"])
    for k, v in r64["buffers"].items():
        b = got["buffers"][k]
        if "num_batches" in k:
            assert int(b) == int(v) == 1, (tag, k)
        else:
            assert torch.allclose(b.double(), v, rtol=1e-5, atol=1e-6), (tag, k, float((b.double() - v).abs().max()))


# ------------------------------------------------------------------------------------------------------------ (a) fp32
@pytest.mark.parametrize("cid", MS.IDS)
def test_fp32_train_step_against_the_fp64_oracle(cid):
    gate_a(cid, hip_step(cid), cid)


# ----------------------------------------------------------------------------------------------- (b) engine switches
SWITCHES = ("FUSE_UP", "LAZY_BN", "POOL_BN", "BN_TAIL", "DEFER_WGRAD_REDUCE", "SPLIT_CAT0", "SPLIT_CAT1")
MATRIX_IDS = [f"{n_}-{b}x{c}x32x32x32" for n_, c in (("UNet", 1), ("UNetSP", 2), ("recAE_v2_fixed", 1)) for b in (1, 2)]
assert all(c in MS.BY_ID for c in MATRIX_IDS)


@pytest.mark.parametrize("variant", ["flip_" + k for k in SWITCHES] + ["all_off"])
@pytest.mark.parametrize("cid", MATRIX_IDS)
def test_every_engine_switch_against_the_fp64_oracle(cid, variant, monkeypatch):
    """Each single flip from the engine's default (read from the engine, so a default that changes keeps its flip a
    flip), and everything off, on a fresh module each: held to the fp64 oracle like the default path, not to the default path
    -- the references stay independent, a shared wiring error cannot cancel.  (The engine reads the switches at every call.
    SPLIT_CAT0, SPLIT_CAT1 and DEFER_WGRAD_REDUCE give the default path's bits by design, and recAE_v2_fixed has no fused
    up-convolution or lazy BatchNorm to switch: equal figures there are expected.)"""
    from ctunet_amd import engine
    for k in SWITCHES:
        assert isinstance(getattr(engine, k), bool), k
        value = False if variant == "all_off" else (not getattr(engine, k) if variant == "flip_" + k else getattr(engine, k))
        monkeypatch.setattr(engine, k, value)
    gate_a(cid, hip_step(cid), f"{cid} {variant}")


# ------------------------------------------------------------------------------------------------------------ (c) eval
def _head_probe(name, outs):
    """What of the logits the head's outputs still determine, as float64, with the probabilities it is read from (None: the
    probe is a difference of outputs, well conditioned everywhere).  Sigmoid heads: every logit.  Shape-prior heads
    ([bg, flap + full], [1 - flap, flap]): the three logits, full as a difference.  Softmax over two channels (the legacy
    nets; UNetSPSmall's softmax of each pair): the difference of its two arguments."""
    spec = O.SPECS[name]
    o = [t.double() for t in outs]
    logit = lambda p: torch.log(p / (1 - p))
    if spec.family == "legacy" or spec.head == "sp_softmax":
        return [(torch.log(t[:, 1] / t[:, 0]), None) for t in o]
    if spec.head == "plain":
        return [(logit(o[0]), o[0])]
    p = torch.stack((o[0][:, 0], o[1][:, 1], o[0][:, 1] - o[1][:, 1]), 1)
    return [(logit(p), p)]


def _logit_reference(name, lg):
    spec = O.SPECS[name]
    lg = lg.double()
    if spec.family == "legacy":
        return [lg[:, 1] - lg[:, 0]]
    if spec.head == "sp_softmax":
        s = torch.sigmoid(lg)
        return [(s[:, 1] + s[:, 2]) - s[:, 0], 2 * s[:, 1] - 1]
    return [lg]


@pytest.mark.parametrize("cid", MS.IDS)
def test_eval_forward_with_the_stable_state(cid):
    """The folded eval-mode BatchNorm (bn_eval_affine) with random gamma of both signs, beta, mean and variance at every
    width: outputs against the fp32 oracle, rel_err < 1e-4; logits through the inverted head as in
    test_full_size_gpu.test_cfg2_unet_128_batch2_eval, 1e-4; no buffer changes."""
    name = MS.BY_ID[cid][0]
    sd = {k: v.clone() for k, v in MS.state(cid).items()}
    x, _ = MS.case_inputs(MS.BY_ID[cid])
    ref = O.forward(O.SPECS[name], sd, x, training=False)
    refs = ref if isinstance(ref, tuple) else (ref,)
    lg_ref = O.forward(O.SPECS[name], sd, x, training=False, return_logits=True)
    net = hip_net(cid).eval()
    with torch.no_grad():
        out = net(x.cuda())
    outs = [o.cpu() for o in (out if isinstance(out, tuple) else (out,))]
    errs = [rel_err(o, r) for o, r in zip(outs, refs)]
    assert len(outs) == len(refs) and all(o.is_contiguous() and o.shape == r.shape for o, r in zip(outs, refs))
    probe_errs = []
    for (got, prob), want in zip(_head_probe(name, outs), _logit_reference(name, lg_ref)):
        assert got.shape == want.shape
        # a probability is an fp32 number: half an ulp of it (6e-8 below 1) moves its logit by 6e-8 / (p (1 - p)), which
        # stays below the 1e-4 gate for p in [1e-3, 1 - 1e-3]; saturated voxels are held by the output gate alone
        ok = torch.ones_like(want, dtype=torch.bool) if prob is None else (prob > 1e-3) & (prob < 1 - 1e-3)
        assert float(ok.double().mean()) > 0.25               # (UNet: 0.57 of the voxels; every other class: all)
        probe_errs.append(float((got - want)[ok].abs().max()) / max(1.0, float(want.abs().max())))
    print(f"[{cid} eval] outputs {max(errs):.1e}, logits {max(probe_errs):.1e}")
    assert max(errs) < 1e-4 and max(probe_errs) < 1e-4, (errs, probe_errs)
    for k, v in net.state_dict().items():                       # eval mode updates nothing
        assert torch.equal(v.cpu(), MS.state(cid)[k]), k


# --------------------------------------------------------------------------------------------------------- (d) graphed
def test_graphed_step_replays_the_eager_gradients_bit_for_bit():
    """GraphedTrainStep on UNet with the stable state.  The optimizer is this package's SGD at learning rate 0, so the weights
    -- and with them the margin -- stay put; its step first copies every gradient it is handed into a buffer of its own (the
    step clears .grad), inside the captured graph.  Three replays: each leaves the eager step's gradients, bit for bit, and
    those are within gate (a)."""
    from ctunet_amd import optim
    from ctunet_amd.graph import GraphedTrainStep

    class KeepGrads(optim.SGD):
        kept = None

        def step(self, closure=None):
            if self.kept is None:                      # (first warm-up step: allocated outside the capture)
                self.kept = {}
            for p in (p for g in self.param_groups for p in g["params"] if p.grad is not None):
                if p not in self.kept:
                    assert not torch.cuda.is_current_stream_capturing()
                    self.kept[p] = torch.empty_like(p.grad)
                self.kept[p].copy_(p.grad)
            return super().step(closure)

    cid = MS.IDS[0]
    assert MS.BY_ID[cid][0] == "UNet"
    eager = hip_step(cid)
    gate_a(cid, eager, f"{cid} eager")
    net = hip_net(cid)
    opt = KeepGrads(net.parameters(), lr=0.0)
    x, tg = MS.case_inputs(MS.BY_ID[cid])
    gs = GraphedTrainStep(net, opt, x.cuda(), [t.cuda() for t in tg], 1.0, 1.0, warmup=1)
    names = {p: n_ for n_, p in net.named_parameters()}
    assert {names[p] for p in opt.kept} == {n_ for n_, g in eager["grads"].items() if g is not None}
    for it in range(3):
        for buf in opt.kept.values():
            buf.fill_(float("nan"))
        values = gs()
        torch.cuda.synchronize()
        assert abs(float(values[-1]) - eager["loss"]) < 1e-5
        for p, buf in opt.kept.items():
            a, b = buf.cpu(), eager["grads"][names[p]]
            ndiff = int((a.view(torch.int32) != b.view(torch.int32)).sum())
            assert ndiff == 0, f"replay {it}: {names[p]}: {ndiff} of {a.numel()} words differ from the eager step's"
    for k, v in net.state_dict().items():
        if "running" not in k and "num_batches" not in k:      # learning rate 0: the stable weights are still in place
            assert torch.equal(v.cpu(), MS.state(cid)[k]), k
        elif "num_batches" in k:
            assert int(v) == 1 + 3                              # one warm-up step, three replays


# ---------------------------------------------------------------------------------------------------------- (e) 16 bit
# Tensors that need more than 2 x the yardstick's relative L2 + 0.02, with the factor they are held to instead: (class,
# precision, tensor) -> factor.  Both are the weight gradient of the deepest encoder convolution that still has a value in
# fp16, and in both the yardstick's gradient is identically zero (L2 = 1).  MEASURED: 2.26 and 2.25 x (UNet4b2i3o, LP_FUSE_UP
# on / off), 11.98 and 12.17 x (UNetSPSmall); the factors below are those with a quarter on top.  They are left out of this
# path's worst-tensor L2 (UNet4b2i3o: 2.25 against 1.3 x 1.60 + 0.05), which every other tensor enters.
# Cause, from the fp64 oracle (profiles/mask_stable_gates.md has the figures): the 16-bit path stores the activation
# gradient of every layer in fp16, times the loss scale.  At d_blocks.3.block.0's output that product is at most 3.6e-8
# (UNet4b2i3o: 1.8e-11 x 2^11) and 1.1e-7 (UNetSPSmall: 6.9e-12 x 2^14) -- fp16's smallest step is 6.0e-8, so an entry is
# stored as 0 or +-1 .. 2 steps (3 of 3584 and 764 of 16384 entries are not 0), and the weight gradient summed from them
# is rounding noise of 1.6 x and 2.2 x the true gradient's norm already when only this one store is rounded (more with the
# stores of the levels above, through which the gradient arrives).  One level up the product is 5.5e-7 and the same
# tensor's error 0.2.  The weight gradient itself (5e-10 x scale) would fit; it is the per-voxel gradient that does not.
NEEDS_MORE = {("UNet4b2i3o", "fp16", "d_blocks.3.block.0.weight"): 2.8,
              ("UNetSPSmall", "fp16", "d_blocks.3.block.0.weight"): 15.0}


@pytest.mark.parametrize("fuse", [True, False], ids=["lp_fused", "lp_unfused"])
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("cid", MS.LOWP_IDS)
def test_16_bit_train_step_next_to_the_autocast_yardstick(cid, precision, fuse, monkeypatch):
    """The nine classes in bf16 / fp16, both values of engine.LP_FUSE_UP.  Ties in 2 x 2 x 2 max-pool windows still route
    gradients differently after 16-bit rounding, so this is no 1e-4 test: it keeps the form of
    test_lowp_gpu.test_lowp_nets_against_the_fp32_oracle -- the oracle graph under torch.autocast("cpu", dtype) on the same
    stable state is the yardstick, and this path's deviation from the FP64 oracle is held against the yardstick's with that
    test's margins.  With the masks pinned two more things can be asked: the yardstick's own margin stays positive (else
    the case is unfit: raise its multiplier), and EVERY gradient tensor keeps its sign pattern and scale -- relative L2
    against fp64 <= 2 x the yardstick's for the same tensor + 0.02 (2: reassociation between two correct 16-bit
    pipelines), not only the worst tensor against the worst tensor.

    fp16: on these states the gradients fall by about 1e-2 per level, and the yardstick, which runs without a loss scale,
    returns an identically zero gradient for 30 to 65 of a class's 59 to 73 tensors (relative L2 exactly 1: the gate is
    2.02 there) and noise for most others.  This path scales the loss (2^11 at 32^3, 2^14 at 64^3) and stays inside every
    gate but for the two tensors of NEEDS_MORE, which are listed with their measured ratios as the issue provides."""
    from ctunet_amd import engine
    monkeypatch.setattr(engine, "LP_FUSE_UP", fuse)
    r64, yard_run = MS.reference(cid, "fp64"), MS.reference(cid, precision)
    assert r64["margin"][0] >= 1.0 and yard_run["margin"][0] > 0, (r64["margin"], yard_run["margin"])
    y = MS.metrics(yard_run["outs"], yard_run["loss"], yard_run["grads"], yard_run["dx"], r64, yardstick=True)
    got = hip_step(cid, precision)
    r = MS.metrics(got["outs"], got["loss"], got["grads"], got["dx"], r64)
    for n_ in list(yard_run["grads"]) + ["dx"]:
        g = yard_run["dx"] if n_ == "dx" else yard_run["grads"][n_]
        # (a yardstick with inf / NaN in it would switch gates off: the case is unfit on this host, not passed)
        assert g is None or bool(torch.isfinite(g.float()).all()), f"unfit: the autocast yardstick's {n_} is not finite"
    more = {t: f for (c, p, t), f in NEEDS_MORE.items() if (c, p) == (MS.BY_ID[cid][0], precision)}
    par = [n_ for n_ in r["l2"] if n_ != "dx"]
    cos_r, cos_y = min(r["cos"][n_] for n_ in par), min(y["cos"][n_] for n_ in par)
    l2_r, l2_y = max(r["l2"][n_] for n_ in par if n_ not in more), max(y["l2"][n_] for n_ in par)
    ratio = max((r["l2"][n_] / max(y["l2"][n_], 1e-300), n_) for n_ in r["l2"])
    over = max((r["l2"][n_] - 2 * y["l2"][n_], n_) for n_ in r["l2"])
    zero = sum(bool(((yard_run["dx"] if n_ == "dx" else yard_run["grads"][n_]) == 0).all()) for n_ in r["l2"])
    tag = f"{cid} {precision} {'fused' if fuse else 'unfused'}"
    print(f"[{tag}] margin fp64 {r64['margin'][0]:.3f} autocast {yard_run['margin'][0]:.3f}; {zero} of {len(r['l2'])} tensors zero in "
          f"the yardstick\n"
          f"[{tag}] hip      out {r['out_err']:.2e} loss {r['loss_err']:.2e} dice {r['dice']:.4f} cos min {cos_r:.4f} dx cos "
          f"{r['cos']['dx']:.5f} l2 max {l2_r:.3e}\n"
          f"[{tag}] autocast out {y['out_err']:.2e} loss {y['loss_err']:.2e} dice {y['dice']:.4f} cos min {cos_y:.4f} dx cos "
          f"{y['cos']['dx']:.5f} l2 max {l2_y:.3e}\n"
          f"[{tag}] same tensor: largest l2 ratio {ratio[0]:.2f} ({ratio[1]}: {r['l2'][ratio[1]]:.2e} vs {y['l2'][ratio[1]]:.2e}), "
          f"largest l2 - 2 x yardstick {over[0]:.2e} ({over[1]})")
    assert r["out_err"] <= 1.5 * y["out_err"] and r["loss_err"] <= max(3 * y["loss_err"], 2e-4), (r["out_err"], y["out_err"])
    assert r["dice"] >= y["dice"] - 0.004, (r["dice"], y["dice"])
    assert cos_r >= cos_y - 0.05 and r["cos"]["dx"] >= y["cos"]["dx"] - 0.05, (cos_r, cos_y, r["cos"]["dx"], y["cos"]["dx"])
    assert l2_r <= 1.3 * l2_y + 0.05, (l2_r, l2_y)
    bad = [(n_, r["l2"][n_], y["l2"][n_]) for n_ in r["l2"] if r["l2"][n_] > more.get(n_, 2.0) * y["l2"][n_] + 0.02]
    assert not bad, bad
