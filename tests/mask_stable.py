"""Mask-stable states of the SHIPPED classes (test infrastructure, not product code; no GPU needed).

At default initialisation every BatchNorm has gamma = 1, beta = 0 and the ReLU masks sit on zero: a layer that is handed
the gamma, beta or coefficient row of a sibling of equal width computes the same thing, and one mask flip moves a gradient
entry by percents, so the whole-net gates are loose.  Here every BatchNorm of a shipped class gets

    gamma = +-U(0.5, 1.5)      beta = +-mult * |gamma|, every third channel negative ("off")
    running mean ~ 0.1 N(0, 1)  running variance ~ U(0.5, 1.5)

(the rule of tests/golden/make_golden.py::stabilize_bn with the multiplier as a parameter, restated because that file imports
the reference).  A channel's pre-activation gamma * yhat + beta then stays `mult` standard deviations away from zero: it is
always on or always off, forward and backward are smooth in the weights, and a tight gradient gate has no mask flip to
hide behind.  The MARGIN of a run is the smallest sign(beta) * (BatchNorm output) over every BatchNorm of the train-mode
forward: positive = no mask can flip.  tests/test_mask_stable_cpu.py holds CASES to their margins in the oracle alone;
tests/test_mask_stable_gpu.py holds the HIP path to the fp64 oracle on them."""
import functools

import torch
import torch.nn.functional as F

from oracle import unet_oracle as O
from util import CLASS_INPUT, gen, onehot_target, rel_err

# (class, ctor kwargs, input shape, mult, seed).  mult / seed: picked until the fp64 oracle ALONE meets the margin condition
# (a condition on the inputs; measured margins in profiles/mask_stable_gates.md) -- from mult 8, seed 8; the 5-block classes
# at 64^3 normalise 262 144 voxels per channel, whose extremes lie further out, and need more.  mult <= 16 keeps the
# pre-activations within a few tens, so one bf16 ulp (2^-8 relative) of one stays below a margin of 1.
CASES = [
    ("UNet", {}, (1, 1, 32, 32, 32), 8.0, 8),
    ("UNet4b2i3o", {}, (1, 2, 32, 32, 32), 8.0, 8),
    ("UNet5b2i3o", {}, (1, 2, 64, 64, 64), 12.0, 8),
    ("UNet4b1i3o", {}, (1, 1, 32, 32, 32), 8.0, 8),
    ("UNetSP", {}, (1, 2, 32, 32, 32), 8.0, 8),
    ("UNetSPSmall", {}, (1, 2, 64, 64, 64), 12.0, 8),
    ("UNetDO", {}, (1, 1, 32, 32, 32), 8.0, 8),
    ("recAE_v2_fixed", {}, (1, 1, 32, 32, 32), 8.0, 8),
    ("UNet4_2IC", {}, (1, 2, 32, 32, 32), 8.0, 8),
    ("UNet", {}, (2, 1, 32, 32, 32), 8.0, 8),
    ("UNetSP", {}, (2, 2, 32, 32, 32), 8.0, 8),
    ("UNet", {}, (1, 1, 32, 48, 64), 8.0, 8),
    ("recAE_v2_fixed", {}, (2, 1, 32, 32, 32), 10.0, 8),
]
assert [(c[0], c[2]) for c in CASES[:9]] == [(n_, (1, ch, s, s, s)) for n_, (ch, s) in CLASS_INPUT.items()]


def case_id(case):
    return f"{case[0]}-{'x'.join(str(s) for s in case[2])}"


IDS = [case_id(c) for c in CASES]
BY_ID = dict(zip(IDS, CASES))
LOWP_IDS = IDS[:9]                  # the 16-bit tests run the nine classes at batch 1: margin >= 1.0; fp32-only cases >= 0.5
DTYPES = {"fp64": torch.float64, "fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def min_margin(cid):
    return 1.0 if cid in LOWP_IDS else 0.5


def build(name, **ctor_kwargs):
    """The shipped class on the CPU with the seeded default initialisation every whole-net test uses."""
    import ctunet_amd
    torch.manual_seed(0)
    net = getattr(ctunet_amd, name)(**ctor_kwargs)
    net.chk = False
    return net


def stable_state(name, mult, seed, **ctor_kwargs):
    """State dict of the class with the rule of the module docstring applied to every BatchNorm, in the sorted order of
    their running_mean keys, from one generator."""
    sd = {k: v.detach().clone() for k, v in build(name, **ctor_kwargs).state_dict().items()}
    g = gen(seed)
    for key in sorted(k for k in sd if k.endswith(".running_mean")):
        p = key[:-len("running_mean")]
        c = sd[key].numel()
        gam = (torch.rand(c, generator=g) + 0.5) * (torch.randint(0, 2, (c,), generator=g).float() * 2 - 1)
        on = torch.tensor([1.0 if (i % 3 != 2 or c == 1) else -1.0 for i in range(c)])
        sd[p + "weight"].copy_(gam)
        sd[p + "bias"].copy_(mult * gam.abs() * on)
        sd[p + "running_mean"].copy_(torch.randn(c, generator=g) * 0.1)
        sd[p + "running_var"].copy_(torch.rand(c, generator=g) + 0.5)
    return sd


def case_inputs(case):
    """(x, targets) of a case: the generators of test_models_gpu.oracle_train_check."""
    name, _, shape, _, _ = case
    x = torch.randn(shape, generator=gen(1234))
    two = O.SPECS[name].head != "plain"
    return x, [onehot_target((shape[0], 2) + tuple(shape[2:]), 4321 + i, 0.2) for i in range(2 if two else 1)]


def loss_kind(name):
    """'double' (shape-prior heads), 'single' (2-channel heads: the handler's CE + Dice) or 'mse' (3-channel plain classes),
    the selection of test_models_gpu.oracle_train_check."""
    spec = O.SPECS[name]
    return "double" if spec.head != "plain" else ("single" if spec.out_ch == 2 else "mse")


def oracle_run(name, sd, x, targets, dtype):
    """One train-mode forward + loss + backward of the oracle on state `sd` (left untouched).  dtype float64 / float32: the
    whole graph in that type; bfloat16 / float16: the fp32 graph under torch.autocast("cpu", dtype), the yardstick of the
    16-bit tests.  Returns a dict: outs (tuple), loss, grads {parameter: gradient or None}, dx, buffers (the BatchNorm
    buffers after the step) and margin = (value, BatchNorm prefix), taken by wrapping O._bn for the duration of the call."""
    spec, kind = O.SPECS[name], loss_kind(name)
    auto = dtype in (torch.bfloat16, torch.float16)
    wd = torch.float32 if auto else dtype
    sd = {k: (v.to(wd, copy=True) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    tg = [t.to(wd) for t in targets]
    if kind == "double":
        fn = lambda o: O.loss_double([t.float() for t in o] if auto else o, tg, 1.0, 1.0)[0]
    elif kind == "single":
        fn = lambda o: O.loss_single(o.float() if auto else o, tg[0], 1.0, 1.0)[0]
    else:
        fn = lambda o: ((o.float() if auto else o) ** 2).mean()
    worst = [float("inf"), None]
    inner = O._bn

    def watched(x_, sd_, prefix, training, stat_updates):
        y = inner(x_, sd_, prefix, training, stat_updates)
        sign = torch.sign(sd_[prefix + ".bias"].detach()).to(y.dtype).view(1, -1, 1, 1, 1)
        m = float((y.detach() * sign).min())
        if m < worst[0]:
            worst[:] = [m, prefix]
        return y
    O._bn = watched
    threads = torch.get_num_threads()
    if dtype == torch.bfloat16:
        # ATen-CPU's threaded bf16 run of the k = 5 nets is not reproducible on hosts with native bf16 units (same call, 16
        # threads: relative L2 of ublock1.1.weight 1.08, inf, inf, 1.6e35); on one thread it is (0.2 s per case)
        torch.set_num_threads(1)
    try:
        if auto:
            with torch.autocast("cpu", dtype=dtype):
                out, loss, g, dx = O.grads(spec, sd, x.to(wd), fn, training=True)
        else:
            out, loss, g, dx = O.grads(spec, sd, x.to(wd), fn, training=True)
    finally:
        O._bn = inner
        torch.set_num_threads(threads)
    outs = out if isinstance(out, tuple) else (out,)
    return {"outs": tuple(o.detach() for o in outs), "loss": float(loss), "grads": g, "dx": dx, "margin": tuple(worst),
            "buffers": {k: v for k, v in sd.items() if "running_" in k or "num_batches" in k}}


@functools.lru_cache(maxsize=None)
def state(cid):
    name, kw, _, mult, seed = BY_ID[cid]
    return stable_state(name, mult, seed, **kw)


@functools.lru_cache(maxsize=None)
def reference(cid, precision):
    """oracle_run of a case, once per process: the engine-switch matrix and both LP_FUSE_UP values share it.  Read only."""
    case = BY_ID[cid]
    x, tg = case_inputs(case)
    return oracle_run(case[0], state(cid), x, tg, DTYPES[precision])


def live(r64):
    """Names of the gradients that carry a value: not the dead centre block's (None), not a conv bias in front of a
    BatchNorm (key <block>.<i>.bias with a 5-D weight and a BatchNorm at <block>.<i + 1>), whose true gradient is zero --
    rounding noise on every side.  Told by structure, not by size: on these states the gradients of the deep levels are
    1e-9 .. 1e-13 in fp64, far below the head's, and they are live."""
    g = r64["grads"]
    names = []
    for n_, r in g.items():
        if r is None:
            continue
        head, _, leaf = n_.rpartition(".")
        block, _, idx = head.rpartition(".")
        if leaf == "bias" and idx.isdigit() and g[head + ".weight"].dim() == 5 and f"{block}.{int(idx) + 1}.running_mean" in r64["buffers"]:
            continue
        names.append(n_)
    return names


def metrics(outs, loss, grads, dx, r64, yardstick=False):
    """Deviation of one run from the fp64 oracle in the terms of test_lowp_gpu._metrics, the gradient terms per tensor.
    Every gradient of the run under test must be finite; the caller looks at the yardstick's."""
    refs = r64["outs"]
    res = {"out_err": max(rel_err(o.float(), r) for o, r in zip(outs, refs)),
           "dice": min(float(O.hard_dice(o.detach().float().cpu(), F.one_hot(O.argmax1(r), r.shape[1]).movedim(-1, 1).float()))
                       for o, r in zip(outs, refs)),
           "loss_err": abs(float(loss) - r64["loss"]), "cos": {}, "l2": {}}
    for n_ in live(r64) + ["dx"]:
        got = dx if n_ == "dx" else grads[n_]
        a, b = got.detach().cpu().double().flatten(), (r64["dx"] if n_ == "dx" else r64["grads"][n_]).flatten()
        assert yardstick or torch.isfinite(a).all(), n_
        res["cos"][n_] = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300))
        res["l2"][n_] = float((a - b).norm() / b.norm())
    return res


def worst_error(grads, dx, r64):
    """(error, tensor): the largest |got - fp64| of dx and every live gradient, as a fraction of the tensor's largest fp64 entry."""
    worst = (0.0, None)
    for n_ in live(r64) + ["dx"]:
        got, ref = (dx, r64["dx"]) if n_ == "dx" else (grads[n_], r64["grads"][n_])
        e = float((got.detach().cpu().double() - ref).abs().max() / ref.abs().max())
        worst = max(worst, (e, n_))
    return worst
