"""Learning rate, plateau schedule and gradient clipping kept on the device (MI355X): the new kernels against the existing
Adam entry point (bit for bit), numpy float64 and torch's scheduler, and the host layer in eager steps, replayed graphs
(single and the one-rank distributed chain), float16 dynamic loss scaling, StepRunner and checkpoints.

Kernel cases use pointer tables that reach every path of a table kernel: sizes below one wave, ragged vector tails, more
than one grid-stride trip, 65 tensors (second 64-tensor chunk) and one tensor whose base is 4- but not 16-byte aligned.
Network cases use UNet() at 32^3: the smallest patch its four pooling levels train on (16^3 leaves BatchNorm one value per
channel in the centre block, which raises as in torch)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

import train_controls_ref as R
from util import gen, onehot_target

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [1, 3, 63, 257, 4099, 70001]
B1, B2, EPS = 0.9, 0.999, 1e-8


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tensors(seed, scale=1.0, count=65):
    """65 tensors: SIZES, then the five small ones again and again; tensor 4 (4099 values) is a view one float into its
    storage, so its base is 4- but not 16-byte aligned."""
    g = gen(seed)
    sizes = SIZES + [SIZES[i % 5] for i in range(count - len(SIZES))]
    out = []
    for i, n in enumerate(sizes):
        if i == 4:
            base = (torch.randn(n + 1, generator=g) * scale).cuda()
            t = base[1:]
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        else:
            t = (torch.randn(n, generator=g) * scale).cuda()
            assert t.data_ptr() % 16 == 0
        out.append(t)
    return out


def _like(ts, fn):
    """New tensors with the same sizes AND the same alignment as ts, filled by fn(t)."""
    out = []
    for t in ts:
        if t.storage_offset():
            b = torch.empty(t.numel() + t.storage_offset(), device=t.device)
            v = b[t.storage_offset():]
        else:
            v = torch.empty_like(t)
        v.copy_(fn(t))
        out.append(v)
    return out


class _State:
    """Parameters + the three moments + the step counter of one synthetic 'group'."""

    def __init__(self, params):
        self.p = _like(params, lambda t: t)
        self.m = _like(params, torch.zeros_like)
        self.v = _like(params, torch.zeros_like)
        self.vm = _like(params, torch.zeros_like)
        self.step = torch.zeros(1, device="cuda")

    def table(self, grads):
        ptrs = []
        for p, g, m, v, vm in zip(self.p, grads, self.m, self.v, self.vm):
            ptrs += [p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), vm.data_ptr()]
        n = len(self.p)
        return (C.c_void_p * (5 * n))(*ptrs), (C.c_int64 * n)(*[p.numel() for p in self.p]), n

    def host(self, grads, lr, wd=0.0, dec=0, skip=None):
        from ctunet_amd import _lib
        pa, sa, n = self.table(grads)
        _lib.check(_lib.load().ctu_adam_amsgrad(pa, sa, n, self.step.data_ptr(), lr, B1, B2, EPS, wd, dec,
                                                None if skip is None else skip.data_ptr(), _stream()), "adam")

    def dev(self, grads, lr_t, wd=0.0, dec=0, coef=None, skip=None):
        from ctunet_amd import _lib
        assert lr_t.dtype == torch.float64
        pa, sa, n = self.table(grads)
        _lib.check(_lib.load().ctu_adam_amsgrad_dev(pa, sa, n, self.step.data_ptr(), lr_t.data_ptr(), B1, B2, EPS, wd, dec,
                                                    None if coef is None else coef.data_ptr(),
                                                    None if skip is None else skip.data_ptr(), _stream()), "adam_dev")

    def clone(self):
        c = _State(self.p)
        c.m, c.v, c.vm = (_like(x, lambda t: t) for x in (self.m, self.v, self.vm))
        c.step = self.step.clone()
        return c

    def assert_equal(self, other, what=""):
        torch.cuda.synchronize()
        assert torch.equal(self.step, other.step), what
        for k in ("p", "m", "v", "vm"):
            for i, (a, b) in enumerate(zip(getattr(self, k), getattr(other, k))):
                assert torch.equal(a, b), (what, k, i, a.numel())


def _grads(params, it, scale=1.0):
    g = gen(1000 + it)
    return _like(params, lambda t: (torch.randn(t.numel(), generator=g) * scale * (1.0 + it)).cuda())


def _clip(grads, max_norm):
    """ctu_grad_clip_coef on a list of tensors -> (norm, coef) float32[1] device tensors."""
    from ctunet_amd import _lib
    lib = _lib.load()
    n = len(grads)
    sa = (C.c_int64 * n)(*[g.numel() for g in grads])
    nb = lib.ctu_grad_norm_num_blocks(sa, n)
    assert nb >= n
    ws = torch.full((nb + 8,), float("nan"), device="cuda")             # (the tail must stay untouched)
    norm, coef = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    ga = (C.c_void_p * n)(*[g.data_ptr() for g in grads])
    _lib.check(lib.ctu_grad_clip_coef(ga, sa, n, max_norm, ws.data_ptr(), norm.data_ptr(), coef.data_ptr(), _stream()), "clip")
    torch.cuda.synchronize()
    assert torch.isnan(ws[nb:]).all()
    return norm, coef


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("wd,dec", [(0.0, 0), (0.01, 0), (0.01, 1)])
@pytest.mark.parametrize("coef_one", [False, True])
def test_adam_dev_is_bit_equal_to_the_host_entry_point(wd, dec, coef_one):
    params = _tensors(1)
    a, b = _State(params), _State(params)
    lr_t = torch.full((1,), 1e-2, dtype=torch.float64, device="cuda")
    coef = torch.ones(1, device="cuda") if coef_one else None
    for it in range(5):
        g = _grads(params, it)
        a.host(g, 1e-2, wd, dec)
        b.dev(g, lr_t, wd, dec, coef)
    a.assert_equal(b)
    assert float(a.step) == 5.0
    assert not torch.equal(a.p[5], params[5])
    # the skip flag set: nothing changes, the step counter included
    flag = torch.ones(1, device="cuda")
    before = b.clone()
    b.dev(_grads(params, 9), lr_t, wd, dec, coef, skip=flag)
    b.assert_equal(before, "skipped")
    flag.zero_()                                                         # cleared: the same call now steps
    b.dev(_grads(params, 9), lr_t, wd, dec, coef, skip=flag)
    a.host(_grads(params, 9), 1e-2, wd, dec)
    a.assert_equal(b, "after the skip")


def test_a_changed_device_learning_rate_is_what_the_host_entry_point_does_with_that_rate():
    params = _tensors(2)
    a, b = _State(params), _State(params)
    lrs = [1e-2, 1e-2, 1e-2 * 0.1, 1e-2 * 0.1, 3.3e-4]                   # (1e-3 as a double product: not float(1e-3)'s double)
    lr_t = torch.zeros(1, dtype=torch.float64, device="cuda")
    for it, lr in enumerate(lrs):
        g = _grads(params, it)
        lr_t.fill_(lr)
        a.host(g, lr, 0.01, 0)
        b.dev(g, lr_t, 0.01, 0)
    a.assert_equal(b)


@pytest.mark.parametrize("scale", [1e-4, 1.0, 1e3])
def test_norm_against_float64(scale):
    """Bound 1e-6 relative, derived: the g*g terms are summed in double; each block's non-negative partial is rounded to
    float32 once (2^-24 relative on the sum, half of that on its root) and the root once more (2^-24): 9e-8 in all."""
    grads = _tensors(3, scale)
    exact = R.grad_norm([g.cpu().numpy() for g in grads])
    norm, coef = _clip(grads, exact / 2)
    got = float(norm)
    print(f"norm {got!r} exact {exact!r} rel {abs(got - exact) / exact:.3e}")
    assert abs(got - exact) <= 1e-6 * exact
    max32 = float(np.float32(exact / 2))
    assert np.float32(float(coef)) == R.clip_coef32(got, max32)          # the float32 formula, one IEEE division
    # torch forms reciprocal(norm + 1e-6) * max_norm: two roundings against one, at most 2 float32 ulps apart
    t = torch.clamp(max32 / (norm.cpu() + 1e-6), max=1.0)
    assert abs(float(t) - float(coef)) <= 2 * 2.0 ** -23 * float(coef)
    norm2, coef2 = _clip(grads, exact / 2)
    assert torch.equal(norm, norm2) and torch.equal(coef, coef2)          # fixed order: two calls are bit-equal
    one = _clip(grads, exact * 10)[1]
    assert float(one) == 1.0


def test_non_finite_gradients_propagate_as_in_torch():
    grads = _tensors(4)
    grads[5][12345] = float("inf")
    norm, coef = _clip(grads, 1.0)
    t = torch.clamp(1.0 / (torch.tensor([math.inf]) + 1e-6), max=1.0)     # torch's float32 formula on an inf norm: 0
    assert float(t) == 0.0
    assert math.isinf(float(norm)) and float(norm) > 0 and float(coef) == 0.0
    grads[5][12345] = -float("inf")
    norm, coef = _clip(grads, 1.0)
    assert math.isinf(float(norm)) and float(norm) > 0 and float(coef) == 0.0
    grads[2][7] = float("nan")
    norm, coef = _clip(grads, 1.0)
    t = torch.clamp(1.0 / (torch.tensor([math.nan]) + 1e-6), max=1.0)     # ... on a NaN norm: NaN (clamp propagates it)
    assert math.isnan(float(t))
    assert math.isnan(float(norm)) and math.isnan(float(coef))


@pytest.mark.parametrize("wd,dec", [(0.0, 0), (0.01, 0), (0.01, 1)])
def test_clipped_step_equals_the_host_entry_point_on_scaled_gradients(wd, dec):
    params = _tensors(5)
    g = _grads(params, 0)
    n0 = float(_clip(g, 1.0)[0])
    lr_t = torch.full((1,), 1e-2, dtype=torch.float64, device="cuda")
    # half the norm: the gradients are scaled by the coefficient the kernel wrote (same IEEE multiply, done by torch)
    norm, coef = _clip(g, n0 / 2)
    assert 0.49 < float(coef) < 0.51
    a, b = _State(params), _State(params)
    for _ in range(2):
        a.host([t * coef for t in g], 1e-2, wd, dec)
        b.dev(g, lr_t, wd, dec, coef)
    a.assert_equal(b, "clipped")
    # ten times the norm: the coefficient is exactly 1 and the step is the unclipped one
    norm, coef = _clip(g, n0 * 10)
    assert float(coef) == 1.0
    c, d = _State(params), _State(params)
    c.host(g, 1e-2, wd, dec)
    d.dev(g, lr_t, wd, dec, coef)
    c.assert_equal(d, "not clipped")
    assert not torch.equal(c.p[5], a.p[5])


@pytest.mark.parametrize("mode,tmode", R.MODES)
def test_plateau_kernel_follows_torch_bit_for_bit(mode, tmode):
    from ctunet_amd import optim
    from ctunet_amd.lr_scheduler import ReduceLROnPlateau
    for patience, cooldown, min_lr, eps in R.CONFIGS:
        for name, seq in R.SEQUENCES.items():
            kw = dict(mode=mode, factor=0.5, patience=patience, threshold=1e-2, threshold_mode=tmode, cooldown=cooldown,
                      min_lr=min_lr, eps=eps)
            lrs = [0.1, 0.1 / 3]
            opt = optim.Adam([{"params": [torch.zeros(3, device="cuda", requires_grad=True)], "lr": lr} for lr in lrs],
                             device_lr=True)
            mine = ReduceLROnPlateau(opt, **kw)
            ref = torch.optim.lr_scheduler.ReduceLROnPlateau(
                torch.optim.SGD([{"params": [torch.zeros(1, requires_grad=True)], "lr": lr} for lr in lrs], lr=1.0), **kw)
            reductions = 0
            for i, m in enumerate(R.metric32(seq)):
                m = -m if mode == "max" else m
                before = [g["lr"] for g in ref.optimizer.param_groups]
                ref.step(m)
                reductions += before[0] != ref.optimizer.param_groups[0]["lr"]
                mine.step(torch.tensor([m], dtype=torch.float32, device="cuda"))
                got_lr = opt.get_lr()
                for gi in range(2):
                    c = mine._counters[gi].tolist()
                    got = (np.float64(got_lr[gi]).tobytes(), np.float64(mine._best[gi].item()).tobytes(), c[0], c[1], c[2])
                    assert got == R.torch_snapshot(ref, gi), (kw, name, i, gi, got_lr, c)
                    if gi == 0:
                        assert c[3] == reductions
            assert mine.get_last_lr() == [g["lr"] for g in ref.optimizer.param_groups]


# ------------------------------------------------------------------ the host layer on a network
def _data(seed=2):
    x = torch.randn(1, 1, 32, 32, 32, generator=gen(seed)).cuda()
    t = onehot_target((1, 2, 32, 32, 32), seed + 1, 0.3).cuda()
    return x, t


def _make(lr=1e-3, cls="Adam", use_checkpoint=True, fp16=None, **kw):
    import ctunet_amd
    from ctunet_amd import optim
    torch.manual_seed(0)
    net = ctunet_amd.UNet(use_checkpoint=use_checkpoint).cuda().train()
    if fp16 is not None:
        net.set_precision(torch.float16, loss_scale=fp16)
    return net, getattr(optim, cls)(net.parameters(), lr=lr, amsgrad=True, **kw).guard(net)


def _eager(net, opt, x, t, sched=None):
    from ctunet_amd import losses as L
    ce, dc = L.fused_ce_dice(net(x.clone().requires_grad_(True)), t, 1.0, 1.0, False)
    loss = ce + dc
    loss.backward()
    opt.step()
    if sched is not None:
        sched.step(loss.detach())
    for p in net.parameters():
        p.grad = None
    return loss.detach()


def _assert_same(net_a, net_b, what=""):
    torch.cuda.synchronize()
    for (n, a), (_, b) in zip(net_a.state_dict().items(), net_b.state_dict().items()):
        assert torch.equal(a, b), (what, n)


def _differs(net_a, net_b):
    return any(not torch.equal(a, b) for a, b in zip(net_a.parameters(), net_b.parameters()))


def test_whole_optimizer_with_clipping_against_torch():
    """optim.Adam(max_grad_norm) vs clip_grad_norm_ + torch.optim.Adam(amsgrad=True) on parameter copies fed the same
    gradients, three steps; L2 weight decay, so that the scale of the gradient matters.  Tolerances: those of
    test_models_gpu.py::test_fused_adam_matches_torch."""
    x, t = _data()
    max_norm = 1e-2
    net, opt = _make(lr=1e-2, weight_decay=0.01, max_grad_norm=max_norm)
    from ctunet_amd import losses as L
    twins = {n: p.detach().clone().requires_grad_(True) for n, p in net.named_parameters()}
    ref = torch.optim.Adam(list(twins.values()), lr=1e-2, weight_decay=0.01, amsgrad=True)
    for it in range(3):
        ce, dc = L.fused_ce_dice(net(x.clone().requires_grad_(True)), t, 1.0, 1.0, False)
        (ce + dc).backward()
        for n, p in net.named_parameters():
            twins[n].grad = None if p.grad is None else p.grad.clone()
        total = torch.nn.utils.clip_grad_norm_(list(twins.values()), max_norm)
        ref.step()
        opt.step()
        assert float(total) > max_norm                                   # the clip is active
        assert abs(float(opt.last_grad_norm) - float(total)) <= 1e-5 * float(total)
        for p in net.parameters():
            p.grad = None
    for n, p in net.named_parameters():
        assert torch.allclose(p.detach(), twins[n].detach(), rtol=1e-5, atol=1e-6), n
    live = [(n, p) for n, p in net.named_parameters() if len(opt.state[p])]
    assert len(live) == 58
    for n, p in live:
        for k in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert torch.allclose(opt.state[p][k], ref.state[twins[n]][k], rtol=1e-5, atol=1e-7), (n, k)


def test_a_host_edit_of_the_learning_rate_reaches_the_replayed_graph():
    """The frozen-lr gap: two replays, group['lr'] *= 0.1 on the host, two more -- bit-equal to eager steps with the same
    schedule, and different from replays without the change."""
    from ctunet_amd.graph import GraphedTrainStep
    x, t = _data()

    def graphed(change):
        net, opt = _make(device_lr=True)
        gs = GraphedTrainStep(net, opt, x, [t], 1.0, 1.0, warmup=3)
        for i in range(4):
            if change and i == 2:
                opt.param_groups[0]["lr"] *= 0.1
            gs(x, [t])
        torch.cuda.synchronize()
        return net, opt
    net_e, opt_e = _make(device_lr=True)
    for i in range(3 + 4):
        if i == 3 + 2:
            opt_e.param_groups[0]["lr"] *= 0.1
        _eager(net_e, opt_e, x, t)
    net_g, opt_g = graphed(True)
    assert opt_g.get_lr() == [1e-3 * 0.1] == opt_e.get_lr()
    _assert_same(net_e, net_g)
    net_f, _ = graphed(False)
    assert _differs(net_f, net_g)
    # and the default optimizer is untouched by all this: same steps as device_lr at a constant rate
    net_d, opt_d = _make()
    for _ in range(3 + 4):
        _eager(net_d, opt_d, x, t)
    _assert_same(net_d, net_f, "device_lr=False")


SCHED_LR = 0.3        # three times the scale of the initial weights per Adam step: the loss on the fixed input does not fall
                      # monotonically, so the patience-0 schedule has something to react to (at 2e-2 it fell 27 steps in a row)


def _sched_run(graph, steps, distributed=False, lr=SCHED_LR):
    from ctunet_amd.graph import GraphedTrainStep
    from ctunet_amd.lr_scheduler import ReduceLROnPlateau
    x, t = _data()
    net, opt = _make(lr=lr, device_lr=True)
    sched = ReduceLROnPlateau(opt, patience=0, threshold=0, factor=0.5)
    losses, lrs = [], []
    if graph:
        gs = GraphedTrainStep(net, opt, x, [t], 1.0, 1.0, warmup=3, scheduler=sched, distributed=distributed)
        assert sched.last_epoch == 3                                     # the warm-up steps stepped it, the capture did not
        for _ in range(steps):
            losses.append(gs(x, [t])[-1].clone())
            lrs.append(opt.get_lr()[0])
    else:
        for i in range(3 + steps):
            loss = _eager(net, opt, x, t, sched)
            if i >= 3:
                losses.append(loss.clone())
                lrs.append(opt.get_lr()[0])
    torch.cuda.synchronize()
    return net, opt, sched, [float(v) for v in losses], lrs


def _torch_lrs(losses, lr0, state):
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=lr0),
                                                     patience=0, threshold=0, factor=0.5)
    ref.load_state_dict(state)
    out = []
    for v in losses:
        ref.step(v)
        out.append(ref.optimizer.param_groups[0]["lr"])
    return out


def test_scheduler_inside_the_graph_follows_the_eager_loop_and_torch():
    steps = 24
    net_e, opt_e, sch_e, losses_e, lrs_e = _sched_run(False, steps)
    # torch's scheduler fed the logged losses gives the same trajectory (from the state after the three warm-up steps)
    x, t = _data()
    net_w, opt_w = _make(lr=SCHED_LR, device_lr=True)
    from ctunet_amd.lr_scheduler import ReduceLROnPlateau
    sch_w = ReduceLROnPlateau(opt_w, patience=0, threshold=0, factor=0.5)
    for _ in range(3):
        _eager(net_w, opt_w, x, t, sch_w)
    state3, lr3 = sch_w.state_dict(), opt_w.get_lr()[0]
    net_g, opt_g, sch_g, losses_g, lrs_g = _sched_run(True, steps)
    print("losses", losses_g, "lrs", lrs_g, "reductions", sch_g.num_reductions)
    assert sch_g.num_reductions >= 2                                     # the schedule acted inside the replays
    assert lrs_g[-1] < lrs_g[0] or lrs_g[0] < SCHED_LR
    assert losses_g == losses_e and lrs_g == lrs_e
    assert sch_g.state_dict() == sch_e.state_dict()
    _assert_same(net_e, net_g)
    assert lrs_g == _torch_lrs(losses_g, lr3, state3)


def test_clipping_inside_the_graph_is_bit_equal_to_eager():
    from ctunet_amd.graph import GraphedTrainStep
    x, t = _data()
    kw = dict(lr=1e-2, weight_decay=0.01, max_grad_norm=1e-2)
    net_e, opt_e = _make(**kw)
    norms_e = []
    for _ in range(3 + 3):
        _eager(net_e, opt_e, x, t)
        norms_e.append(float(opt_e.last_grad_norm))
    net_g, opt_g = _make(**kw)
    gs = GraphedTrainStep(net_g, opt_g, x, [t], 1.0, 1.0, warmup=3)
    norms_g = []
    for _ in range(3):
        gs(x, [t])
        norms_g.append(float(opt_g.last_grad_norm))
    _assert_same(net_e, net_g)
    assert norms_g == norms_e[3:]
    assert len(set(norms_g)) == 3 and all(math.isfinite(v) and v > 1e-2 for v in norms_g)       # not frozen, and active


def test_fp16_overflow_skips_the_clipped_device_lr_step():
    import ctunet_amd
    from ctunet_amd.graph import GraphedTrainStep
    x, t = _data()
    cfg = ctunet_amd.DynamicLossScale(init_scale=2.0 ** 40, growth_interval=10 ** 6)
    kw = dict(lr=1e-3, fp16=cfg, device_lr=True, max_grad_norm=1e-2, weight_decay=0.01)
    net_e, opt_e = _make(**kw)
    start = [p.detach().clone() for p in net_e.parameters()]
    for _ in range(4):
        _eager(net_e, opt_e, x, t)                                       # 2^40: every one overflows
    net_e.loss_scaler.scale.fill_(2.0 ** 8)
    _eager(net_e, opt_e, x, t)                                           # the clean step
    net_g, opt_g = _make(**kw)
    gs = GraphedTrainStep(net_g, opt_g, x, [t], 1.0, 1.0, warmup=3)
    sc = net_g.loss_scaler
    gs(x, [t])
    torch.cuda.synchronize()
    assert sc.skipped_steps() == 4 and sc.get_scale() == 2.0 ** 36       # backed off four times
    assert float(opt_g.param_groups[0]["step_t"]) == 0.0
    for p, b in zip(net_g.parameters(), start):
        assert torch.equal(p.detach(), b)
    assert not math.isfinite(float(opt_g.last_grad_norm))
    sc.scale.fill_(2.0 ** 8)
    gs(x, [t])
    torch.cuda.synchronize()
    assert sc.skipped_steps() == 4 and float(opt_g.param_groups[0]["step_t"]) == 1.0
    assert math.isfinite(float(opt_g.last_grad_norm))
    assert any(not torch.equal(p.detach(), b) for p, b in zip(net_g.parameters(), start))
    _assert_same(net_e, net_g)


def test_one_rank_distributed_graph_with_scheduler_follows_eager():
    import torch.distributed as dist
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29561", rank=0, world_size=1,
                                device_id=torch.device("cuda", 0))
    try:
        steps = 12
        net_e, opt_e, sch_e, losses_e, lrs_e = _sched_run(False, steps)
        net_g, opt_g, sch_g, losses_g, lrs_g = _sched_run(True, steps, distributed=True)
        assert lrs_g == lrs_e and sch_g.state_dict() == sch_e.state_dict()
        for (n, a), (_, b) in zip(net_e.state_dict().items(), net_g.state_dict().items()):
            assert torch.allclose(a.float(), b.float(), rtol=2e-3, atol=1e-5), n       # test_loss_scale_gpu.py's bound
    finally:
        from ctunet_amd import parallel
        parallel.close_communicators()
        dist.destroy_process_group()


def _two_rank_worker(rank, world, port, tmp):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd"), os.path.join(ROOT, "tests")]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    try:
        import ctunet_amd
        from ctunet_amd import optim, parallel
        from ctunet_amd.graph import GraphedTrainStep
        from ctunet_amd.lr_scheduler import ReduceLROnPlateau
        torch.manual_seed(0)
        net = ctunet_amd.UNet(n_blocks=2, use_checkpoint=False).cuda().train()
        parallel.broadcast_parameters(net)
        opt = optim.Adam(net.parameters(), lr=SCHED_LR, device_lr=True)
        sched = ReduceLROnPlateau(opt, patience=0, threshold=0, factor=0.5)
        x = torch.randn(1, 1, 32, 32, 32, generator=gen(100 + rank)).cuda()          # different data: different losses
        t = onehot_target((1, 2, 32, 32, 32), 200 + rank, 0.2).cuda()
        gs = GraphedTrainStep(net, opt, x, [t], 1.0, 1.0, warmup=1, distributed=True, scheduler=sched)
        loss = None
        for _ in range(40):
            loss = gs(x, [t])[-1].clone()
            if sched.num_reductions >= 1:
                break
        mine = torch.tensor([opt.get_lr()[0], float(sched.num_reductions), float(loss)], dtype=torch.float64, device="cuda")
        both = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(both, mine)
        assert float(both[0][1]) >= 1                                    # a reduction happened ...
        assert float(both[0][2]) != float(both[1][2])                    # ... the ranks' own losses differ ...
        assert torch.equal(both[0][:2], both[1][:2])                     # ... and their learning rates do not
        open(os.path.join(tmp, f"ok{rank}"), "w").write("ok")
    finally:
        from ctunet_amd import parallel as par
        par.close_communicators()
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL refuses two ranks on one device)")
def test_two_ranks_keep_one_learning_rate(tmp_path):
    import torch.multiprocessing as mp
    world = 2
    port = 31600 + (os.getpid() % 2000)
    mp.spawn(_two_rank_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))


# ------------------------------------------------------------------ StepRunner
def _runner(**extra):
    from ctunet_amd.trainer import StepRunner
    torch.manual_seed(0)
    return StepRunner(dict(dict(model_class="UNet", problem_handler="FlapRec", learning_rate=1e-2, optimizer="adam",
                                weight_decay=0.01, ce_lambda=1.0, dice_lambda=1.0, device="cuda"), **extra))


def _loader(n=3):
    from ctunet_amd.datasets import SyntheticFlapDataset
    return torch.utils.data.DataLoader(SyntheticFlapDataset(n, size=32, seed=3, double_out=False, append_atlas=False),
                                       batch_size=1)


CONTROLS = dict(device_lr=True, max_grad_norm=1e-2, scheduler=None)


def test_step_runner_with_device_controls_equals_a_hand_written_loop(monkeypatch):
    from ctunet_amd import ProblemHandler as PH, lr_scheduler, optim
    loader = _loader()
    # the hand-written loop
    torch.manual_seed(0)
    import ctunet_amd
    net = ctunet_amd.UNet().cuda().train()
    opt = optim.Adam(net.parameters(), lr=1e-2, weight_decay=0.01, amsgrad=True, device_lr=True, max_grad_norm=1e-2).guard(net)
    sched = lr_scheduler.ReduceLROnPlateau(opt)

    class H:
        verbose = False
        params = dict(ce_lambda=1.0, dice_lambda=1.0, save_dice_plots=False, save_hd_plots=False)
        losses_and_metrics = {}
        pt_loss = None
    for i, s in enumerate(loader):
        out = net(s["image"].cuda().requires_grad_())
        PH.FlapRec.comp_losses_metrics(H, out, s["target"].cuda(), i, len(loader))
        H.pt_loss.backward()
        opt.step()
        sched.step(H.pt_loss.detach())
        for p in net.parameters():
            p.grad = None
    # host reads: count float(tensor) / tensor.item() during forward_pass
    calls = {"n": 0}
    real_float, real_item = torch.Tensor.__float__, torch.Tensor.item

    def counted_float(self):
        calls["n"] += 1
        return real_float(self)

    def counted_item(self):
        calls["n"] += 1
        return real_item(self)

    def count(run):
        monkeypatch.setattr(torch.Tensor, "__float__", counted_float)
        monkeypatch.setattr(torch.Tensor, "item", counted_item)
        calls["n"] = 0
        run.forward_pass("train", loader)
        monkeypatch.undo()
        return calls["n"]
    run = _runner(**CONTROLS)
    assert isinstance(run.params["scheduler"], lr_scheduler.ReduceLROnPlateau)
    with_controls = count(run)
    logging_only = count(_runner())                                      # no scheduler at all: what logging alone reads
    host_scheduler = count(_runner(scheduler=None))                      # torch's: one float(loss) more per batch
    assert with_controls == logging_only
    assert host_scheduler >= logging_only + len(loader)
    assert run.losses_and_metrics == H.losses_and_metrics and len(H.losses_and_metrics["epoch_loss"]) == len(loader)
    _assert_same(run.models["main"], net)
    assert run.params["scheduler"].state_dict() == sched.state_dict() and sched.last_epoch == len(loader)


def test_checkpoint_round_trip_continues_bit_equal(tmp_path):
    from ctunet_amd import checkpoint
    loader = _loader(2)
    whole = _runner(**CONTROLS)
    whole.forward_pass("train", loader)
    # a device-side reduction the host float has not seen: lr_t is ahead of group["lr"]
    whole.params["optimizer"].param_groups[0]["lr_t"].mul_(0.5)
    checkpoint.save_state(whole.models["main"], str(tmp_path / "model.pt"))
    checkpoint.save_train_state(whole.params["optimizer"], str(tmp_path / "train.pt"), whole.params["scheduler"])
    whole.forward_pass("train", loader)
    resumed = _runner(**CONTROLS)
    checkpoint.load_state(resumed.models["main"], str(tmp_path / "model.pt"))
    checkpoint.load_train_state(resumed.params["optimizer"], str(tmp_path / "train.pt"), resumed.params["scheduler"])
    assert resumed.params["scheduler"].last_epoch == 2
    resumed.forward_pass("train", loader)
    assert resumed.params["optimizer"].get_lr() == [1e-2 * 0.5] == whole.params["optimizer"].get_lr()
    assert resumed.params["scheduler"].state_dict() == whole.params["scheduler"].state_dict()
    _assert_same(whole.models["main"], resumed.models["main"])
    assert whole.losses_and_metrics["epoch_loss"][2:] == resumed.losses_and_metrics["epoch_loss"]
