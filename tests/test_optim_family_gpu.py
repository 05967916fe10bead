"""Fused SGD / RMSprop on the MI355X: the kernels against torch.optim over a tensor list that reaches every path of the
launch (a tensor past the grid stride, tensors below one 16-byte group, views that are only 4-byte aligned, more than 64
tensors, a parameter without gradient), then the device-side train controls on a small network: device learning rate,
clipping, overflow skip, HIP-graph replay with a plateau schedule, float16 loss scaling, StepRunner, checkpoints."""
import copy
import math

import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-5, atol=1e-6)                 # the project's optimizer tolerance (test_models_gpu.py::test_fused_adam_matches_torch)
SHAPES = [(8, 1, 3, 3, 3), (8,), (1,), (3,), (1000003,), (4099,), (4099,)] + [(5,)] * 70
ODD_OWNED, ODD_MIXED = 5, 6                      # views one float into their storage; ODD_OWNED's state sits there too
LR = {"SGD": 1e-2, "RMSprop": 1e-2}
STATE = {"SGD": ("momentum_buffer",), "RMSprop": ("square_avg", "momentum_buffer", "grad_avg")}
FULL = {"SGD": dict(momentum=0.9, nesterov=True, weight_decay=0.01),
        "RMSprop": dict(momentum=0.9, centered=True, weight_decay=0.01)}


def _odd(values):
    """The same values as a view that starts one float into its storage: 4-byte aligned only."""
    base = torch.empty(values.numel() + 1, dtype=torch.float32, device="cuda")
    view = base[1:]
    view.copy_(values.reshape(-1))
    assert view.data_ptr() % 16 == 4
    return view


@pytest.fixture(scope="module")
def base():
    """Parameters, gradients and the parameter without gradient, computed once and never modified.

    Parameters are N(0, 1); gradients are sign(z) * (0.5 + |z|), z ~ N(0, 1), so that every |gradient| is at least 0.5.
    The comparison with torch.optim is between two float32 evaluations that round differently (torch's kernels contract
    a + alpha * b into FMAs and take the clip norm in float32), so it can hold to rtol 1e-5 / atol 1e-6 only where the rule
    is well conditioned.  It is not where g = coef * grad + wd * p cancels to ~0: RMSprop's first step is
    g / (sqrt((1 - alpha) g^2) + eps) = 10 sign(g) outside |g| ~ 1e-7, a step function that turns the last bit of g into a
    parameter difference of lr * 10, and a momentum buffer whose terms (each up to ~10, rounded to ~1e-6) change sign
    cancels to a value below what atol resolves.  Among a million N(0, 1) gradients such elements exist; with |grad| >= 0.5
    the weight decay term (0.01 * |p| < 0.1, |p| stays below 10 over the five steps) cannot flip the sign of g, also
    under the clipping of test 3 (coefficient >= 0.35 / (1 + it) on gradients scaled by 1 + it), and every sum the rules
    form has terms of one sign."""
    assert len(SHAPES) == 77                                             # two 64-tensor launches per step
    assert max(math.prod(s) for s in SHAPES) > 128 * 256 * 4            # the large tensor crosses the grid stride
    g = torch.Generator().manual_seed(11)
    params = [torch.randn(s, generator=g).cuda() for s in SHAPES]
    z = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [(torch.where(v < 0, -1.0, 1.0) * (0.5 + v.abs())).cuda() for v in z]
    return params, grads, torch.randn(7, generator=g).cuda()


def _params(base, fused):
    ps = [(_odd(p) if fused and i in (ODD_OWNED, ODD_MIXED) else p.clone()) for i, p in enumerate(base[0])]
    ps.append(base[2].clone())
    return [p.requires_grad_(True) for p in ps]


def _set_grads(ps, base, scale, fused):
    for i, g in enumerate(base[1]):
        ps[i].grad = _odd(g * scale) if fused and i in (ODD_OWNED, ODD_MIXED) else g * scale
    assert ps[-1].grad is None


def _fused(name, ps, lr=None, **kw):
    """The fused optimizer; ODD_OWNED's state is made by the test at the same odd offset as the parameter and its gradient,
    so that tensor takes the scalar-head + 16-byte path, ODD_MIXED's (aligned state) the all-scalar one."""
    from ctunet_amd import optim
    opt = getattr(optim, name)(ps, lr=LR[name] if lr is None else lr, **kw)
    p, group = ps[ODD_OWNED], opt.param_groups[0]
    zeros = lambda: _odd(torch.zeros(p.numel(), device="cuda"))
    if name == "SGD":
        if group["momentum"] != 0:
            opt.state[p]["momentum_buffer"] = zeros()
            group["step_t"] = torch.zeros(1, dtype=torch.float32, device="cuda")       # (no step has been applied yet)
    else:
        opt.state[p]["square_avg"] = zeros()
        if group["momentum"] > 0:
            opt.state[p]["momentum_buffer"] = zeros()
        if group["centered"]:
            opt.state[p]["grad_avg"] = zeros()
    return opt


def _torch(name, ps, lr=None, **kw):
    kw = {k: v for k, v in kw.items() if k not in ("device_lr", "max_grad_norm")}
    return getattr(torch.optim, name)(ps, lr=LR[name] if lr is None else lr, **kw)


def _state(opt, p, k):
    v = opt.state[p].get(k) if p in opt.state else None
    return v if torch.is_tensor(v) else None


def _assert_close(name, ps, opt, twins, ref):
    torch.cuda.synchronize()
    for i, (p, t) in enumerate(zip(ps[:-1], twins[:-1])):
        assert torch.allclose(p.detach(), t.detach(), **TOL), (i, float((p.detach() - t.detach()).abs().max()))
        for k in STATE[name]:
            mine, want = _state(opt, p, k), _state(ref, t, k)
            assert (mine is None) == (want is None), (i, k)
            if mine is not None:
                assert torch.allclose(mine, want, **TOL), (i, k, float((mine - want).abs().max()))


def _assert_untouched(ps, opt, base):
    assert torch.equal(ps[-1].detach(), base[2]) and len(opt.state[ps[-1]]) == 0     # no gradient: untouched and stateless


def _parity(name, kw, base, clip=None):
    ps, twins = _params(base, True), _params(base, False)
    opt = _fused(name, ps, **kw, **({} if clip is None else dict(max_grad_norm=clip)))
    ref = _torch(name, twins, **kw)
    for it in range(5):
        _set_grads(ps, base, 1.0 + it, True)
        _set_grads(twins, base, 1.0 + it, False)
        if clip is not None:
            total = torch.nn.utils.clip_grad_norm_(twins, clip)
        opt.step()
        ref.step()
        if clip is not None:
            got, want = float(opt.last_grad_norm), float(total)
            assert want > clip                                           # the clip is active
            assert abs(got - want) <= 1e-6 * want, (it, got, want)
    _assert_close(name, ps, opt, twins, ref)
    _assert_untouched(ps, opt, base)
    assert float(opt.param_groups[0]["step_t"]) == 5.0
    if name == "RMSprop":
        assert all(opt.state[p]["step"] is opt.param_groups[0]["step_t"] for p in ps[:-1])


# ------------------------------------------------------------------ 1. parity with torch.optim
@pytest.mark.parametrize("kw", R.SGD_GRID, ids=R.grid_id)
def test_sgd_matches_torch_over_five_steps(kw, base):
    _parity("SGD", kw, base)


@pytest.mark.parametrize("kw", R.RMS_GRID, ids=R.grid_id)
def test_rmsprop_matches_torch_over_five_steps(kw, base):
    _parity("RMSprop", kw, base)


# ------------------------------------------------------------------ 2. the learning rate on the device
@pytest.mark.parametrize("name", ["SGD", "RMSprop"])
def test_device_learning_rate_is_bit_equal_to_the_host_one(name, base):
    def run(device_lr, edit):
        ps = _params(base, True)
        opt = _fused(name, ps, device_lr=device_lr, **FULL[name])
        for it in range(4):
            if edit and it == 2:
                opt.param_groups[0]["lr"] = 0.003
                opt.sync_lr()
            _set_grads(ps, base, 1.0 + it, True)
            opt.step()
        torch.cuda.synchronize()
        return ps, opt
    host, dev = run(False, True), run(True, True)
    assert dev[1].device_lr and dev[1].param_groups[0]["lr_t"].dtype == torch.float64 and "lr_t" not in host[1].param_groups[0]
    assert dev[1].get_lr() == [0.003] == host[1].get_lr()
    for i, (a, b) in enumerate(zip(host[0], dev[0])):
        assert torch.equal(a.detach(), b.detach()), i
        for k in STATE[name]:
            sa, sb = _state(host[1], a, k), _state(dev[1], b, k)
            assert (sa is None) == (sb is None) == (i == len(SHAPES)) and (sa is None or torch.equal(sa, sb)), (i, k)
    unchanged = run(True, False)
    assert not torch.equal(unchanged[0][4].detach(), dev[0][4].detach())       # the edit reached the kernel


# ------------------------------------------------------------------ 3. clipping
@pytest.mark.parametrize("name", ["SGD", "RMSprop"])
def test_clipping_equals_clip_grad_norm_then_torch(name, base):
    _parity(name, FULL[name], base, clip=1000.0)                         # (the norm of the list is ~1430 * (1 + it))


# ------------------------------------------------------------------ 4. the skip flag
def _snapshot(ps, opt, name):
    return [p.detach().clone() for p in ps], \
        [[None if _state(opt, p, k) is None else _state(opt, p, k).clone() for k in STATE[name]] for p in ps]


def _assert_frozen(ps, opt, name, snap):
    torch.cuda.synchronize()
    for i, p in enumerate(ps):
        assert torch.equal(p.detach(), snap[0][i]), i
        for k, was in zip(STATE[name], snap[1][i]):
            now = _state(opt, p, k)
            assert (now is None) == (was is None) and (was is None or torch.equal(now, was)), (i, k)


@pytest.mark.parametrize("name,kw", [("SGD", dict(momentum=0.9, dampening=0.3)),
                                     ("RMSprop", dict(momentum=0.9, centered=True))])
def test_a_set_skip_flag_changes_nothing_and_leaves_the_first_step_to_the_next(name, kw, base):
    ps, twins = _params(base, True), _params(base, False)
    opt, ref = _fused(name, ps, **kw), _torch(name, twins, **kw)
    flag = torch.ones(1, dtype=torch.float32, device="cuda")
    opt.skip_flag = flag
    start = [p.detach().clone() for p in ps]
    _set_grads(ps, base, 1.0, True)
    opt.step()                                                           # the very first step, skipped
    torch.cuda.synchronize()
    assert float(opt.param_groups[0]["step_t"]) == 0.0
    for p, s in zip(ps, start):
        assert torch.equal(p.detach(), s)
        assert all(_state(opt, p, k) is None or not _state(opt, p, k).any() for k in STATE[name])
    flag.zero_()
    _set_grads(ps, base, 2.0, True)
    _set_grads(twins, base, 2.0, False)
    opt.step()
    ref.step()                                                           # torch's first step: buf = g
    _assert_close(name, ps, opt, twins, ref)
    assert float(opt.param_groups[0]["step_t"]) == 1.0
    if name == "SGD":
        for i, p in enumerate(ps[:-1]):
            assert torch.equal(opt.state[p]["momentum_buffer"], p.grad), i          # not 0.7 * g: the dampening did not act
    flag.fill_(1.0)
    snap = _snapshot(ps, opt, name)
    _set_grads(ps, base, 3.0, True)
    opt.step()                                                           # a skipped step in the middle of a run
    _assert_frozen(ps, opt, name, snap)
    assert float(opt.param_groups[0]["step_t"]) == 1.0
    flag.zero_()
    _set_grads(twins, base, 3.0, False)
    opt.step()
    ref.step()
    _assert_close(name, ps, opt, twins, ref)
    assert float(opt.param_groups[0]["step_t"]) == 2.0
    _assert_untouched(ps, opt, base)


# ------------------------------------------------------------------ the controls on a small network
NET_LR = {"SGD": 1e-2, "RMSprop": 1e-3}
CONTROLS = dict(momentum=0.9, device_lr=True, max_grad_norm=1.0)


@pytest.fixture(scope="module")
def sample():
    from ctunet_amd.datasets import SyntheticFlapDataset
    s = SyntheticFlapDataset(1, size=16, seed=3, double_out=False, append_atlas=False)[0]
    return s["image"][None].contiguous(), s["target"][None].contiguous()


def _net(fp16=None):
    import ctunet_amd
    torch.manual_seed(0)
    net = ctunet_amd.UNet(n_blocks=2, i_size=2, use_checkpoint=False).cuda().train()
    if fp16 is not None:
        net.set_precision("fp16", loss_scale=fp16)
    return net


def _make(name, fp16=None, lr=None, **kw):
    from ctunet_amd import optim
    net = _net(fp16)
    return net, getattr(optim, name)(net.parameters(), lr=NET_LR[name] if lr is None else lr, **kw).guard(net)


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


def _assert_same(net_a, opt_a, net_b, opt_b, name):
    torch.cuda.synchronize()
    for (n, a), (_, b) in zip(net_a.state_dict().items(), net_b.state_dict().items()):
        assert torch.equal(a, b), n
    for (n, a), (_, b) in zip(net_a.named_parameters(), net_b.named_parameters()):
        for k in STATE[name]:
            sa, sb = _state(opt_a, a, k), _state(opt_b, b, k)
            assert (sa is None) == (sb is None) and (sa is None or torch.equal(sa, sb)), (n, k)
    assert torch.equal(opt_a.param_groups[0]["step_t"], opt_b.param_groups[0]["step_t"])


def _differs(net_a, net_b):
    return any(not torch.equal(a, b) for a, b in zip(net_a.parameters(), net_b.parameters()))


# ------------------------------------------------------------------ 5. HIP graph
@pytest.mark.parametrize("name", ["SGD", "RMSprop"])
def test_graph_replay_with_device_lr_and_clipping_is_bit_equal_to_eager(name, sample):
    from ctunet_amd.graph import GraphedTrainStep
    x, t = sample
    net_e, opt_e = _make(name, **CONTROLS)
    norms_e = []
    for _ in range(3 + 3):
        _eager(net_e, opt_e, x, t)
        norms_e.append(float(opt_e.last_grad_norm))
    net_g, opt_g = _make(name, **CONTROLS)
    gs = GraphedTrainStep(net_g, opt_g, x, [t], 1.0, 1.0, warmup=3)
    norms_g = []
    for _ in range(3):
        gs(x, [t])
        norms_g.append(float(opt_g.last_grad_norm))
    _assert_same(net_e, opt_e, net_g, opt_g, name)
    assert norms_g == norms_e[3:] and all(math.isfinite(v) and v > 0 for v in norms_g)
    assert len(set(norms_g)) == 3                                        # not frozen at capture time
    assert float(opt_g.param_groups[0]["step_t"]) == 6.0
    assert _differs(net_g, _net())                                       # and it trained


@pytest.mark.parametrize("name", ["SGD", "RMSprop"])
def test_a_host_edit_of_the_learning_rate_reaches_the_replayed_graph(name, sample):
    from ctunet_amd.graph import GraphedTrainStep
    x, t = sample

    def graphed(change):
        net, opt = _make(name, **CONTROLS)
        gs = GraphedTrainStep(net, opt, x, [t], 1.0, 1.0, warmup=3)
        for i in range(4):
            if change and i == 2:
                opt.param_groups[0]["lr"] *= 0.1
            gs(x, [t])
        torch.cuda.synchronize()
        return net, opt
    net_e, opt_e = _make(name, **CONTROLS)
    for i in range(3 + 4):
        if i == 3 + 2:
            opt_e.param_groups[0]["lr"] *= 0.1
        _eager(net_e, opt_e, x, t)
    net_g, opt_g = graphed(True)
    assert opt_g.get_lr() == [NET_LR[name] * 0.1] == opt_e.get_lr()
    _assert_same(net_e, opt_e, net_g, opt_g, name)
    assert _differs(graphed(False)[0], net_g)


@pytest.mark.parametrize("name", ["SGD", "RMSprop"])
def test_plateau_schedule_reduces_the_device_rate_inside_the_replayed_step(name, sample):
    """An improvement of 10 never happens (the loss is O(1)): with patience 0 every step after the first halves the rate, on
    the device, inside the replay -- and exactly as the eager loop with the same scheduler does."""
    from ctunet_amd.graph import GraphedTrainStep
    from ctunet_amd.lr_scheduler import ReduceLROnPlateau
    x, t = sample
    plateau = dict(patience=0, threshold=10.0, threshold_mode="abs", factor=0.5)
    net_e, opt_e = _make(name, **CONTROLS)
    sch_e = ReduceLROnPlateau(opt_e, **plateau)
    for _ in range(3 + 3):
        _eager(net_e, opt_e, x, t, sch_e)
    net_g, opt_g = _make(name, **CONTROLS)
    sch_g = ReduceLROnPlateau(opt_g, **plateau)
    gs = GraphedTrainStep(net_g, opt_g, x, [t], 1.0, 1.0, warmup=3, scheduler=sch_g)
    assert sch_g.last_epoch == 3 and sch_g.num_reductions == 2           # the warm-up steps
    lrs = []
    for _ in range(3):
        gs(x, [t])
        lrs.append(opt_g.get_lr()[0])
    assert sch_g.num_reductions == 5 and sch_g.last_epoch == 6
    assert lrs == [NET_LR[name] * 0.5 ** k for k in (3, 4, 5)]
    assert opt_e.get_lr() == opt_g.get_lr() and sch_e.state_dict() == sch_g.state_dict()
    _assert_same(net_e, opt_e, net_g, opt_g, name)


# ------------------------------------------------------------------ 6. float16
def test_fp16_dynamic_scale_skips_inside_the_graph(sample):
    import ctunet_amd
    from ctunet_amd.graph import GraphedTrainStep
    x, t = sample
    net, opt = _make("SGD", fp16=ctunet_amd.DynamicLossScale(init_scale=2.0 ** 40), momentum=0.9)
    start = [p.detach().clone() for p in net.parameters()]
    gs = GraphedTrainStep(net, opt, x, [t], 1.0, 1.0, warmup=3)          # constructs: the optimizer reads the device flag
    sc = net.loss_scaler
    assert opt.guarded_scaler() is sc and sc.skipped_steps() == 3        # every warm-up step overflowed at 2^40 .. 2^38
    sc.load_state_dict(dict(sc.state_dict(), scale=2.0 ** 40, skipped_steps=0))          # the replays start where it began
    gs(x, [t])
    torch.cuda.synchronize()
    assert sc.skipped_steps() == 1 and sc.get_scale() == 2.0 ** 39       # skipped, and the scale halved
    assert float(opt.param_groups[0]["step_t"]) == 0.0
    for p, s in zip(net.parameters(), start):
        assert torch.equal(p.detach(), s)
    sc.scale.fill_(2.0 ** 8)
    gs(x, [t])
    gs(x, [t])
    torch.cuda.synchronize()
    assert sc.skipped_steps() == 1 and float(opt.param_groups[0]["step_t"]) == 2.0
    assert any(not torch.equal(p.detach(), s) for p, s in zip(net.parameters(), start))
    assert all(torch.isfinite(p).all() for p in net.parameters())
    assert all(torch.isfinite(_state(opt, p, "momentum_buffer")).all() for p in net.parameters() if len(opt.state[p]))


@pytest.mark.parametrize("name", ["SGD", "RMSprop"])
def test_fp16_static_scale_overflow_is_skipped_by_the_guard(name, sample):
    """The gap torch.optim leaves with a static scale: it steps on inf / NaN gradients; the guarded fused class does not."""
    x, t = sample
    net, opt = _make(name, fp16=2.0 ** 40, momentum=0.9)
    assert opt.skip_flag is not None and opt.guarded_scaler() is None
    start = [p.detach().clone() for p in net.parameters()]
    _eager(net, opt, x, t)
    torch.cuda.synchronize()
    assert net.overflowed() and float(opt.param_groups[0]["step_t"]) == 0.0
    for p, s in zip(net.parameters(), start):
        assert torch.equal(p.detach(), s)
        assert all(_state(opt, p, k) is None or not _state(opt, p, k).any() for k in STATE[name])
    net.set_precision("fp16", loss_scale=None)                           # a sane scale: the same optimizer trains
    _eager(net, opt, x, t)
    torch.cuda.synchronize()
    assert not net.overflowed() and float(opt.param_groups[0]["step_t"]) == 1.0
    assert any(not torch.equal(p.detach(), s) for p, s in zip(net.parameters(), start))
    assert all(torch.isfinite(p).all() for p in net.parameters())


# ------------------------------------------------------------------ 7. StepRunner
def test_step_runner_trains_with_the_fused_sgd():
    from ctunet_amd import lr_scheduler, optim
    from ctunet_amd.datasets import SyntheticFlapDataset
    from ctunet_amd.trainer import StepRunner
    torch.manual_seed(0)
    run = StepRunner(dict(model_class="UNet", problem_handler="FlapRec", learning_rate=1e-2, optimizer="sgd", momentum=0.9,
                          fused_optimizer=True, device_lr=True, scheduler=None, ce_lambda=1.0, dice_lambda=1.0, device="cuda"))
    opt, net = run.params["optimizer"], run.models["main"]
    assert type(opt) is optim.SGD and opt.device_lr and isinstance(run.params["scheduler"], lr_scheduler.ReduceLROnPlateau)
    loader = torch.utils.data.DataLoader(SyntheticFlapDataset(1, size=32, seed=3, double_out=False, append_atlas=False),
                                         batch_size=1)
    before = [p.detach().clone() for p in net.parameters()]
    run.forward_pass("train", loader)
    torch.cuda.synchronize()
    moved = sum(not torch.equal(p.detach(), b) for p, b in zip(net.parameters(), before))
    assert 0 < moved <= sum(len(opt.state[p]) > 0 for p in net.parameters())          # only what has a gradient
    assert all(torch.isfinite(p).all() for p in net.parameters())
    assert float(opt.param_groups[0]["step_t"]) == 1.0 and run.params["scheduler"].last_epoch == 1
    assert opt.get_lr() == [1e-2]


# ------------------------------------------------------------------ 8. trajectory
def test_fused_sgd_training_trajectory_matches_torch_sgd(sample):
    """Five eager steps; the tolerance of test_models_gpu.py::test_fused_adam_training_trajectory_matches_torch_adam.  (The
    fused step writes through raw pointers: a missing version bump would leave the engine convolving with stale weights.)"""
    from ctunet_amd import losses as L, optim
    x, t = sample

    def run(fused):
        net = _net()
        opt = optim.SGD(net.parameters(), lr=1e-2, momentum=0.9) if fused else \
            torch.optim.SGD(net.parameters(), lr=1e-2, momentum=0.9)
        out = []
        for _ in range(5):
            ce, dc = L.fused_ce_dice(net(x), t, 1.0, 1.0, False)
            (ce + dc).backward()
            opt.step()
            for p in net.parameters():
                p.grad = None
            out.append((ce + dc).item())
        return out
    a, b = run(True), run(False)
    print("fused", a, "torch", b)
    assert a[0] == b[0] and b[4] != b[0]
    assert all(abs(u - v) < 2e-5 for u, v in zip(a, b)), (a, b)


# ------------------------------------------------------------------ 9. checkpoint
def test_rmsprop_checkpoint_round_trip_continues_bit_equal(sample, tmp_path):
    from ctunet_amd import checkpoint
    x, t = sample
    kw = dict(momentum=0.9, centered=True, device_lr=True, max_grad_norm=1.0)
    net_w, opt_w = _make("RMSprop", **kw)
    for _ in range(2):
        _eager(net_w, opt_w, x, t)
    opt_w.param_groups[0]["lr_t"].mul_(0.5)                              # a device-side reduction the host float has not seen
    model_sd = copy.deepcopy(net_w.state_dict())
    checkpoint.save_train_state(opt_w, str(tmp_path / "train.pt"))
    on_gpu = {"optimizer": copy.deepcopy(opt_w.state_dict()), "scheduler": None}
    _eager(net_w, opt_w, x, t)                                           # the uninterrupted run
    for source in (str(tmp_path / "train.pt"), on_gpu):                  # map_location="cpu", then GPU tensors
        net_r, opt_r = _make("RMSprop", **kw)
        net_r.load_state_dict(model_sd)
        checkpoint.load_train_state(opt_r, source)
        if isinstance(source, str):
            assert opt_r.param_groups[0]["step_t"].device.type == "cpu" and opt_r.param_groups[0]["lr_t"].device.type == "cpu"
        _eager(net_r, opt_r, x, t)
        group = opt_r.param_groups[0]
        assert group["step_t"].is_cuda and group["lr_t"].is_cuda and float(group["step_t"]) == 3.0
        assert all(opt_r.state[p]["step"] is group["step_t"] for p in net_r.parameters() if len(opt_r.state[p]))
        assert opt_r.get_lr() == [NET_LR["RMSprop"] * 0.5] == opt_w.get_lr()
        _assert_same(net_w, opt_w, net_r, opt_r, "RMSprop")
