"""Dynamic loss scaling on the MI355X: the update kernel against torch._amp_update_scale_, and the device-resident scale
in real float16 steps -- back-off, growth, HIP-graph replay (single graph and the segmented distributed chain), gradient
accumulation, an engine rebuild, torch.optim through StepRunner, checkpoints.  Small nets and volumes (UNet(n_blocks=2),
32^3), like test_lowp_gpu.py's static overflow test."""
import pytest
import torch

from util import gen, onehot_target

pytestmark = pytest.mark.gpu

NO_GROWTH = 10 ** 6


def _data():
    x = torch.randn(1, 1, 32, 32, 32, generator=gen(2)).cuda()
    t = onehot_target((1, 2, 32, 32, 32), 3, 0.3).cuda()
    return x, t


def _make(loss_scale, sd=None, use_checkpoint=False):
    import ctunet_amd
    from ctunet_amd import optim
    torch.manual_seed(0)
    net = ctunet_amd.UNet(n_blocks=2, use_checkpoint=use_checkpoint).cuda().train()
    if sd is not None:
        net.load_state_dict(sd)
    net.set_precision(torch.float16, loss_scale=loss_scale)
    return net, optim.Adam(net.parameters(), lr=1e-3, amsgrad=True).guard(net)


def _backward(net, x, t):
    from ctunet_amd import losses as L
    ce, dc = L.fused_ce_dice(net(x.clone().requires_grad_(True)), t, 1.0, 1.0, False)
    (ce + dc).backward()


def _step(net, opt, x, t):
    _backward(net, x, t)
    opt.step()
    for p in net.parameters():
        p.grad = None


def _params(net):
    return [p.detach().clone() for p in net.parameters()]


def _dyn(init_scale, interval=NO_GROWTH):
    import ctunet_amd
    return ctunet_amd.DynamicLossScale(init_scale=init_scale, growth_interval=interval)


@pytest.mark.parametrize("init,growth,backoff,interval,found", [
    (2.0 ** 10, 2.0, 0.5, 1, [0, 0, 1, 0, 1, 1, 0, 0.5, 0]),
    (2.0 ** 10, 2.0, 0.5, 3, [0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0]),
    (2.0 ** 126, 2.0, 0.5, 1, [0, 0, 0, 1, 0, 0]),               # 2^127 must not grow to inf
    (3.0, 3.0, 0.25, 2, [0, 0, 0, 0, 1, 0, 0, 1, 0]),
])
def test_update_kernel_matches_torch(init, growth, backoff, interval, found):
    import ctunet_amd
    from ctunet_amd.loss_scale import LossScaler
    sc = LossScaler(ctunet_amd.DynamicLossScale(init, growth, backoff, interval), "cuda")
    ref_s = torch.full((1,), init, dtype=torch.float32)
    ref_t = torch.zeros(1, dtype=torch.int32)
    skipped = 0
    for f in found:
        sc.found_inf.fill_(f)
        sc.update()
        torch._amp_update_scale_(ref_s, ref_t, torch.full((1,), float(f)), growth, backoff, interval)
        skipped += f != 0
        torch.cuda.synchronize()
        assert torch.equal(sc.scale.cpu(), ref_s) and torch.equal(sc.growth_tracker.cpu(), ref_t), (f, sc.scale, ref_s)
        assert float(sc.found_inf) == 0.0 and sc.skipped_steps() == skipped
        assert torch.isfinite(sc.scale).all()


def test_overflowed_steps_back_off_and_the_first_finite_step_matches_static():
    x, t = _data()
    sd0 = _make(None)[0].state_dict()
    sd0 = {k: v.clone() for k, v in sd0.items()}
    net, opt = _make(_dyn(2.0 ** 40), sd0)
    sc = net.loss_scaler
    finite_scale = None
    for i in range(40):
        before, scale = _params(net), sc.get_scale()
        _step(net, opt, x, t)
        if sc.skipped_steps() == i + 1:                             # skipped: nothing moved, the scale halved
            assert sc.get_scale() == scale / 2
            for p, b in zip(net.parameters(), before):
                assert torch.equal(p.detach(), b)
            for st in opt.state.values():
                assert float(st["step"]) == 0.0 and float(st["exp_avg"].abs().max()) == 0.0
                assert float(st["max_exp_avg_sq"].abs().max()) == 0.0
        else:
            finite_scale = scale
            break
    assert finite_scale is not None and sc.skipped_steps() >= 1
    assert float(opt.param_groups[0]["step_t"]) == 1.0
    # a twin with the static scale the dynamic one had reached: bit-equal parameters after its one step
    twin, opt_t = _make(finite_scale, sd0)
    _step(twin, opt_t, x, t)
    torch.cuda.synchronize()
    assert not twin.overflowed()
    for (n, a), b in zip(net.named_parameters(), twin.parameters()):
        assert torch.equal(a.detach(), b.detach()), n


def test_clean_steps_grow_the_scale():
    x, t = _data()
    net, opt = _make(_dyn(2.0 ** 8, 2))
    for _ in range(4):
        _step(net, opt, x, t)
    sc = net.loss_scaler
    assert sc.get_scale() == 2.0 ** 10 and sc.skipped_steps() == 0 and int(sc.growth_tracker) == 0


def _trajectories(distributed, k):
    """Eager twin vs GraphedTrainStep from 2^40 on the same inputs: per-step scales, skip counts, the models."""
    from ctunet_amd.graph import GraphedTrainStep
    x, t = _data()
    cfg = _dyn(2.0 ** 40, 4)                                   # backs off, then grows (and may back off again)
    net_e, opt_e = _make(cfg, use_checkpoint=distributed)
    scales_e = []
    for _ in range(3 + k):
        _step(net_e, opt_e, x, t)
        scales_e.append(net_e.loss_scaler.get_scale())
    net_g, opt_g = _make(cfg, use_checkpoint=distributed)
    gs = GraphedTrainStep(net_g, opt_g, x, [t], 1.0, 1.0, warmup=3, distributed=distributed)
    sc = net_g.loss_scaler
    at_capture = sc.get_scale()
    scales_g = []
    for _ in range(k):
        gs(x, [t])
        scales_g.append(sc.get_scale())
    torch.cuda.synchronize()
    assert at_capture == scales_e[2]
    assert scales_g == scales_e[3:], (scales_g, scales_e)
    assert sc.skipped_steps() == net_e.loss_scaler.skipped_steps()
    assert scales_g[-1] != at_capture                          # the scale is not frozen into the graph
    assert 0 < sc.skipped_steps() < 3 + k                      # some steps were skipped, some applied
    return net_e, net_g


def test_graph_replay_adapts_the_scale():
    net_e, net_g = _trajectories(False, 24)
    for (n, a), (_, b) in zip(net_e.state_dict().items(), net_g.state_dict().items()):
        assert torch.allclose(a.float(), b.float(), rtol=1e-4, atol=1e-6), n


def test_one_rank_distributed_graph_follows_eager():
    import torch.distributed as dist
    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29557", rank=0, world_size=1,
                                device_id=torch.device("cuda", 0))
    try:
        net_e, net_g = _trajectories(True, 24)
        for (n, a), (_, b) in zip(net_e.state_dict().items(), net_g.state_dict().items()):
            assert torch.allclose(a.float(), b.float(), rtol=2e-3, atol=1e-5), n
    finally:
        from ctunet_amd import parallel
        parallel.close_communicators()
        dist.destroy_process_group()


def test_two_backward_passes_accumulate_the_overflow():
    x, t = _data()
    net, opt = _make(_dyn(2.0 ** 40))
    sc = net.loss_scaler
    before = _params(net)
    _backward(net, x, t)                                       # overflows
    assert float(sc.found_inf) != 0.0
    sc.scale.fill_(2.0 ** 8)                                   # the second pass alone is finite ...
    _backward(net, x, t)
    assert float(sc.found_inf) != 0.0                          # ... and does not erase the first pass's overflow
    opt.step()
    torch.cuda.synchronize()
    for p, b in zip(net.parameters(), before):
        assert torch.equal(p.detach(), b)
    assert sc.get_scale() == 2.0 ** 7 and sc.skipped_steps() == 1 and float(sc.found_inf) == 0.0


def test_the_guard_and_the_state_survive_an_engine_rebuild():
    x, t = _data()
    net, opt = _make(_dyn(2.0 ** 10))
    sc = net.loss_scaler
    _step(net, opt, x, t)
    _step(net, opt, x, t)
    assert sc.skipped_steps() == 0 and int(sc.growth_tracker) == 2
    net.set_precision("bf16")
    assert net.loss_scaler is None
    _step(net, opt, x, t)                                      # a bf16 step leaves the scaler alone
    net.set_precision("fp16", loss_scale="dynamic")
    assert net.loss_scaler is sc and sc.get_scale() == 2.0 ** 10 and int(sc.growth_tracker) == 2
    sc.scale.fill_(2.0 ** 40)                                  # force an overflow
    before = _params(net)
    _step(net, opt, x, t)
    torch.cuda.synchronize()
    for p, b in zip(net.parameters(), before):
        assert torch.equal(p.detach(), b)
    assert sc.skipped_steps() == 1 and sc.get_scale() == 2.0 ** 39


def test_step_runner_with_sgd_skips_overflowed_steps():
    from ctunet_amd.datasets import SyntheticFlapDataset
    from ctunet_amd.trainer import StepRunner
    run = StepRunner(dict(model_class="UNet", problem_handler="FlapRec", learning_rate=1e-2, optimizer="sgd", momentum=0,
                          weight_decay=0.0, ce_lambda=1.0, dice_lambda=1.0, device="cuda"))
    net = run.models["main"]
    net.set_precision("fp16", loss_scale=_dyn(2.0 ** 40))
    sc = net.loss_scaler
    loader = torch.utils.data.DataLoader(SyntheticFlapDataset(1, size=32, seed=3, double_out=False, append_atlas=False),
                                         batch_size=1)
    before = _params(net)
    run.forward_pass("train", loader)
    torch.cuda.synchronize()
    assert sc.skipped_steps() == 1 and sc.get_scale() == 2.0 ** 39
    for p, b in zip(net.parameters(), before):
        assert torch.equal(p.detach(), b)
    for i in range(40):
        run.forward_pass("train", loader)
        if sc.skipped_steps() < i + 2:
            break
    run.forward_pass("train", loader)
    torch.cuda.synchronize()
    assert sc.get_scale() < 2.0 ** 39
    assert any(not torch.equal(p.detach(), b) for p, b in zip(net.parameters(), before))
    assert all(torch.isfinite(p).all() for p in net.parameters())


def test_state_dict_round_trip_and_grad_scaler_compatibility():
    x, t = _data()
    net, opt = _make(_dyn(2.0 ** 10, 5))
    for _ in range(3):
        _step(net, opt, x, t)
    sd = net.loss_scaler.state_dict()
    assert set(torch.amp.GradScaler("cuda").state_dict()) <= set(sd)
    assert sd["scale"] == 2.0 ** 10 and sd["_growth_tracker"] == 3
    other, _ = _make("dynamic")
    other.loss_scaler.load_state_dict(sd)
    assert torch.equal(other.loss_scaler.scale, net.loss_scaler.scale)
    assert torch.equal(other.loss_scaler.growth_tracker, net.loss_scaler.growth_tracker)
    assert other.loss_scaler.growth_interval == 5
    gsd = torch.amp.GradScaler("cuda", init_scale=4096.0, growth_factor=4.0, backoff_factor=0.25, growth_interval=7).state_dict()
    third, _ = _make("dynamic")
    third.loss_scaler.load_state_dict(gsd)
    s = third.loss_scaler
    assert s.get_scale() == 4096.0 and int(s.growth_tracker) == 0
    assert (s.growth_factor, s.backoff_factor, s.growth_interval) == (4.0, 0.25, 7)
