"""Fused SGD / RMSprop, the host side (no GPU): the restated rules against torch.optim on the CPU, the two C ABI entry
points and their argument validation, constructor errors, state-dict interchange with torch, and StepRunner's
``fused_optimizer`` key."""
import copy
import ctypes as C
import os
import re

import pytest
import torch

import optim_ref as R

SHAPES = [(4, 3), (7,), (1,)]
# float64: rtol as the issue sets it; the absolute term is a few ulps of the O(1) values, for entries that cancel to ~0
F64_TOL = dict(rtol=1e-12, atol=1e-15)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=g, dtype=dtype) for s in SHAPES]
    grads = [[torch.randn(s, generator=g, dtype=dtype) for s in SHAPES] for _ in range(5)]
    return params, grads


def _against_torch(rule, cls, lr, kw, dtype, tol):
    params, grads = _data(dtype)
    twins = [p.clone().requires_grad_(True) for p in params]
    ref = cls(twins, lr=lr, **kw)
    mine = R.Runner(rule, params, lr, **kw)
    for gs in grads:
        for t, g in zip(twins, gs):
            t.grad = g.clone()
        ref.step()
        mine.step(gs)
    names = ("momentum_buffer",) if rule == "sgd" else ("square_avg", "momentum_buffer", "grad_avg")
    for i, (p, t) in enumerate(zip(params, twins)):
        assert torch.allclose(p, t.detach(), **tol), (i, (p - t.detach()).abs().max())
        for k in names:
            want = ref.state[t].get(k)
            if mine.state[i][k] is None:
                assert not torch.is_tensor(want), k                     # torch keeps no such tensor either
            else:
                assert torch.allclose(mine.state[i][k], want, **tol), (i, k)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, dict(rtol=1e-5, atol=1e-6)), (torch.float64, F64_TOL)],
                         ids=["f32", "f64"])
@pytest.mark.parametrize("kw", R.SGD_GRID, ids=R.grid_id)
def test_restated_sgd_rule_equals_torch(kw, dtype, tol):
    _against_torch("sgd", torch.optim.SGD, 0.05, kw, dtype, tol)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, dict(rtol=1e-5, atol=1e-6)), (torch.float64, F64_TOL)],
                         ids=["f32", "f64"])
@pytest.mark.parametrize("kw", R.RMS_GRID, ids=R.grid_id)
def test_restated_rmsprop_rule_equals_torch(kw, dtype, tol):
    _against_torch("rmsprop", torch.optim.RMSprop, 0.01, kw, dtype, tol)


def test_the_grids_cover_every_option():
    assert len(R.SGD_GRID) == 20 and len(R.RMS_GRID) == 16
    for key, vals in dict(momentum={0.0, 0.9}, dampening={0.0, 0.3}, nesterov={False, True}, weight_decay={0.0, 0.01},
                          maximize={False, True}).items():
        assert {kw[key] for kw in R.SGD_GRID} == vals
    for key, vals in dict(momentum={0.0, 0.9}, centered={False, True}, weight_decay={0.0, 0.01},
                          maximize={False, True}).items():
        assert {kw[key] for kw in R.RMS_GRID} == vals


def test_skip_and_first_step_semantics_of_the_restatement():
    """A skipped first step leaves the next one to be the first (buf = g, whatever the dampening)."""
    p, g = torch.ones(3), torch.full((3,), 2.0)
    run = R.Runner("sgd", [p], 0.1, momentum=0.9, dampening=0.3)
    run.step([g], skip=True)
    assert run.steps == 0 and run.state == [None] and torch.equal(p, torch.ones(3))
    run.step([g])
    assert run.steps == 1 and torch.equal(run.state[0]["momentum_buffer"], g) and torch.allclose(p, torch.full((3,), 0.8))
    run.step([None])
    assert run.steps == 2 and torch.equal(run.state[0]["momentum_buffer"], g)


# ------------------------------------------------------------------ the C ABI
def test_new_entry_points_and_unchanged_abi_version():
    from ctunet_amd import _lib
    P, I, D = _lib.P, _lib.I, _lib.D
    lib = _lib.load()
    assert lib.ctu_abi_version() == _lib.ABI_VERSION == 8
    want = {"ctu_sgd": (I, [P, P, I, P, P, D, D, D, D, I, I, P, P, P]),
            "ctu_rmsprop": (I, [P, P, I, P, P, D, D, D, D, D, I, I, P, P, P])}
    header = open(os.path.join(ROOT, "include", "ctunet_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        assert getattr(lib, name).argtypes == sig[1] and hasattr(raw, name)
        m = re.search(r"\bint\s+%s\(([^;]*)\);" % name, header)
        assert m is not None, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(sig[1]), name
        for a, ct in zip(args, sig[1]):                                # pointer / double / int, argument by argument
            kind = P if "*" in a else D if a.startswith("double") else I if a.startswith("int ") else None
            assert kind is ct, (name, a)


def _fake(k, *null):
    return (C.c_void_p * k)(*[None if i in null else 64 for i in range(k)])        # non-null, never dereferenced on the host


def _sgd(lib, ptrs, sizes, n, step=64, mu=0.9, damp=0.0, nesterov=0):
    return lib.ctu_sgd(ptrs, sizes, n, step, None, 0.1, mu, damp, 0.0, nesterov, 0, None, None, None)


def _rms(lib, ptrs, sizes, n, step=64, mu=0.9, centered=1):
    return lib.ctu_rmsprop(ptrs, sizes, n, step, None, 0.01, 0.99, 1e-8, 0.0, mu, centered, 0, None, None, None)


def test_bad_arguments_are_refused_without_a_launch():
    """Every validation case answers on the host (this test runs without a GPU, so nothing can launch)."""
    from ctunet_amd import _lib
    lib = _lib.load()
    one, neg = (C.c_int64 * 1)(4), (C.c_int64 * 1)(-1)
    for call, k, name in ((_sgd, 3, b"sgd"), (_rms, 5, b"rmsprop")):
        assert call(lib, None, one, 1) != 0 and name in lib.ctu_last_error()          # null ptrs
        assert call(lib, _fake(k), None, 1) != 0                                       # null sizes
        assert call(lib, _fake(k), one, 1, step=None) != 0                             # null step
        assert call(lib, _fake(k), one, 0) != 0 and call(lib, _fake(k), one, -3) != 0  # n <= 0
        assert call(lib, _fake(k), neg, 1) != 0 and name in lib.ctu_last_error()       # a negative size
        assert call(lib, _fake(k, 0), one, 1) != 0                                     # null p
        assert call(lib, _fake(k, 1), one, 1) != 0                                     # null g
    assert _sgd(lib, _fake(3, 2), one, 1, mu=0.9) != 0                                 # null buf although mu != 0
    assert _sgd(lib, _fake(3), one, 1, mu=0.0, nesterov=1) != 0                        # nesterov without momentum
    assert _sgd(lib, _fake(3), one, 1, mu=0.9, damp=0.3, nesterov=1) != 0              # nesterov with dampening
    assert b"Nesterov" in lib.ctu_last_error()
    assert _rms(lib, _fake(5, 2), one, 1) != 0                                         # null sq
    assert _rms(lib, _fake(5, 3), one, 1, mu=0.9) != 0                                 # null buf although mu != 0
    assert _rms(lib, _fake(5, 4), one, 1, centered=1) != 0                             # null ga although centered
    # the second tensor of a list is checked like the first
    two = (C.c_int64 * 2)(4, 4)
    assert _sgd(lib, (C.c_void_p * 6)(64, 64, 64, 64, None, 64), two, 2) != 0
    assert _rms(lib, (C.c_void_p * 10)(64, 64, 64, 64, 64, 64, 64, None, 64, 64), two, 2) != 0


# ------------------------------------------------------------------ the host classes
def _p(n=1):
    return [torch.zeros(3, requires_grad=True) for _ in range(n)]


def test_constructor_errors_are_torchs():
    from ctunet_amd import optim
    for cls, ref in ((optim.SGD, torch.optim.SGD), (optim.RMSprop, torch.optim.RMSprop)):
        for bad in (dict(lr=-1.0), dict(momentum=-0.5), dict(weight_decay=-0.1)):
            with pytest.raises(ValueError):
                ref(_p(), **bad)
            with pytest.raises(ValueError):
                cls(_p(), **bad)
        for bad in (0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="max_grad_norm"):
                cls(_p(), max_grad_norm=bad)
    for bad in (dict(eps=-1e-8), dict(alpha=-0.1)):
        with pytest.raises(ValueError):
            torch.optim.RMSprop(_p(), **bad)
        with pytest.raises(ValueError):
            optim.RMSprop(_p(), **bad)
    for bad in (dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
            torch.optim.SGD(_p(), lr=0.1, **bad)
        with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
            optim.SGD(_p(), **bad)
    optim.SGD(_p(), nesterov=True, momentum=0.9)


def test_defaults_and_control_attributes():
    from ctunet_amd import optim
    sgd, rms = optim.SGD(_p()), optim.RMSprop(_p())
    for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize"):
        assert sgd.defaults[k] == torch.optim.SGD(_p()).defaults[k], k
    for k in ("lr", "alpha", "eps", "weight_decay", "momentum", "centered", "maximize"):
        assert rms.defaults[k] == torch.optim.RMSprop(_p()).defaults[k], k
    for cls in (optim.SGD, optim.RMSprop):
        o = cls(_p())
        assert o.device_lr is False and o.max_grad_norm is None and o.skip_flag is None and o.guarded_scaler() is None
        assert o.last_grad_norm is None and o.get_lr() == [cls(_p()).defaults["lr"]]
        assert cls(_p(), max_grad_norm=2).device_lr is True             # clipping implies the device learning rate
        assert cls(_p(), device_lr=True, max_grad_norm=0.5).max_grad_norm == 0.5
        o.sync_lr()                                                      # nothing to do on the host
        assert isinstance(o, torch.optim.Optimizer) and isinstance(optim.Adam(_p()), type(o).__mro__[1])   # one base
        with pytest.raises(RuntimeError, match="float32 on the GPU"):
            p = _p()
            p[0].grad = torch.ones(3)
            cls(p).step()
    assert optim.SGD(_p(), maximize=True).defaults["maximize"] is True
    with pytest.raises(TypeError):
        optim.SGD(_p(), 0.1, 0.9, 0, 0, False, True)                     # maximize and the controls are keyword-only


def _stepped_torch(cls, **kw):
    ps = _p(2)
    opt = cls(ps, **kw)
    for it in range(2):
        for i, p in enumerate(ps):
            p.grad = torch.full((3,), 0.5 + i + it)
        opt.step()
    return ps, opt


@pytest.mark.parametrize("name,kw,keys", [
    ("SGD", dict(lr=0.1, momentum=0.9), {"momentum_buffer"}),
    ("RMSprop", dict(lr=0.01, momentum=0.9, centered=True), {"square_avg", "momentum_buffer", "grad_avg", "step"}),
])
def test_state_dict_round_trip_with_torch(name, kw, keys):
    """torch -> fused -> torch on CPU tensors: torch's state names, and a torch optimizer that continues from the fused
    class's state dict exactly as the original does."""
    from ctunet_amd import optim
    tcls, fcls = getattr(torch.optim, name), getattr(optim, name)
    ps, ref = _stepped_torch(tcls, **kw)
    tsd = ref.state_dict()
    assert all(set(s) == keys for s in tsd["state"].values())
    fused = fcls(_p(2), **kw)
    fused.load_state_dict(copy.deepcopy(tsd))                            # (load_state_dict keeps CPU tensors by reference)
    fsd = fused.state_dict()
    assert all(set(s) == keys for s in fsd["state"].values()) and len(fsd["state"]) == 2
    for i in tsd["state"]:
        for k in keys:
            assert torch.equal(torch.as_tensor(fsd["state"][i][k]), torch.as_tensor(tsd["state"][i][k])), (i, k)
    for k in kw:
        assert fsd["param_groups"][0][k] == kw[k]
    twins = [p.detach().clone().requires_grad_(True) for p in ps]
    back = tcls(twins, **kw)
    back.load_state_dict(copy.deepcopy(fsd))
    for p, t in zip(ps, twins):
        p.grad, t.grad = torch.full((3,), -0.25), torch.full((3,), -0.25)
    ref.step()
    back.step()
    for p, t in zip(ps, twins):
        assert torch.equal(p.detach(), t.detach())


def test_sgd_without_momentum_keeps_no_state_names():
    from ctunet_amd import optim
    _, ref = _stepped_torch(torch.optim.SGD, lr=0.1)
    fused = optim.SGD(_p(2), lr=0.1)
    fused.load_state_dict(ref.state_dict())
    assert all("momentum_buffer" not in s or s["momentum_buffer"] is None for s in fused.state_dict()["state"].values())


def test_a_loaded_torch_state_is_not_taken_for_a_first_step():
    """The device counter a group starts from when the state dict came from torch.optim, which keeps none for SGD and one
    per tensor for RMSprop."""
    from ctunet_amd import optim
    _, ref = _stepped_torch(torch.optim.SGD, lr=0.1, momentum=0.9)
    fused = optim.SGD(_p(2), lr=0.1, momentum=0.9)
    assert fused._first_count(fused.param_groups[0]["params"]) == 0.0
    fused.load_state_dict(ref.state_dict())
    assert fused._first_count(fused.param_groups[0]["params"]) == 1.0
    _, ref = _stepped_torch(torch.optim.RMSprop, lr=0.1)
    fused = optim.RMSprop(_p(2), lr=0.1)
    assert fused._first_count(fused.param_groups[0]["params"]) == 0.0
    fused.load_state_dict(ref.state_dict())
    assert fused._first_count(fused.param_groups[0]["params"]) == 2.0


# ------------------------------------------------------------------ StepRunner
BASE = dict(model_class="UNet", problem_handler="FlapRec", learning_rate=1e-2, ce_lambda=1.0, dice_lambda=1.0, device="cpu",
            momentum=0.9, weight_decay=0.01)


@pytest.mark.parametrize("name,cls", [("sgd", "SGD"), ("rmsprop", "RMSprop")])
def test_step_runner_fused_optimizer_key(name, cls):
    from ctunet_amd import lr_scheduler, optim
    from ctunet_amd.trainer import StepRunner
    fused_cls, torch_cls = getattr(optim, cls), getattr(torch.optim, cls)
    opt = StepRunner(dict(BASE, optimizer=name, fused_optimizer=True)).params["optimizer"]
    assert type(opt) is fused_cls and opt.device_lr is False and opt.max_grad_norm is None
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"]) == (1e-2, 0.9, 0.01)
    run = StepRunner(dict(BASE, optimizer=name, fused_optimizer=True, device_lr=True, max_grad_norm=3.0, scheduler=None))
    opt = run.params["optimizer"]
    assert type(opt) is fused_cls and opt.device_lr is True and opt.max_grad_norm == 3.0
    assert isinstance(run.params["scheduler"], lr_scheduler.ReduceLROnPlateau)
    # without the key: today's objects and today's error
    run = StepRunner(dict(BASE, optimizer=name, scheduler=None))
    assert type(run.params["optimizer"]) is torch_cls
    assert isinstance(run.params["scheduler"], torch.optim.lr_scheduler.ReduceLROnPlateau)
    assert type(StepRunner(dict(BASE, optimizer=name, fused_optimizer=False)).params["optimizer"]) is torch_cls
    with pytest.raises(ValueError, match="device_lr"):
        StepRunner(dict(BASE, optimizer=name, device_lr=True))
    with pytest.raises(ValueError, match="device_lr"):
        StepRunner(dict(BASE, optimizer=name, device_lr=True, fused_optimizer=False))


def test_step_runner_adam_ignores_the_key():
    from ctunet_amd import optim
    from ctunet_amd.trainer import StepRunner
    for name, cls in (("adam", optim.Adam), ("adamw", optim.AdamW)):
        for key in (True, False):
            assert type(StepRunner(dict(BASE, optimizer=name, fused_optimizer=key)).params["optimizer"]) is cls


def test_graphed_step_error_names_the_new_classes():
    import inspect
    from ctunet_amd import graph
    src = inspect.getsource(graph.GraphedTrainStep.__init__)
    assert "dynamic loss scaling" in src and "SGD" in src and "RMSprop" in src
