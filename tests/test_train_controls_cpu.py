"""Device learning rate, plateau schedule and gradient clipping, the host side (no GPU): the restated plateau rule against
torch's scheduler bit for bit, state-dict interchange with torch, the new C ABI entry points and argument validation."""
import ctypes as C
import re
import os

import pytest
import torch

import train_controls_ref as R


def _torch_sched(lr, **kw):
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=lr)
    return torch.optim.lr_scheduler.ReduceLROnPlateau(opt, **kw)


@pytest.mark.parametrize("mode,tmode", R.MODES)
@pytest.mark.parametrize("patience,cooldown,min_lr,eps", R.CONFIGS)
@pytest.mark.parametrize("seq", list(R.SEQUENCES))
def test_restated_plateau_rule_equals_torch_bit_for_bit(mode, tmode, patience, cooldown, min_lr, eps, seq):
    kw = dict(mode=mode, factor=0.5, patience=patience, threshold=1e-2, threshold_mode=tmode, cooldown=cooldown,
              min_lr=min_lr, eps=eps)
    metrics = R.metric32(R.SEQUENCES[seq])
    if mode == "max":
        metrics = [-m for m in metrics]                 # so that "improving" improves in max mode too
    ref, mine = _torch_sched(0.1, **kw), R.PlateauRef(0.1, **kw)
    for i, m in enumerate(metrics):
        ref.step(m)
        mine.step(m)
        assert mine.snapshot() == R.torch_snapshot(ref), (i, m, mine.__dict__, ref.state_dict())


def test_the_configurations_reach_the_branches_they_are_meant_to():
    """min_lr binds, eps blocks, cooldown swallows bad epochs, patience delays -- on the worsening sequence."""
    def run(patience, cooldown, min_lr, eps):
        p = R.PlateauRef(0.1, factor=0.5, patience=patience, threshold=1e-2, cooldown=cooldown, min_lr=min_lr, eps=eps)
        for m in R.SEQUENCES["worsening"]:
            p.step(m)
        return p
    base = run(*R.CONFIGS[0])
    assert base.num_reductions == 11 and base.lr == 0.1 * 0.5 ** 11
    assert run(*R.CONFIGS[1]).num_reductions == 3                       # patience 2: every third bad step
    assert run(*R.CONFIGS[2]).num_reductions == 4                       # cooldown 2
    bound = run(*R.CONFIGS[4])
    assert bound.lr == 0.04 and bound.num_reductions == 2               # 0.1 -> 0.05 -> min_lr, then lr - new = 0
    assert run(*R.CONFIGS[5]).lr == 0.1                                 # 0.1 - 0.05 < eps: never applied


def _fused(device_lr=True, groups=1):
    from ctunet_amd import optim
    ps = [{"params": [torch.zeros(3, requires_grad=True)], "lr": 0.1 / (i + 1)} for i in range(groups)]
    return optim.Adam(ps, lr=0.1, device_lr=device_lr)


def test_scheduler_constructor_validation():
    from ctunet_amd.lr_scheduler import ReduceLROnPlateau
    with pytest.raises(ValueError):
        ReduceLROnPlateau(_fused(), factor=1.0)
    with pytest.raises(ValueError):
        ReduceLROnPlateau(_fused(), factor=1.5)
    with pytest.raises(ValueError):
        ReduceLROnPlateau(_fused(), mode="best")
    with pytest.raises(ValueError):
        ReduceLROnPlateau(_fused(), threshold_mode="ratio")
    with pytest.raises(ValueError):
        ReduceLROnPlateau(_fused(), min_lr=[0.0, 0.0])                   # one group
    with pytest.raises(ValueError):
        ReduceLROnPlateau(_fused(device_lr=False))
    with pytest.raises(ValueError):
        ReduceLROnPlateau(torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=0.1))
    with pytest.raises(TypeError):
        ReduceLROnPlateau(object())
    s = ReduceLROnPlateau(_fused(), patience=3)
    with pytest.raises(TypeError):
        s.step(0.5)                                                      # a host float: exactly what this class removes
    with pytest.raises(TypeError):
        s.step(torch.zeros(1))                                           # not on the GPU


def test_optimizer_arguments():
    from ctunet_amd import optim
    p = [torch.zeros(3, requires_grad=True)]
    assert optim.Adam(p).device_lr is False and optim.Adam(p).max_grad_norm is None
    assert optim.Adam(p, max_grad_norm=2).device_lr is True             # clipping implies the device entry point
    assert optim.AdamW(p, device_lr=True, max_grad_norm=0.5).max_grad_norm == 0.5
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            optim.Adam(p, max_grad_norm=bad)
    assert optim.Adam(p, lr=0.25).get_lr() == [0.25]


def test_state_dict_interchanges_with_torch():
    from ctunet_amd.lr_scheduler import ReduceLROnPlateau
    ref = _torch_sched(0.1, mode="max", factor=0.5, patience=1, threshold=1e-3, threshold_mode="abs", cooldown=2, min_lr=1e-3)
    for m in (0.5, 0.4, 0.3, 0.2):
        ref.step(m)
    tsd = ref.state_dict()
    mine = ReduceLROnPlateau(_fused())
    assert set(tsd) <= set(mine.state_dict())                            # torch's key names, all of them
    mine.load_state_dict(tsd)
    msd = mine.state_dict()
    for k in tsd:
        if k != "_last_lr":                                              # (the optimizers differ)
            assert msd[k] == tsd[k], k
    assert (mine.best, mine.num_bad_epochs, mine.cooldown_counter, mine.last_epoch) == \
        (ref.best, ref.num_bad_epochs, ref.cooldown_counter, ref.last_epoch)
    # the other direction: a fresh torch scheduler continues from this class's state exactly as the original does
    other = _torch_sched(0.1)
    other.load_state_dict(msd)
    other.optimizer.param_groups[0]["lr"] = ref.optimizer.param_groups[0]["lr"]
    for m in (0.1, 0.6, 0.1, 0.1, 0.1, 0.1):
        ref.step(m)
        other.step(m)
        assert R.torch_snapshot(other) == R.torch_snapshot(ref)
    with pytest.raises(ValueError):
        mine.load_state_dict(dict(tsd, factor=2.0))


def test_new_entry_points_and_unchanged_abi_version():
    from ctunet_amd import _lib
    P, I, F, D = _lib.P, _lib.I, _lib.F, _lib.D
    assert _lib.ABI_VERSION == 8
    lib = _lib.load()
    assert lib.ctu_abi_version() == 8
    want = {"ctu_adam_amsgrad_dev": (I, [P, P, I, P, P, D, D, D, D, I, P, P, P]),
            "ctu_grad_norm_num_blocks": (I, [P, I]),
            "ctu_grad_clip_coef": (I, [P, P, I, F, P, P, P, P]),
            "ctu_plateau_update": (I, [P, P, P, P, I, I, D, I, D, I, D, D, P])}
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
        assert getattr(lib, name).argtypes == sig[1]
    assert _lib.SIGNATURES["ctu_adam_amsgrad"] == (I, [P, P, I, P, D, D, D, D, D, I, P, P])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ctunet_hip.h")).read()
    for name, (_, args) in want.items():
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m is not None, name
        assert len(m.group(1).split(",")) == len(args), name


def test_bad_arguments_are_refused_without_a_launch():
    """Null pointers / n <= 0: CTU_REQUIRE answers on the host (this test runs without a GPU, so nothing can launch)."""
    from ctunet_amd import _lib
    lib = _lib.load()
    one = (C.c_int64 * 1)(4)
    fake = (C.c_void_p * 5)(64, 64, 64, 64, 64)                          # non-null, never dereferenced on the host
    bad = _lib.load().ctu_plateau_update(None, None, None, None, 0, 1, 0.1, 10, 1e-4, 0, 0.0, 1e-8, None)
    assert bad != 0 and b"plateau_update" in lib.ctu_last_error()
    assert lib.ctu_plateau_update(64, 64, None, 64, 0, 1, 0.1, 10, 1e-4, 0, 0.0, 1e-8, None) != 0
    assert lib.ctu_plateau_update(64, 64, 64, 64, 0, 1, 1.0, 10, 1e-4, 0, 0.0, 1e-8, None) != 0          # factor >= 1
    assert lib.ctu_adam_amsgrad_dev(None, one, 1, 64, 64, 0.9, 0.999, 1e-8, 0.0, 0, None, None, None) != 0
    assert b"adam_amsgrad_dev" in lib.ctu_last_error()
    assert lib.ctu_adam_amsgrad_dev(fake, one, 0, 64, 64, 0.9, 0.999, 1e-8, 0.0, 0, None, None, None) != 0
    assert lib.ctu_adam_amsgrad_dev(fake, one, 1, None, 64, 0.9, 0.999, 1e-8, 0.0, 0, None, None, None) != 0
    assert lib.ctu_adam_amsgrad_dev(fake, one, 1, 64, None, 0.9, 0.999, 1e-8, 0.0, 0, None, None, None) != 0   # lr
    assert lib.ctu_adam_amsgrad_dev((C.c_void_p * 5)(64, None, 64, 64, 64), one, 1, 64, 64, 0.9, 0.999, 1e-8, 0.0, 0, None,
                                    None, None) != 0
    assert lib.ctu_grad_clip_coef(None, one, 1, 1.0, 64, 64, 64, None) != 0
    assert b"grad_clip_coef" in lib.ctu_last_error()
    assert lib.ctu_grad_clip_coef(fake, one, 0, 1.0, 64, 64, 64, None) != 0
    assert lib.ctu_grad_clip_coef(fake, one, -2, 1.0, 64, 64, 64, None) != 0
    assert lib.ctu_grad_clip_coef(fake, one, 1, 1.0, None, 64, 64, None) != 0
    assert lib.ctu_grad_clip_coef(fake, one, 1, 1.0, 64, None, 64, None) != 0
    assert lib.ctu_grad_clip_coef(fake, one, 1, 1.0, 64, 64, None, None) != 0
    assert lib.ctu_grad_clip_coef((C.c_void_p * 1)(None), one, 1, 1.0, 64, 64, 64, None) != 0
    assert lib.ctu_grad_norm_num_blocks(None, 1) == 0 and lib.ctu_grad_norm_num_blocks(one, 0) == 0


def _table_calls(lib):
    """(entry point's message prefix, pointers per tensor, call(ptrs, sizes, n)) for every entry point that takes a tensor
    list; every other argument is valid, so only the list can be refused."""
    adam = (0.9, 0.999, 1e-8, 0.0, 0)
    return [
        (b"adam_amsgrad:", 5, lambda p, s, n: lib.ctu_adam_amsgrad(p, s, n, 64, 1e-3, *adam, None, None)),
        (b"adam_amsgrad_dev:", 5, lambda p, s, n: lib.ctu_adam_amsgrad_dev(p, s, n, 64, 64, *adam, None, None, None)),
        (b"sgd:", 3, lambda p, s, n: lib.ctu_sgd(p, s, n, 64, None, 0.1, 0.9, 0.0, 0.0, 0, 0, None, None, None)),
        (b"rmsprop:", 5, lambda p, s, n: lib.ctu_rmsprop(p, s, n, 64, None, 0.01, 0.99, 1e-8, 0.0, 0.9, 1, 0, None, None, None)),
        (b"grad_clip_coef:", 1, lambda p, s, n: lib.ctu_grad_clip_coef(p, s, n, 1.0, 64, 64, 64, None)),
        (b"scale_tensors:", 1, lambda p, s, n: lib.ctu_scale_tensors(p, s, n, 0.5, None, None)),
        (b"unscale_tensors:", 1, lambda p, s, n: lib.ctu_unscale_tensors(p, s, n, 64, 64, None)),
    ]


@pytest.mark.parametrize("fault", ["null", "negative-size", "misaligned"])
def test_a_bad_tensor_in_the_second_chunk_refuses_the_whole_list(fault):
    """65 tensors, the last one bad: CTU_EINVAL (-1) names the entry point and tensor 64.  Without a GPU a launch of the first
    64 tensors or of the step counter would have answered CTU_ELAUNCH (-2) instead: nothing was launched."""
    from ctunet_amd import _lib
    lib = _lib.load()
    n = 65
    for name, k, call in _table_calls(lib):
        ptrs = [64] * (k * n)
        sizes = [4] * n
        if fault == "null":
            ptrs[64 * k + k - 1] = None                                  # the tensor's last slot: required in every call above
        elif fault == "misaligned":
            ptrs[64 * k + k - 1] = 66
        else:
            sizes[64] = -1
        rc = call((C.c_void_p * len(ptrs))(*ptrs), (C.c_int64 * n)(*sizes), n)
        msg = lib.ctu_last_error()
        assert rc == -1, (name, fault, rc, msg)
        assert msg.startswith(name) and b"64" in msg, (name, fault, msg)


def test_workspace_size_follows_the_launch_plan():
    """One partial per block: per 64-tensor chunk, (blocks along the largest tensor, at most 64) x tensors."""
    from ctunet_amd import _lib
    lib = _lib.load()

    def nb(sizes):
        return lib.ctu_grad_norm_num_blocks((C.c_int64 * len(sizes))(*sizes), len(sizes))
    assert nb([1]) == 1 and nb([4096]) == 1 and nb([4097]) == 2
    assert nb([1, 3, 63, 257, 4099, 70001]) == 6 * 18                    # ceil(70001 / 4096) = 18
    assert nb([10 ** 7]) == 64
    assert nb([5000] * 64 + [10]) == 64 * 2 + 1                          # the 65th tensor opens a second chunk


def test_step_runner_device_lr_needs_the_fused_optimizer():
    from ctunet_amd.trainer import StepRunner
    base = dict(model_class="UNet", problem_handler="FlapRec", learning_rate=1e-2, ce_lambda=1.0, dice_lambda=1.0, device="cpu")
    for name in ("sgd", "rmsprop"):
        with pytest.raises(ValueError, match="device_lr"):
            StepRunner(dict(base, optimizer=name, device_lr=True))
    run = StepRunner(dict(base, optimizer="adamw", device_lr=True, max_grad_norm=3.0, scheduler=None))
    from ctunet_amd import lr_scheduler, optim
    assert isinstance(run.params["optimizer"], optim.AdamW) and run.params["optimizer"].max_grad_norm == 3.0
    assert isinstance(run.params["scheduler"], lr_scheduler.ReduceLROnPlateau)
    run = StepRunner(dict(base, optimizer="adam", scheduler=None))       # default: today's objects
    assert run.params["optimizer"].device_lr is False
    assert isinstance(run.params["scheduler"], torch.optim.lr_scheduler.ReduceLROnPlateau)
