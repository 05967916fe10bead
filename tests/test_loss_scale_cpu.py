"""Dynamic loss scaling, the host side (no GPU): argument validation, where the state lives, and the C ABI entry points
the device side needs."""
import ctypes
import math

import pytest
import torch


def _net():
    import ctunet_amd
    torch.manual_seed(0)
    return ctunet_amd.UNet(n_blocks=2, use_checkpoint=False)


@pytest.mark.parametrize("kw", [
    dict(growth_factor=1.0), dict(growth_factor=0.5), dict(backoff_factor=0.0), dict(backoff_factor=1.0),
    dict(backoff_factor=1.5), dict(backoff_factor=-0.5), dict(growth_interval=0), dict(growth_interval=-3),
    dict(growth_interval=2.5), dict(init_scale=0.0), dict(init_scale=-1.0), dict(init_scale=math.inf),
    dict(init_scale=math.nan),
])
def test_bad_hyper_parameters_raise(kw):
    import ctunet_amd
    with pytest.raises(ValueError):
        ctunet_amd.DynamicLossScale(**kw)


@pytest.mark.parametrize("dtype", ["bf16", "fp32", torch.bfloat16, torch.float32])
def test_dynamic_scaling_is_float16_only(dtype):
    import ctunet_amd
    net = _net()
    with pytest.raises(ValueError):
        net.set_precision(dtype, loss_scale="dynamic")
    with pytest.raises(ValueError):
        net.set_precision(dtype, loss_scale=ctunet_amd.DynamicLossScale(init_scale=2.0 ** 10))
    assert net.loss_scaler is None


def test_unknown_loss_scale_string_raises():
    with pytest.raises(ValueError):
        _net().set_precision("fp16", loss_scale="auto")


def test_the_scaler_belongs_to_the_model():
    import ctunet_amd
    net = _net()
    assert net.loss_scaler is None
    net.set_precision("fp16", loss_scale=2.0 ** 12)                      # static: no scaler
    assert net.loss_scaler is None
    net.set_precision("fp16", loss_scale=ctunet_amd.DynamicLossScale(init_scale=2.0 ** 20, growth_interval=7))
    sc = net.loss_scaler
    assert sc is not None and sc.get_scale() == 2.0 ** 20 and sc.growth_interval == 7
    assert sc.scale.dtype == torch.float32 and sc.growth_tracker.dtype == torch.int32 and sc.found_inf.dtype == torch.float32
    assert net.overflow_flag() is sc.found_inf
    eng = net._engine()
    assert eng.scaler is sc
    net.set_precision("bf16")                                            # engine rebuilt; no scaler while bf16
    assert net.loss_scaler is None and net._engine().scaler is None
    net.set_precision("fp16", loss_scale="dynamic")                      # back: the same state, the new hyper-parameters
    assert net.loss_scaler is sc and sc.get_scale() == 2.0 ** 20 and sc.growth_interval == 2000
    assert net._engine() is not eng and net._engine().scaler is sc


def test_default_init_scale_is_the_static_default():
    from ctunet_amd.loss_scale import default_loss_scale
    net = _net().set_precision("fp16", loss_scale="dynamic")
    sc = net.loss_scaler
    assert sc.get_scale() is None                                        # seeded by the first float16 backward
    sc.prepare("cpu", 32 ** 3)
    assert sc.get_scale() == default_loss_scale(32 ** 3) == 2.0 ** 11
    assert default_loss_scale(256 ** 3) == 2.0 ** 20


def test_state_dict_carries_the_grad_scaler_keys():
    import ctunet_amd
    net = _net().set_precision("fp16", loss_scale=ctunet_amd.DynamicLossScale(init_scale=512.0, growth_interval=3))
    sd = net.loss_scaler.state_dict()
    assert {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"} <= set(sd)
    assert sd["scale"] == 512.0 and sd["growth_interval"] == 3 and sd["_growth_tracker"] == 0
    other = _net().set_precision("fp16", loss_scale="dynamic")
    other.loss_scaler.load_state_dict(dict(sd, _growth_tracker=2, skipped_steps=5))
    assert other.loss_scaler.get_scale() == 512.0 and int(other.loss_scaler.growth_tracker) == 2
    assert other.loss_scaler.skipped_steps() == 5 and other.loss_scaler.growth_interval == 3
    with pytest.raises(RuntimeError):
        other.loss_scaler.load_state_dict({})                            # what a disabled GradScaler saves
    with pytest.raises(ValueError):
        other.loss_scaler.load_state_dict(dict(sd, backoff_factor=2.0))


def test_graphed_step_refuses_an_unguarded_optimizer_for_a_dynamic_model():
    from ctunet_amd.graph import GraphedTrainStep
    net = _net().set_precision("fp16", loss_scale="dynamic")
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    x = torch.zeros(1, 1, 16, 16, 16)
    with pytest.raises(RuntimeError, match="dynamic loss scaling"):
        GraphedTrainStep(net, opt, x, [torch.zeros(1, 2, 16, 16, 16)], 1.0, 1.0)


def test_library_exports_the_loss_scale_entry_points():
    from ctunet_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ctu_loss_scale_update", "ctu_unscale_tensors", "ctu_lp_head_bwd_bn_dscale"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 8 and _lib.load().ctu_abi_version() == 8
