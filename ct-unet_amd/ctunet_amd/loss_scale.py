"""Dynamic loss scaling for the float16 path, kept in device memory (``torch.amp.GradScaler`` semantics).

The static loss scale of ``set_precision("fp16", loss_scale=<float>)`` reaches the kernels as a host float, so a captured
step freezes it.  Here the scale, the growth tracker, the overflow flag and the skip count are float32 / int32 device
tensors: the backward reads the scale through ``ctu_lp_head_bwd_bn_dscale`` / ``ctu_unscale_tensors`` and the update is
one single-thread kernel (``ctu_loss_scale_update``, the rule of ``torch._amp_update_scale_``) that the fused optimizer
launches right after its own kernels.  All of it replays inside a HIP graph and adapts there.

The state belongs to the model (``model.loss_scaler``), not to its engine: it survives the engine rebuild of a
``set_precision`` round trip.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib


def default_loss_scale(nvox: int) -> float:
    """The static float16 default: a power of two near voxels / 16 (``UNetEngine``)."""
    return float(2 ** max(0, int(nvox).bit_length() - 5))


@dataclass(frozen=True)
class DynamicLossScale:
    """Hyper-parameters of dynamic loss scaling (``torch.amp.GradScaler``'s names and defaults, except ``init_scale``).
    init_scale None: the static default for the volume of the first float16 backward (``default_loss_scale``)."""
    init_scale: Optional[float] = None
    growth_factor: float = 2.0
    backoff_factor: float = 0.5
    growth_interval: int = 2000

    def __post_init__(self):
        if self.init_scale is not None and not (math.isfinite(self.init_scale) and self.init_scale > 0):
            raise ValueError(f"ctunet_amd: init_scale must be finite and positive, got {self.init_scale}")
        if not self.growth_factor > 1.0:
            raise ValueError(f"ctunet_amd: growth_factor must be > 1, got {self.growth_factor}")
        if not 0.0 < self.backoff_factor < 1.0:
            raise ValueError(f"ctunet_amd: backoff_factor must lie in (0, 1), got {self.backoff_factor}")
        if isinstance(self.growth_interval, bool) or int(self.growth_interval) != self.growth_interval or self.growth_interval < 1:
            raise ValueError(f"ctunet_amd: growth_interval must be an integer >= 1, got {self.growth_interval}")


class LossScaler:
    """Device state of dynamic loss scaling: ``scale`` (float32[1]), ``growth_tracker`` (int32[1]), ``found_inf``
    (float32[1]: set by the un-scaling launches of every float16 backward, cleared only by ``update``) and ``skipped``
    (float32[1]: number of steps whose gradients overflowed).  Tensors are allocated once; their pointers stay stable, as
    captured graphs and the fused optimizer need."""

    def __init__(self, cfg: DynamicLossScale, device):
        device = torch.device(device)
        self.growth_factor = float(cfg.growth_factor)
        self.backoff_factor = float(cfg.backoff_factor)
        self.growth_interval = int(cfg.growth_interval)
        self.scale = torch.full((1,), cfg.init_scale or 0.0, dtype=torch.float32, device=device)
        self.growth_tracker = torch.zeros(1, dtype=torch.int32, device=device)
        self.found_inf = torch.zeros(1, dtype=torch.float32, device=device)
        self.skipped = torch.zeros(1, dtype=torch.float32, device=device)
        self.initialized = cfg.init_scale is not None

    def configure(self, cfg: DynamicLossScale) -> None:
        """New hyper-parameters; the state (scale, tracker, skip count) is kept -- init_scale only seeds a fresh scale."""
        self.growth_factor = float(cfg.growth_factor)
        self.backoff_factor = float(cfg.backoff_factor)
        self.growth_interval = int(cfg.growth_interval)
        if not self.initialized and cfg.init_scale is not None:
            self.scale.fill_(float(cfg.init_scale))
            self.initialized = True

    @property
    def device(self) -> torch.device:
        return self.scale.device

    def prepare(self, device, nvox: int) -> None:
        """Called by every float16 backward (and by ``GraphedTrainStep`` before its warm-up): moves the state to the
        model's GPU and seeds a scale given as ``init_scale=None`` with the static default for ``nvox`` voxels."""
        device = torch.device(device)
        if self.scale.device != device or not self.initialized:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ctunet_amd: the dynamic loss scale must be initialised on its GPU before a graph capture "
                                   "(run one eager step, pass init_scale, or use GraphedTrainStep)")
            if self.scale.device != device:
                for name in ("scale", "growth_tracker", "found_inf", "skipped"):
                    setattr(self, name, getattr(self, name).to(device))
            if not self.initialized:
                self.scale.fill_(default_loss_scale(nvox))
                self.initialized = True

    # ------------------------------------------------------------------ the step
    def update(self) -> None:
        """One single-thread launch on the current stream, no host sync: back off / grow the scale, count a skipped step,
        clear ``found_inf``."""
        _lib.check(_lib.load().ctu_loss_scale_update(self.scale.data_ptr(), self.growth_tracker.data_ptr(),
                                                     self.found_inf.data_ptr(), self.skipped.data_ptr(),
                                                     self.growth_factor, self.backoff_factor, self.growth_interval,
                                                     torch.cuda.current_stream(self.device).cuda_stream),
                   "loss_scale_update")

    def step(self, optimizer: torch.optim.Optimizer):
        """GradScaler's eager contract for optimizers that cannot read a device flag (torch.optim.*): one host sync,
        ``optimizer.step()`` only if the gradients are finite, then ``update()``.  A fused optimizer guarded on this
        scaler (``optim.Adam.guard``) already does both on the device: it is simply stepped."""
        if getattr(optimizer, "guarded_scaler", lambda: None)() is self:
            return optimizer.step()
        ret = None
        if float(self.found_inf.item()) == 0.0:
            ret = optimizer.step()
        self.update()
        return ret

    # ------------------------------------------------------------------ inspection / checkpoints
    def get_scale(self) -> Optional[float]:
        """The current scale (one sync); None while init_scale=None and no float16 backward has run yet."""
        return float(self.scale.item()) if self.initialized else None

    def skipped_steps(self) -> int:
        """Steps skipped so far because their gradients overflowed (one sync)."""
        return int(self.skipped.item())

    def state_dict(self) -> dict:
        """GradScaler's five keys with the same meaning, plus ``skipped_steps``."""
        return {"scale": self.get_scale(), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(self.growth_tracker.item()),
                "skipped_steps": self.skipped_steps()}

    def load_state_dict(self, sd: dict) -> None:
        """Accepts this class's and ``torch.amp.GradScaler``'s state dicts; the tensors are written in place."""
        if "scale" not in sd:
            raise RuntimeError("ctunet_amd: the loss-scale state dict is empty (a GradScaler that was disabled saves {})")
        DynamicLossScale(sd["scale"], sd["growth_factor"], sd["backoff_factor"], sd["growth_interval"])    # validation
        self.growth_factor = float(sd["growth_factor"])
        self.backoff_factor = float(sd["backoff_factor"])
        self.growth_interval = int(sd["growth_interval"])
        if sd["scale"] is not None:
            self.scale.fill_(float(sd["scale"]))
            self.initialized = True
        self.growth_tracker.fill_(int(sd["_growth_tracker"]))
        if "skipped_steps" in sd:
            self.skipped.fill_(float(sd["skipped_steps"]))
