"""Fused Adam / AdamW with amsgrad on the MI355X (one kernel launch for all parameter tensors).

Drop-in for ``optim.Adam(params, lr, weight_decay, amsgrad=True)`` / ``optim.AdamW(...)`` as the reference
builds them (ctunet/pytorch/Model.py:514-527): same hyper-parameter names and defaults, same state entries
(``exp_avg``, ``exp_avg_sq``, ``max_exp_avg_sq``, ``step``), same update rule; parameters whose ``.grad`` is
``None`` (the dead centre block) are skipped and keep no state, as in torch.  torch's own capturable
amsgrad path issues two elementwise kernels per parameter tensor (116 launches per step for UNet()); this
issues two launches in total and is safe to capture in a HIP graph (the step counter lives on the device).
Deviation from torch: ONE step counter per parameter group (``group["step_t"]``, also what ``state[p]["step"]``
refers to), where torch keeps one per tensor -- a parameter that receives its first gradient later than the others
of its group therefore shares their bias correction (no shipped model has such a parameter: the dead centre block
never gets a gradient at all).

Opt-in train controls that stay on the device, so a replayed graph follows them:
``device_lr=True`` keeps each group's learning rate in a float64[1] device tensor (``group["lr_t"]``) that the kernel
reads; ``group["lr"]`` stays the Python float every torch scheduler edits, and ``sync_lr()`` uploads it when it changed.
``max_grad_norm=x`` clips the global gradient norm as ``clip_grad_norm_(model.parameters(), x)`` does: two launches
form the norm and the coefficient, the Adam launch multiplies each gradient by it.

``SGD`` and ``RMSprop`` (the reference's other two optimizers, Model.py:528-541) are the same construction over
``ctu_sgd`` / ``ctu_rmsprop``: torch's hyper-parameter names, defaults, constructor errors and state entries
(``momentum_buffer``; ``square_avg``, ``momentum_buffer``, ``grad_avg``, ``step``), so a ``torch.optim`` state dict loads
into them and back, and every control above -- overflow guard, device learning rate, clipping, graph capture.  The
shared counter shows in SGD's first step: ``momentum_buffer = grad`` happens on the group's first APPLIED step (an
overflowed first step leaves it to the next one, as ``GradScaler.step`` leaves torch's state empty); a parameter that
receives its first gradient later starts from a zero buffer instead.
"""
from __future__ import annotations

import ctypes as C
from typing import List

import torch

from . import _lib


class _Fused(torch.optim.Optimizer):
    """What every fused optimizer shares: the control protocol ``graph.py``, ``lr_scheduler.py``, ``loss_scale.py``,
    ``checkpoint.py`` and ``trainer.py`` reach by duck typing, and the step around one group's launch.  A subclass names
    itself (``_NAME``, for messages), lists one tensor's pointers (``_slots``, creating its state) and launches
    (``_launch``)."""

    _NAME = "Adam"

    def _init_controls(self, device_lr, max_grad_norm) -> None:
        # fp16 training: a float32[1] device flag (model.overflow_flag()) that the backward sets when a loss-scaled gradient
        # overflowed; a step that sees it set changes nothing (torch.amp.GradScaler.step's found_inf), also inside a replayed
        # HIP graph.  None: every step is applied.
        self.skip_flag = None
        self._guarded = None
        # the learning rate as a device operand (ctu_adam_amsgrad_dev); clipping needs that entry point too
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.device_lr = bool(device_lr) or self.max_grad_norm is not None
        self.last_grad_norm = None             # float32[1] device tensor: the global gradient norm of the last step (clipping)
        self._clip_coef = None
        self._clip_ws = None

    @classmethod
    def _check_max_grad_norm(cls, max_grad_norm) -> None:
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError(f"ctunet_amd.optim.{cls._NAME}: max_grad_norm must be positive, got {max_grad_norm}")

    def guard(self, model):
        """Skip every step whose float16 backward overflowed (``model.overflow_flag()``); no-op for fp32 / bf16 models.
        Dynamic loss scaling (``model.loss_scaler``): the flag is the scaler's ``found_inf``, and every ``step()`` also
        launches ``loss_scaler.update()`` behind its own kernels.  The scaler is looked up on the model at each step, so
        the guard survives a ``set_precision`` round trip of the model."""
        fp16 = model.__dict__.get("_act_dtype", torch.float32) == torch.float16
        self.skip_flag = model.overflow_flag() if fp16 and hasattr(model, "overflow_flag") else None
        self._guarded = model if hasattr(model, "loss_scaler") else None
        return self

    def guarded_scaler(self):
        """The dynamic loss scaler of the guarded model (None: static scaling or none)."""
        return None if self._guarded is None else self._guarded.loss_scaler

    # ------------------------------------------------------------------ the learning rate on the device
    @staticmethod
    def _group_device(group):
        for p in group["params"]:
            return p.device
        return None

    def sync_lr(self) -> None:
        """Uploads every ``group["lr"]`` that differs from what its device tensor was last given (one ``fill_``, no host
        sync); creates the tensor on first use and moves it behind ``load_state_dict(map_location="cpu")``.  Nothing to do
        during a capture, where both agree."""
        if not self.device_lr:
            return
        for group in self.param_groups:
            lr, dev = float(group["lr"]), self._group_device(group)
            if dev is None or dev.type != "cuda":
                continue
            lr_t = group.get("lr_t")
            if lr_t is not None and lr_t.device == dev and group.get("lr_shadow") == lr:
                continue
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"ctunet_amd.optim.{self._NAME}: the device learning rate must be in place before a graph "
                                   "capture (run one eager step or call sync_lr() first, and edit group['lr'] between replays "
                                   "only)")
            if lr_t is None:
                group["lr_t"] = torch.full((1,), lr, dtype=torch.float64, device=dev)
            elif lr_t.device != dev:
                group["lr_t"] = lr_t.to(dev)               # a checkpoint's value, kept: it may be ahead of group["lr"]
                if group.get("lr_shadow") != lr:
                    group["lr_t"].fill_(lr)
            else:
                lr_t.fill_(lr)
            group["lr_shadow"] = lr

    def get_lr(self) -> List[float]:
        """The learning rates the kernels read (one sync); refreshes ``group["lr"]`` with them, which matters after a
        device-side scheduler reduced them."""
        if not self.device_lr:
            return [float(g["lr"]) for g in self.param_groups]
        self.sync_lr()
        have = [g for g in self.param_groups if "lr_t" in g]
        vals = torch.cat([g["lr_t"] for g in have]).tolist() if have else []
        for g, v in zip(have, vals):
            g["lr"] = g["lr_shadow"] = v
        return [float(g["lr"]) for g in self.param_groups]

    def _clip(self, lib, grads: List[torch.Tensor]):
        """Global norm of ``grads`` and its clip coefficient (``ctu_grad_clip_coef``); returns the coefficient tensor."""
        n = len(grads)
        sa = (C.c_int64 * n)(*[g.numel() for g in grads])
        need = int(lib.ctu_grad_norm_num_blocks(sa, n))
        dev = grads[0].device
        if self._clip_ws is None or self._clip_ws.numel() < need or self._clip_ws.device != dev:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"ctunet_amd.optim.{self._NAME}: the clipping workspace is allocated by the first eager "
                                   "step; run one before capturing a graph (GraphedTrainStep's warm-up does)")
            self._clip_ws = torch.empty(need, dtype=torch.float32, device=dev)
            if self.last_grad_norm is None or self.last_grad_norm.device != dev:
                self.last_grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)
                self._clip_coef = torch.ones(1, dtype=torch.float32, device=dev)
        ga = (C.c_void_p * n)(*[g.data_ptr() for g in grads])
        _lib.check(lib.ctu_grad_clip_coef(ga, sa, n, self.max_grad_norm, self._clip_ws.data_ptr(),
                                          self.last_grad_norm.data_ptr(), self._clip_coef.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), "grad_clip_coef")
        return self._clip_coef

    # ------------------------------------------------------------------ what a subclass provides
    def _first_count(self, live) -> float:
        """The value a group's step counter starts from when the group carries none."""
        return 0.0

    def _slots(self, group, p, g, st) -> List[int]:
        """The device pointers of one tensor in the entry point's order; creates the state entries that are missing."""
        raise NotImplementedError

    def _launch(self, lib, group, pa, sa, n, lr_ptr, coef_ptr, skip_ptr, stream) -> None:
        """One group's update; ``lr_ptr`` is None for the host learning rate ``group["lr"]``."""
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        scaler = self.guarded_scaler()
        skip = scaler.found_inf if scaler is not None else self.skip_flag
        stepped = False
        if self.device_lr and not torch.cuda.is_current_stream_capturing():
            self.sync_lr()
        work = []
        for group in self.param_groups:
            live: List[torch.Tensor] = [p for p in group["params"] if p.grad is not None]
            if not live:
                continue
            for p in live:
                if not p.is_cuda or p.dtype != torch.float32:
                    raise RuntimeError(f"ctunet_amd.optim.{self._NAME}: parameters must be float32 on the GPU (no CPU "
                                       "fallback)")
            work.append((group, live, [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in live]))
        coef = None
        if self.max_grad_norm is not None and work:
            coef = self._clip(lib, [g for _, _, grads in work for g in grads])      # ONE norm over all groups
        for group, live, grads in work:
            if "step_t" not in group:
                group["step_t"] = torch.full((1,), self._first_count(live), dtype=torch.float32, device=live[0].device)
            elif group["step_t"].device != live[0].device:
                # load_state_dict casts per-parameter state to the parameter's device but leaves param_groups values
                # where the checkpoint had them (map_location="cpu"): the kernel must never see a host pointer
                group["step_t"] = group["step_t"].to(live[0].device)
            ptrs, sizes = [], []
            for p, g in zip(live, grads):
                ptrs += self._slots(group, p, g, self.state[p])
                sizes.append(p.numel())
            n = len(live)
            pa = (C.c_void_p * len(ptrs))(*ptrs)
            sa = (C.c_int64 * n)(*sizes)
            lr_ptr = None
            if self.device_lr:
                if "lr_t" not in group or group["lr_t"].device != live[0].device:
                    raise RuntimeError(f"ctunet_amd.optim.{self._NAME}: the device learning rate must be in place before a "
                                       "graph capture (run one eager step or call sync_lr() first)")
                lr_ptr = group["lr_t"].data_ptr()
            self._launch(lib, group, pa, sa, n, lr_ptr, None if coef is None else coef.data_ptr(),
                         None if skip is None else skip.data_ptr(), torch.cuda.current_stream().cuda_stream)
            # the kernel wrote the parameters through raw pointers: tell autograd / every (version-keyed) cache of
            # derived data -- the engine's MFMA-ordered weight copies -- that they changed
            torch.autograd.graph.increment_version(live)
            stepped = True
        if scaler is not None and stepped:
            scaler.update()            # same stream, after every group's kernels have read found_inf: back off / grow, clear it
        return loss


def _zeros(p):
    return torch.zeros_like(p, memory_format=torch.preserve_format)


class Adam(_Fused):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=True,
                 decoupled_weight_decay=False, device_lr=False, max_grad_norm=None):
        if not amsgrad:
            raise NotImplementedError("ctunet_amd.optim.Adam implements the amsgrad variant the reference uses")
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameter")
        self._check_max_grad_norm(max_grad_norm)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=True,
                                      decoupled_weight_decay=decoupled_weight_decay))
        self._init_controls(device_lr, max_grad_norm)

    def _slots(self, group, p, g, st):
        if not st:
            st["step"] = group["step_t"]                    # shared device counter (torch keeps one per tensor)
            st["exp_avg"] = _zeros(p)
            st["exp_avg_sq"] = _zeros(p)
            st["max_exp_avg_sq"] = _zeros(p)
        return [p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                st["max_exp_avg_sq"].data_ptr()]

    def _launch(self, lib, group, pa, sa, n, lr_ptr, coef_ptr, skip_ptr, stream):
        b1, b2 = group["betas"]
        hyper = (float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                 int(bool(group["decoupled_weight_decay"])))
        if lr_ptr is None:
            _lib.check(lib.ctu_adam_amsgrad(pa, sa, n, group["step_t"].data_ptr(), float(group["lr"]), *hyper, skip_ptr,
                                            stream), "adam_amsgrad")
        else:
            _lib.check(lib.ctu_adam_amsgrad_dev(pa, sa, n, group["step_t"].data_ptr(), lr_ptr, *hyper, coef_ptr, skip_ptr,
                                                stream), "adam_amsgrad_dev")


class AdamW(Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=True, device_lr=False,
                 max_grad_norm=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, decoupled_weight_decay=True, device_lr=device_lr,
                         max_grad_norm=max_grad_norm)


class SGD(_Fused):
    """``torch.optim.SGD`` (momentum, dampening, weight decay, Nesterov, maximize) in one launch per 64 tensors."""

    _NAME = "SGD"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 device_lr=False, max_grad_norm=None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        self._check_max_grad_norm(max_grad_norm)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, maximize=maximize))
        self._init_controls(device_lr, max_grad_norm)

    def _first_count(self, live):
        # momentum buffers without a counter: a torch.optim.SGD state dict was loaded, and its first step is behind it
        return 1.0 if any("momentum_buffer" in self.state[p] for p in live) else 0.0

    def _slots(self, group, p, g, st):
        buf = None
        if group["momentum"] != 0:
            if st.get("momentum_buffer") is None:
                st["momentum_buffer"] = _zeros(p)           # the kernel's first applied step overwrites it with the gradient
            buf = st["momentum_buffer"].data_ptr()
        return [p.data_ptr(), g.data_ptr(), buf]

    def _launch(self, lib, group, pa, sa, n, lr_ptr, coef_ptr, skip_ptr, stream):
        _lib.check(lib.ctu_sgd(pa, sa, n, group["step_t"].data_ptr(), lr_ptr, float(group["lr"]), float(group["momentum"]),
                               float(group["dampening"]), float(group["weight_decay"]), int(bool(group["nesterov"])),
                               int(bool(group.get("maximize", False))), coef_ptr, skip_ptr, stream), "sgd")


class RMSprop(_Fused):
    """``torch.optim.RMSprop`` (alpha, eps, weight decay, momentum, centered, maximize) in one launch per 64 tensors."""

    _NAME = "RMSprop"

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, *,
                 maximize=False, device_lr=False, max_grad_norm=None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if alpha < 0.0:
            raise ValueError(f"Invalid alpha value: {alpha}")
        self._check_max_grad_norm(max_grad_norm)
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum,
                                      centered=centered, maximize=maximize))
        self._init_controls(device_lr, max_grad_norm)

    def _first_count(self, live):
        # a loaded torch.optim.RMSprop state dict keeps one count per tensor: the group's counter continues from it
        for p in live:
            if "step" in self.state[p]:
                return float(self.state[p]["step"])
        return 0.0

    def _slots(self, group, p, g, st):
        if st.get("step") is not group["step_t"]:
            st["step"] = group["step_t"]                    # shared device counter (torch keeps one per tensor)
        if "square_avg" not in st:
            st["square_avg"] = _zeros(p)
        buf = ga = None
        if group["momentum"] > 0:
            if "momentum_buffer" not in st:
                st["momentum_buffer"] = _zeros(p)
            buf = st["momentum_buffer"].data_ptr()
        if group["centered"]:
            if "grad_avg" not in st:
                st["grad_avg"] = _zeros(p)
            ga = st["grad_avg"].data_ptr()
        return [p.data_ptr(), g.data_ptr(), st["square_avg"].data_ptr(), buf, ga]

    def _launch(self, lib, group, pa, sa, n, lr_ptr, coef_ptr, skip_ptr, stream):
        _lib.check(lib.ctu_rmsprop(pa, sa, n, group["step_t"].data_ptr(), lr_ptr, float(group["lr"]), float(group["alpha"]),
                                   float(group["eps"]), float(group["weight_decay"]), float(group["momentum"]),
                                   int(bool(group["centered"])), int(bool(group.get("maximize", False))), coef_ptr,
                                   skip_ptr, stream), "rmsprop")
