"""``ReduceLROnPlateau`` kept in device memory, so it can be stepped every batch without a host sync and inside a
replayed HIP graph.

The reference steps ``torch.optim.lr_scheduler.ReduceLROnPlateau`` once per batch with the batch loss
(ctunet/pytorch/Model.py:343-374), and ``step`` starts with ``float(metrics)``: the host waits for the device every step.
Here ``best`` (float64), the counters (int32) and the learning rate (``optim.Adam(device_lr=True)``'s float64 ``lr_t``)
are device tensors and one single-thread kernel (``ctu_plateau_update``) applies torch's rule to a device metric -- what
``loss_scale.LossScaler`` does for the loss scale.  Arguments, validation and ``state_dict`` keys are torch's, so a
checkpoint moves between the two classes in both directions.
"""
from __future__ import annotations

from math import inf
from typing import List

import torch

from . import _lib

_HYPER = ("factor", "patience", "cooldown", "eps", "mode", "threshold", "threshold_mode")


class ReduceLROnPlateau:
    def __init__(self, optimizer, mode="min", factor=0.1, patience=10, threshold=1e-4, threshold_mode="rel", cooldown=0,
                 min_lr=0, eps=1e-8):
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        if not isinstance(optimizer, torch.optim.Optimizer):
            raise TypeError(f"{type(optimizer).__name__} is not an Optimizer")
        if not (getattr(optimizer, "device_lr", False) and hasattr(optimizer, "sync_lr")):
            raise ValueError("ctunet_amd.lr_scheduler.ReduceLROnPlateau needs a ctunet_amd.optim.Adam / AdamW / SGD / RMSprop "
                             "built with device_lr=True (the kernel writes the learning rate the optimizer's kernel reads); "
                             "use torch.optim.lr_scheduler.ReduceLROnPlateau for any other optimizer")
        groups = optimizer.param_groups
        if isinstance(min_lr, (list, tuple)):
            if len(min_lr) != len(groups):
                raise ValueError(f"expected {len(groups)} min_lrs, got {len(min_lr)}")
            self.default_min_lr = None
            self.min_lrs = list(min_lr)
        else:
            self.default_min_lr = min_lr
            self.min_lrs = [min_lr] * len(groups)
        self._init_is_better(mode, threshold, threshold_mode)
        self.optimizer = optimizer
        self.factor, self.patience, self.cooldown, self.eps = factor, patience, cooldown, eps
        # per group (every launch advances its own copy; all copies see the same metric and stay equal):
        # best float64[1]; counters int32[4] = num_bad_epochs, cooldown_counter, last_epoch, reductions applied
        self._best: List[torch.Tensor] = []
        self._counters: List[torch.Tensor] = []
        self._pending = {"best": self.mode_worse, "num_bad_epochs": 0, "cooldown_counter": 0, "last_epoch": 0,
                         "num_reductions": 0}

    def _init_is_better(self, mode, threshold, threshold_mode) -> None:
        if mode not in {"min", "max"}:
            raise ValueError("mode " + mode + " is unknown!")
        if threshold_mode not in {"rel", "abs"}:
            raise ValueError("threshold mode " + threshold_mode + " is unknown!")
        self.mode_worse = inf if mode == "min" else -inf
        self.mode, self.threshold, self.threshold_mode = mode, threshold, threshold_mode

    # ------------------------------------------------------------------ device state
    def prepare(self) -> None:
        """Creates the device state and the optimizer's ``lr_t`` (first ``step`` does it too; never inside a capture)."""
        groups = self.optimizer.param_groups
        if len(self._best) == len(groups):
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ctunet_amd.lr_scheduler: the scheduler state must be on the GPU before a graph capture "
                               "(step it once eagerly, or let GraphedTrainStep's warm-up do it)")
        if len(groups) != len(self.min_lrs):
            if self.default_min_lr is None:
                raise RuntimeError(f"The number of param groups in the `optimizer` ({len(groups)}) differs from when "
                                   f"`ReduceLROnPlateau` was initialized ({len(self.min_lrs)})")
            self.min_lrs = [self.default_min_lr] * len(groups)
        self.optimizer.sync_lr()
        st = self._host_state() if self._best else self._pending
        self._best, self._counters = [], []
        for g in groups:
            dev = g["lr_t"].device
            self._best.append(torch.full((1,), float(st["best"]), dtype=torch.float64, device=dev))
            self._counters.append(torch.tensor([st["num_bad_epochs"], st["cooldown_counter"], st["last_epoch"],
                                                st["num_reductions"]], dtype=torch.int32, device=dev))

    def step(self, metric: torch.Tensor) -> None:
        """metric: a float32 GPU tensor of one element (or 0-d).  One ``ctu_plateau_update`` launch per parameter group on
        the current stream; no host sync, nothing returned."""
        if not isinstance(metric, torch.Tensor) or metric.numel() != 1 or metric.dtype != torch.float32 or not metric.is_cuda:
            raise TypeError("ctunet_amd.lr_scheduler.ReduceLROnPlateau.step takes a float32 GPU tensor of one element (the "
                            "device loss; no float() -- that is the host sync this class removes)")
        if not torch.cuda.is_current_stream_capturing():
            self.optimizer.sync_lr()
        self.prepare()
        lib = _lib.load()
        stream = torch.cuda.current_stream(metric.device).cuda_stream
        for i, g in enumerate(self.optimizer.param_groups):
            _lib.check(lib.ctu_plateau_update(metric.data_ptr(), g["lr_t"].data_ptr(), self._best[i].data_ptr(),
                                              self._counters[i].data_ptr(), int(self.mode == "max"),
                                              int(self.threshold_mode == "rel"), float(self.factor), int(self.patience),
                                              float(self.threshold), int(self.cooldown), float(self.min_lrs[i]),
                                              float(self.eps), stream), "plateau_update")

    # ------------------------------------------------------------------ inspection / checkpoints (each one sync)
    def _host_state(self) -> dict:
        if not self._best:
            return dict(self._pending)
        c = self._counters[0].tolist()
        return {"best": float(self._best[0].item()), "num_bad_epochs": c[0], "cooldown_counter": c[1], "last_epoch": c[2],
                "num_reductions": c[3]}

    def get_last_lr(self) -> List[float]:
        return self.optimizer.get_lr()

    @property
    def best(self) -> float:
        return self._host_state()["best"]

    @property
    def num_bad_epochs(self) -> int:
        return self._host_state()["num_bad_epochs"]

    @property
    def cooldown_counter(self) -> int:
        return self._host_state()["cooldown_counter"]

    @property
    def last_epoch(self) -> int:
        return self._host_state()["last_epoch"]

    @property
    def num_reductions(self) -> int:
        """How many times the learning rate was actually lowered."""
        return self._host_state()["num_reductions"]

    def state_dict(self) -> dict:
        """Every key of ``torch.optim.lr_scheduler.ReduceLROnPlateau.state_dict()`` with the same meaning (that class can
        load the result), plus ``num_reductions``."""
        sd = {k: getattr(self, k) for k in _HYPER}
        sd.update(default_min_lr=self.default_min_lr, min_lrs=list(self.min_lrs), mode_worse=self.mode_worse)
        sd.update(self._host_state())
        sd["_last_lr"] = self.get_last_lr()
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Accepts this class's and torch's state dicts; existing device tensors are written in place."""
        if sd["factor"] >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        self._init_is_better(sd["mode"], sd["threshold"], sd["threshold_mode"])
        self.factor, self.patience, self.cooldown, self.eps = sd["factor"], sd["patience"], sd["cooldown"], sd["eps"]
        self.default_min_lr, self.min_lrs = sd.get("default_min_lr"), list(sd["min_lrs"])
        st = {"best": float(sd["best"]), "num_bad_epochs": int(sd["num_bad_epochs"]),
              "cooldown_counter": int(sd["cooldown_counter"]), "last_epoch": int(sd["last_epoch"]),
              "num_reductions": int(sd.get("num_reductions", 0))}
        self._pending = st
        for b, c in zip(self._best, self._counters):
            b.fill_(st["best"])
            c.copy_(torch.tensor([st["num_bad_epochs"], st["cooldown_counter"], st["last_epoch"], st["num_reductions"]],
                                 dtype=torch.int32))
