"""Plain-Python float64 restatement of the device train controls (test infrastructure, not product code):
``ctu_plateau_update``'s rule, written from the kernel's contract (include/ctunet_hip.h), and the global gradient norm /
clip coefficient of ``ctu_grad_clip_coef``.  The CPU tests hold the plateau rule against torch's scheduler; the GPU tests
hold the kernels against torch's scheduler and against numpy."""
import math

import numpy as np

INF, NAN = math.inf, math.nan

# metric sequences shared by the CPU and the GPU tests
SEQUENCES = {
    "improving": [1.0, 0.9, 0.8, 0.7, 0.65, 0.6, 0.5, 0.4, 0.3, 0.2],
    "flat": [0.5] * 10,
    "worsening": [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2],
    "alternating": [0.5, 0.7, 0.4, 0.8, 0.39999, 0.9, 0.3, 1.0, 0.3, 0.3, 0.31, 0.29],
    "nonfinite": [0.5, NAN, 0.4, INF, 0.6, -INF, NAN, NAN, 0.7, 0.1, INF, 0.2],
}

# (patience, cooldown, min_lr, eps): patience 0 and 2, cooldown 0 and 2, a min_lr that binds after one reduction of
# lr = 0.1 by factor 0.5, an eps larger than the first reduction (which it therefore blocks)
CONFIGS = [(0, 0, 0.0, 1e-8), (2, 0, 0.0, 1e-8), (0, 2, 0.0, 1e-8), (2, 2, 0.0, 1e-8), (0, 0, 0.04, 1e-8), (0, 0, 0.0, 0.06)]
MODES = [("min", "rel"), ("min", "abs"), ("max", "rel"), ("max", "abs")]


class PlateauRef:
    """State of one parameter group: lr, best (float64) and the four counters of the kernel."""

    def __init__(self, lr, mode="min", factor=0.1, patience=10, threshold=1e-4, threshold_mode="rel", cooldown=0, min_lr=0.0,
                 eps=1e-8):
        self.lr = float(lr)
        self.mode_max, self.rel = mode == "max", threshold_mode == "rel"
        self.factor, self.patience, self.threshold = float(factor), int(patience), float(threshold)
        self.cooldown, self.min_lr, self.eps = int(cooldown), float(min_lr), float(eps)
        self.best = -INF if self.mode_max else INF
        self.num_bad_epochs = self.cooldown_counter = self.last_epoch = self.num_reductions = 0

    def step(self, metric):
        cur = float(np.float32(metric))                   # the kernel reads a float32 metric
        self.last_epoch += 1
        if not self.mode_max and self.rel:
            better = cur < self.best * (1.0 - self.threshold)
        elif not self.mode_max:
            better = cur < self.best - self.threshold
        elif self.rel:
            better = cur > self.best * (self.threshold + 1.0)
        else:
            better = cur > self.best + self.threshold
        if better:
            self.best, self.num_bad_epochs = cur, 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            scaled = self.lr * self.factor
            new = scaled if scaled > self.min_lr else self.min_lr
            if self.lr - new > self.eps:
                self.lr = new
                self.num_reductions += 1
            self.cooldown_counter = self.cooldown
            self.num_bad_epochs = 0

    def snapshot(self):
        """(lr bits, best bits, counters): NaN-proof bit-for-bit comparison."""
        return (np.float64(self.lr).tobytes(), np.float64(self.best).tobytes(), self.num_bad_epochs, self.cooldown_counter,
                self.last_epoch)


def torch_snapshot(sched, group=0):
    """The same tuple from a torch.optim.lr_scheduler.ReduceLROnPlateau."""
    return (np.float64(sched.optimizer.param_groups[group]["lr"]).tobytes(), np.float64(sched.best).tobytes(),
            sched.num_bad_epochs, sched.cooldown_counter, sched.last_epoch)


def metric32(seq):
    """The sequence as the float32 values a device metric holds (what both sides of a comparison are fed)."""
    return [float(np.float32(v)) for v in seq]


def grad_norm(arrays):
    """float64 sqrt(sum g^2) over a list of numpy arrays."""
    return math.sqrt(sum(float(np.sum(np.asarray(a, dtype=np.float64) ** 2)) for a in arrays))


def clip_coef32(norm32, max_norm):
    """torch's clip coefficient in float32 from a float32 norm: clamp(max_norm / (norm + 1e-6), max=1) -- NaN stays NaN."""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6))
    return c if (np.isnan(c) or c <= np.float32(1.0)) else np.float32(1.0)
