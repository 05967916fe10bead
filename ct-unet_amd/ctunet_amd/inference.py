"""Whole-volume sliding-window inference with Gaussian blending.

``predict_volume`` turns a trained model and a CT volume of any size into blended probabilities and hard labels.  The
reference never predicts a volume larger than the network input: its datasets resize every volume to the network size on
the CPU (/root/reference/ctunet/pytorch/datasets.py:89-112,195-235).  Here the volume is tiled into patch-sized windows
(``tiling.tile_starts``, z-major, exactly the tiles of ``VolumeTiler.coords``), the windows are streamed through the eval
forward in fixed-size batches, and every batch is blended into whole-volume fp32 accumulators by one gather kernel
(``ctu_window_accumulate``); a last pass (``ctu_window_finalize``) divides and takes the first argmax.  Device memory is
the volume, the accumulators and the outputs plus one batch: the patches are never all materialised.

Blend rule (pinned; ``tests/test_sliding_window_*.py`` restate it):

    w(i, j, k) = max(g_z(i) * g_y(j) * g_x(k), 1e-3)       patch-local voxel (i, j, k), the same for every patch
    g_a(i)     = exp(-(i - (P_a - 1) / 2)^2 / (2 sigma_a^2)),   sigma_a = sigma_scale * P_a    ("gaussian", peak 1)
    g_a(i)     = 1                                                                         ("constant": the plain mean)
    out(v)     = sum_p w_p(v) y_p(v) / sum_p w_p(v)     over the patches p covering voxel v, in tile order

The 1-D tables are formed in float64 and rounded to float32; the kernel forms the product in float32 in the order
(g_z * g_y) * g_x and accumulates in float32 in tile order, so results do not depend on the batch size up to the rounding
of that order (bit-equal across batch sizes in practice) and are bit-equal between eager and graph mode.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops
from .tiling import tile_starts

WEIGHT_FLOOR = 1e-3
MAX_BATCH = 64            # ctu_window_accumulate's limit on patches per launch
BLENDS = ("gaussian", "constant")

Int3 = Tuple[int, int, int]


@dataclass
class Prediction:
    """probs: float32 [K,D,H,W] blended head output (a tuple of two [2,D,H,W] for the two-output SP heads);
    labels: uint8 [D,H,W] first argmax over K (a tuple for the SP heads), None when not requested."""
    probs: Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]
    labels: Optional[Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]]


def _triple(v, name: str) -> Int3:
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        return (int(v),) * 3
    if isinstance(v, (tuple, list)) and len(v) == 3 and all(isinstance(a, (int, np.integer)) and not isinstance(a, bool)
                                                          for a in v):
        return tuple(int(a) for a in v)
    raise ValueError(f"predict_volume: {name} must be an int or a 3-tuple of ints, got {v!r}")


def window_tables(patch: Int3, blend: str = "gaussian", sigma_scale: float = 0.125) -> Tuple[np.ndarray, ...]:
    """The three 1-D float32 weight tables (g_z, g_y, g_x) of the blend rule in the module docstring."""
    out = []
    for p in patch:
        if blend == "constant":
            out.append(np.ones(p, np.float32))
            continue
        sigma = sigma_scale * p
        i = np.arange(p, dtype=np.float64)
        out.append(np.exp(-((i - (p - 1) / 2.0) ** 2) / (2.0 * sigma * sigma)).astype(np.float32))
    return tuple(out)


def window_weight(patch: Int3, blend: str = "gaussian", sigma_scale: float = 0.125) -> np.ndarray:
    """float32 [pd,ph,pw]: the per-patch weight exactly as the kernel forms it, max((g_z * g_y) * g_x, 1e-3) in float32."""
    gz, gy, gx = window_tables(patch, blend, sigma_scale)
    w = (gz[:, None, None] * gy[None, :, None]) * gx[None, None, :]
    return np.maximum(w, np.float32(WEIGHT_FLOOR))


def tile_grid(shape: Sequence[int], patch: Int3, overlap: Int3) -> np.ndarray:
    """int32 [T,3] patch origins (z0,y0,x0) in z-major order: the tiles of ``VolumeTiler.coords``."""
    zs, ys, xs = (tile_starts(int(s), p, o) for s, p, o in zip(shape, patch, overlap))
    return np.array([(z, y, x) for z in zs for y in ys for x in xs], dtype=np.int32).reshape(-1, 3)


@dataclass
class BatchPlan:
    """The tile list cut into batches of B slots.  coords int32 [nb,B,3], valid int32 [nb,B] (0 = padding slot of a partial
    last batch; its coords repeat the batch's first tile, so extraction stays in bounds), box int32 [nb,3] (origin of each
    batch's bounding box, x rounded down to a multiple of 4), extent (bz,by,bx): the largest box of any batch, clipped to
    the volume, bx a multiple of 4 -- the launch shape shared by every batch."""
    coords: np.ndarray
    valid: np.ndarray
    box: np.ndarray
    extent: Int3

    def meta(self) -> np.ndarray:
        """int32 [nb, 4B+3]: per batch coords | valid | box, the layout of the device word block a step reads."""
        nb = self.coords.shape[0]
        return np.concatenate([self.coords.reshape(nb, -1), self.valid, self.box], axis=1).astype(np.int32)


def plan_batches(tiles: np.ndarray, batch: int, shape: Sequence[int], patch: Int3) -> BatchPlan:
    t = tiles.shape[0]
    nb = -(-t // batch)
    coords = np.zeros((nb, batch, 3), np.int32)
    valid = np.zeros((nb, batch), np.int32)
    box = np.zeros((nb, 3), np.int32)
    ext = [1, 1, 4]
    for b in range(nb):
        tb = tiles[b * batch:(b + 1) * batch]
        n = tb.shape[0]
        coords[b, :n] = tb
        coords[b, n:] = tb[0]
        valid[b, :n] = 1
        lo = tb.min(axis=0)
        lo[2] -= lo[2] % 4
        hi = np.minimum(tb.max(axis=0) + np.asarray(patch), np.asarray(shape))
        box[b] = lo
        e = hi - lo
        e[2] = -(-e[2] // 4) * 4
        ext = [max(a, int(c)) for a, c in zip(ext, e)]
    return BatchPlan(coords, valid, box, tuple(ext))


def _levels(model) -> int:
    plan = getattr(model, "_plan", None)
    if plan is None:
        raise ValueError(f"predict_volume: {type(model).__name__} is not a ctunet_amd model")
    return len(plan.enc)


def _validate(model, volume, patch, overlap, batch, blend, sigma_scale):
    nlev = _levels(model)
    patch, overlap = _triple(patch, "patch"), _triple(overlap, "overlap")
    div = 1 << nlev
    for p, o in zip(patch, overlap):
        if p <= 0 or p % div:
            raise ValueError(f"predict_volume: patch {patch} must be positive and divisible by 2^levels = {div} "
                             f"for {type(model).__name__}")
        if not 0 <= o < p:
            raise ValueError(f"predict_volume: need 0 <= overlap < patch, got overlap {overlap} for patch {patch}")
    if blend not in BLENDS:
        raise ValueError(f"predict_volume: blend must be one of {BLENDS}, got {blend!r}")
    if blend == "gaussian" and not (isinstance(sigma_scale, (int, float)) and sigma_scale > 0):
        raise ValueError(f"predict_volume: sigma_scale must be positive, got {sigma_scale!r}")
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
        raise ValueError(f"predict_volume: batch must be an int >= 1, got {batch!r}")
    if not isinstance(volume, torch.Tensor):
        raise ValueError("predict_volume: volume must be a torch.Tensor")
    if volume.dim() == 5:
        if volume.shape[0] != 1:
            raise ValueError(f"predict_volume: a 5-D volume must be [1,C,D,H,W], got {tuple(volume.shape)}")
        volume = volume[0]
    if volume.dim() != 4:
        raise ValueError(f"predict_volume: volume must be [C,D,H,W] or [1,C,D,H,W], got {tuple(volume.shape)}")
    if volume.dtype != torch.float32:
        raise ValueError(f"predict_volume: volume must be float32, got {volume.dtype}")
    if volume.shape[0] != model._plan.in_ch:
        raise ValueError(f"predict_volume: {type(model).__name__} takes {model._plan.in_ch} input channels, "
                         f"the volume has {volume.shape[0]}")
    if min(volume.shape[1:]) < 1:
        raise ValueError(f"predict_volume: empty volume {tuple(volume.shape)}")
    return volume, patch, overlap


class _Window:
    """Device state of one predict_volume call: the volume, the accumulators, the batch plan and the step
    extract -> eval forward -> accumulate.  Everything a step reads that changes between batches sits in ``meta`` (device
    int32 [4B+3]), written by a device copy before the step, so the step can be captured once and replayed."""

    def __init__(self, model, vol: torch.Tensor, patch: Int3, overlap: Int3, batch: int, blend: str,
                 sigma_scale: float, dev: torch.device):
        shape = tuple(int(s) for s in vol.shape[1:])
        tiles = tile_grid(shape, patch, overlap)
        b = min(batch, tiles.shape[0])
        if b > MAX_BATCH:
            raise ValueError(f"predict_volume: batch {batch} above the kernel's limit of {MAX_BATCH}")
        self.model, self.patch, self.shape, self.batch = model, patch, shape, b
        self.plan = plan_batches(tiles, b, shape, patch)
        self.all_meta = torch.from_numpy(self.plan.meta()).to(dev)
        self.meta = torch.empty(self.all_meta.shape[1], dtype=torch.int32, device=dev)
        self.coords = self.meta[:3 * b].view(b, 3)
        self.valid = self.meta[3 * b:4 * b]
        self.box = self.meta[4 * b:]
        self.tables = tuple(torch.from_numpy(t).to(dev) for t in window_tables(patch, blend, sigma_scale))
        mp = model._plan
        self.two = mp.head_mode != 0
        k = 2 if self.two else mp.out_ch
        self.vol = vol
        self.nums = [torch.zeros((k,) + shape, dtype=torch.float32, device=dev) for _ in range(2 if self.two else 1)]
        self.wsum = torch.zeros(shape, dtype=torch.float32, device=dev)

    @property
    def n_batches(self) -> int:
        return self.all_meta.shape[0]

    def load(self, i: int) -> None:
        self.meta.copy_(self.all_meta[i])

    def step(self) -> None:
        x = ops.extract_patches(self.vol, self.coords, self.patch)
        out = self.model(x)
        outs = out if isinstance(out, tuple) else (out,)
        for j, (y, num) in enumerate(zip(outs, self.nums)):
            ops.window_accumulate(y, self.coords, self.valid, self.box, self.tables, WEIGHT_FLOOR, self.plan.extent, num,
                                  self.wsum if j == 0 else None)

    def reset(self) -> None:
        for n in self.nums:
            n.zero_()
        self.wsum.zero_()


def _param_ptrs(model) -> Tuple[int, ...]:
    return tuple(t.data_ptr() for t in model.parameters()) + tuple(t.data_ptr() for t in model.buffers())


def predict_volume(model, volume: torch.Tensor, patch=192, overlap=48, batch: int = 2, blend: str = "gaussian",
                   sigma_scale: float = 0.125, labels: bool = True, graph: bool = False) -> Prediction:
    """Blended whole-volume prediction of ``model`` (any ctunet_amd model class, in its current ``set_precision``).

    volume: float32 [C,D,H,W] or [1,C,D,H,W] of any spatial size, on the model's GPU or on the CPU (copied once).
    patch / overlap: ints or 3-tuples; patch divisible by 2^levels of the model (16 for the 4-level nets, 32 for
    UNet5b2i3o / UNetSPSmall), 0 <= overlap < patch.  Tiles: ``tiling.tile_starts`` per axis, z-major (an axis shorter
    than the patch gets one zero-padded tile).  batch: patches per forward; a partial last batch is padded with slots
    flagged invalid, so every batch has the same launch shape.  blend / sigma_scale: the rule of the module docstring,
    w = max(g_z*g_y*g_x, 1e-3), g_a(i) = exp(-(i-(P_a-1)/2)^2 / (2 (sigma_scale P_a)^2)), or w = 1 for "constant";
    out = sum_p w_p y_p / sum_p w_p in tile order.  labels: also return the first argmax over K as uint8.
    graph: capture one batch step (extract -> eval forward -> accumulate) on the first call and replay it for every batch;
    the capture is kept on the model and reused by later calls of the same volume shape and arguments.  Bit-equal to
    graph=False.

    The model runs in eval mode for the call (its mode is restored afterwards); no parameter or BatchNorm buffer changes.
    Raises ValueError on bad arguments before anything is launched."""
    volume, patch, overlap = _validate(model, volume, patch, overlap, batch, blend, sigma_scale)
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("predict_volume: the model runs on the MI355X only (call .to('cuda') first)")
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            if graph:
                win = _graphed(model, volume, patch, overlap, batch, blend, sigma_scale, dev)
            else:
                win = _Window(model, volume.to(dev).contiguous(), patch, overlap, batch, blend, sigma_scale, dev)
                for i in range(win.n_batches):
                    win.load(i)
                    win.step()
            return _finalize(win, labels, in_place=not graph)
    finally:
        model.train(was_training)


def _graphed(model, volume, patch, overlap, batch, blend, sigma_scale, dev) -> _Window:
    eng = model._engine()
    key = (tuple(volume.shape), patch, overlap, batch, blend, float(sigma_scale), str(dev), _param_ptrs(model))
    cache = model.__dict__.get("_window_graph")
    if cache is not None and cache[0] == key and cache[1] is eng:
        _, _, win, g = cache
        win.vol.copy_(volume)
        win.reset()
        first = 0
    else:
        model.__dict__.pop("_window_graph", None)          # (one capture per model: free the old one first)
        vol = torch.empty(volume.shape, dtype=torch.float32, device=dev)
        vol.copy_(volume)
        win = _Window(model, vol, patch, overlap, batch, blend, sigma_scale, dev)
        # the first batch runs eagerly: it also creates the engine's packed weights and index maps outside the capture
        win.load(0)
        win.step()
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with ops.gc_paused(), torch.cuda.graph(g):
            win.step()
        model.__dict__["_window_graph"] = (key, eng, win, g)
        first = 1
    for i in range(first, win.n_batches):
        win.load(i)
        g.replay()
    return win


def _finalize(win: _Window, want_labels: bool, in_place: bool) -> Prediction:
    probs: List[torch.Tensor] = []
    labs: List[Optional[torch.Tensor]] = []
    for num in win.nums:
        p = num if in_place else torch.empty_like(num)
        lab = torch.empty(win.shape, dtype=torch.uint8, device=num.device) if want_labels else None
        ops.window_finalize(num, win.wsum, p, lab)
        probs.append(p)
        labs.append(lab)
    if win.two:
        return Prediction(tuple(probs), tuple(labs) if want_labels else None)
    return Prediction(probs[0], labs[0])
