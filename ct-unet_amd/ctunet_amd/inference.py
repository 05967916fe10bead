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

Mirrored passes, ensembles and uncertainty (pinned; ``tests/tta_ref.py`` restates it in numpy).  A *contribution* is
c = (model m, flip mask f, tile p), ordered by m, then f (identity first, then the masks in the order given), then tile in
the z-major order above.  A flip mask has bit 0 = x, 1 = y, 2 = z; i^ = P_z-1-i if the z bit is set and i^ = i otherwise, y
and x alike.

    input     the net sees x~[c,i,j,k] = x_p[c,i^,j^,k^], x_p the zero-padded patch of tile p (the padding is mirrored with
              it; channels are never permuted)
    output    y_c[k,i,j,k] = y~[k,i^,j^,k^], the same involution, placed at the tile's position; only voxels inside the
              volume count
    weights   w_p = max((g_z g_y) g_x, 1e-3) from the tables above, indexed by the UN-mirrored patch-local position
    sums      float32, added in contribution order:  S0 += w,  S1_k += w y_k,  S2_k += w (y_k y_k)  (variance only),
              SH += w h(y)  (mutual information only); the second head of an SP net shares the first head's S0
    h(y)      = -sum_k q_k ln q_k / ln K,  q_k = max(y_k, 0) / sum_j max(y_j, 0);  h = 0 for a zero sum, 0 ln 0 = 0
    finalize  probs = S1 / S0 (0 where S0 == 0), labels = first argmax, variance_k = max(S2_k / S0 - probs_k^2, 0),
              entropy = h(probs), mutual_information = max(entropy - SH / S0, 0); uncovered voxels give 0 everywhere

The variance is the raw-moment form: both terms carry the rounding of their float32 sums, so it has a cancellation floor
of about (n + 3) 2^-22 max(y^2) for n contributions per voxel, below which it reads as noise or 0.  No atomics, gather
kernels, fixed order: bit-equal between eager and graph mode and between two calls.
"""
from __future__ import annotations

import weakref
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops
from .tiling import tile_starts

WEIGHT_FLOOR = 1e-3
MAX_BATCH = 64            # ctu_window_accumulate's limit on patches per launch
BLENDS = ("gaussian", "constant")
FLIP_BITS = {"x": 1, "y": 2, "z": 4}
STATISTICS = ("entropy", "variance", "mutual_information")

Int3 = Tuple[int, int, int]


@dataclass
class Prediction:
    """probs: float32 [K,D,H,W] blended head output (a tuple of two [2,D,H,W] for the two-output SP heads);
    labels: uint8 [D,H,W] first argmax over K (a tuple for the SP heads), None when not requested;
    uncertainty: None, or a dict from each requested statistic to float32 [K,D,H,W] ("variance") or [D,H,W] ("entropy",
    "mutual_information"), a tuple of two for the SP heads like probs."""
    probs: Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]
    labels: Optional[Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]]
    uncertainty: Optional[dict] = None


def parse_flips(flips) -> Tuple[int, ...]:
    """The masks (x = 1, y = 2, z = 4) of the mirrored passes, in order; the identity pass is not listed.  None / (): no
    mirrored pass; "all": the seven non-empty axis sets in ascending mask order (x, y, yx, z, zx, zy, zyx); otherwise a
    sequence of non-empty strings over "zyx" without a repeated letter, no two naming the same axis set."""
    if flips is None:
        return ()
    if flips == "all":
        return tuple(range(1, 8))
    if not isinstance(flips, (tuple, list)):          # (a bare "zy" would read as two passes: refused)
        raise ValueError(f'predict_volume: flips must be None, "all" or a sequence of axis strings, got {flips!r}')
    masks = []
    for f in flips:
        if not isinstance(f, str) or not f:
            raise ValueError(f"predict_volume: each flip is a non-empty string over 'zyx', got {f!r}")
        m = 0
        for a in f:
            if a not in FLIP_BITS:
                raise ValueError(f"predict_volume: flip {f!r} names an axis other than z, y, x")
            if m & FLIP_BITS[a]:
                raise ValueError(f"predict_volume: flip {f!r} repeats axis {a}")
            m |= FLIP_BITS[a]
        if m in masks:
            raise ValueError(f"predict_volume: flip {f!r} names the axes of an earlier entry")
        masks.append(m)
    return tuple(masks)


def parse_uncertainty(uncertainty, k: int) -> Tuple[str, ...]:
    """The requested statistics in the order of STATISTICS.  k: channels of a head (entropy needs at least 2)."""
    if uncertainty is None:
        return ()
    names = (uncertainty,) if isinstance(uncertainty, str) else uncertainty
    if not isinstance(names, (tuple, list)) or not names:
        raise ValueError(f"predict_volume: uncertainty must be None, one of {STATISTICS} or a tuple of them, "
                         f"got {uncertainty!r}")
    for n in names:
        if n not in STATISTICS:
            raise ValueError(f"predict_volume: unknown uncertainty {n!r} (one of {STATISTICS})")
    if len(set(names)) != len(names):
        raise ValueError(f"predict_volume: uncertainty {uncertainty!r} names a statistic twice")
    if k < 2 and ("entropy" in names or "mutual_information" in names):
        raise ValueError(f"predict_volume: entropy and mutual_information need at least 2 output channels, the model has {k}")
    return tuple(n for n in STATISTICS if n in names)


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


def _models(model_or_models) -> list:
    """One model or a non-empty list / tuple of them: all ctunet_amd models on one device with equal in_ch, out_ch,
    head_mode and number of levels."""
    if isinstance(model_or_models, (list, tuple)):
        models = list(model_or_models)
        if not models:
            raise ValueError("predict_volume: an empty list of models")
    else:
        models = [model_or_models]
    sig = None
    for m in models:
        s = (_levels(m), m._plan.in_ch, m._plan.out_ch, m._plan.head_mode, next(m.parameters()).device)
        if sig is None:
            sig = s
        elif s != sig:
            raise ValueError("predict_volume: the models of an ensemble must share the device, in_ch, out_ch, head_mode and "
                             f"number of levels; got (levels, in_ch, out_ch, head_mode, device) = {sig} and {s}")
    return models


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


def _head_channels(model) -> int:
    return 2 if model._plan.head_mode != 0 else model._plan.out_ch


class _Window:
    """Device state of one predict_volume call: the volume, the accumulators, the batch plan and the step
    extract -> eval forward -> accumulate of one model.  Everything a step reads that changes between batches and passes
    sits in ``meta`` (device int32 [4B+4]: coords | valid | box | flip word), written by one device copy before the step,
    so the step can be captured once per model and replayed for every (flip, batch).

    ``plain`` (no mirrored pass, no statistic): the accumulation is ``ctu_window_accumulate``, the launches of a call
    without the new arguments; otherwise ``ctu_window_accumulate_flip`` blends every pass, the identity included."""

    def __init__(self, model, vol: torch.Tensor, patch: Int3, overlap: Int3, batch: int, blend: str,
                 sigma_scale: float, dev: torch.device, masks: Tuple[int, ...] = (), stats: Tuple[str, ...] = ()):
        shape = tuple(int(s) for s in vol.shape[1:])
        tiles = tile_grid(shape, patch, overlap)
        b = min(batch, tiles.shape[0])
        if b > MAX_BATCH:
            raise ValueError(f"predict_volume: batch {batch} above the kernel's limit of {MAX_BATCH}")
        self.patch, self.shape, self.batch, self.dev = patch, shape, b, dev
        self.plan = plan_batches(tiles, b, shape, patch)
        self.plain, self.stats = not masks and not stats, stats
        self.holders = weakref.WeakSet()          # the models whose captured step works on this window (graph mode)
        self.set_masks(masks)
        self.meta = torch.empty(4 * b + 4, dtype=torch.int32, device=dev)
        self.coords = self.meta[:3 * b].view(b, 3)
        self.valid = self.meta[3 * b:4 * b]
        self.box = self.meta[4 * b:4 * b + 3]
        self.flip = self.meta[4 * b + 3:]
        self.tables = tuple(torch.from_numpy(t).to(dev) for t in window_tables(patch, blend, sigma_scale))
        self.two = model._plan.head_mode != 0
        k, heads = _head_channels(model), 2 if self.two else 1
        self.vol = vol
        self.nums = [torch.zeros((k,) + shape, dtype=torch.float32, device=dev) for _ in range(heads)]
        self.wsum = torch.zeros(shape, dtype=torch.float32, device=dev)
        # accumulators exist only for what was asked for: S2 for the variance, SH for the mutual information
        self.sqs = [torch.zeros_like(n) for n in self.nums] if "variance" in stats else [None] * heads
        self.shs = [torch.zeros_like(self.wsum) for _ in self.nums] if "mutual_information" in stats else [None] * heads

    def set_masks(self, masks: Tuple[int, ...]) -> None:
        """all_meta int32 [passes, nb, 4B+4]: the plan's word block of every batch with the pass's flip word appended."""
        m = self.plan.meta()
        passes = (0,) + tuple(masks)
        full = np.empty((len(passes),) + m.shape[:1] + (m.shape[1] + 1,), np.int32)
        full[:, :, :-1] = m
        full[:, :, -1] = np.asarray(passes, np.int32)[:, None]
        self.all_meta = torch.from_numpy(full).to(self.dev)

    @property
    def n_passes(self) -> int:
        return self.all_meta.shape[0]

    @property
    def n_batches(self) -> int:
        return self.all_meta.shape[1]

    def load(self, i: int, f: int = 0) -> None:
        self.meta.copy_(self.all_meta[f, i])

    def step(self, model) -> None:
        x = ops.extract_patches_flip(self.vol, self.coords, self.patch, self.flip)
        out = model(x)
        outs = out if isinstance(out, tuple) else (out,)
        for j, (y, num) in enumerate(zip(outs, self.nums)):
            ws = self.wsum if j == 0 else None
            if self.plain:
                ops.window_accumulate(y, self.coords, self.valid, self.box, self.tables, WEIGHT_FLOOR, self.plan.extent,
                                      num, ws)
            else:
                ops.window_accumulate_flip(y, self.coords, self.valid, self.box, self.flip, self.tables, WEIGHT_FLOOR,
                                           self.plan.extent, num, ws, self.sqs[j], self.shs[j])

    def reset(self) -> None:
        for n in self.nums + self.sqs + self.shs:
            if n is not None:
                n.zero_()
        self.wsum.zero_()


def _param_ptrs(model) -> Tuple[int, ...]:
    return tuple(t.data_ptr() for t in model.parameters()) + tuple(t.data_ptr() for t in model.buffers())


def predict_volume(model_or_models, volume: torch.Tensor, patch=192, overlap=48, batch: int = 2, blend: str = "gaussian",
                   sigma_scale: float = 0.125, labels: bool = True, graph: bool = False, flips=None,
                   uncertainty=None) -> Prediction:
    """Blended whole-volume prediction of a model (any ctunet_amd model class, in its current ``set_precision``) or of an
    ensemble: a non-empty list / tuple of models on one device with equal in_ch, out_ch, head_mode and levels, each in its
    own precision.

    volume: float32 [C,D,H,W] or [1,C,D,H,W] of any spatial size, on the model's GPU or on the CPU (copied once).
    patch / overlap: ints or 3-tuples; patch divisible by 2^levels of the model (16 for the 4-level nets, 32 for
    UNet5b2i3o / UNetSPSmall), 0 <= overlap < patch.  Tiles: ``tiling.tile_starts`` per axis, z-major (an axis shorter
    than the patch gets one zero-padded tile).  batch: patches per forward; a partial last batch is padded with slots
    flagged invalid, so every batch has the same launch shape.  blend / sigma_scale: the rule of the module docstring,
    w = max(g_z*g_y*g_x, 1e-3), g_a(i) = exp(-(i-(P_a-1)/2)^2 / (2 (sigma_scale P_a)^2)), or w = 1 for "constant";
    out = sum_c w_c y_c / sum_c w_c over the contributions in order.  labels: also return the first argmax over K as uint8.
    flips: test-time mirroring.  None or (): the identity pass only; "all": the seven mirrored passes x, y, yx, z, zx, zy,
    zyx after it; or a sequence of strings over "zyx" such as ("x", "zy"), one mirrored pass each in the order given.  A
    pass mirrors each patch on the way into the net and its output on the way into the blend.
    uncertainty: None, "entropy", "variance", "mutual_information" or a tuple of them: per-voxel statistics over the
    contributions (models x passes x overlapping tiles; a single pass has the overlapping tiles only), returned in
    ``Prediction.uncertainty``.  variance [K,D,H,W] is the weighted variance of each channel, entropy [D,H,W] the
    normalised entropy of the blended probabilities, mutual_information [D,H,W] that entropy minus the weighted mean
    entropy of the contributions; the last two need K >= 2.
    graph: capture one batch step (extract -> eval forward -> accumulate) per model on the first call and replay it for
    every pass and batch; the capture is kept on the model and reused by later calls of the same volume shape and
    arguments, whichever flips they run.  Bit-equal to graph=False.

    The models run in eval mode for the call (their modes are restored afterwards, also on an exception); no parameter or
    BatchNorm buffer changes.  Raises ValueError on bad arguments before anything is launched."""
    models = _models(model_or_models)
    volume, patch, overlap = _validate(models[0], volume, patch, overlap, batch, blend, sigma_scale)
    masks = parse_flips(flips)
    stats = parse_uncertainty(uncertainty, _head_channels(models[0]))
    dev = next(models[0].parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("predict_volume: the model runs on the MI355X only (call .to('cuda') first)")
    was_training = [m.training for m in models]
    try:
        for m in models:
            m.eval()
        with torch.no_grad():
            if graph:
                win = _graphed(models, volume, patch, overlap, batch, blend, sigma_scale, dev, masks, stats)
            else:
                win = _Window(models[0], volume.to(dev).contiguous(), patch, overlap, batch, blend, sigma_scale, dev, masks,
                              stats)
                for m in models:
                    for f in range(win.n_passes):
                        for i in range(win.n_batches):
                            win.load(i, f)
                            win.step(m)
            return _finalize(win, labels, in_place=not graph)
    finally:
        for m, t in zip(models, was_training):
            m.train(t)


def _graphed(models, volume, patch, overlap, batch, blend, sigma_scale, dev, masks, stats) -> _Window:
    """One captured step per model, kept on the model as (key, engine, window, graph); the models of an ensemble share the
    window.  The key covers what changes the captured launches -- the statistics accumulated, and whether the mirrored
    accumulation runs at all -- not which flips are run: those are words of the window's device table."""
    plain = not masks and not stats
    base = (tuple(volume.shape), patch, overlap, batch, blend, float(sigma_scale), str(dev))
    keys = [base + (_param_ptrs(m),) + (() if plain else (stats,)) for m in models]
    caches = [m.__dict__.get("_window_graph") for m in models]
    if all(c is not None and c[0] == k and c[1] is m._engine() and c[2] is caches[0][2]
           for c, k, m in zip(caches, keys, models)):
        win = caches[0][2]
        win.vol.copy_(volume)
        win.reset()
        win.set_masks(masks)
    else:
        # one capture per model: free the old ones first, also those of models outside this call that share a window about
        # to lose a member (no model keeps a volume copy and accumulators it can no longer hit)
        for c in caches:
            for h in list(c[2].holders) if c is not None else ():
                h.__dict__.pop("_window_graph", None)
        del caches, c
        vol = torch.empty(volume.shape, dtype=torch.float32, device=dev)
        vol.copy_(volume)
        win = _Window(models[0], vol, patch, overlap, batch, blend, sigma_scale, dev, masks, stats)
    for m, key in zip(models, keys):
        cache = m.__dict__.get("_window_graph")
        first = 0
        if cache is None or cache[2] is not win:
            # the first batch runs eagerly: it also creates the engine's packed weights and index maps outside the capture
            win.load(0)
            win.step(m)
            torch.cuda.synchronize(dev)
            g = torch.cuda.CUDAGraph()
            with ops.gc_paused(), torch.cuda.graph(g):
                win.step(m)
            m.__dict__["_window_graph"] = (key, m._engine(), win, g)
            win.holders.add(m)
            first = 1
        else:
            g = cache[3]
        for f in range(win.n_passes):
            for i in range(first if f == 0 else 0, win.n_batches):
                win.load(i, f)
                g.replay()
    return win


def _finalize(win: _Window, want_labels: bool, in_place: bool) -> Prediction:
    probs: List[torch.Tensor] = []
    labs: List[Optional[torch.Tensor]] = []
    unc = {n: [] for n in win.stats}
    for num, sq, sh in zip(win.nums, win.sqs, win.shs):
        p = num if in_place else torch.empty_like(num)
        lab = torch.empty(win.shape, dtype=torch.uint8, device=num.device) if want_labels else None
        if not win.stats:
            ops.window_finalize(num, win.wsum, p, lab)
        else:
            var = None if sq is None else (sq if in_place else torch.empty_like(sq))
            ent, mi = (torch.empty_like(win.wsum) if n in win.stats else None for n in ("entropy", "mutual_information"))
            ops.window_finalize_stats(num, win.wsum, p, lab, sq, sh, var, ent, mi)
            for n, t in (("variance", var), ("entropy", ent), ("mutual_information", mi)):
                if n in unc:
                    unc[n].append(t)
        probs.append(p)
        labs.append(lab)
    if win.two:
        return Prediction(tuple(probs), tuple(labs) if want_labels else None,
                          {n: tuple(t) for n, t in unc.items()} if unc else None)
    return Prediction(probs[0], labs[0], {n: t[0] for n, t in unc.items()} if unc else None)
