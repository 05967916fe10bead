"""Class-balanced random patch sampling for training on the MI355X (csrc/patch_sample.hip): a stated share of the patches
is centred on a voxel of a chosen label class, the rest start anywhere in the volume.  Three launches, no atomics and no
host sync, so index -> draw -> crop can be captured in a graph and draws new patches on every replay.  The reference has
no counterpart: its datasets feed whole volumes resized to the network size (ctunet/pytorch/datasets.py:89-112,195-235).

    sampler = PatchSampler((192, 192, 192), class_p=0.67, jitter=16, seed=7)
    index = sampler.index(labels)                 # uint8 [M, D, H, W]; once per dataset
    coords = sampler.draw(index)                  # int32 [P, 4] = (item, z0, y0, x0), on the device
    x = crop(volumes, coords, sampler.patch)      # [P, C, pd, ph, pw]

The index.  Labels are uint8 [M, D, H, W] (bool as its bytes), V = D H W < 2^31.  There are K classes, 1 <= K <= 4:
``classes=None`` is one class, the voxels != 0; otherwise class i holds the voxels == classes[i], each in 0..255.  The
index is counts int32 [M, K, ceil(V / 8192)]: the voxels of class i in each run ("chunk") of 8192 flat C-order indices
of item m.  It is built once for a static dataset and read by every draw.

The draw rule.  Patch j of a call is drawn from volume items[j]; seq = counter + j, with counter the sampler's device
sample counter, which the call then advances by P.  Philox4x32-10 is keyed by the sampler's 64-bit seed (lo, hi) with
counter (c0, stream, seq lo, seq hi), as in transforms.py.  Stream 0 gives
    c0 = 0 -> (r_class, r_k, -, -)
    c0 = 1 -> (r_z, r_y, r_x, -)
With draw_int(r, lo, span) = lo + ((r span) >> 32):
  * u = (r_class >> 8) 2^-24 in float64.
  * cum_i is the running sum of class_p, formed on the host in float64 in the order the classes are given.
  * Class i is chosen iff cum_{i-1} <= u < cum_i (cum_{-1} = 0).  Otherwise the patch is uniform.
  * Per axis a, with volume side n_a and patch side p_a: hi_a = max(0, n_a - p_a).
  * Uniform patch: s_a = draw_int(r_a, 0, hi_a + 1).
  * Class patch:
      - count is the number of voxels of class i in the item, taken from the index.
      - If count == 0 the patch falls back to the uniform rule, with the same words, and its record has fallback = 1
        (and keeps the class index i, count 0, k 0, centre -1).
      - Otherwise k = draw_int(r_k, 0, count) and the centre c is the k-th voxel of the class in C order
        (``np.argwhere(pred)[k]``).
      - j_a = draw_int(r_a, -J_a, 2 J_a + 1).
      - s_a = min(max(c_a - p_a // 2 + j_a, 0), hi_a).
  * Jitter bound: 0 <= J_a <= (p_a - 1) // 2.  Under it the centre voxel always lies inside the patch (checked
    exhaustively for all n, p < 30 in tests/test_patch_sample_cpu.py).
  * An item outside [0, M) is the caller's error and reads nothing: coords (-1, 0, 0, 0), record item -1, start
    (0, 0, 0), class -1, fallback 0, count 0, k 0, centre (-1, -1, -1).
Outputs: coords int32 [P, 4] = (item, z0, y0, x0) and records int32 [P, 12] = item, start z y x, class index (-1 =
uniform), fallback, count, k, centre z y x (-1 without one), 0.

The crop.  ``crop(src, coords, patch)`` gathers the window [z0, z0 + pd) x [y0, y0 + ph) x [x0, x0 + pw) of every
channel of src [Ms, C, D, H, W] item coords[p, 0] (Ms == 1: one source, e.g. an atlas, shared by every patch whose item is
>= 0) into out [P, Ctot, pd, ph, pw], channels [out_channel, out_channel + C).  src is uint8, int16 or float32; the output
is the source's dtype or float32, both exact.  coords may hold any int32: a voxel outside the volume, and every voxel of a
patch whose item is negative or (Ms > 1) >= Ms, reads as ``fill``.
"""
from __future__ import annotations

from numbers import Integral, Real
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _args, _lib
from .transforms import _DeviceRng, _seed

CHUNK = 8192               # CTU_PATCH_CHUNK of ctunet_hip.h
MAX_CLASSES = 4            # CTU_PATCH_MAX_CLASSES
RECORD = 12                # CTU_PATCH_RECORD

_PATCH = _args.Grid(side="sampling: every patch side must be at least 1, got {vals}",
                    voxels="sampling: a patch of {vals} has 2^31 voxels or more",
                    shape="sampling: patch must be a (pd, ph, pw) triple of integers, got {v!r}",
                    integers="sampling: patch must be a (pd, ph, pw) triple of integers, got {v!r}", shape_error=TypeError)
_CROP_DTYPES = (torch.uint8, torch.int16, torch.float32)


class PatchIndex(NamedTuple):
    """What ``PatchSampler.index`` returns: counts int32 [M, K, nchunks], the uint8 labels [M, D, H, W] they count (kept:
    the draw rescans one chunk of them), their shape (M, D, H, W) and the classes (None = nonzero)."""
    counts: torch.Tensor
    labels: torch.Tensor
    shape: Tuple[int, int, int, int]
    classes: Optional[Tuple[int, ...]]


def _int_array(values):
    return _lib.array(_lib.I, values)


def _classes(classes) -> Optional[Tuple[int, ...]]:
    if classes is None:
        return None
    try:
        cl = tuple(classes)
    except TypeError:
        raise TypeError(f"sampling: classes must be None or a sequence of labels, got {classes!r}") from None
    if any(isinstance(c, bool) or not isinstance(c, Integral) for c in cl):
        raise TypeError(f"sampling: classes must be integer labels, got {classes!r}")
    if not 1 <= len(cl) <= MAX_CLASSES:
        raise ValueError(f"sampling: between 1 and {MAX_CLASSES} classes are supported, got {len(cl)}")
    if any(not 0 <= c <= 255 for c in cl):
        raise ValueError(f"sampling: a class is a uint8 label in 0..255, got {classes!r}")
    return tuple(int(c) for c in cl)


def _jitter(jitter, patch) -> Tuple[int, int, int]:
    js = (jitter,) * 3 if isinstance(jitter, Integral) and not isinstance(jitter, bool) else jitter
    try:
        js = tuple(js)
    except TypeError:
        raise TypeError(f"sampling: jitter must be an integer or a (z, y, x) triple of integers, got {jitter!r}") from None
    if len(js) != 3 or any(isinstance(j, bool) or not isinstance(j, Integral) for j in js):
        raise TypeError(f"sampling: jitter must be an integer or a (z, y, x) triple of integers, got {jitter!r}")
    if any(not 0 <= j <= (p - 1) // 2 for j, p in zip(js, patch)):
        raise ValueError(f"sampling: jitter must satisfy 0 <= J <= (p - 1) // 2 per axis (so the centre stays inside the "
                         f"patch), got {jitter!r} for patch {patch}")
    return tuple(int(j) for j in js)


def _decode(records: torch.Tensor) -> List[Dict]:
    out = []
    for r in records.cpu().tolist():
        out.append({"item": r[0], "start": (r[1], r[2], r[3]), "class_index": r[4], "fallback": bool(r[5]), "count": r[6],
                    "k": r[7], "centre": (r[8], r[9], r[10])})
    return out


class PatchSampler:
    """Random patch origins on the device, a share ``class_p`` of them centred on a voxel of a class (module docstring).

    patch: (pd, ph, pw).  classes: None (one class: the voxels != 0) or up to 4 uint8 labels.  class_p: a number (the
    probability of the single class) or one number per class; their sum must be <= 1 and the remainder is the uniform
    share.  jitter: an integer or a (z, y, x) triple, 0 <= J <= (p - 1) // 2.  seed: 64-bit (None: fresh
    entropy)."""

    def __init__(self, patch, classes=None, class_p=0.67, jitter=0, seed: Optional[int] = None):
        self.patch = _args.grid(patch, _PATCH)
        self.classes = _classes(classes)
        k = 1 if self.classes is None else len(self.classes)
        if isinstance(class_p, Real) and not isinstance(class_p, bool):
            if k != 1:
                raise ValueError(f"sampling: class_p must give one probability per class ({k}), got {class_p!r}")
            ps = (class_p,)
        else:
            try:
                ps = tuple(class_p)
            except TypeError:
                raise TypeError(f"sampling: class_p must be a number or one number per class, got {class_p!r}") from None
            if any(isinstance(p, bool) or not isinstance(p, Real) for p in ps):
                raise TypeError(f"sampling: class_p must be a number or one number per class, got {class_p!r}")
            if len(ps) != k:
                raise ValueError(f"sampling: class_p must give one probability per class ({k}), got {class_p!r}")
        if any(not 0.0 <= float(p) <= 1.0 for p in ps):
            raise ValueError(f"sampling: every class probability must lie in [0, 1], got {class_p!r}")
        self.class_p = tuple(float(p) for p in ps)
        cum, run = [], 0.0
        for p in self.class_p:                     # float64 running sums, in the order the classes are given
            run = run + p
            cum.append(run)
        if run > 1.0:
            raise ValueError(f"sampling: the class probabilities sum to {run}, above 1; the remainder is the uniform share")
        self._cum = tuple(cum)
        self.jitter = _jitter(jitter, self.patch)
        self._rng = _DeviceRng(seed)
        self._records: Optional[torch.Tensor] = None
        self._items: Dict = {}

    @property
    def seed(self) -> int:
        return self._rng.seed

    def to(self, device) -> "PatchSampler":
        self._rng.to(device)
        return self

    def state_dict(self) -> Dict:
        c, _ = self._rng.state()
        return {"seed": self._rng.seed, "counter": c}

    def load_state_dict(self, sd: Dict) -> None:
        self._rng.seed = _seed(sd["seed"])
        self._rng.load(sd["counter"], None)

    @property
    def last_records(self) -> List[Dict]:
        """Per-patch records of the last draw (syncs): item, start, class_index (-1 = uniform), fallback, count, k, centre."""
        if self._records is None:
            raise RuntimeError("ctunet_amd: the sampler has not drawn yet")
        return _decode(self._records)

    def index(self, labels: torch.Tensor) -> PatchIndex:
        """Count the voxels of every class per chunk of labels uint8 / bool [M, D, H, W] on the GPU: one streaming read."""
        if not isinstance(labels, torch.Tensor):
            raise TypeError(f"sampling: labels must be a torch.Tensor, got {type(labels).__name__}")
        if labels.dtype not in (torch.uint8, torch.bool):
            raise TypeError(f"sampling: labels must be uint8 (or bool), got {labels.dtype}")
        if labels.dim() != 4 or labels.numel() == 0:
            raise ValueError(f"sampling: labels must be a non-empty [M, D, H, W] tensor, got {tuple(labels.shape)}")
        m, d, h, w = labels.shape
        v = d * h * w
        if v >= 1 << 31 or m > 65535:
            raise ValueError(f"sampling: {m} volumes of {d}x{h}x{w} voxels (at most 65535 of fewer than 2^31 supported)")
        _lib.check_device("sampling: labels must live on the GPU (MI355X); this path has no CPU fallback", labels)
        labels = _lib.as_bytes(labels)
        k = 1 if self.classes is None else len(self.classes)
        counts = torch.empty((m, k, -(-v // CHUNK)), dtype=torch.int32, device=labels.device)
        with _lib.on(labels.device) as run:
            run("ctu_patch_index", labels.data_ptr(), m, v, k, _int_array(self.classes), counts.data_ptr())
        return PatchIndex(counts, labels, (m, d, h, w), self.classes)

    def _default_items(self, m: int, per: int, device) -> torch.Tensor:
        key = (m, per, device)
        if key not in self._items:
            flat = torch.arange(m * per, dtype=torch.int32, device=device)
            self._items[key] = torch.div(flat, per, rounding_mode="floor")     # 0 .. 0, 1 .. 1, ...: no host sync
        return self._items[key]

    def draw(self, index: PatchIndex, patches_per_volume: int = 1, items=None,
             coords: Optional[torch.Tensor] = None) -> torch.Tensor:
        """coords int32 [P, 4] = (item, z0, y0, x0) on the device.  items=None: ``patches_per_volume`` patches from every
        volume of the index, in order (P = M patches_per_volume).  items: a host sequence (validated against [0, M)) or a
        device int32 tensor (read by the kernel; an entry outside [0, M) gives item -1).  coords: caller-supplied output."""
        if not isinstance(index, PatchIndex):
            raise TypeError(f"sampling: index must be what PatchSampler.index returns, got {type(index).__name__}")
        if index.classes != self.classes:
            raise ValueError(f"sampling: the index counts classes {index.classes}, the sampler draws {self.classes}")
        m, d, h, w = index.shape
        dev = index.labels.device
        if items is None:
            if isinstance(patches_per_volume, bool) or not isinstance(patches_per_volume, Integral) or patches_per_volume < 1:
                raise ValueError(f"sampling: patches_per_volume must be a positive integer, got {patches_per_volume!r}")
            p = m * int(patches_per_volume)
        elif isinstance(items, torch.Tensor) and items.is_cuda:
            if items.dtype != torch.int32 or items.dim() != 1 or items.numel() == 0 or items.device != dev:
                raise ValueError(f"sampling: device items must be a non-empty int32 [P] tensor on {dev}")
            items = items.contiguous()
            p = items.numel()
        else:
            host = items.tolist() if isinstance(items, torch.Tensor) else list(items)
            if not host or any(isinstance(i, bool) or not isinstance(i, Integral) for i in host):
                raise TypeError(f"sampling: items must be a non-empty sequence of integers, got {items!r}")
            bad = [i for i in host if not 0 <= i < m]
            if bad:
                raise ValueError(f"sampling: items must lie in [0, {m}), got {bad[0]}")
            p = len(host)
            items = host
        _args.check_out(coords, (p, 4), torch.int32, dev, "sampling.draw")
        _lib.check_device("sampling: the index must live on the GPU (MI355X); this path has no CPU fallback",
                          index.labels, index.counts)
        if items is None:
            items = self._default_items(m, int(patches_per_volume), dev)
        elif not isinstance(items, torch.Tensor):
            items = torch.tensor(items, dtype=torch.int32).to(dev)
        self._rng.to(dev)
        if coords is None:
            coords = torch.empty((p, 4), dtype=torch.int32, device=dev)
        records = torch.empty((p, RECORD), dtype=torch.int32, device=dev)
        k = 1 if self.classes is None else len(self.classes)
        with _lib.on(dev) as run:
            run("ctu_patch_draw", index.labels.data_ptr(), index.counts.data_ptr(), m, d, h, w, k, _int_array(self.classes),
                items.data_ptr(), p, self._rng.counter.data_ptr(), self._rng.seed, _int_array(self.patch),
                _int_array(self.jitter), _lib.double_array(self._cum), coords.data_ptr(), records.data_ptr())
        self._records = records
        return coords


def _fill_ok(fill, dtype: torch.dtype) -> bool:
    if isinstance(fill, bool) or not isinstance(fill, Real):
        return False
    f = float(fill)
    if dtype == torch.float32:
        return f == f and float(torch.tensor(f, dtype=torch.float32)) == f
    lo, hi = (0, 255) if dtype == torch.uint8 else (-32768, 32767)
    return f == int(f) and lo <= f <= hi


def crop(src: torch.Tensor, coords: torch.Tensor, patch, *, fill=0, dtype: Optional[torch.dtype] = None,
         out: Optional[torch.Tensor] = None, out_channel: int = 0) -> torch.Tensor:
    """The windows of src [Ms, C, D, H, W] (uint8, int16 or float32; bool as its bytes) at coords int32 [P, 4] =
    (item, z0, y0, x0) -> [P, C, pd, ph, pw] of ``dtype`` (the source's, or float32), ``fill`` outside the volume.
    out: a caller-supplied [P, Ctot, pd, ph, pw] tensor of that dtype, of which channels [out_channel, out_channel + C) are
    written and the others left alone (image and atlas into the two channels of one network input)."""
    pd, ph, pw = _args.grid(patch, _PATCH)
    if not isinstance(src, torch.Tensor) or not isinstance(coords, torch.Tensor):
        raise TypeError("sampling.crop: src and coords must be tensors")
    sdt = torch.uint8 if src.dtype == torch.bool else src.dtype
    if sdt not in _CROP_DTYPES:
        raise TypeError(f"sampling.crop: src must be uint8, int16 or float32, got {src.dtype}")
    if src.dim() != 5 or src.numel() == 0:
        raise ValueError(f"sampling.crop: src must be a non-empty [Ms, C, D, H, W] tensor, got {tuple(src.shape)}")
    if coords.dtype != torch.int32 or coords.dim() != 2 or coords.shape[1] != 4 or coords.shape[0] == 0:
        raise ValueError(f"sampling.crop: coords must be int32 [P, 4] = (item, z0, y0, x0), got {coords.dtype} "
                         f"{tuple(coords.shape)}")
    odt = sdt if dtype is None else dtype
    if odt not in (sdt, torch.float32):
        raise TypeError(f"sampling.crop: dtype must be the source's ({sdt}) or float32, got {dtype}")
    if not _fill_ok(fill, odt):
        raise ValueError(f"sampling.crop: fill must be a number that {odt} holds exactly, got {fill!r}")
    ms, c, d, h, w = src.shape
    p = coords.shape[0]
    if isinstance(out_channel, bool) or not isinstance(out_channel, Integral) or out_channel < 0:
        raise ValueError(f"sampling.crop: out_channel must be a non-negative integer, got {out_channel!r}")
    if out is None:
        if out_channel != 0:
            raise ValueError("sampling.crop: out_channel needs out=")
        ctot = c
    else:
        if not isinstance(out, torch.Tensor):
            raise TypeError(f"sampling.crop: out must be a tensor, got {type(out).__name__}")
        ctot = out.shape[1] if out.dim() == 5 else c
        if ctot < out_channel + c:
            raise ValueError(f"sampling.crop: out must hold channels [{out_channel}, {out_channel + c}), got "
                             f"{tuple(out.shape)}")
        _args.check_out(out, (p, ctot, pd, ph, pw), odt, src.device, "sampling.crop")
    _lib.check_device("sampling.crop: src and coords must live on the GPU (MI355X); this path has no CPU fallback",
                      src, coords)
    if coords.device != src.device:
        raise ValueError(f"sampling.crop: coords are on {coords.device}, src on {src.device}")
    src, coords = _lib.as_bytes(src), coords.contiguous()
    if out is None:
        out = torch.empty((p, c, pd, ph, pw), dtype=odt, device=src.device)
    with _lib.on(src.device) as run:
        run("ctu_patch_crop", src.data_ptr(), _lib.DTYPE_CODE[sdt], ms, c, d, h, w, coords.data_ptr(), p, pd, ph, pw,
            float(fill), out.data_ptr(), _lib.DTYPE_CODE[odt], ctot, int(out_channel))
    return out
