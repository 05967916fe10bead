"""CT preprocessing on the GPU: from a scanner's int16 Hounsfield volume to the binary skull that the networks, the
registration and the implant extraction take.  Gaussian filter, histogram, Otsu's threshold, a range test and their
composition (``csrc/preprocess.hip``), and the rank filters: median, percentile, grey minimum and maximum
(``csrc/rank_filter.hip``); no CPU fallback.

    smooth = gaussian_filter(scan, 1.0, spacing=(0.8, 0.45, 0.45))            # float32, sigma in mm
    skull = extract_skull(scan, 300, spacing=(0.8, 0.45, 0.45), sigma=0.5)    # uint8 0 / 1
    t = threshold_otsu(scan, range=(-200, 3000))                              # float64 0-dim DEVICE tensor, no sync
    mask = binarize(scan, t)                                                  # reads t on the device
    clean = median_filter(scan, 3)                                            # int16 in, int16 out: edges kept
    skull = extract_skull(scan, 300, median=3)                                # the median first, then the chain above
    lo, hi = minimum_filter(scan, 3), maximum_filter(scan, (1, 5, 5))         # grey erosion / dilation with a box

Every volume is contiguous ``[..., D, H, W]`` with all leading dimensions a batch; ``histogram`` and ``binarize`` take a
tensor of any shape.  Inputs are float32, int16 or uint8 and are converted in the kernel.  ``tests/preprocess_ref.py``
(the rank filters: ``tests/rank_ref.py``) restates each rule in numpy and every device result is bit-equal to it.

**gaussian_filter** (``scipy.ndimage.gaussian_filter`` up to float32 rounding):

- ``sigma`` is a number or a (z, y, x) triple; with ``spacing`` it is in the spacing's units,
  ``sigma_vox_a = sigma_a / spacing_a``.  Per axis the radius is ``R_a = int(truncate * sigma_vox_a + 0.5)`` (scipy's).
- Weights, in float64: ``p_k = exp(-0.5 k^2 / sigma_vox^2)`` for ``k = 0..R``,
  ``w_k = float32(p_k / (p_0 + 2 sum_{k>=1} p_k))``.  ``sigma = 0`` gives ``R = 0`` and ``w_0 = 1``: the identity.
- One axis: ``acc = w_0 v[i]``, then for ``k = 1..R`` in order ``acc = acc + w_k (v[i-k] + v[i+k])``; float32, each
  operation rounded on its own, no fused multiply-add.  The input is converted to float32 first; the axes go x, then y,
  then z.
- Outside the axis ``v`` reads, by ``mode``: ``"nearest"`` the clamped index; ``"reflect"`` scipy's reflect,
  ``d c b a | a b c d | d c b a`` with period ``2 n`` (also where ``R > n``); ``"constant"`` ``float32(cval)``.
- Limits: ``R_a <= 32``, every side ``<= 1024``, ``D * H * W < 2^31``.  Anything beyond raises.

**histogram** (``numpy.histogram`` with equal bins), int64 ``[bins]`` over the whole tensor, ``bins`` in 2..4096:

- ``range`` is ``(lo, hi)`` host numbers, a float64 ``[2]`` DEVICE tensor, or ``None``: the smallest and largest finite
  value, found on the device and read by the histogram kernel there (a tensor without a finite value counts nothing).
- In float64: ``hi == lo`` widens both by 0.5 (numpy's rule); ``scale = bins / (hi - lo)``; a value with
  ``lo <= v <= hi`` counts in bin ``min(floor((v - lo) * scale), bins - 1)``; values outside, and NaN, are not counted.

**threshold_otsu** (scikit-image's definition, restated: scikit-image is not a dependency and no parity is claimed), on the
counts ``h`` with ``N = sum h`` and ``S = sum k h_k``:

- exact int64 prefixes ``w1_k = sum_{j<=k} h_j`` and ``s1_k = sum_{j<=k} j h_j`` for ``k = 0..bins-2``;
- in float64 ``m1 = s1 / w1``, ``m2 = (S - s1) / (N - w1)``, ``var_k = (double(w1) double(N - w1)) ((m1 - m2) (m1 - m2))``,
  and ``var_k = 0`` where ``w1 = 0`` or ``w1 = N``;
- ``k*`` is the first maximum: 0 for a constant volume (every ``var_k`` is 0), the bin of the lower value for a volume of
  two values;
- the threshold is ``lo + (k* + 0.5) ((hi - lo) / bins)``, a float64 0-dim DEVICE tensor; foreground is ``x > threshold``.

On a head CT the full range separates air from the head; a range such as ``(-200, 3000)`` separates soft tissue from
bone (on a synthetic three-class volume the restatement gives -904 and 494 HU).

**binarize**: uint8 ``(x > lower) & (x <= upper)``, compared in float64; each bound a number or a 0-dim float64 DEVICE
tensor (Otsu's result, consumed without a synchronisation); ``upper=None`` is no upper bound.

**extract_skull**: ``gaussian_filter`` (skipped at ``sigma == 0``), ``binarize`` (``threshold="otsu"``: above Otsu's
threshold of the filtered volume over ``otsu_range``), ``postprocess.keep_largest_connected_component``
(``components=0`` skips it), ``postprocess.ball_closing`` when ``closing_radius > 0`` (in the units of ``spacing``).

**rank filters** (``median_filter``, ``percentile_filter``, ``rank_filter``, ``minimum_filter``, ``maximum_filter``;
``scipy.ndimage``'s functions of those names with a box ``size``), the result in the INPUT's dtype:

- ``size`` is an odd integer or a (z, y, x) triple of odd integers, each in 1..7: a box centred on the voxel.  Even sizes,
  sizes above 7, footprint arrays and ``origin`` are out of scope and raise.
- Key: every element maps to an unsigned key that preserves the order and is a bijection on its bits.  uint8: the value;
  int16: value + 32768; float32 with bits ``b``: ``~b`` if the sign bit is set, else ``b | 0x80000000``.
- Window: the ``n = sz sy sx`` elements around the output voxel; a position outside the volume is read through ``mode``,
  per axis, as in ``gaussian_filter`` (``"constant"`` reads ``cval``, which must be representable in the input's dtype: an
  integer in range for int16 and uint8, finite as a float32 for float32).  The default ``mode`` is ``"nearest"``, as for
  ``gaussian_filter``; scipy's default is ``"reflect"``.
- Output: the element whose key is the ``rank``-th smallest (0-based) of that multiset, with its own bits.  Equal keys
  mean equal bits, so ties cannot matter.
- float32: the key order is total, negative-sign NaNs < -inf < ... < -0 < +0 < ... < +inf < positive-sign NaNs.  That is the
  rule; parity with scipy is claimed for NaN-free input only, and by value (``==``), not by bits, where both zeros occur.
- Rank (scipy's arithmetic): median ``n // 2``; percentile ``p``: ``p += 100`` if ``p < 0``, then ``p`` must lie in
  [0, 100], ``p == 100`` gives ``n - 1``, otherwise ``int(float(n) * p / 100.0)``; ``rank_filter``: a negative rank counts
  from the end (``rank + n``), outside ``[-n, n)`` raises; minimum 0; maximum ``n - 1``.
- Limits: every side ``<= 1024``; ``out=`` may not share memory with the input (every output reads neighbours).
- Kernels: 3 x 3 x 3 selects in registers by sorting networks; rank 0 and ``n - 1`` run a separable running minimum /
  maximum; everything else searches the key bit by bit (``path_of``).  A block owns a ``TILE`` of (8, 4, 64) outputs.

**extract_skull** with ``median=m`` (``size`` rules; 0 and 1 skip it) runs ``median_filter(scan, m, mode="nearest")`` first.

No call synchronises with the host, so each can be captured into a graph (outputs and workspaces are ``torch.empty``
tensors, which a capture draws from the graph's pool); the only atomics add integers, so two calls are bit-equal.  Bad
arguments raise ``ValueError`` before anything is launched.
"""
from __future__ import annotations

import ctypes as C
import math
from numbers import Integral, Real
from typing import Optional

import numpy as np
import torch

from . import _args, _lib

MODES = ("nearest", "reflect", "constant")
MAX_RADIUS = 32              # CTU_GAUSS_MAX_RADIUS
MAX_SIDE = 1024
MAX_BINS = 4096              # CTU_HISTOGRAM_MAX_BINS
MAX_SIZE = 7                 # CTU_RANK_MAX_SIZE
TILE = {"fast3": (8, 4, 64), "separable": (8, 4, 64), "generic": (8, 4, 64)}   # CTU_RANK_TILE_Z, _Y, _X: outputs of a block
_DTYPES = (torch.float32, torch.int16, torch.uint8)
_NOT_NEGATIVE = _args.Triple(shape="{who}: {what} must be a number or a (z, y, x) triple, got {v!r}",
                             value="{who}: {what} must be finite and not negative, got {v!r}", sign=_args.NOT_NEGATIVE,
                             optional=False, tensors=False)
_POSITIVE = _NOT_NEGATIVE._replace(value="{who}: {what} must be finite and positive, got {v!r}", sign=_args.POSITIVE)
# MAX_SIDE^3 is below 2^31, so the sides bound the voxels too
_GRID = _args.Grid(side=f"{{who}}: every side may be at most {MAX_SIDE}, got {{vals}}", max_side=MAX_SIDE, max_voxels=None)
_ON_GPU = "{}: the input must live on the GPU; this path has no CPU fallback"


def _check_input(x, who: str, volume: bool) -> None:
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{who}: the input must be a tensor, got {type(x).__name__}")
    if x.dtype not in _DTYPES:
        raise ValueError(f"{who}: the input must be float32, int16 or uint8, got {x.dtype}")
    if volume and x.dim() < 3:
        raise ValueError(f"{who}: the input needs at least the three dimensions (D, H, W), got shape {tuple(x.shape)}")
    if x.numel() < 1:
        raise ValueError(f"{who}: the input is empty, got shape {tuple(x.shape)}")


def gaussian_weights(sigma_vox: float, truncate: float = 4.0) -> np.ndarray:
    """``w_0..w_R`` (float32) of one axis: the weights of the module docstring."""
    r = int(truncate * sigma_vox + 0.5)
    if r == 0:
        return np.ones(1, np.float32)
    k = np.arange(0, r + 1, dtype=np.float64)
    p = np.exp(-0.5 / (np.float64(sigma_vox) * np.float64(sigma_vox)) * k * k)
    return (p / (p[0] + 2.0 * p[1:].sum())).astype(np.float32)


def gaussian_filter(x: torch.Tensor, sigma, *, spacing=None, truncate: float = 4.0, mode: str = "nearest",
                    cval: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 Gaussian filter of ``x [..., D, H, W]`` (float32, int16 or uint8); the rule is the module docstring's."""
    who = "gaussian_filter"
    _check_input(x, who, True)
    sig = _args.triple(sigma, _NOT_NEGATIVE, who=who, what="sigma")
    if spacing is not None:
        sp = _args.triple(spacing, _POSITIVE, who=who, what="spacing")
        sig = tuple(s / q for s, q in zip(sig, sp))
    if isinstance(truncate, bool) or not isinstance(truncate, Real) or not math.isfinite(truncate) or truncate < 0:
        raise ValueError(f"{who}: truncate must be a finite number >= 0, got {truncate!r}")
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"{who}: mode must be one of {', '.join(MODES)}, got {mode!r}")
    if isinstance(cval, bool) or not isinstance(cval, Real) or not math.isfinite(C.c_float(float(cval)).value):
        raise ValueError(f"{who}: cval must be finite in float32, got {cval!r}")
    radius = tuple(int(float(truncate) * s + 0.5) if math.isfinite(float(truncate) * s) else MAX_RADIUS + 1 for s in sig)
    if any(r > MAX_RADIUS for r in radius):
        raise ValueError(f"{who}: the radius int(truncate * sigma + 0.5) of an axis may be at most {MAX_RADIUS} voxels, got "
                         f"{radius} (z, y, x) from sigma {sig} voxels")
    shape = _args.grid(x.shape[-3:], _GRID, who=who)
    _args.check_out(out, x.shape, torch.float32, x.device, who)
    _lib.check_device(_ON_GPU.format(who), x)
    weights = np.concatenate([gaussian_weights(s, float(truncate)) for s in sig])
    assert weights.size == sum(radius) + 3
    lib = _lib.load()
    n = x.numel() // (shape[0] * shape[1] * shape[2])
    src = x.contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    nbytes = int(lib.ctu_gaussian_ws_bytes(n, *shape, radius[0]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    with _lib.on(x.device) as run:
        run("ctu_gaussian_filter", src.data_ptr(), _lib.DTYPE_CODE[x.dtype], n, *shape, _lib.array(C.c_int, radius),
            _lib.float_array(weights.tolist()), MODES.index(mode), float(cval), out.data_ptr(),
            ws.data_ptr() if nbytes else None, what=who)
    return out


def _range_arg(rng, device, who: str):
    """(device tensor or None, lo, hi) of a ``range`` argument that is not None."""
    if isinstance(rng, torch.Tensor):
        if rng.dtype != torch.float64 or tuple(rng.shape) != (2,):
            raise ValueError(f"{who}: a range tensor must be float64 [2], got {rng.dtype} {tuple(rng.shape)}")
        if rng.device != device:
            raise ValueError(f"{who}: the range tensor lives on {rng.device}, the input on {device}: the kernel reads it "
                             f"from device memory")
        return rng.contiguous(), 0.0, 0.0
    try:
        lo, hi = rng
    except (TypeError, ValueError):
        raise ValueError(f"{who}: range must be (lo, hi), a float64 [2] device tensor or None, got {rng!r}") from None
    if any(isinstance(v, bool) or not isinstance(v, Real) or not math.isfinite(v) for v in (lo, hi)) or lo > hi:
        raise ValueError(f"{who}: range must be finite numbers with lo <= hi, got {rng!r}")
    return None, float(lo), float(hi)


def _check_bins(bins, who: str) -> int:
    if isinstance(bins, bool) or not isinstance(bins, Integral) or not 2 <= bins <= MAX_BINS:
        raise ValueError(f"{who}: bins must be an integer in 2..{MAX_BINS}, got {bins!r}")
    return int(bins)


def finite_range(x: torch.Tensor) -> torch.Tensor:
    """float64 ``[2]`` DEVICE tensor: the smallest and the largest finite value of ``x`` (``+inf, -inf`` without one)."""
    who = "finite_range"
    _check_input(x, who, False)
    _lib.check_device(_ON_GPU.format(who), x)
    lib = _lib.load()
    src = x.contiguous()
    rng = torch.empty(2, dtype=torch.float64, device=x.device)
    ws = torch.empty(int(lib.ctu_minmax_ws_bytes(src.numel())), dtype=torch.uint8, device=x.device)
    with _lib.on(x.device) as run:
        run("ctu_finite_minmax", src.data_ptr(), _lib.DTYPE_CODE[x.dtype], src.numel(), rng.data_ptr(), ws.data_ptr(), what=who)
    return rng


def _histogram(x, bins: int, rng, out, who: str):
    """The counts and the range they were taken over, as ``(hist, range tensor or None, lo, hi)``."""
    if rng is None:
        _lib.check_device(_ON_GPU.format(who), x)
        rt, lo, hi = finite_range(x), 0.0, 0.0
    else:
        rt, lo, hi = _range_arg(rng, x.device, who)
    _args.check_out(out, (bins,), torch.int64, x.device, who)
    _lib.check_device(_ON_GPU.format(who), x)
    src = x.contiguous()
    if out is None:
        out = torch.empty(bins, dtype=torch.int64, device=x.device)
    with _lib.on(x.device) as run:
        run("ctu_histogram", src.data_ptr(), _lib.DTYPE_CODE[x.dtype], src.numel(), bins,
            None if rt is None else rt.data_ptr(), lo, hi, out.data_ptr(), what=who)
    return out, rt, lo, hi


def histogram(x: torch.Tensor, bins: int = 256, range=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 ``[bins]`` counts of the whole tensor ``x`` over equal bins of ``range`` (module docstring)."""
    who = "histogram"
    _check_input(x, who, False)
    bins = _check_bins(bins, who)
    if range is not None:
        _range_arg(range, x.device, who)
    _args.check_out(out, (bins,), torch.int64, x.device, who)
    return _histogram(x, bins, range, out, who)[0]


def threshold_otsu(x: Optional[torch.Tensor] = None, *, hist: Optional[torch.Tensor] = None, bins: int = 256, range=None,
                   return_index: bool = False):
    """Otsu's threshold (module docstring) of ``x``, or of the counts ``hist`` (int64 ``[bins]``, taken over ``range``,
    which is required then).  A float64 0-dim DEVICE tensor; with ``return_index`` the pair ``(threshold, k*)``, ``k*`` an
    int64 0-dim DEVICE tensor."""
    who = "threshold_otsu"
    if (x is None) == (hist is None):
        raise ValueError(f"{who}: give the volume or hist=, not both and not neither")
    if hist is not None:
        if not isinstance(hist, torch.Tensor) or hist.dtype != torch.int64 or hist.dim() != 1:
            raise ValueError(f"{who}: hist must be an int64 [bins] tensor")
        bins = _check_bins(int(hist.shape[0]), who)
        if range is None:
            raise ValueError(f"{who}: hist= needs the range its counts were taken over")
        rt, lo, hi = _range_arg(range, hist.device, who)
        _lib.check_device(_ON_GPU.format(who), hist)
        h = hist.contiguous()
    else:
        _check_input(x, who, False)
        bins = _check_bins(bins, who)
        if range is not None:
            _range_arg(range, x.device, who)
        h, rt, lo, hi = _histogram(x, bins, range, None, who)
    thr = torch.empty((), dtype=torch.float64, device=h.device)
    idx = torch.empty((), dtype=torch.int64, device=h.device)
    with _lib.on(h.device) as run:
        run("ctu_threshold_otsu", h.data_ptr(), bins, None if rt is None else rt.data_ptr(), lo, hi, thr.data_ptr(),
            idx.data_ptr(), what=who)
    return (thr, idx) if return_index else thr


def _bound(b, device, what: str, who: str):
    """(device tensor or None, value) of a bound of ``binarize``."""
    if isinstance(b, torch.Tensor):
        if b.dtype != torch.float64 or b.numel() != 1:
            raise ValueError(f"{who}: a {what} tensor must hold one float64, got {b.dtype} {tuple(b.shape)}")
        if b.device != device:
            raise ValueError(f"{who}: the {what} tensor lives on {b.device}, the input on {device}: the kernel reads it "
                             f"from device memory")
        return b, 0.0
    if isinstance(b, bool) or not isinstance(b, Real) or math.isnan(b):
        raise ValueError(f"{who}: {what} must be a number or a 0-dim float64 device tensor, got {b!r}")
    return None, float(b)


def binarize(x: torch.Tensor, lower, upper=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 ``(x > lower) & (x <= upper)`` of the shape of ``x``; a bound is a number or a 0-dim float64 DEVICE tensor."""
    who = "binarize"
    _check_input(x, who, False)
    lt, lv = _bound(lower, x.device, "lower", who)
    ut, uv = (None, math.inf) if upper is None else _bound(upper, x.device, "upper", who)
    _args.check_out(out, x.shape, torch.uint8, x.device, who)
    _lib.check_device(_ON_GPU.format(who), x)
    src = x.contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    with _lib.on(x.device) as run:
        run("ctu_binarize", src.data_ptr(), _lib.DTYPE_CODE[x.dtype], src.numel(), None if lt is None else lt.data_ptr(), lv,
            None if ut is None else ut.data_ptr(), uv, out.data_ptr(), what=who)
    return out


def _box_size(size, who: str, what: str = "size"):
    """(sz, sy, sx) of a ``size`` argument: an odd integer or three of them, each in 1..MAX_SIZE."""
    if isinstance(size, Integral) and not isinstance(size, bool):
        vals = (size, size, size)
    else:
        try:
            vals = tuple(size)
        except TypeError:
            raise ValueError(f"{who}: {what} must be an odd integer or a (z, y, x) triple of them, got {size!r}") from None
        if len(vals) != 3 or any(isinstance(s, bool) or not isinstance(s, Integral) for s in vals):
            raise ValueError(f"{who}: {what} must be an odd integer or a (z, y, x) triple of them (no footprint arrays), got "
                             f"{size!r}")
    if any(s < 1 or s > MAX_SIZE or s % 2 == 0 for s in vals):
        raise ValueError(f"{who}: every {what} must be odd and lie in 1..{MAX_SIZE}, got {size!r}")
    return tuple(int(s) for s in vals)


def percentile_rank(percentile, n: int) -> int:
    """The rank ``scipy.ndimage.percentile_filter`` takes of ``n`` elements (module docstring)."""
    if isinstance(percentile, bool) or not isinstance(percentile, Real) or math.isnan(percentile):
        raise ValueError(f"percentile_filter: percentile must be a number, got {percentile!r}")
    p = percentile
    if p < 0.0:
        p += 100
    if p < 0 or p > 100:
        raise ValueError(f"percentile_filter: percentile must lie in [-100, 100], got {percentile!r}")
    return n - 1 if p == 100 else int(float(n) * p / 100.0)


def path_of(size, rank: int) -> str:
    """The kernel a filter of box ``size`` and ``rank`` (0-based, not negative) runs: ``"fast3"``, ``"separable"`` or
    ``"generic"``; each owns a ``TILE`` of outputs per block."""
    sz = _box_size(size, "path_of")
    n = sz[0] * sz[1] * sz[2]
    if rank in (0, n - 1):
        return "separable"
    return "fast3" if sz == (3, 3, 3) else "generic"


def _overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _rank_filter(x, size, rank_of, mode, cval, out, who: str) -> torch.Tensor:
    """The one call behind the five filters; ``rank_of(n)`` gives the 0-based rank or raises."""
    _check_input(x, who, True)
    sz = _box_size(size, who)
    n = sz[0] * sz[1] * sz[2]
    rank = rank_of(n)
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"{who}: mode must be one of {', '.join(MODES)}, got {mode!r}")
    if isinstance(cval, bool) or not isinstance(cval, Real):
        raise ValueError(f"{who}: cval must be a number, got {cval!r}")
    if x.dtype == torch.float32:
        if not math.isfinite(C.c_float(float(cval)).value):
            raise ValueError(f"{who}: cval must be finite in float32, got {cval!r}")
    else:
        lo, hi = (-32768, 32767) if x.dtype == torch.int16 else (0, 255)
        if not math.isfinite(cval) or cval != int(cval) or not lo <= cval <= hi:
            raise ValueError(f"{who}: cval must be an integer in {lo}..{hi} for {x.dtype}, got {cval!r}")
    shape = _args.grid(x.shape[-3:], _GRID, who=who)
    _args.check_out(out, x.shape, x.dtype, x.device, who)
    if out is not None and _overlap(x, out):
        raise ValueError(f"{who}: out shares memory with the input; every output reads its neighbours")
    _lib.check_device(_ON_GPU.format(who), x)
    src = x.contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    with _lib.on(x.device) as run:
        run("ctu_rank_filter", src.data_ptr(), _lib.DTYPE_CODE[x.dtype], x.numel() // (shape[0] * shape[1] * shape[2]), *shape,
            _lib.array(C.c_int, sz), rank, MODES.index(mode), float(cval), out.data_ptr(), None, what=who)
    return out


def median_filter(x: torch.Tensor, size=3, *, mode: str = "nearest", cval=0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The median (rank ``n // 2``) of the box ``size`` around every voxel of ``x [..., D, H, W]``, in the dtype of ``x``
    (module docstring, "rank filters").  ``scipy.ndimage.median_filter``, whose default mode is ``"reflect"``."""
    return _rank_filter(x, size, lambda n: n // 2, mode, cval, out, "median_filter")


def percentile_filter(x: torch.Tensor, percentile, size=3, *, mode: str = "nearest", cval=0,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The ``percentile`` (-100..100, scipy's rank arithmetic) of the box around every voxel (module docstring)."""
    return _rank_filter(x, size, lambda n: percentile_rank(percentile, n), mode, cval, out, "percentile_filter")


def rank_filter(x: torch.Tensor, rank, size=3, *, mode: str = "nearest", cval=0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The element of 0-based ``rank`` (negative: from the end) of the box around every voxel (module docstring)."""
    def rank_of(n):
        if isinstance(rank, bool) or not isinstance(rank, Integral) or not -n <= rank < n:
            raise ValueError(f"rank_filter: rank must be an integer in [-{n}, {n}) for a box of {n} elements, got {rank!r}")
        return int(rank) + (n if rank < 0 else 0)
    return _rank_filter(x, size, rank_of, mode, cval, out, "rank_filter")


def minimum_filter(x: torch.Tensor, size=3, *, mode: str = "nearest", cval=0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Grey erosion with a box: the smallest element of the box around every voxel (module docstring)."""
    return _rank_filter(x, size, lambda n: 0, mode, cval, out, "minimum_filter")


def maximum_filter(x: torch.Tensor, size=3, *, mode: str = "nearest", cval=0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Grey dilation with a box: the largest element of the box around every voxel (module docstring)."""
    return _rank_filter(x, size, lambda n: n - 1, mode, cval, out, "maximum_filter")


def extract_skull(scan: torch.Tensor, threshold, *, spacing=None, sigma=0.0, otsu_range=None, bins: int = 256,
                  components: int = 1, closing_radius: float = 0.0, median=0) -> torch.Tensor:
    """The binary skull (uint8 0 / 1) of a CT ``scan [D,H,W]`` or ``[N,D,H,W]``: smoothed by ``sigma`` (units of ``spacing``),
    ``> threshold`` (a number in the scan's units, or ``"otsu"`` over ``otsu_range``), reduced to its ``components`` largest
    components (0: all kept) and closed by a ball of ``closing_radius`` (module docstring).  ``threshold`` has no default:
    the Hounsfield value that counts as bone is the user's clinical choice.  ``median`` (an odd size or triple, 1..7; 0 or 1
    skips it) runs ``median_filter`` on the scan before everything else."""
    from . import postprocess
    who = "extract_skull"
    _check_input(scan, who, True)
    if scan.dim() not in (3, 4):
        raise ValueError(f"{who}: scan must be [D,H,W] or [N,D,H,W], got shape {tuple(scan.shape)}")
    otsu = isinstance(threshold, str)
    if otsu:
        if threshold != "otsu":
            raise ValueError(f"{who}: threshold must be a number or 'otsu', got {threshold!r}")
        if otsu_range is None:
            raise ValueError(f"{who}: threshold='otsu' needs otsu_range, e.g. (-200, 3000) to separate soft tissue from "
                             f"bone: over the full range Otsu separates air from the head")
        _range_arg(otsu_range, scan.device, who)
        bins = _check_bins(bins, who)
    elif isinstance(threshold, bool) or not isinstance(threshold, Real) or math.isnan(threshold):
        raise ValueError(f"{who}: threshold must be a number or 'otsu', got {threshold!r}")
    sig = _args.triple(sigma, _NOT_NEGATIVE, who=who, what="sigma")
    if isinstance(components, bool) or not isinstance(components, Integral) or not 0 <= components <= postprocess.MAX_COMPONENTS:
        raise ValueError(f"{who}: components must lie in 0..{postprocess.MAX_COMPONENTS}, got {components!r}")
    if (isinstance(closing_radius, bool) or not isinstance(closing_radius, Real) or not math.isfinite(closing_radius)
            or closing_radius < 0):
        raise ValueError(f"{who}: closing_radius must be a finite number >= 0, got {closing_radius!r}")
    if spacing is not None:
        _args.triple(spacing, _POSITIVE, who=who, what="spacing")
    med = None
    if not (isinstance(median, Integral) and not isinstance(median, bool) and median == 0):
        med = _box_size(median, who, "median")
        if med == (1, 1, 1):
            med = None
    v = scan
    if med is not None:
        v = scan = median_filter(scan, med, mode="nearest")
    if any(s > 0 for s in sig):
        v = gaussian_filter(scan, sig, spacing=spacing)
    else:
        _lib.check_device(_ON_GPU.format(who), scan)
    t = threshold_otsu(v, bins=bins, range=otsu_range) if otsu else threshold
    m = binarize(v, t)
    if components:
        m = postprocess.keep_largest_connected_component(m, num_components=int(components))
    if closing_radius > 0:
        m = postprocess.ball_closing(m, float(closing_radius), sampling=spacing)
    return m
