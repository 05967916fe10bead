"""Resampling of volumes between voxel grids and spacings on the GPU: the step between a scanner's grid and the
network's, in both directions.  A deterministic, separable, axis-aligned change of grid (``ctu_resample`` of
``csrc/resample.hip``); no CPU fallback.

    y = resample(x, size=(179, 230, 230))                              # to a grid
    y = resample(x, spacing=(0.8, 0.45, 0.45), new_spacing=1.0)        # to a spacing
    r = Resampler(x.shape[-3:], in_spacing=(0.8, 0.45, 0.45), out_spacing=1.0).to(x.device)
    y = r(x)                                                           # in grid -> out grid (r.out_shape, r.out_spacing)
    back = r.inverse(labels, mode="label_linear", num_classes=2)       # out grid -> in grid, exactly in_shape

``x`` has at least three dimensions; the last three are (D, H, W) and all leading ones are a batch.

The pinned rule (``tests/resample_ref.py`` restates it; it is ``scipy.ndimage.zoom(order=1, mode="nearest",
grid_mode=True)`` and torch's ``trilinear, align_corners=False`` up to float32 rounding, and its ``near`` table is torch's
``nearest-exact``, bit for bit).

Geometry, per axis, with ``n`` input and ``m`` output voxels, in float64:

- ``size`` alone: ``a = n / m``.
- ``spacing`` and ``new_spacing`` (a number or a (D, H, W) triple each): ``a = s_new / s`` and
  ``m = max(1, floor(n * s / s_new + 0.5))`` unless ``size`` is given as well.
- The inverse of a ``Resampler`` maps the out grid to ``in_shape`` with ``m / n`` in size mode, ``s / s_new`` in spacing mode.

Tables, per axis, of length ``m``, formed on the host in float64 and then rounded::

    src_j  = clip((j + 0.5) * a - 0.5, 0, n - 1)
    i0_j   = min(floor(src_j), max(n - 2, 0))     int32
    i1_j   = min(i0_j + 1, n - 1)
    w_j    = float32(src_j - i0_j)
    near_j = min(floor((j + 0.5) * a), n - 1)     int32

Modes:

- ``"nearest"``: ``out[k,j,i] = in[near_z[k], near_y[j], near_x[i]]``; bool, uint8, int16, int32, int64 or float32, the same
  dtype out.
- ``"linear"``: with ``lerp(p, q, w) = p + w * (q - p)``, every float32 subtraction, multiplication and addition rounded
  separately (no fused multiply-add), four lerps along x, then two along y, then one along z:
  ``c00 = lerp(in[z0,y0,x0], in[z0,y0,x1], wx)``, likewise ``c01`` (z0, y1), ``c10`` (z1, y0), ``c11`` (z1, y1); the result
  is ``lerp(lerp(c00, c01, wy), lerp(c10, c11, wy), wz)``.  float32, int16 (raw CT) or uint8 in, converted in the kernel;
  float32 out.
- ``"label_linear"``: for each class ``c`` in increasing order the linear rule runs on the 0/1 indicator ``in == c``; the
  output is the smallest ``c`` with the largest score.  bool, uint8 or int64 label maps with values in
  ``[0, num_classes)``, ``2 <= num_classes <= 16``; a voxel ``>= num_classes`` belongs to no class.  The same dtype out.  No
  one-hot or score volume is written to memory.

A call is one launch: no host synchronisation, no atomics, and with ``out=`` and a contiguous input no allocation, so it
can be captured into a graph; two calls are bit-equal.  A ``Resampler`` uploads its tables once (``.to(device)``, or the
first call on a device: do that before a capture); ``resample`` keeps the tables of its recent geometries.  D*H*W is
below 2^31 on either grid; offsets across the batch are 64-bit.

Affine resampling (``ctu_affine_resample`` of ``csrc/affine.hip``) moves a volume through a rigid or affine matrix: into the
frame of an atlas that ``registration.register`` found, and a result back out::

    y = affine_resample(x, out_to_in, out_shape, spacing=, origin=, out_spacing=, out_origin=, mode="linear", fill=0)

``out_to_in`` is a DEVICE float64 tensor ``[3,4]`` or ``[4,4]`` that maps world coordinates (z, y, x) of the OUTPUT grid to
world coordinates of the INPUT grid (the pull convention of ``scipy.ndimage.affine_transform``); the world coordinate of
voxel index ``k`` is ``origin + k * spacing`` per axis, as in ``mesh.extract_surface``.  The kernel reads the matrix from
device memory: a registration result feeds it without a host synchronisation, and a captured call follows later changes of
the tensor.  The pinned rule (``tests/affine_ref.py`` restates it), per output voxel with index ``idx``, in float64 with
every operation rounded on its own::

    w_a = out_origin_a + idx_a * out_spacing_a
    s_a = ((m_a0 * w_0 + m_a1 * w_1) + m_a2 * w_2) + m_a3
    u_a = (s_a - origin_a) / spacing_a

- ``"nearest"``: ``n_a = floor(u_a + 0.5)``; ``in[n]``, or ``fill`` where an ``n_a`` lies outside ``[0, size_a)`` or ``u`` is
  not finite.  uint8, int16 or float32, the same dtype out.
- ``"linear"``: ``i0_a = floor(u_a)``, ``w_a = float32(u_a - i0_a)``; the eight neighbours ``i0 + {0,1}^3``, one outside the
  volume reading as ``float32(fill)`` (scipy's ``mode="grid-constant"``); the lerps of the linear rule above, x then y then
  z.  Where a ``u_a`` lies outside ``[-1, size_a)`` (all eight neighbours outside) or is not finite the output is
  ``float32(fill)``.  float32, int16 or uint8 in, float32 out.
- ``"label_linear"``: the label rule above on those eight neighbours; one outside the volume carries the label ``fill``.
  uint8 (or bool) in and out.

One launch, no workspace, no synchronisation and with ``out=`` no allocation; every read is bounded whatever the matrix holds
(a NaN matrix gives ``fill`` everywhere).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from numbers import Integral, Real
from typing import Optional

import numpy as np
import torch

from . import _args, _lib, ops

MODES = ("nearest", "linear", "label_linear")
MAX_CLASSES = 16
_IN_DTYPES = {
    "nearest": (torch.bool, torch.uint8, torch.int16, torch.int32, torch.int64, torch.float32),
    "linear": (torch.float32, torch.int16, torch.uint8),
    "label_linear": (torch.bool, torch.uint8, torch.int64),
}
_MODE_CODE = {"nearest": ops.RESAMPLE_NEAREST, "linear": ops.RESAMPLE_LINEAR, "label_linear": ops.RESAMPLE_LABEL_LINEAR}
_GRID_SHAPE = "{who}: {what} must be a (D, H, W) triple of positive integers, got {v!r}"
_GRID = _args.Grid(shape=_GRID_SHAPE, integers=_GRID_SHAPE, side="{who}: every side of {what} must be >= 1, got {v!r}",
                   voxels="{who}: {what} must hold fewer than 2^31 voxels, got {v!r}", shape_error=TypeError)
_SPACING = _args.Triple(shape="{who}: {what} must be a positive number or a (D, H, W) triple, got {v!r}",
                        value="{who}: {what} must be positive and finite, got {v!r}", sign=_args.POSITIVE,
                        shape_error=TypeError, optional=False, tensors=False)
# the frame of an affine resampling: host (z, y, x) float64 triples; None stays None (the entry point's default)
_REAL = _args.Triple(shape="{who}: {what} must be a number or a (z, y, x) triple, got {v!r}",
                     value="{who}: {what} must be finite, got {v!r}", shape_error=TypeError)
_REAL_POSITIVE = _REAL._replace(value="{who}: {what} must be positive and finite, got {v!r}", sign=_args.POSITIVE)


def geometry(in_shape, size=None, spacing=None, new_spacing=None, who: str = "resample"):
    """``(in_shape, out_shape, a)`` of the module docstring's geometry: ``a`` the per-axis float64 scale of the tables."""
    n = _args.grid(in_shape, _GRID, who=who, what="the input grid")
    if (spacing is None) != (new_spacing is None):
        raise ValueError(f"{who}: spacing and new_spacing go together (with or without size); got only one of them")
    if size is None and spacing is None:
        raise ValueError(f"{who}: give size, or spacing and new_spacing")
    m = None if size is None else _args.grid(size, _GRID, who=who, what="size")
    if spacing is not None:
        s = _args.triple(spacing, _SPACING, who=who, what="spacing")
        t = _args.triple(new_spacing, _SPACING, who=who, what="new_spacing")
        a = tuple(tj / sj for sj, tj in zip(s, t))
        if m is None:
            m = _args.grid(tuple(max(1, int(math.floor(nj * sj / tj + 0.5))) for nj, sj, tj in zip(n, s, t)), _GRID,
                           who=who, what="the output grid")
    else:
        a = tuple(nj / mj for nj, mj in zip(n, m))
    return n, m, a


def axis_tables(n: int, m: int, a: float):
    """``(i0 int32, w float32, near int32)`` of one axis: the tables of the module docstring."""
    j = np.arange(m, dtype=np.float64)
    src = np.clip((j + 0.5) * np.float64(a) - 0.5, 0.0, float(n - 1))
    i0 = np.minimum(np.floor(src), float(max(n - 2, 0)))
    near = np.minimum(np.floor((j + 0.5) * np.float64(a)), float(n - 1))
    return i0.astype(np.int32), (src - i0).astype(np.float32), near.astype(np.int32)


def _check_call(x, mode, num_classes, who: str, dtypes=None):
    dtypes = _IN_DTYPES if dtypes is None else dtypes
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"{who}: mode must be one of {', '.join(MODES)}, got {mode!r}")
    if mode == "label_linear":
        if isinstance(num_classes, bool) or not isinstance(num_classes, Integral):
            raise TypeError(f"{who}: label_linear needs num_classes, an integer in 2..{MAX_CLASSES}, got {num_classes!r}")
        if not 2 <= num_classes <= MAX_CLASSES:
            raise ValueError(f"{who}: num_classes must lie in 2..{MAX_CLASSES}, got {num_classes!r}")
    elif num_classes is not None:
        raise ValueError(f"{who}: num_classes belongs to mode 'label_linear' only, got {num_classes!r} with mode {mode!r}")
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{who}: the input must be a tensor, got {type(x).__name__}")
    if x.dim() < 3:
        raise ValueError(f"{who}: the input needs at least the three dimensions (D, H, W), got shape {tuple(x.shape)}")
    if x.dtype not in dtypes[mode]:
        raise TypeError(f"{who}: mode {mode!r} takes {', '.join(str(d) for d in dtypes[mode])}, got {x.dtype}")


def _lead(x, who: str):
    """The leading dimensions of ``x [..., D, H, W]`` and the number of volumes they hold."""
    lead = tuple(x.shape[:-3])
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if n < 1:
        raise ValueError(f"{who}: the batch is empty, got shape {tuple(x.shape)}")
    return lead, n


class Resampler:
    """The tables of one change of grid, ``in_shape -> out_shape``, and of its inverse; uploaded once per device.

    ``out_shape`` alone, or ``in_spacing`` and ``out_spacing`` (with or without ``out_shape``).  ``r(x)`` maps the in grid
    to the out grid, ``r.inverse(y)`` the out grid to exactly ``in_shape``.  ``r.out_shape`` and ``r.out_spacing`` (None in
    size mode) say what the grid became."""

    def __init__(self, in_shape, out_shape=None, in_spacing=None, out_spacing=None, _who: str = "Resampler"):
        self.in_shape, self.out_shape, a = geometry(in_shape, out_shape, in_spacing, out_spacing, _who)
        spaced = in_spacing is not None
        self.in_spacing = _args.triple(in_spacing, _SPACING, who=_who, what="spacing") if spaced else None
        self.out_spacing = _args.triple(out_spacing, _SPACING, who=_who, what="new_spacing") if spaced else None
        if spaced:
            inv = tuple(s / t for s, t in zip(self.in_spacing, self.out_spacing))
        else:
            inv = tuple(m / n for n, m in zip(self.in_shape, self.out_shape))
        self.scale, self.inverse_scale = a, inv
        # host tables per direction: (i0, w, near), each the z, y and x table one after the other
        self._host = tuple(
            tuple(np.concatenate(t) for t in zip(*(axis_tables(n, m, s) for n, m, s in zip(src, dst, sc))))
            for src, dst, sc in ((self.in_shape, self.out_shape, a), (self.out_shape, self.in_shape, inv)))
        self._device = {}

    def to(self, device) -> "Resampler":
        """Upload the tables of both directions to ``device`` (once); returns self."""
        self._tables(torch.device(device))
        return self

    def _tables(self, device: torch.device):
        if device.type != "cuda":
            raise ValueError("Resampler: the tables live on the GPU; this path has no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._device.get(device)
        if t is None:
            t = self._device[device] = tuple(tuple(torch.from_numpy(h).to(device) for h in d) for d in self._host)
        return t

    def _run(self, x, direction: int, mode, num_classes, out, who: str):
        _check_call(x, mode, num_classes, who)
        src, dst = (self.in_shape, self.out_shape) if direction == 0 else (self.out_shape, self.in_shape)
        if tuple(x.shape[-3:]) != src:
            raise ValueError(f"{who}: the input's grid is {tuple(x.shape[-3:])}, this Resampler maps {src} -> {dst}")
        lead, n = _lead(x, who)
        out_dtype = torch.float32 if mode == "linear" else x.dtype
        _args.check_out(out, lead + dst, out_dtype, x.device, who, TypeError)
        _lib.check_device(f"{who}: the input must live on the GPU; this path has no CPU fallback", x)
        tables = self._tables(x.device)[direction]
        if out is None:
            out = torch.empty(lead + dst, dtype=out_dtype, device=x.device)
        with torch.cuda.device(x.device.index):                # the index spares torch the parsing of a device
            ops.resample(x.contiguous(), out, _MODE_CODE[mode], int(num_classes or 0), n, src, dst, tables)
        return out

    def __call__(self, x, mode: str = "linear", num_classes: Optional[int] = None, out=None) -> torch.Tensor:
        """``x [..., *in_shape]`` on the out grid."""
        return self._run(x, 0, mode, num_classes, out, "Resampler")

    def inverse(self, y, mode: str = "linear", num_classes: Optional[int] = None, out=None) -> torch.Tensor:
        """``y [..., *out_shape]`` back on the in grid: exactly ``in_shape``."""
        return self._run(y, 1, mode, num_classes, out, "Resampler.inverse")


@functools.lru_cache(maxsize=16)
def _cached(in_shape, size, spacing, new_spacing) -> Resampler:
    return Resampler(in_shape, size, spacing, new_spacing, _who="resample")


def _key(v):
    return v if v is None or isinstance(v, Real) else tuple(v)


def resample(x, size=None, *, spacing=None, new_spacing=None, mode: str = "linear", num_classes: Optional[int] = None,
             out=None) -> torch.Tensor:
    """``x [..., D, H, W]`` on the grid ``size``, or on the grid that ``spacing -> new_spacing`` gives (module docstring)."""
    _check_call(x, mode, num_classes, "resample")
    in_shape = tuple(int(s) for s in x.shape[-3:])
    geometry(in_shape, size, spacing, new_spacing, "resample")           # raises before the cache sees an unhashable value
    r = _cached(in_shape, _key(size), _key(spacing), _key(new_spacing))
    return r._run(x, 0, mode, num_classes, out, "resample")


_AFFINE_DTYPES = {
    "nearest": (torch.uint8, torch.int16, torch.float32),
    "linear": (torch.float32, torch.int16, torch.uint8),
    "label_linear": (torch.bool, torch.uint8),
}


def _check_matrix(m, device, who: str) -> torch.Tensor:
    if not isinstance(m, torch.Tensor) or m.dtype != torch.float64 or tuple(m.shape) not in ((3, 4), (4, 4)):
        raise TypeError(f"{who}: the matrix must be a float64 tensor [3,4] or [4,4], got "
                        f"{m.dtype if isinstance(m, torch.Tensor) else type(m).__name__} "
                        f"{tuple(m.shape) if isinstance(m, torch.Tensor) else ''}")
    if m.device != device:
        raise ValueError(f"{who}: the matrix lives on {m.device}, the volume on {device}: the kernel reads it from device memory")
    return m if m.is_contiguous() else m.contiguous()


def affine_resample(x, out_to_in, out_shape, *, spacing=None, origin=None, out_spacing=None, out_origin=None,
                    mode: str = "linear", num_classes: Optional[int] = None, fill=0, out=None) -> torch.Tensor:
    """``x [..., D, H, W]`` on the grid ``out_shape`` through the device matrix ``out_to_in`` (module docstring)."""
    who = "affine_resample"
    _check_call(x, mode, num_classes, who, _AFFINE_DTYPES)
    src = _args.grid(tuple(int(s) for s in x.shape[-3:]), _GRID, who=who, what="the input grid")
    dst = _args.grid(out_shape, _GRID, who=who, what="out_shape")
    sp = _args.triple(spacing, _REAL_POSITIVE, who=who, what="spacing")
    org = _args.triple(origin, _REAL, who=who, what="origin")
    osp = _args.triple(out_spacing, _REAL_POSITIVE, who=who, what="out_spacing")
    oorg = _args.triple(out_origin, _REAL, who=who, what="out_origin")
    if isinstance(fill, bool) or not isinstance(fill, Real):
        raise TypeError(f"{who}: fill must be a number, got {fill!r}")
    out_dtype = torch.float32 if mode == "linear" else x.dtype
    fillv = float(fill) + 0.0                                            # -0.0 -> 0.0
    if out_dtype == torch.float32:
        if not math.isfinite(fillv) or not math.isfinite(C.c_float(fillv).value):
            raise ValueError(f"{who}: fill must be finite in float32, got {fill!r}")
    else:
        lo, hi = (-32768, 32767) if out_dtype == torch.int16 else ((0, 1) if out_dtype == torch.bool else (0, 255))
        if fillv != math.floor(fillv) or not lo <= fillv <= hi:
            raise ValueError(f"{who}: fill must be an integer in {lo}..{hi} for {out_dtype}, got {fill!r}")
    lead, n = _lead(x, who)
    _args.check_out(out, lead + dst, out_dtype, x.device, who, TypeError)
    _lib.check_device(f"{who}: the input must live on the GPU; this path has no CPU fallback", x)
    m = _check_matrix(out_to_in, x.device, who)
    if out is None:
        out = torch.empty(lead + dst, dtype=out_dtype, device=x.device)
    with torch.cuda.device(x.device.index):                # the index spares torch the parsing of a device
        ops.affine_resample(_lib.as_bytes(x), _lib.as_bytes(out), _MODE_CODE[mode], int(num_classes or 0), n, src, dst, m,
                            sp, org, osp, oorg, fillv)
    return out


def deformable_resample(x, result, out_shape, *, spacing=None, origin=None, out_spacing=None, out_origin=None,
                        mode: str = "linear", num_classes: Optional[int] = None, fill=0, out=None) -> torch.Tensor:
    """``x [..., D, H, W]`` (fixed frame, grid ``spacing`` / ``origin``) pulled onto the moving-frame grid ``out_shape`` /
    ``out_spacing`` / ``out_origin`` through ``result`` (a ``registration.DeformableResult``): per output voxel the world
    coordinate ``w``, ``s = T(w) = M w + u(M w)``, then ``affine_resample``'s rule per mode from ``u_a = (s_a - origin_a) /
    spacing_a`` on; same dtypes, limits and fill.  With zero controls it is ``affine_resample(x, result.matrix, ...)`` bit
    for bit."""
    from . import registration
    who = "deformable_resample"
    _check_call(x, mode, num_classes, who, _AFFINE_DTYPES)
    src = _args.grid(tuple(int(s) for s in x.shape[-3:]), _GRID, who=who, what="the input grid")
    dst = _args.grid(out_shape, _GRID, who=who, what="out_shape")
    sp = _args.triple(spacing, _REAL_POSITIVE, who=who, what="spacing")
    org = _args.triple(origin, _REAL, who=who, what="origin")
    osp = _args.triple(out_spacing, _REAL_POSITIVE, who=who, what="out_spacing")
    oorg = _args.triple(out_origin, _REAL, who=who, what="out_origin")
    if isinstance(fill, bool) or not isinstance(fill, Real):
        raise TypeError(f"{who}: fill must be a number, got {fill!r}")
    out_dtype = torch.float32 if mode == "linear" else x.dtype
    fillv = float(fill) + 0.0                                            # -0.0 -> 0.0
    if out_dtype == torch.float32:
        if not math.isfinite(fillv) or not math.isfinite(C.c_float(fillv).value):
            raise ValueError(f"{who}: fill must be finite in float32, got {fill!r}")
    else:
        lo, hi = (-32768, 32767) if out_dtype == torch.int16 else ((0, 1) if out_dtype == torch.bool else (0, 255))
        if fillv != math.floor(fillv) or not lo <= fillv <= hi:
            raise ValueError(f"{who}: fill must be an integer in {lo}..{hi} for {out_dtype}, got {fill!r}")
    r = registration._check_result(result)
    lead, n = _lead(x, who)
    _args.check_out(out, lead + dst, out_dtype, x.device, who, TypeError)
    _lib.check_device(f"{who}: the input must live on the GPU; this path has no CPU fallback", x)
    if r.matrix.device != x.device:
        raise ValueError(f"{who}: the result lives on {r.matrix.device}, the volume on {x.device}: the kernel reads it from "
                         "device memory")
    if out is None:
        out = torch.empty(lead + dst, dtype=out_dtype, device=x.device)
    xin, xout = _lib.as_bytes(x), _lib.as_bytes(out)
    with _lib.on(x.device) as run:
        run("ctu_ffd_resample", xin.data_ptr(), ops.RESAMPLE_CODE[xin.dtype], _MODE_CODE[mode], int(num_classes or 0), n, *src,
            *dst, r.matrix.data_ptr(), r.control.data_ptr(),
            *registration._lattice_args(tuple(r.control.shape[1:]), r.control_spacing, r.box_origin), _lib.double_array(sp),
            _lib.double_array(org), _lib.double_array(osp), _lib.double_array(oorg), fillv, xout.data_ptr())
    return out
