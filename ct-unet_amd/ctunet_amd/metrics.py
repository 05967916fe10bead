"""Surface-distance metrics of segmentations on the GPU: HD, HD_p, ASSD, surface Dice (NSD) and hard Dice, with spacing.

Argument names follow monai's ``compute_*`` functions.  Everything is computed by ``ctu_surface_metrics``
(``csrc/surface.hip``): per (item, class, side) plane one edge pass and one exact distance transform, from which every
metric is derived.  Results are float32 ``[N, C']`` device tensors, C' = the scored classes (background dropped unless
``include_background``).

Definitions (the tests restate them on scipy in float64):

- **Surface** of a mask: ``mask & ~binary_erosion(mask)``, 6-neighbourhood, background outside the volume
  (``ctu_hausdorff`` / ``ops.hausdorff`` is the HD row of the same kernels on ``argmax(pred)``).
- **Directed distances** d(A->B): for each surface voxel of A, the Euclidean distance in physical units to the nearest
  surface voxel of B, i.e. ``scipy.ndimage.distance_transform_edt(~edges_B, sampling=spacing)`` at A's surface voxels.
  P = prediction, G = target.
- **HD** = ``max(max d(P->G), max d(G->P))``; ``directed=True``: ``max d(P->G)``.
- **HD_p** = ``max(q_p(d(P->G)), q_p(d(G->P)))`` (directed: the first term), q_p = numpy's default ("linear")
  percentile, in float64 from the two bracketing order statistics (found exactly on the device), rounded to float32.
  ``percentile=100`` equals HD exactly.
- **ASSD** (``symmetric=True``): sum of both directed distance sets / (|dP| + |dG|); otherwise the mean of d(P->G).
- **NSD** = ``(#{d(P->G) <= tau_c} + #{d(G->P) <= tau_c}) / (|dP| + |dG|)``.
- **Dice**: hard Dice ``2|P & G| / (|P| + |G|)`` of the masks, 1.0 when both are empty (as ``utilities.dice_coeff``).
- **Empty surfaces**: HD, HD_p and ASSD are NaN when either surface is empty; NSD is NaN when both are empty and 0 when
  exactly one is.  PARITY UNPINNED: monai is not available here and its conventions for these cases change between
  versions.

With unit spacing the squared distances are exact int32 integers; otherwise they are fp32 physical squared distances
``sum (k_i s_i)^2``.  Results are deterministic (integer counts, fixed-order float64 sums) and the launch sequence has no
host synchronisation, so a call can be captured into a CUDA/HIP graph.
"""
from __future__ import annotations

import math
from numbers import Real
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib

MAX_CLASSES = 16
MAX_SIDE = 1024
_ON_GPU = "metrics: inputs must live on the GPU; this path has no CPU fallback"
# rows of the kernel's output block
_DICE, _HD, _HD_DIR, _HDP, _HDP_DIR, _ASSD, _ASD_DIR, _NSD = range(8)


def _positive(v, what: str) -> float:
    if isinstance(v, bool) or not isinstance(v, Real):
        raise ValueError(f"{what} must be a real number, got {v!r}")
    v = float(v)
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"{what} must be positive and finite, got {v!r}")
    return v


def parse_spacing(spacing, n: int, what: str = "metrics: spacing") -> Optional[List[List[float]]]:
    """None -> None (unit spacing); one number, a (D, H, W) triple or N triples -> N lists of three positive floats.
    ``what`` names the argument in a refusal (``postprocess`` and ``mesh`` parse their own through this)."""
    if spacing is None:
        return None
    if isinstance(spacing, torch.Tensor):
        spacing = spacing.tolist()
    if isinstance(spacing, Real) and not isinstance(spacing, bool):
        s = _positive(spacing, what)
        return [[s, s, s] for _ in range(n)]
    if not isinstance(spacing, (list, tuple)) and not hasattr(spacing, "__len__"):
        raise ValueError(f"{what} must be a number, a 3-sequence or N 3-sequences, got {spacing!r}")
    items = list(spacing)
    if len(items) == 3 and all(isinstance(v, Real) for v in items):
        t = [_positive(v, what) for v in items]
        return [list(t) for _ in range(n)]
    if len(items) == n and all(hasattr(v, "__len__") and len(v) == 3 for v in items):
        return [[_positive(v, what) for v in t] for t in items]
    raise ValueError(f"{what} must be a number, a (D, H, W) triple or {n} such triples, got {spacing!r}")


def _check_metric(distance_metric) -> None:
    if distance_metric != "euclidean":
        raise ValueError(f"metrics: only distance_metric='euclidean' is supported, got {distance_metric!r}")


def _check_percentile(percentile) -> Optional[float]:
    if percentile is None:
        return None
    if isinstance(percentile, bool) or not isinstance(percentile, Real) or not (0.0 <= float(percentile) <= 100.0):
        raise ValueError(f"metrics: percentile must lie in [0, 100], got {percentile!r}")
    return float(percentile)


def _thresholds(values, cs: int, what: str) -> List[float]:
    if isinstance(values, Real) and not isinstance(values, bool):
        values = [values] * cs
    values = list(values)
    if len(values) != cs:
        raise ValueError(f"metrics: {what} needs one value per scored class ({cs}), got {len(values)}")
    out = []
    for v in values:
        if isinstance(v, bool) or not isinstance(v, Real) or not (math.isfinite(float(v)) and float(v) >= 0.0):
            raise ValueError(f"metrics: {what} must be finite and non-negative, got {v!r}")
        out.append(float(v))
    return out


def _dtype_code(t: torch.Tensor, allowed, what: str) -> int:
    if t.dtype not in allowed:
        raise ValueError(f"metrics: {what} must be one of {', '.join(str(a) for a in allowed)}, got {t.dtype}")
    return _lib.DTYPE_CODE[t.dtype]


def _check_sides(shape) -> None:
    if any(s <= 0 or s > MAX_SIDE for s in shape):
        raise ValueError(f"metrics: every side must lie in [1, {MAX_SIDE}], got {tuple(shape)}")


def _run(a: torch.Tensor, a_code: int, a_onehot: bool, b: torch.Tensor, b_code: int, b_onehot: bool, n: int, c: int,
         cls0: int, shape, spacing, tau, percentile) -> torch.Tensor:
    """float32 [8, n, Cs] rows of the kernel's output block (see include/ctunet_hip.h)."""
    cs = c - cls0
    d, h, w = shape
    lib = _lib.load()
    a, b = _lib.as_bytes(a), _lib.as_bytes(b)
    sp = None if spacing is None else _lib.float_array(v for t in spacing for v in t)
    ws = torch.empty(lib.ctu_surface_ws_bytes(n, cs, d, h, w), dtype=torch.uint8, device=a.device)
    out = torch.empty((8, n, cs), dtype=torch.float32, device=a.device)
    with _lib.on(a.device) as run:
        run("ctu_surface_metrics", a.data_ptr(), a_code, int(a_onehot), b.data_ptr(), b_code, int(b_onehot), n, c, cls0, cs,
            d, h, w, sp, _lib.double_array(tau), -1.0 if percentile is None else percentile, out.data_ptr(), ws.data_ptr())
    return out


def _onehot_inputs(y_pred, y, include_background):
    for t, nm in ((y_pred, "y_pred"), (y, "y")):
        if not isinstance(t, torch.Tensor) or t.dim() != 5:
            raise ValueError(f"metrics: {nm} must be a one-hot [N,C,D,H,W] tensor")
    if y_pred.shape != y.shape:
        raise ValueError(f"metrics: y_pred {tuple(y_pred.shape)} and y {tuple(y.shape)} differ in shape")
    n, c = y_pred.shape[:2]
    cls0 = 0 if include_background else 1
    if c - cls0 < 1 or c - cls0 > MAX_CLASSES:
        raise ValueError(f"metrics: 1 to {MAX_CLASSES} scored classes are supported, got {c - cls0}")
    _check_sides(y_pred.shape[2:])
    allowed = (torch.float32, torch.uint8, torch.bool)
    ca, cb = _dtype_code(y_pred, allowed, "y_pred"), _dtype_code(y, allowed, "y")
    return n, c, cls0, ca, cb


def compute_hausdorff_distance(y_pred: torch.Tensor, y: torch.Tensor, include_background: bool = False,
                               distance_metric: str = "euclidean", percentile: Optional[float] = None,
                               directed: bool = False, spacing=None) -> torch.Tensor:
    """float32 [N, C']: HD (``percentile=None``) or HD_p of binarised one-hot [N,C,D,H,W] tensors (float or uint8)."""
    _check_metric(distance_metric)
    pct = _check_percentile(percentile)
    n, c, cls0, ca, cb = _onehot_inputs(y_pred, y, include_background)
    sp = parse_spacing(spacing, n)
    _lib.check_device(_ON_GPU, y_pred, y)
    out = _run(y_pred, ca, True, y, cb, True, n, c, cls0, y.shape[2:], sp, None, pct)
    if pct is None:
        return out[_HD_DIR if directed else _HD]
    return out[_HDP_DIR if directed else _HDP]


def compute_average_surface_distance(y_pred: torch.Tensor, y: torch.Tensor, include_background: bool = False,
                                     symmetric: bool = False, distance_metric: str = "euclidean",
                                     spacing=None) -> torch.Tensor:
    """float32 [N, C']: ASSD (``symmetric=True``) or the mean distance from the prediction's surface to the target's."""
    _check_metric(distance_metric)
    n, c, cls0, ca, cb = _onehot_inputs(y_pred, y, include_background)
    sp = parse_spacing(spacing, n)
    _lib.check_device(_ON_GPU, y_pred, y)
    out = _run(y_pred, ca, True, y, cb, True, n, c, cls0, y.shape[2:], sp, None, None)
    return out[_ASSD if symmetric else _ASD_DIR]


def compute_surface_dice(y_pred: torch.Tensor, y: torch.Tensor, class_thresholds: Sequence[float],
                         include_background: bool = False, distance_metric: str = "euclidean",
                         spacing=None) -> torch.Tensor:
    """float32 [N, C']: surface Dice (NSD) with one tolerance per scored class, in the units of ``spacing``."""
    _check_metric(distance_metric)
    if isinstance(class_thresholds, Real):
        raise ValueError("metrics: class_thresholds must be a sequence with one value per scored class")
    if isinstance(y_pred, torch.Tensor) and y_pred.dim() == 5:
        _thresholds(class_thresholds, y_pred.shape[1] - (0 if include_background else 1), "class_thresholds")
    n, c, cls0, ca, cb = _onehot_inputs(y_pred, y, include_background)
    tau = _thresholds(class_thresholds, c - cls0, "class_thresholds")
    sp = parse_spacing(spacing, n)
    _lib.check_device(_ON_GPU, y_pred, y)
    return _run(y_pred, ca, True, y, cb, True, n, c, cls0, y.shape[2:], sp, tau, None)[_NSD]


def surface_metrics(pred_labels: torch.Tensor, target_labels: torch.Tensor, num_classes: int, spacing=None,
                    percentile: Optional[float] = 95.0, tolerance=None,
                    include_background: bool = False) -> Dict[str, torch.Tensor]:
    """Every metric of label maps [D,H,W] or [N,D,H,W] (uint8 or int64, read directly: no one-hot copy) from one pass.

    Returns float32 [N, C'] device tensors: ``dice``, ``hd``, ``hd_p`` (NaN with ``percentile=None``), ``assd``
    (symmetric) and, when ``tolerance`` (one value, or one per scored class) is given, ``nsd``.
    """
    pct = _check_percentile(percentile)
    if isinstance(num_classes, bool) or not isinstance(num_classes, int):
        raise ValueError(f"metrics: num_classes must be an int, got {num_classes!r}")
    cls0 = 0 if include_background else 1
    cs = num_classes - cls0
    if cs < 1 or cs > MAX_CLASSES:
        raise ValueError(f"metrics: 1 to {MAX_CLASSES} scored classes are supported, got {cs}")
    tau = None if tolerance is None else _thresholds(tolerance, cs, "tolerance")
    for t, nm in ((pred_labels, "pred_labels"), (target_labels, "target_labels")):
        if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4):
            raise ValueError(f"metrics: {nm} must be a label map [D,H,W] or [N,D,H,W]")
    if pred_labels.shape != target_labels.shape:
        raise ValueError(f"metrics: label maps differ in shape: {tuple(pred_labels.shape)} vs {tuple(target_labels.shape)}")
    n = 1 if pred_labels.dim() == 3 else pred_labels.shape[0]
    shape = pred_labels.shape[-3:]
    _check_sides(shape)
    allowed = (torch.uint8, torch.int64)
    ca, cb = _dtype_code(pred_labels, allowed, "pred_labels"), _dtype_code(target_labels, allowed, "target_labels")
    sp = parse_spacing(spacing, n)
    _lib.check_device(_ON_GPU, pred_labels, target_labels)
    out = _run(pred_labels, ca, False, target_labels, cb, False, n, num_classes, cls0, shape, sp, tau, pct)
    res = {"dice": out[_DICE], "hd": out[_HD], "hd_p": out[_HDP], "assd": out[_ASSD]}
    if tau is not None:
        res["nsd"] = out[_NSD]
    return res


def _linear_percentile(d: torch.Tensor, pct: float) -> torch.Tensor:
    """numpy's default ("linear") percentile of a non-empty float64 vector, on the device, without a synchronisation."""
    s = torch.sort(d).values
    pos = pct / 100.0 * (s.shape[0] - 1)
    lo = min(int(math.floor(pos)), s.shape[0] - 1)
    hi = min(lo + 1, s.shape[0] - 1)
    t = pos - lo
    a, b = s[lo], s[hi]
    return b - (b - a) * (1.0 - t) if t >= 0.5 else a + (b - a) * t   # numpy's two-sided form: exact at t = 0 and t = 1


def mesh_surface_metrics(a, b, percentile: Optional[float] = 95.0, tolerance: Optional[float] = None, grid_a=None,
                         grid_b=None) -> Dict[str, torch.Tensor]:
    """HD, HD_p, ASSD and NSD between two surface meshes (``mesh.Mesh``, both on one GPU, in the same physical frame), without
    the round trip through voxels: float32 scalar device tensors ``hd``, ``hd_p`` (NaN with ``percentile=None``), ``assd`` and,
    when ``tolerance`` is given, ``nsd``.

    The samples are the vertices, unweighted: d(A->B) holds, for every vertex of ``a``, its exact distance to the surface of
    ``b`` (``mesh.point_distance``: to the nearest point of a face, not to the nearest vertex), and d(B->A) the same the other
    way.  A mesh with vertices of very uneven density weighs its dense regions more; a vertex that no face uses counts like
    any other.  From the two vectors the definitions of the module docstring apply with mesh vertices in place of surface
    voxels: ``hd`` = the larger maximum, ``hd_p`` = the larger of the two numpy "linear" percentiles, ``assd`` = the sum of both
    vectors over the number of samples, ``nsd`` = the share of samples within ``tolerance``; sums and percentiles in float64,
    rounded to float32 once.  Empty surfaces (no vertex or no face): ``hd``, ``hd_p`` and ``assd`` are NaN when either is
    empty, ``nsd`` is NaN when both are and 0 when exactly one is.

    ``grid_a`` / ``grid_b``: the ``mesh.build_face_grid`` of ``a`` / ``b`` to reuse.  The metrics are computed on the device with
    torch; the call synchronises only where it builds a grid."""
    from . import mesh as _mesh
    pct = _check_percentile(percentile)
    tau = None if tolerance is None else _thresholds(tolerance, 1, "tolerance")[0]
    va, fa = _mesh._check_mesh(a, "mesh_surface_metrics")
    vb, fb = _mesh._check_mesh(b, "mesh_surface_metrics")
    if va.device != vb.device:
        raise ValueError(f"metrics: the meshes live on different devices: {va.device} and {vb.device}")
    _lib.check_device("metrics: mesh_surface_metrics takes meshes on the GPU; this path has no CPU fallback", va)
    dev = va.device
    empty_a, empty_b = va.shape[0] == 0 or fa.shape[0] == 0, vb.shape[0] == 0 or fb.shape[0] == 0
    nan = torch.full((), float("nan"), dtype=torch.float32, device=dev)
    if empty_a or empty_b:
        res = {"hd": nan, "hd_p": nan.clone(), "assd": nan.clone()}
        if tau is not None:
            res["nsd"] = nan.clone() if empty_a and empty_b else torch.zeros((), dtype=torch.float32, device=dev)
        return res
    dab = _mesh.point_distance(va, b, grid=grid_b).to(torch.float64)
    dba = _mesh.point_distance(vb, a, grid=grid_a).to(torch.float64)
    n = dab.shape[0] + dba.shape[0]
    res = {"hd": torch.maximum(dab.max(), dba.max()).to(torch.float32),
           "hd_p": nan if pct is None else torch.maximum(_linear_percentile(dab, pct), _linear_percentile(dba, pct)).to(torch.float32),
           "assd": ((dab.sum() + dba.sum()) / n).to(torch.float32)}
    if tau is not None:
        res["nsd"] = (((dab <= tau).sum() + (dba <= tau).sum()).to(torch.float64) / n).to(torch.float32)
    return res


def workspace_bytes(n: int, num_scored: int, shape) -> int:
    """Device workspace of one call (bytes) for n items, num_scored classes and a (D, H, W) volume."""
    return int(_lib.load().ctu_surface_ws_bytes(n, num_scored, *shape))
