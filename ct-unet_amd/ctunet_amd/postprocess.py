"""Connected components of segmentations on the GPU: labelling and the two usual clean-ups of a predicted label map.

Names and arguments follow monai's transforms (``KeepLargestConnectedComponent``, ``RemoveSmallObjects``) and
``scipy.ndimage.label``.  Everything runs in ``ctu_label_components`` / ``ctu_filter_components`` (``csrc/components.hip``):
union-find over the voxels, no host synchronisation, so a call can be captured into a CUDA/HIP graph.

Definitions (the tests restate them on scipy / numpy):

- **Foreground**: a voxel whose label is nonzero; with ``applied_labels``, only a voxel whose label is in that list.
- **Connection**: two neighbouring voxels are connected iff both are foreground and carry the **same label**, so every
  component has one class and one pass handles every class.  ``label`` binarises its mask first (scipy's rule).
- **Connectivity**: scipy's rank, ``ndi.generate_binary_structure(3, connectivity)``: 1 = 6 face neighbours, 2 = 18,
  3 = 26.  Nothing connects across the volume border.
- **Numbering** (``label``): the root of a component is its first voxel in C order; a component's number is 1 + the rank
  of its root in C order, per item, background 0.  This is ``scipy.ndimage.label``'s numbering, bit for bit.
- **Keep-largest**: per (item, class) the ``num_components`` largest components are kept; between equal sizes the one
  whose first voxel comes first in C order wins (``np.argsort(-sizes, kind="stable")``).  The classes are the applied
  labels, or with ``applied_labels=None`` every label 1..255 (labels above 255 of an int64 map are never dropped then:
  list them in ``applied_labels``).
- **Remove-small**: a component is kept iff it has at least ``min_size`` voxels (skimage's ``remove_small_objects``).
- Foreground voxels of dropped components become 0; every other voxel keeps its label.

Results are deterministic: every value is an integer and every order is fixed.
"""
from __future__ import annotations

from numbers import Integral
from typing import Optional, Sequence, Tuple

import torch

from . import _lib

MAX_APPLIED = 16
MAX_COMPONENTS = 8
CTU_U8, CTU_I64 = 3, 4
_LARGEST, _MIN_SIZE = 0, 1


def _volume(t, what: str, allowed) -> Tuple[int, Tuple[int, int, int]]:
    if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4):
        raise ValueError(f"postprocess: {what} must be a [D,H,W] or [N,D,H,W] tensor")
    if t.dtype not in allowed:
        raise ValueError(f"postprocess: {what} must be one of {', '.join(str(a) for a in allowed)}, got {t.dtype}")
    n = 1 if t.dim() == 3 else t.shape[0]
    shape = tuple(t.shape[-3:])
    if n < 1 or n > 65535 or any(s < 1 for s in shape):
        raise ValueError(f"postprocess: every side must be >= 1 and N <= 65535, got {tuple(t.shape)}")
    if shape[0] * shape[1] * shape[2] >= 1 << 31:
        raise ValueError(f"postprocess: an item must hold fewer than 2^31 voxels, got {shape}")
    return n, shape


def _connectivity(connectivity) -> int:
    if isinstance(connectivity, bool) or not isinstance(connectivity, Integral) or connectivity not in (1, 2, 3):
        raise ValueError(f"postprocess: connectivity must be 1, 2 or 3, got {connectivity!r}")
    return int(connectivity)


def _applied(applied_labels, dtype) -> Optional[list]:
    if applied_labels is None:
        return None
    if isinstance(applied_labels, torch.Tensor):
        applied_labels = applied_labels.flatten().tolist()
    elif isinstance(applied_labels, Integral) and not isinstance(applied_labels, bool):
        applied_labels = [applied_labels]
    vals = list(applied_labels)
    hi = 255 if dtype == torch.uint8 else (1 << 63) - 1
    lo = 1 if dtype == torch.uint8 else -(1 << 63)
    if not 1 <= len(vals) <= MAX_APPLIED:
        raise ValueError(f"postprocess: applied_labels must hold 1 to {MAX_APPLIED} labels, got {len(vals)}")
    for v in vals:
        if isinstance(v, bool) or not isinstance(v, Integral) or v == 0 or not lo <= v <= hi:
            raise ValueError(f"postprocess: applied_labels must be nonzero labels of the map's dtype, got {v!r}")
    if len(set(int(v) for v in vals)) != len(vals):
        raise ValueError(f"postprocess: applied_labels must be distinct, got {vals!r}")
    return [int(v) for v in vals]


def _check_device(t: torch.Tensor) -> None:
    if not t.is_cuda:
        raise ValueError("postprocess: inputs must live on the GPU; this path has no CPU fallback")


def _ws(lib, n, shape, device) -> torch.Tensor:
    return torch.empty(lib.ctu_components_ws_bytes(n, *shape), dtype=torch.uint8, device=device)


def _host_labels(vals):
    import ctypes
    if not vals:
        return None, 0
    return (ctypes.c_int64 * len(vals))(*vals), len(vals)


def label(mask: torch.Tensor, connectivity: int = 3) -> Tuple[torch.Tensor, torch.Tensor]:
    """Connected components of a bool or uint8 mask [D,H,W] or [N,D,H,W] (nonzero = foreground).

    Returns ``(labels, num)``: int32 labels of the mask's shape numbered as ``scipy.ndimage.label`` numbers them
    (0 = background), and the int32 [N] device tensor of component counts per item.
    """
    n, shape = _volume(mask, "mask", (torch.bool, torch.uint8))
    conn = _connectivity(connectivity)
    _check_device(mask)
    lib = _lib.load()
    m = mask.contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else (m != 0).view(torch.uint8)
    labels = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    num = torch.empty(n, dtype=torch.int32, device=mask.device)
    ws = _ws(lib, n, shape, mask.device)
    with torch.cuda.device(mask.device):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.ctu_label_components(m.data_ptr(), CTU_U8, n, *shape, conn, None, 0, labels.data_ptr(),
                                            num.data_ptr(), ws.data_ptr(), stream), "label_components")
    return labels, num


def _filter(labels: torch.Tensor, mode: int, param: int, applied, conn: int, n: int, shape) -> torch.Tensor:
    _check_device(labels)
    lib = _lib.load()
    src = labels.contiguous()
    out = torch.empty_like(src)
    al, nal = _host_labels(applied)
    ws = _ws(lib, n, shape, labels.device)
    code = CTU_U8 if src.dtype == torch.uint8 else CTU_I64
    with torch.cuda.device(labels.device):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.ctu_filter_components(src.data_ptr(), code, n, *shape, conn, al, nal, mode, param, out.data_ptr(),
                                             ws.data_ptr(), stream), "filter_components")
    return out


def keep_largest_connected_component(labels: torch.Tensor, applied_labels: Optional[Sequence[int]] = None,
                                     connectivity: int = 3, num_components: int = 1) -> torch.Tensor:
    """Keep the ``num_components`` (1..8) largest components of each class of a uint8 / int64 label map [D,H,W] or
    [N,D,H,W] (each item on its own); a new tensor of the same dtype and shape."""
    n, shape = _volume(labels, "labels", (torch.uint8, torch.int64))
    al = _applied(applied_labels, labels.dtype)
    conn = _connectivity(connectivity)
    if (isinstance(num_components, bool) or not isinstance(num_components, Integral)
            or not 1 <= num_components <= MAX_COMPONENTS):
        raise ValueError(f"postprocess: num_components must lie in 1..{MAX_COMPONENTS}, got {num_components!r}")
    return _filter(labels, _LARGEST, int(num_components), al, conn, n, shape)


def remove_small_objects(labels: torch.Tensor, min_size: int, applied_labels: Optional[Sequence[int]] = None,
                         connectivity: int = 3) -> torch.Tensor:
    """Remove the components with fewer than ``min_size`` voxels from a uint8 / int64 label map [D,H,W] or [N,D,H,W];
    a new tensor of the same dtype and shape."""
    n, shape = _volume(labels, "labels", (torch.uint8, torch.int64))
    al = _applied(applied_labels, labels.dtype)
    conn = _connectivity(connectivity)
    if isinstance(min_size, bool) or not isinstance(min_size, Integral) or min_size < 0:
        raise ValueError(f"postprocess: min_size must be an integer >= 0, got {min_size!r}")
    # a component has at most D*H*W < 2^31 voxels: larger thresholds all mean "remove every component"
    param = min(int(min_size), shape[0] * shape[1] * shape[2] + 1, (1 << 31) - 1)
    return _filter(labels, _MIN_SIZE, param, al, conn, n, shape)


def workspace_bytes(n: int, shape) -> int:
    """Device workspace of one call (bytes) for n items of a (D, H, W) volume."""
    return int(_lib.load().ctu_components_ws_bytes(n, *shape))
