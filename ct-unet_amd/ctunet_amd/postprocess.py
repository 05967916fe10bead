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

Binary morphology (``binary_erosion`` / ``binary_dilation`` / ``binary_opening`` / ``binary_closing`` /
``binary_fill_holes`` / ``extract_implant``; ``ctu_binary_morphology``, ``ctu_fill_holes``, ``ctu_implant_mask`` of
``csrc/morphology.hip`` and ``csrc/components.hip``) follows ``scipy.ndimage`` in 3-D, bit for bit:

- **Foreground**: a nonzero voxel of a bool, uint8 or int64 tensor; with ``label=k`` a voxel equal to ``k`` (tested in the
  kernel that reads the map).  The result is bool for bool input, otherwise uint8 holding 0 / 1.
- **Structure**: an int 1 / 2 / 3 is ``scipy.ndimage.generate_binary_structure(3, c)`` (6 / 18 / 26 neighbours plus the
  centre); any 3x3x3 bool array or tensor with at least one true entry is taken as it is (with or without its centre,
  symmetric or not).  It travels as a 27-bit code, bit ``(i*3+j)*3+k`` for ``structure[i, j, k]``.
- **Offsets**: with ``S`` the offsets ``s = (i-1, j-1, k-1)`` of the true entries, every voxel outside the volume reads as
  ``border_value`` (0 or 1).
- **Erosion**: ``out[v] = AND_{s in S} in[v+s]``.  **Dilation**: ``out[v] = OR_{s in S} in[v-s]`` (the reflection).
- **Iterations**: ``iterations=k`` (1..64) is k successive applications.  scipy's ``iterations < 1`` (repeat until nothing
  changes) is refused: it needs a decision on the host per step.  ``mask=`` and ``origin=`` are not offered.
- **Opening**: ``dilation(erosion(x, k), k)``.  **Closing**: ``erosion(dilation(x, k), k)``.  Both with border value 0, as
  scipy does, so closing erodes at the volume border.
- **Fill holes**: ``x OR (background voxels whose background component, at the given connectivity, touches no face of the
  volume)``; ``connectivity=1`` is scipy's default structure.
- **Implant extraction**, in order: ``m = (full_skull != 0) AND (defective_skull == 0)``; ``opening_iterations > 0``:
  ``binary_opening(m, structure, opening_iterations)``; ``fill_holes``: ``binary_fill_holes(., 1)``;
  ``keep_largest_connected_component(., connectivity=connectivity, num_components=num_components)``; a uint8 0 / 1 mask.

Distance transform and ball morphology (``distance_transform_edt`` / ``signed_distance`` / ``ball_erosion`` /
``ball_dilation`` / ``ball_opening`` / ``ball_closing``; ``ctu_distance_transform`` of ``csrc/distance.hip``) follow
``scipy.ndimage.distance_transform_edt``:

- **Foreground** as above (nonzero, or ``== label``).  The **sites** are the background voxels; every voxel gets the
  Euclidean distance ``sqrt(sum_i ((v_i - p_i) s_i)^2)`` to its nearest site ``p``, a site gets 0; ``s`` is ``sampling``
  (z, y, x), a scalar, a triple or one triple per item, ``None`` = 1.
- **Exactness**: with unit sampling (``None`` or all 1) the squared distances are int32 and exact, and the distance is the
  correctly rounded float32 square root; otherwise squared distances are float32 sums of ``(k_i s_i)^2``.
  ``squared=True`` returns the squared map: int32 at unit sampling, float32 otherwise.
- **Indices**: ``return_indices=True`` gives int32 ``[3,D,H,W]`` / ``[N,3,D,H,W]``, the (z, y, x) of *a* nearest site;
  between equidistant sites the choice is fixed (two calls agree) but need not be scipy's.
- **Empty site set**: an item without background gives ``+inf`` (``INT32_MAX`` for the int32 squared map) everywhere and
  indices -1.  scipy's result is undefined there; this is a documented divergence.
- **Signed distance**: ``edt(sites = foreground) - edt(sites = background)``: positive outside the object, negative
  inside, never 0; ``-inf`` / ``+inf`` everywhere for an all-foreground / all-background item.
- **Ball**: with ``B = {o : ||o * s|| <= radius}`` (``radius`` in the units of ``sampling``), dilation is
  ``{v : d(v, foreground) <= radius}`` and erosion ``{v : d(v, background or outside the volume) > radius}``: scipy's
  ``binary_dilation`` / ``binary_erosion`` with the structure ``B`` and ``border_value=0``, at the cost of one transform
  whatever the radius.  Opening is erosion then dilation, closing dilation then erosion (which erodes at the border, as
  scipy's does).  The comparison is made on squared distances (``d2 <= float32(radius^2)``): a radius within float32
  rounding (about 1e-6 relative) of an offset's length may fall on either side.
- **Limits**: every side at most 1024 (the line passes keep 6 bytes per line element in LDS; 1365 elements is their hard
  limit), fewer than 2^31 voxels per item, N <= 65535.  Anything larger raises.
- ``extract_implant(..., opening_radius=r, sampling=s)`` replaces the iterated opening with ``ball_opening(m, r, s)``.

Local thickness (``local_thickness`` / ``thickness_summary``; ``ctu_local_thickness``, ``ctu_thickness_summary`` of
``csrc/thickness.hip``) is Hildebrand and Rüegsegger's (1997): every foreground voxel gets the diameter of the largest
inscribed ball that contains it.

- **Foreground** as above.  ``D2`` is ``distance_transform_edt(mask, sampling, squared=True, label=label)``: int32 and exact
  at unit sampling, float32 otherwise, 0 on background; the outside of the volume is not background, so an object cut by
  the volume's face reads as continuing.
- **Offset length** ``dd(p, q)``: at unit sampling the integer ``dz^2 + dy^2 + dx^2``; otherwise float32,
  ``t_a = float32(k_a) * s_a`` and ``dd = (t_z t_z + t_y t_y) + t_x t_x``, every product and sum rounded on its own.
- **Covering**: the centre ``q`` covers ``p`` iff both are foreground and ``dd(p, q) < D2(q)``, strictly: the open ball
  (the closed one holds a background voxel's centre).  ``p`` covers itself.
- **Result**: ``thickness(p) = 2 sqrt(max {D2(q) : q covers p})``, float32, the correctly rounded root; 0 on background;
  ``+inf`` everywhere in an item without background.  The units are those of ``sampling``.
- **Bias**: with voxel centres (ImageJ's convention too) a plate of ``k`` voxels reads ``2 ceil(k / 2)`` voxels: 1 -> 2,
  2 -> 2, 3 -> 4, 4 -> 4, 5 -> 6.  The result is the true thickness plus 0 to 1 voxel and is not corrected.
- **Summary**: per item ``(foreground count, min, max, mean, count below min_thickness)`` as float64 on the device;
  foreground is ``thickness > 0``, below is ``t < float32(min_thickness)``, the mean a float64 sum in a fixed order.  An
  item without foreground gives ``(0, +inf, 0, NaN, 0)``.
- The search is exact (its pruning never shows in the result), uses no atomics and no host synchronisation, and two
  calls are bit-equal.  Limits as the distance transform's.  Not offered: a radius cap, the bias correction, the thickness
  of the background (pass the inverted mask), per-vertex thickness of meshes, a virtual border.

Region properties (``region_properties`` / ``bounding_box`` / ``crop_to_box``; ``ctu_region_moments``, ``ctu_region_derive`` of
``csrc/regionprops.hip``; ``tests/regionprops_ref.py`` restates the rule in numpy) are what ``scipy.ndimage.sum_labels`` /
``find_objects`` / ``center_of_mass`` give on the host, from one pass over a label map on the device:

- **Regions**: ``labels`` is bool, uint8, int32 (what ``label`` returns) or int64, [D,H,W] or [N,D,H,W]; region ``r``
  (1 <= r <= R = ``num_regions``, at most 65536) is the set of voxels whose value is ``r`` (a bool mask is region 1), 0 is
  background, and a voxel whose value is negative or above R belongs to no region and is counted in ``overflow``.  R is a
  capacity the caller chooses: nothing is read back to size the result.
- **Limits**: every side at most 1024, fewer than 2^31 voxels per item, N <= 65535.  With sides up to 1024 every sum below
  stays under 2^31 * 2^20 = 2^51 < 2^53, so each converts to float64 exactly.
- ``moments`` int64 [N,R,10]: (count, Sz, Sy, Sx, Szz, Szy, Szx, Syy, Syx, Sxx), sums over the voxel indices (z, y, x) of the
  region.  Exact integers, summed with integer atomics: independent of any order of arrival.
- ``boxes`` int32 [N,R,6]: (z0, y0, x0, z1, y1, x1), half open, the slices of ``scipy.ndimage.find_objects``; six zeros for an
  empty region.  ``overflow`` int64 [N].
- ``centroid`` float64 [N,R,3], world units: with ``n = count`` and ``m_a = S_a / n``, ``origin_a + sampling_a * m_a``; NaN for
  an empty region.  ``sampling`` and ``origin`` are a scalar, a (z, y, x) triple or one triple per item (``None``: 1 and 0).
- ``covariance`` float64 [N,R,3,3], world units squared: ``c_ab = S_ab / n - m_a * m_b``, then
  ``(c_ab * sampling_min(a,b)) * sampling_max(a,b)`` (the population covariance of the voxel centres); float64, every
  operation rounded on its own; NaN for an empty region.
- ``extent`` float64 [N,R,3] and ``axes`` float64 [N,R,3,3]: the eigenvalues of the covariance in descending order and the
  unit eigenvectors as columns (``axes[..., :, j]`` belongs to ``extent[..., j]``), by 8 cyclic Jacobi sweeps over the pairs
  (0,1), (0,2), (1,2) from ``E = I``: a pair with ``a_pq != 0`` takes ``theta = (a_qq - a_pp) / (2 a_pq)``,
  ``t = sign(theta) / (|theta| + sqrt(theta theta + 1))``, ``c = 1 / sqrt(t t + 1)``, ``s = t c``; ``a_pp -= t a_pq``,
  ``a_qq += t a_pq``, ``a_pq = 0``, with ``r`` the third index ``(a_rp, a_rq) <- (c a_rp - s a_rq, s a_rp + c a_rq)`` and the
  same for the columns p, q of every row of ``E``.  Equal eigenvalues keep their index order.  Each of the first two axes is
  signed so that its component of largest magnitude (the first one of equals) is positive; the third axis is the cross
  product of the first two, so the frame is right-handed in (z, y, x) index order.  A region of fewer than 2 voxels gives NaN
  axes (one voxel: extent 0; none: NaN).  A region with nearly equal extents has ill-defined axes.
- No host synchronisation and no allocation besides the result and the workspace (24 bytes per region): a call can be
  captured into a graph, and two calls are bit-equal.
- **Boxes as regions of interest** (``bounding_box``): per axis of size ``S``, from the region's ``(lo, hi)``: ``lo -= margin``,
  ``hi += margin``; ``side = ceil((hi - lo) / multiple_of) * multiple_of``, ``lo -= (side - (hi - lo)) // 2``; if ``side <= S``
  the box is shifted inside, ``lo = max(min(lo, S - side), 0)``, ``hi = lo + side``; otherwise it is clipped to ``(0, S)``.  An
  empty region gives the whole volume.  Integer arithmetic on the device.

Each item of a batch is processed on its own.  The morphology calls use no atomics and no host synchronisation, so a
call can be captured into a graph.  The output and the workspace are ``torch.empty`` tensors, which a capture draws from
the graph's private pool.  Under capture give ``structure`` as an int or a host array: a structure tensor on the device
is copied to the host to form its 27-bit code, which synchronises and is refused during capture.
"""
from __future__ import annotations

import ctypes as C
import math
from numbers import Integral, Real
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from .metrics import parse_spacing

MAX_APPLIED = 16
MAX_COMPONENTS = 8
MAX_ITERATIONS = 64
_ERODE, _DILATE, _OPEN, _CLOSE = 0, 1, 2, 3
_WS_MORPH, _WS_FILL, _WS_IMPLANT = 0, 1, 2
_MASK_DTYPES = (torch.bool, torch.uint8, torch.int64)
_ON_GPU = "postprocess: inputs must live on the GPU; this path has no CPU fallback"
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


def _ws(lib, n, shape, device) -> torch.Tensor:
    return torch.empty(lib.ctu_components_ws_bytes(n, *shape), dtype=torch.uint8, device=device)


def label(mask: torch.Tensor, connectivity: int = 3) -> Tuple[torch.Tensor, torch.Tensor]:
    """Connected components of a bool or uint8 mask [D,H,W] or [N,D,H,W] (nonzero = foreground).

    Returns ``(labels, num)``: int32 labels of the mask's shape numbered as ``scipy.ndimage.label`` numbers them
    (0 = background), and the int32 [N] device tensor of component counts per item.
    """
    n, shape = _volume(mask, "mask", (torch.bool, torch.uint8))
    conn = _connectivity(connectivity)
    _lib.check_device(_ON_GPU, mask)
    lib = _lib.load()
    m = mask.contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else (m != 0).view(torch.uint8)
    labels = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    num = torch.empty(n, dtype=torch.int32, device=mask.device)
    ws = _ws(lib, n, shape, mask.device)
    with _lib.on(mask.device) as run:
        run("ctu_label_components", m.data_ptr(), _lib.DTYPE_CODE[m.dtype], n, *shape, conn, None, 0, labels.data_ptr(),
            num.data_ptr(), ws.data_ptr())
    return labels, num


def _filter(labels: torch.Tensor, mode: int, param: int, applied, conn: int, n: int, shape) -> torch.Tensor:
    _lib.check_device(_ON_GPU, labels)
    lib = _lib.load()
    src = labels.contiguous()
    out = torch.empty_like(src)
    ws = _ws(lib, n, shape, labels.device)
    with _lib.on(labels.device) as run:
        run("ctu_filter_components", src.data_ptr(), _lib.DTYPE_CODE[src.dtype], n, *shape, conn,
            _lib.array(C.c_int64, applied or None), len(applied or ()), mode, param, out.data_ptr(), ws.data_ptr())
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


# ------------------------------------------------------------------------------------------------ binary morphology
def _structure_code(structure) -> int:
    """27-bit code of a structure: bit (i*3+j)*3+k for structure[i, j, k] (a device tensor is read back to the host)."""
    if isinstance(structure, Integral) and not isinstance(structure, bool):
        if structure not in (1, 2, 3):
            raise ValueError(f"postprocess: an integer structure must be 1, 2 or 3, got {structure!r}")
        return sum(1 << ((i * 3 + j) * 3 + k) for i in range(3) for j in range(3) for k in range(3)
                   if abs(i - 1) + abs(j - 1) + abs(k - 1) <= structure)
    try:
        st = torch.as_tensor(structure)
    except Exception as e:
        raise ValueError(f"postprocess: structure must be 1, 2, 3 or a 3x3x3 bool array, got {structure!r}") from e
    if tuple(st.shape) != (3, 3, 3):
        raise ValueError(f"postprocess: structure must be 1, 2, 3 or a 3x3x3 bool array, got shape {tuple(st.shape)}")
    bits = (st != 0).flatten().tolist()
    code = sum(1 << i for i, b in enumerate(bits) if b)
    if code == 0:
        raise ValueError("postprocess: structure has no true entry")
    return code


def _iterations(iterations, lo: int = 1, what: str = "iterations") -> int:
    if isinstance(iterations, bool) or not isinstance(iterations, Integral) or not lo <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"postprocess: {what} must be an integer in {lo}..{MAX_ITERATIONS} (repeat-until-stable is not "
                         f"offered), got {iterations!r}")
    return int(iterations)


def _border(border_value) -> int:
    if isinstance(border_value, bool):
        return int(border_value)
    if not isinstance(border_value, Integral) or border_value not in (0, 1):
        raise ValueError(f"postprocess: border_value must be 0 or 1, got {border_value!r}")
    return int(border_value)


def _label_arg(label):
    if label is None:
        return 0, 0
    if isinstance(label, bool) or not isinstance(label, Integral) or not -(1 << 63) <= label < (1 << 63):
        raise ValueError(f"postprocess: label must be an integer of the map's range, got {label!r}")
    return 1, int(label)


def _mask_out(src: torch.Tensor) -> torch.Tensor:
    return torch.empty(src.shape, dtype=torch.uint8, device=src.device)


def _finish(out: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    return out.view(torch.bool) if like.dtype == torch.bool else out


def _morphology(mask, mode: int, structure, iterations, border_value, label) -> torch.Tensor:
    n, shape = _volume(mask, "mask", _MASK_DTYPES)
    code = _structure_code(structure)
    it = _iterations(iterations)
    border = _border(border_value)
    has_label, lab = _label_arg(label)
    _lib.check_device(_ON_GPU, mask)
    lib = _lib.load()
    src = _lib.as_bytes(mask)
    out = _mask_out(mask)
    ws = torch.empty(lib.ctu_morphology_ws_bytes(n, *shape, _WS_MORPH), dtype=torch.uint8, device=mask.device)
    with _lib.on(mask.device) as run:
        run("ctu_binary_morphology", src.data_ptr(), _lib.DTYPE_CODE[src.dtype], n, *shape, mode, code, it, border, has_label,
            lab, out.data_ptr(), ws.data_ptr())
    return _finish(out, mask)


def binary_erosion(mask: torch.Tensor, structure=1, iterations: int = 1, border_value: int = 0,
                   label: Optional[int] = None) -> torch.Tensor:
    """``scipy.ndimage.binary_erosion`` of a bool / uint8 / int64 mask [D,H,W] or [N,D,H,W] (each item on its own)."""
    return _morphology(mask, _ERODE, structure, iterations, border_value, label)


def binary_dilation(mask: torch.Tensor, structure=1, iterations: int = 1, border_value: int = 0,
                    label: Optional[int] = None) -> torch.Tensor:
    """``scipy.ndimage.binary_dilation`` of a bool / uint8 / int64 mask [D,H,W] or [N,D,H,W]."""
    return _morphology(mask, _DILATE, structure, iterations, border_value, label)


def binary_opening(mask: torch.Tensor, structure=1, iterations: int = 1, label: Optional[int] = None) -> torch.Tensor:
    """``scipy.ndimage.binary_opening``: ``iterations`` erosions, then as many dilations, border value 0."""
    return _morphology(mask, _OPEN, structure, iterations, 0, label)


def binary_closing(mask: torch.Tensor, structure=1, iterations: int = 1, label: Optional[int] = None) -> torch.Tensor:
    """``scipy.ndimage.binary_closing``: ``iterations`` dilations, then as many erosions, border value 0."""
    return _morphology(mask, _CLOSE, structure, iterations, 0, label)


def binary_fill_holes(mask: torch.Tensor, connectivity: int = 1, label: Optional[int] = None) -> torch.Tensor:
    """``scipy.ndimage.binary_fill_holes`` with ``generate_binary_structure(3, connectivity)``: the background components
    that touch no face of the volume become foreground."""
    n, shape = _volume(mask, "mask", _MASK_DTYPES)
    conn = _connectivity(connectivity)
    has_label, lab = _label_arg(label)
    _lib.check_device(_ON_GPU, mask)
    lib = _lib.load()
    src = _lib.as_bytes(mask)
    out = _mask_out(mask)
    ws = torch.empty(lib.ctu_morphology_ws_bytes(n, *shape, _WS_FILL), dtype=torch.uint8, device=mask.device)
    with _lib.on(mask.device) as run:
        run("ctu_fill_holes", src.data_ptr(), _lib.DTYPE_CODE[src.dtype], n, *shape, conn, has_label, lab, out.data_ptr(),
            ws.data_ptr())
    return _finish(out, mask)


def extract_implant(full_skull: torch.Tensor, defective_skull: torch.Tensor, opening_iterations: int = 1, structure=1,
                    connectivity: int = 3, num_components: int = 1, fill_holes: bool = False, *,
                    opening_radius: Optional[float] = None, sampling=None) -> torch.Tensor:
    """The implant of a (full skull, defective skull) prediction pair: ``full AND NOT defective``, opened, optionally
    hole-filled, reduced to its ``num_components`` largest components (module docstring); a uint8 0 / 1 mask.  With
    ``opening_radius`` (in the units of ``sampling``) the opening is ``ball_opening`` instead of the iterated one."""
    n, shape = _volume(full_skull, "full_skull", _MASK_DTYPES)
    n2, shape2 = _volume(defective_skull, "defective_skull", _MASK_DTYPES)
    if tuple(full_skull.shape) != tuple(defective_skull.shape):
        raise ValueError(f"postprocess: full_skull and defective_skull must have the same shape, got "
                         f"{tuple(full_skull.shape)} and {tuple(defective_skull.shape)}")
    it = _iterations(opening_iterations, 0, "opening_iterations")
    code = _structure_code(structure)
    conn = _connectivity(connectivity)
    if (isinstance(num_components, bool) or not isinstance(num_components, Integral)
            or not 1 <= num_components <= MAX_COMPONENTS):
        raise ValueError(f"postprocess: num_components must lie in 1..{MAX_COMPONENTS}, got {num_components!r}")
    if not isinstance(fill_holes, (bool, Integral)):
        raise ValueError(f"postprocess: fill_holes must be a bool, got {fill_holes!r}")
    if opening_radius is None and sampling is not None:
        raise ValueError("postprocess: sampling is the unit of opening_radius; give both or neither")
    if opening_radius is not None:
        if it != 1:
            raise ValueError(f"postprocess: give opening_radius or opening_iterations, not both (got "
                             f"opening_iterations={opening_iterations!r}, opening_radius={opening_radius!r})")
        _distance_sides(shape)
        r2 = _radius2(opening_radius, "opening_radius")
        spacing = _sampling(sampling, n)
    _lib.check_device(_ON_GPU, full_skull, defective_skull)
    if full_skull.device != defective_skull.device:
        raise ValueError("postprocess: full_skull and defective_skull must live on the same GPU")
    if opening_radius is not None:
        m = ((full_skull != 0) & (defective_skull == 0)).view(torch.uint8)
        m = _ball(m, _ERODE, r2, spacing)
        m = _ball(m, _DILATE, r2, spacing)
        if fill_holes:
            m = binary_fill_holes(m, 1)
        return keep_largest_connected_component(m, connectivity=conn, num_components=int(num_components))
    lib = _lib.load()
    a, b = _lib.as_bytes(full_skull), _lib.as_bytes(defective_skull)
    out = _mask_out(full_skull)
    ws = torch.empty(lib.ctu_morphology_ws_bytes(n, *shape, _WS_IMPLANT), dtype=torch.uint8, device=full_skull.device)
    with _lib.on(full_skull.device) as run:
        run("ctu_implant_mask", a.data_ptr(), _lib.DTYPE_CODE[a.dtype], b.data_ptr(), _lib.DTYPE_CODE[b.dtype], n, *shape, code,
            it, int(bool(fill_holes)), conn, int(num_components), out.data_ptr(), ws.data_ptr())
    return out


def morphology_workspace_bytes(n: int, shape, iterations: int = 1) -> int:
    """Device workspace (bytes) of one erosion / dilation / opening / closing call on n items of a (D, H, W) volume: two
    bit images, whatever ``iterations`` is (``ctu_morphology_ws_bytes`` also sizes fill-holes and implant calls)."""
    _iterations(iterations)
    return int(_lib.load().ctu_morphology_ws_bytes(n, *shape, _WS_MORPH))


# ------------------------------------------------------------------------------------------------ distance transform
MAX_DISTANCE_SIDE = 1024
_DIST_EDT, _DIST_SQUARED, _DIST_SIGNED, _DIST_BALL = 0, 1, 2, 3


def _distance_sides(shape) -> None:
    if any(s > MAX_DISTANCE_SIDE for s in shape):
        raise ValueError(f"postprocess: the distance transform takes sides up to {MAX_DISTANCE_SIDE}, got {tuple(shape)}")


def _sampling(sampling, n: int):
    """None for unit sampling (the exact int32 path), else N (z, y, x) triples."""
    sp = parse_spacing(sampling, n, "postprocess: sampling")
    if sp is None or all(C.c_float(v).value == 1.0 for t in sp for v in t):
        return None
    return sp


def _radius2(radius, what: str = "radius") -> float:
    if isinstance(radius, bool) or not isinstance(radius, Real):
        raise ValueError(f"postprocess: {what} must be a real number, got {radius!r}")
    r = float(radius)
    if not (math.isfinite(r) and r > 0.0 and r * r < 3.0e38):
        raise ValueError(f"postprocess: {what} must be positive and finite, got {radius!r}")
    return r * r


def _flag(v, what: str) -> bool:
    if not isinstance(v, (bool, Integral)):
        raise ValueError(f"postprocess: {what} must be a bool, got {v!r}")
    return bool(v)


def _distance(mask, n, shape, kind: int, spacing, has_label: int, lab: int, invert: int, border: int, want_indices: bool,
              r2: float = -1.0):
    lib = _lib.load()
    src = _lib.as_bytes(mask)
    dev = mask.device
    unit = spacing is None
    if kind == _DIST_BALL:
        out = torch.empty(mask.shape, dtype=torch.uint8, device=dev)
    else:
        out = torch.empty(mask.shape, dtype=torch.int32 if (kind == _DIST_SQUARED and unit) else torch.float32, device=dev)
    idx = None
    if want_indices:
        idx = torch.empty(tuple(mask.shape[:-3]) + (3,) + tuple(shape), dtype=torch.int32, device=dev)
    sp = None if unit else _lib.float_array(v for t in spacing for v in t)
    ws = torch.empty(lib.ctu_distance_ws_bytes(n, *shape, kind, int(want_indices)), dtype=torch.uint8, device=dev)
    with _lib.on(dev) as run:
        run("ctu_distance_transform", src.data_ptr(), _lib.DTYPE_CODE[src.dtype], n, *shape, has_label, lab, invert, border, sp,
            kind, out.data_ptr(), idx.data_ptr() if want_indices else None, r2, ws.data_ptr())
    return out, idx


def distance_transform_edt(mask: torch.Tensor, sampling=None, return_distances: bool = True, return_indices: bool = False,
                           label: Optional[int] = None, squared: bool = False):
    """``scipy.ndimage.distance_transform_edt`` of a bool / uint8 / int64 mask [D,H,W] or [N,D,H,W]: the distance of every
    voxel to the nearest background voxel (module docstring).  Returns the float32 distances (``squared=True``: the squared
    distances, int32 at unit sampling), the int32 indices, or the tuple of both, as scipy does."""
    n, shape = _volume(mask, "mask", _MASK_DTYPES)
    _distance_sides(shape)
    sp = _sampling(sampling, n)
    has_label, lab = _label_arg(label)
    want_d, want_i, sq = _flag(return_distances, "return_distances"), _flag(return_indices, "return_indices"), \
        _flag(squared, "squared")
    if not (want_d or want_i):
        raise ValueError("postprocess: at least one of return_distances and return_indices must be true")
    _lib.check_device(_ON_GPU, mask)
    out, idx = _distance(mask, n, shape, _DIST_SQUARED if sq else _DIST_EDT, sp, has_label, lab, 0, 0, want_i)
    if want_d and want_i:
        return out, idx
    return out if want_d else idx


def signed_distance(mask: torch.Tensor, sampling=None, label: Optional[int] = None) -> torch.Tensor:
    """float32 signed distance of a bool / uint8 / int64 mask [D,H,W] or [N,D,H,W]: the distance to the object outside it,
    minus the distance to the background inside it (module docstring)."""
    n, shape = _volume(mask, "mask", _MASK_DTYPES)
    _distance_sides(shape)
    sp = _sampling(sampling, n)
    has_label, lab = _label_arg(label)
    _lib.check_device(_ON_GPU, mask)
    return _distance(mask, n, shape, _DIST_SIGNED, sp, has_label, lab, 0, 0, False)[0]


def _ball(mask: torch.Tensor, mode: int, r2: float, spacing, has_label: int = 0, lab: int = 0) -> torch.Tensor:
    """One ball erosion / dilation of a validated device mask; uint8 0 / 1."""
    n = 1 if mask.dim() == 3 else mask.shape[0]
    erode = mode == _ERODE
    return _distance(mask, n, tuple(mask.shape[-3:]), _DIST_BALL, spacing, has_label, lab, 0 if erode else 1,
                     1 if erode else 0, False, r2)[0]


def _ball_op(mask, modes, radius, sampling, label) -> torch.Tensor:
    n, shape = _volume(mask, "mask", _MASK_DTYPES)
    _distance_sides(shape)
    r2 = _radius2(radius)
    sp = _sampling(sampling, n)
    has_label, lab = _label_arg(label)
    _lib.check_device(_ON_GPU, mask)
    out = _ball(mask, modes[0], r2, sp, has_label, lab)
    for mode in modes[1:]:
        out = _ball(out, mode, r2, sp)
    return _finish(out, mask)


def ball_erosion(mask: torch.Tensor, radius: float, sampling=None, label: Optional[int] = None) -> torch.Tensor:
    """Erosion by the ball of ``radius`` (units of ``sampling``): the voxels farther than ``radius`` from every background
    voxel and from the outside of the volume; ``scipy.ndimage.binary_erosion`` with the ball structure, border value 0."""
    return _ball_op(mask, (_ERODE,), radius, sampling, label)


def ball_dilation(mask: torch.Tensor, radius: float, sampling=None, label: Optional[int] = None) -> torch.Tensor:
    """Dilation by the ball of ``radius``: the voxels within ``radius`` of a foreground voxel."""
    return _ball_op(mask, (_DILATE,), radius, sampling, label)


def ball_opening(mask: torch.Tensor, radius: float, sampling=None, label: Optional[int] = None) -> torch.Tensor:
    """Ball erosion, then ball dilation."""
    return _ball_op(mask, (_ERODE, _DILATE), radius, sampling, label)


def ball_closing(mask: torch.Tensor, radius: float, sampling=None, label: Optional[int] = None) -> torch.Tensor:
    """Ball dilation, then ball erosion (border value 0: closing erodes at the volume border, as scipy's does)."""
    return _ball_op(mask, (_DILATE, _ERODE), radius, sampling, label)


def distance_workspace_bytes(n: int, shape, return_indices: bool = False) -> int:
    """Device workspace (bytes) of one ``distance_transform_edt`` call on n items of a (D, H, W) volume: the maps are
    computed inside the result, so only the indices need room (three int16 planes, 6 bytes per voxel)."""
    return int(_lib.load().ctu_distance_ws_bytes(n, *shape, _DIST_EDT, int(bool(return_indices))))


# ------------------------------------------------------------------------------------------------ local thickness
def local_thickness(mask: torch.Tensor, sampling=None, label: Optional[int] = None) -> torch.Tensor:
    """Local thickness of a bool / uint8 / int64 mask [D,H,W] or [N,D,H,W] (each item on its own, with its own sampling
    triple where given): every foreground voxel gets the diameter, in the units of ``sampling``, of the largest ball
    inscribed in the foreground that contains it; background gets 0, an item without background ``+inf`` (module
    docstring).  float32, of the mask's shape.  With voxel centres a plate of ``k`` voxels reads ``2 ceil(k / 2)``: the
    result is the true thickness plus 0 to 1 voxel, as ImageJ's, and is not corrected."""
    n, shape = _volume(mask, "mask", _MASK_DTYPES)
    _distance_sides(shape)
    sp = _sampling(sampling, n)
    has_label, lab = _label_arg(label)
    _lib.check_device(_ON_GPU, mask)
    lib = _lib.load()
    d2 = _distance(mask, n, shape, _DIST_SQUARED, sp, has_label, lab, 0, 0, False)[0]
    is_float = int(sp is not None)
    out = torch.empty(mask.shape, dtype=torch.float32, device=mask.device)
    ws = torch.empty(lib.ctu_thickness_ws_bytes(n, *shape, is_float), dtype=torch.uint8, device=mask.device)
    with _lib.on(mask.device) as run:
        run("ctu_local_thickness", d2.data_ptr(), is_float, n, *shape,
            None if sp is None else _lib.float_array(v for t in sp for v in t), out.data_ptr(), ws.data_ptr())
    return out


def _min_thickness(min_thickness) -> float:
    if min_thickness is None:
        return 0.0
    if isinstance(min_thickness, bool) or not isinstance(min_thickness, Real):
        raise ValueError(f"postprocess: min_thickness must be a real number or None, got {min_thickness!r}")
    m = float(min_thickness)
    if not m >= 0.0:
        raise ValueError(f"postprocess: min_thickness must be >= 0 and not NaN, got {min_thickness!r}")
    return m


def thickness_summary(thickness: torch.Tensor, min_thickness: Optional[float] = None) -> torch.Tensor:
    """Summary of a ``local_thickness`` map [D,H,W] or [N,D,H,W]: the float64 device tensor [5] or [N,5] of (foreground
    count, min, max, mean, count below ``min_thickness``) per item, with no read-back.  Foreground is ``thickness > 0``;
    ``min_thickness=None`` counts nothing as below; an item without foreground gives (0, +inf, 0, NaN, 0)."""
    n, shape = _volume(thickness, "thickness", (torch.float32,))
    mt = _min_thickness(min_thickness)
    _lib.check_device(_ON_GPU, thickness)
    lib = _lib.load()
    src = thickness.contiguous()
    v = shape[0] * shape[1] * shape[2]
    out = torch.empty((n, 5) if thickness.dim() == 4 else (5,), dtype=torch.float64, device=thickness.device)
    ws = torch.empty(lib.ctu_thickness_summary_ws_bytes(n, v), dtype=torch.uint8, device=thickness.device)
    with _lib.on(thickness.device) as run:
        run("ctu_thickness_summary", src.data_ptr(), n, v, mt, out.data_ptr(), ws.data_ptr())
    return out


def thickness_workspace_bytes(n: int, shape, sampling=None) -> int:
    """Temporary device memory (bytes) of one ``local_thickness`` call on n items of a (D, H, W) volume, the result not
    counted: the squared distance map (4 bytes per voxel), the transform's own workspace and the search's (the pruned
    candidate map, 4 bytes per voxel, and one maximum per 8x8x8 cell and per item)."""
    sp = _sampling(sampling, n)
    lib = _lib.load()
    own = int(lib.ctu_thickness_ws_bytes(n, *shape, int(sp is not None)))
    if own == 0:
        raise ValueError(f"postprocess: local_thickness takes 1..65535 items of sides 1..{MAX_DISTANCE_SIDE} with fewer "
                         f"than 2^31 voxels, got n={n!r}, shape={tuple(shape)}")
    return own + 4 * n * shape[0] * shape[1] * shape[2] + int(lib.ctu_distance_ws_bytes(n, *shape, _DIST_SQUARED, 0))


# ------------------------------------------------------------------------------------------------ region properties
MAX_REGIONS = 65536                    # CTU_REGION_MAX
MAX_REGION_SIDE = 1024                 # the volume kernels' MAX_SIDE: keeps every moment below 2^53, exact in float64
_LABEL_DTYPES = (torch.bool, torch.uint8, torch.int32, torch.int64)


class RegionProperties(NamedTuple):
    """Device tensors of ``region_properties`` (module docstring): ``moments`` int64 [N,R,10], ``boxes`` int32 [N,R,6],
    ``overflow`` int64 [N], ``centroid`` float64 [N,R,3], ``covariance`` float64 [N,R,3,3], ``extent`` float64 [N,R,3],
    ``axes`` float64 [N,R,3,3]."""
    moments: torch.Tensor
    boxes: torch.Tensor
    overflow: torch.Tensor
    centroid: torch.Tensor
    covariance: torch.Tensor
    extent: torch.Tensor
    axes: torch.Tensor


def _num_regions(num_regions) -> int:
    if isinstance(num_regions, bool) or not isinstance(num_regions, Integral) or not 1 <= num_regions <= MAX_REGIONS:
        raise ValueError(f"postprocess: num_regions must be an integer in 1..{MAX_REGIONS}, got {num_regions!r}")
    return int(num_regions)


def _region_sides(shape) -> None:
    if any(s > MAX_REGION_SIDE for s in shape):
        raise ValueError(f"postprocess: region properties take sides up to {MAX_REGION_SIDE} (the sums stay exact in float64), "
                         f"got {tuple(shape)}")


def _origin(origin, n: int):
    """None (origin 0), else N (z, y, x) triples of finite floats: a scalar, a triple or one triple per item."""
    def finite(v):
        if isinstance(v, bool) or not isinstance(v, Real) or not math.isfinite(v):
            raise ValueError(f"postprocess: origin must hold finite numbers, got {v!r}")
        return float(v)
    if origin is None:
        return None
    if isinstance(origin, torch.Tensor):
        origin = origin.tolist()
    if isinstance(origin, Real) and not isinstance(origin, bool):
        return [[finite(origin)] * 3 for _ in range(n)]
    if not hasattr(origin, "__len__"):
        raise ValueError(f"postprocess: origin must be a number, a (z, y, x) triple or {n} such triples, got {origin!r}")
    items = list(origin)
    if len(items) == 3 and all(isinstance(v, Real) for v in items):
        return [[finite(v) for v in items] for _ in range(n)]
    if len(items) == n and all(hasattr(v, "__len__") and len(v) == 3 for v in items):
        return [[finite(v) for v in t] for t in items]
    raise ValueError(f"postprocess: origin must be a number, a (z, y, x) triple or {n} such triples, got {origin!r}")


def region_properties(labels: torch.Tensor, num_regions: int, sampling=None, origin=None) -> RegionProperties:
    """Voxel count, first and second moments, bounding box, centroid, covariance and principal axes of the regions
    1..``num_regions`` of a bool / uint8 / int32 / int64 label map [D,H,W] or [N,D,H,W] (module docstring, "Region
    properties").  Every result keeps the leading N (1 for a [D,H,W] map).  One pass over the map, no read-back."""
    n, shape = _volume(labels, "labels", _LABEL_DTYPES)
    _region_sides(shape)
    R = _num_regions(num_regions)
    sp = parse_spacing(sampling, n, "postprocess: sampling")
    org = _origin(origin, n)
    _lib.check_device(_ON_GPU, labels)
    lib = _lib.load()
    src = _lib.as_bytes(labels)
    dev = labels.device
    moments = torch.empty((n, R, 10), dtype=torch.int64, device=dev)
    boxes = torch.empty((n, R, 6), dtype=torch.int32, device=dev)
    overflow = torch.empty((n,), dtype=torch.int64, device=dev)
    centroid = torch.empty((n, R, 3), dtype=torch.float64, device=dev)
    covariance = torch.empty((n, R, 3, 3), dtype=torch.float64, device=dev)
    extent = torch.empty((n, R, 3), dtype=torch.float64, device=dev)
    axes = torch.empty((n, R, 3, 3), dtype=torch.float64, device=dev)
    ws = torch.empty(lib.ctu_region_moments_ws_bytes(n, R), dtype=torch.uint8, device=dev)
    frame = None
    if sp is not None or org is not None:
        frame = _lib.double_array(v for i in range(n) for v in ((sp[i] if sp else [1.0] * 3) + (org[i] if org else [0.0] * 3)))
    with _lib.on(dev) as run:
        run("ctu_region_moments", src.data_ptr(), _lib.DTYPE_CODE[src.dtype], n, *shape, R, moments.data_ptr(), boxes.data_ptr(),
            overflow.data_ptr(), ws.data_ptr())
        run("ctu_region_derive", moments.data_ptr(), n, R, frame, centroid.data_ptr(), covariance.data_ptr(), extent.data_ptr(),
            axes.data_ptr())
    return RegionProperties(moments, boxes, overflow, centroid, covariance, extent, axes)


def region_workspace_bytes(n: int, num_regions: int) -> int:
    """Device workspace (bytes) of one ``region_properties`` call: the box accumulators, 24 bytes per (item, region)."""
    return int(_lib.load().ctu_region_moments_ws_bytes(int(n), _num_regions(num_regions)))


def _margin(margin):
    if isinstance(margin, Integral) and not isinstance(margin, bool):
        margin = (margin,) * 3
    try:
        m = tuple(margin)
    except TypeError:
        m = ()
    if len(m) != 3 or any(isinstance(v, bool) or not isinstance(v, Integral) or not 0 <= v <= MAX_REGION_SIDE for v in m):
        raise ValueError(f"postprocess: margin must be an integer or a (z, y, x) triple of integers in 0..{MAX_REGION_SIDE}, "
                         f"got {margin!r}")
    return tuple(int(v) for v in m)


def bounding_box(labels: torch.Tensor, region: int = 1, margin=0, multiple_of: int = 1,
                 num_regions: Optional[int] = None) -> torch.Tensor:
    """The box of region ``region`` of a label map [D,H,W] or [N,D,H,W] as a region of interest: device int32 [N,6] =
    (z0, y0, x0, z1, y1, x1), half open, grown by ``margin`` voxels (an int or a (z, y, x) triple), then to sides that are
    multiples of ``multiple_of``, shifted back inside the volume where that fits and clipped where it does not (module
    docstring); the whole volume for an empty region.  ``num_regions`` (default ``region``) is the capacity handed to
    ``region_properties``.  Integer arithmetic on the device, no read-back."""
    n, shape = _volume(labels, "labels", _LABEL_DTYPES)
    _region_sides(shape)
    R = _num_regions(region if num_regions is None else num_regions)
    if isinstance(region, bool) or not isinstance(region, Integral) or not 1 <= region <= R:
        raise ValueError(f"postprocess: region must be an integer in 1..num_regions = {R}, got {region!r}")
    mg = _margin(margin)
    if isinstance(multiple_of, bool) or not isinstance(multiple_of, Integral) or not 1 <= multiple_of <= MAX_REGION_SIDE:
        raise ValueError(f"postprocess: multiple_of must be an integer in 1..{MAX_REGION_SIDE}, got {multiple_of!r}")
    m = int(multiple_of)
    p = region_properties(labels, R)
    return _grow_boxes(p.boxes[:, region - 1], p.moments[:, region - 1, 0] != 0, shape, mg, m)


def _grow_boxes(boxes: torch.Tensor, some: torch.Tensor, shape, mg, m: int) -> torch.Tensor:
    """The arithmetic of ``bounding_box`` on one region's boxes [N,6] and its "not empty" flags [N], on their device."""
    box = boxes.to(torch.int64)
    cols = [None] * 6
    for a in range(3):
        S = shape[a]
        lo, hi = box[:, a] - mg[a], box[:, 3 + a] + mg[a]
        side = (hi - lo + (m - 1)) // m * m
        lo = lo - (side - (hi - lo)) // 2
        lo = torch.clamp(torch.minimum(lo, S - side), min=0)
        fits = (side <= S) & some
        zero = torch.zeros_like(lo)
        cols[a] = torch.where(fits, lo, zero)
        cols[3 + a] = torch.where(fits, lo + side, zero + S)
    return torch.stack(cols, dim=1).to(torch.int32)


def crop_to_box(x: torch.Tensor, box) -> Tuple[torch.Tensor, tuple]:
    """``(view, slices)``: the part of ``x`` [..., D, H, W] inside ``box`` = (z0, y0, x0, z1, y1, x1) (a [6] or [1,6] tensor, as
    ``bounding_box`` returns for one item, or six integers).  The shape of the result depends on the data, so the six
    integers of a device box are read back: the one synchronisation.  ``view`` is ``x[(..., *slices)]``, a view, never a
    copy; a result computed on it goes back with ``out[(..., *slices)] = result``."""
    if not isinstance(x, torch.Tensor) or x.dim() < 3:
        raise ValueError("postprocess: x must be a tensor whose last three dimensions are (D, H, W)")
    vals = box.flatten().tolist() if isinstance(box, torch.Tensor) else list(box)
    if len(vals) != 6 or any(isinstance(v, bool) or not isinstance(v, Integral) for v in vals):
        raise ValueError(f"postprocess: box must hold the six integers (z0, y0, x0, z1, y1, x1) of one item, got {box!r}")
    for a in range(3):
        if not 0 <= vals[a] < vals[3 + a] <= x.shape[-3 + a]:
            raise ValueError(f"postprocess: box {vals} does not lie inside a volume of shape {tuple(x.shape[-3:])}")
    slices = tuple(slice(int(vals[a]), int(vals[3 + a])) for a in range(3))
    return x[(..., *slices)], slices
