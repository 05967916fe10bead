"""Rigid registration of a binary skull to a fixed mask (the atlas) on the GPU, by chamfer matching against a distance
field: the step that takes a scan into the atlas frame ``UNetSP`` expects, and with ``resample.affine_resample`` and
``mesh.transform`` a result back out (``ctu_registration_*`` of ``csrc/registration.hip``); no CPU fallback.

    r = register(skull, atlas, moving_spacing=(0.8, 0.45, 0.45), fixed_spacing=1.0)     # RegistrationResult
    in_atlas = resample.affine_resample(skull, r.inverse, atlas.shape, spacing=(0.8, 0.45, 0.45), mode="label_linear",
                                        num_classes=2)
    r.report()                                                                          # the one read-back

``register_points(points, field)`` is the optimiser itself: ``points`` float32 ``[P,3]`` in the world mm of the moving frame,
order (z, y, x) -- surface voxels, or the vertices of ``mesh.extract_surface``; callers who want fewer slice them -- and
``field`` float32 ``[D,H,W]``, the distance in mm to the fixed object on the fixed grid (world coordinate of voxel index ``k``:
``origin + k * spacing``).  The distance is DIRECTED from the moving set to the fixed object: every point of a skull with a
hole still has a counterpart on the full atlas, so the defect does not bias the fit.  ``register`` is plumbing over existing
operations: points = the world coordinates of ``mask & ~binary_erosion(mask)``, field =
``distance_transform_edt(fixed == 0, sampling)``, ``init="centroid"`` translates the moving mask's centroid onto the fixed
mask's (or pass a ``[4,4]`` tensor).

The result: ``matrix`` device float64 ``[4,4]``, moving world -> fixed world; ``inverse`` its closed form
(``R^T, -R^T t``), written by the same kernel -- the ``out_to_in`` of ``affine_resample`` onto the fixed grid; ``history``
device float64 ``[iterations + 1, 4]`` = (cost / P, inliers, lambda, 1 accepted / 0 rejected / -1 refused).

The pinned rule (``tests/registration_ref.py`` restates it in numpy), all float64, every operation rounded on its own:

Sample, for ``q = R p + t`` (``q_a = ((m_a0 p_0 + m_a1 p_1) + m_a2 p_2) + m_a3``): ``u_a = (q_a - origin_a) / spacing_a``; the
point is *inside* iff ``u`` is finite and every ``0 <= u_a <= n_a - 1``; ``i0_a = min(floor(u_a), n_a - 2)``,
``f_a = u_a - i0_a``; ``v`` is the trilinear interpolant of the eight float32 samples widened to float64,
``lerp(p, q, w) = p + w (q - p)`` along x, then y, then z; ``g`` is the analytic gradient of that interpolant divided by the
spacing per axis.  A field with a side of 1 is refused.

Residual: a point is an *inlier* iff it is inside and ``v <= max_distance`` (``None``: +inf).  Inlier: ``r = v`` and the
Jacobian row ``J = [(q - pivot) x g, g]`` (rotation increment about ``pivot``, then translation; the cross product in the
index order of the vectors), ``pivot = R mean(points) + t`` of the candidate, the mean taken over the finite points.  Any
other point (a non-finite one included): ``r = max_distance`` (0 without a bound), ``J = 0``.  ``cost = sum r^2``,
``H = sum J^T J``, ``b = sum J^T v`` over the inliers.

Iteration (Levenberg-Marquardt): state ``M = init``, ``cost = +inf``, ``lambda = 1e-3``, candidate ``M_c = init``.  For ``it``
in ``0..iterations``: accumulate at ``M_c``; if ``cost_c < cost`` accept (``(M, cost, H, b, pivot, inliers) <- candidate``,
``lambda <- max(lambda / 3, 1e-9)``), otherwise ``lambda <- min(10 lambda, 1e9)``; solve
``(H + lambda diag(H) + 1e-12 I) delta = -b`` by a 6x6 Cholesky factorisation; the next candidate is ``M_c = E M`` with
``E = [Rod(delta_w), pivot - Rod(delta_w) pivot + delta_t]``.  The step is *refused* -- the candidate stays, the history row
holds -1 -- when the accepted state has fewer than 6 inliers (fewer than unknowns: only the damping would make the system
solvable), a pivot of the factorisation is not positive, or the result is not finite; no NaN matrix is ever produced.
Scale, shear, intensity metrics, pyramids, principal-axis starts, subsampling and random warps are out of scope.

A ``register_points`` call is ``1 + 2 (iterations + 1)`` launches on one stream (the mean of the points and the start
state; then accumulate and update per iteration): no host synchronisation, no float atomics, no allocation besides the
result and the workspace (``workspace_bytes(P)``; pass ``workspace=`` to bring your own), so it can be captured into a graph,
and two calls are bit-equal.  ``RegistrationResult.report()`` is the one read-back.
"""
from __future__ import annotations

import math
from numbers import Integral, Real
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _args, _lib

MAX_BLOCKS = 1024                      # CTU_REG_MAX_BLOCKS of ctunet_hip.h
_HEAD_DOUBLES = 128                    # the workspace head: 1024 bytes
_PIVOT_C = 62                          # the candidate's pivot in the head (layout: ctunet_hip.h)
_ROW = 32                              # doubles of a slab row


class RegistrationResult(NamedTuple):
    """``matrix`` / ``inverse`` device float64 [4,4] (moving world -> fixed world and back), ``history`` device float64
    [iterations + 1, 4] = (cost / P, inliers, lambda, 1 accepted / 0 rejected / -1 refused), ``num_points`` P."""
    matrix: torch.Tensor
    inverse: torch.Tensor
    history: torch.Tensor
    num_points: int = 0

    def report(self) -> dict:
        """Reads the history back (one synchronisation): ``rms`` distance in mm of the accepted matrix, ``inlier_fraction``,
        ``accepted`` steps and ``status`` (0, or -1 when the last step was refused: too few inliers to move at all)."""
        h = self.history.cpu().numpy()
        last = h[-1]
        return dict(rms=float(np.sqrt(last[0])), inlier_fraction=float(last[1] / max(self.num_points, 1)),
                    accepted=int((h[:, 3] == 1).sum()), status=-1 if last[3] < 0 else 0, iterations=int(h.shape[0] - 1))


_REAL = _args.Triple(shape="registration: {what} must be a number or a (z, y, x) triple, got {v!r}",
                     value="registration: {what} must be finite, got {v!r}")
_REAL_POSITIVE = _REAL._replace(value="registration: {what} must be positive and finite, got {v!r}", sign=_args.POSITIVE)
_ON_GPU = "registration: {} must live on the GPU; this path has no CPU fallback"


def _frame(spacing, origin, prefix: str = ""):
    """The host (z, y, x) triples of a grid's ``spacing`` and ``origin`` arguments; None stays None."""
    return (_args.triple(spacing, _REAL_POSITIVE, what=prefix + "spacing"),
            _args.triple(origin, _REAL, what=prefix + "origin"))


def _bound(max_distance) -> float:
    if max_distance is None:
        return math.inf
    if isinstance(max_distance, bool) or not isinstance(max_distance, Real) or math.isnan(max_distance) or max_distance < 0:
        raise ValueError(f"registration: max_distance must be None or a number >= 0, got {max_distance!r}")
    return float(max_distance)


def _check_inputs(points, field):
    if not isinstance(points, torch.Tensor) or not isinstance(field, torch.Tensor):
        raise TypeError("registration: points and field must be tensors")
    if points.dtype != torch.float32 or field.dtype != torch.float32:
        raise TypeError(f"registration: points and field must be float32, got {points.dtype} and {field.dtype}")
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError(f"registration: points must be [P,3] with P >= 1, got {tuple(points.shape)}")
    if field.dim() != 3:
        raise ValueError(f"registration: field must be one [D,H,W] volume, got {tuple(field.shape)}")
    if min(field.shape) < 2:
        raise ValueError(f"registration: a field with a side of 1 has no gradient along it, got {tuple(field.shape)}")
    if field.numel() >= 1 << 31:
        raise ValueError(f"registration: the field must hold fewer than 2^31 voxels, got {tuple(field.shape)}")


def _check_init(init, device):
    if init is None:
        return None
    if not isinstance(init, torch.Tensor) or init.dtype != torch.float64 or tuple(init.shape) != (4, 4):
        raise ValueError("registration: init must be a float64 [4,4] tensor (moving world -> fixed world)")
    if init.device != device:
        raise ValueError(f"registration: init lives on {init.device}, the points on {device}")
    return init.contiguous()


def workspace_bytes(P: int) -> int:
    """Device workspace (bytes) of a registration of ``P`` points: the state (1024 bytes) and one slab row of 256 bytes per
    block of the accumulation, at most 1024 blocks; 0 for P < 1."""
    return int(_lib.load().ctu_registration_ws_bytes(int(P)))


def _workspace(P: int, device, workspace):
    need = workspace_bytes(P)
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=device)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != device \
            or not workspace.is_contiguous() or workspace.numel() < need or workspace.data_ptr() % 8:
        raise ValueError(f"registration: workspace must be a contiguous, 8-byte aligned uint8 tensor of at least {need} bytes "
                         f"on {device}")
    return workspace


def register_points(points: torch.Tensor, field: torch.Tensor, *, spacing=None, origin=None, init=None, iterations: int = 30,
                    max_distance=None, workspace=None) -> RegistrationResult:
    """Fit the rigid matrix that takes ``points`` (float32 [P,3], moving world) onto the zero set of ``field`` (float32
    [D,H,W] distances on the fixed grid of ``spacing`` / ``origin``) by the module docstring's rule."""
    _check_inputs(points, field)
    if isinstance(iterations, bool) or not isinstance(iterations, Integral) or not 0 <= iterations <= 10000:
        raise ValueError(f"registration: iterations must be an integer in 0..10000, got {iterations!r}")
    bound = _bound(max_distance)
    sp, org = _frame(spacing, origin)
    _lib.check_device(_ON_GPU.format("points and field"), points, field)
    if points.device != field.device:
        raise ValueError(f"registration: points live on {points.device}, the field on {field.device}")
    dev = points.device
    init = _check_init(init, dev)
    pts, fld = points.contiguous(), field.contiguous()
    P, rows = int(pts.shape[0]), int(iterations) + 1
    ws = _workspace(P, dev, workspace)
    out = torch.empty((32 + 4 * rows,), dtype=torch.float64, device=dev)
    matrix, inverse, history = out[:16].view(4, 4), out[16:32].view(4, 4), out[32:].view(rows, 4)
    c_sp, c_org = _lib.double_array(sp), _lib.double_array(org)
    with _lib.on(dev) as run:
        run("ctu_registration_init", pts.data_ptr(), P, None if init is None else init.data_ptr(), ws.data_ptr())
        for it in range(rows):
            run("ctu_registration_accumulate", pts.data_ptr(), P, fld.data_ptr(), *fld.shape, c_sp, c_org, bound, ws.data_ptr())
            run("ctu_registration_update", P, it, matrix.data_ptr(), inverse.data_ptr(), history.data_ptr(), rows, ws.data_ptr())
    return RegistrationResult(matrix, inverse, history, P)


def accumulate(points: torch.Tensor, field: torch.Tensor, matrix: torch.Tensor, *, spacing=None, origin=None,
               max_distance=None) -> dict:
    """One accumulation at ``matrix`` (device float64 [4,4]), read back for inspection: ``H`` [21] (upper triangle, row by
    row), ``b`` [6], ``cost``, ``count``, and the ``pivot`` the Jacobian rows were taken about -- numpy float64, the slab rows
    summed in block order as the update kernel sums them."""
    _check_inputs(points, field)
    bound = _bound(max_distance)
    sp, org = _frame(spacing, origin)
    _lib.check_device(_ON_GPU.format("points and field"), points, field)
    dev = points.device
    matrix = _check_init(matrix, dev)
    pts, fld = points.contiguous(), field.contiguous()
    P = int(pts.shape[0])
    ws = _workspace(P, dev, None)
    with _lib.on(dev) as run:
        run("ctu_registration_init", pts.data_ptr(), P, None if matrix is None else matrix.data_ptr(), ws.data_ptr())
        run("ctu_registration_accumulate", pts.data_ptr(), P, fld.data_ptr(), *fld.shape, _lib.double_array(sp),
            _lib.double_array(org), bound, ws.data_ptr())
    host = ws.cpu().numpy().view(np.float64)
    slab = host[_HEAD_DOUBLES:].reshape(-1, _ROW)
    tot = np.zeros(28)
    for row in slab:                                                   # block order
        tot += row[:28]
    return dict(H=tot[:21], b=tot[21:27], cost=float(tot[27]), count=int(slab[:, 28].copy().view(np.int64).sum()),
                pivot=host[_PIVOT_C:_PIVOT_C + 3].copy(), blocks=int(slab.shape[0]))


def _mask(t, what: str):
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"registration: {what} must be one bool or uint8 [D,H,W] mask")


def _world(index: torch.Tensor, spacing, origin) -> torch.Tensor:
    """float64 world coordinates origin + k spacing of int64 voxel indices [P,3]."""
    sp = torch.tensor(spacing or (1.0, 1.0, 1.0), dtype=torch.float64, device=index.device)
    org = torch.tensor(origin or (0.0, 0.0, 0.0), dtype=torch.float64, device=index.device)
    return org + index.to(torch.float64) * sp


def surface_points(mask: torch.Tensor, spacing=None, origin=None) -> torch.Tensor:
    """float32 [P,3] world coordinates (z, y, x) of the surface voxels ``mask & ~binary_erosion(mask)``, in C order."""
    from . import postprocess
    _mask(mask, "mask")
    sp, org = _frame(spacing, origin)
    _lib.check_device(_ON_GPU.format("the masks"), mask)
    m = mask != 0
    surf = m & ~(postprocess.binary_erosion(m) != 0)
    return _world(torch.nonzero(surf), sp, org).to(torch.float32)


def register(moving_mask: torch.Tensor, fixed_mask: torch.Tensor, *, moving_spacing=None, moving_origin=None,
             fixed_spacing=None, fixed_origin=None, iterations: int = 30, max_distance=None, init="centroid") -> RegistrationResult:
    """Register the binary ``moving_mask`` to ``fixed_mask`` (the atlas), each a bool / uint8 [D,H,W] volume on its own grid:
    the surface voxels of the moving mask against the exact distance field of the fixed one (module docstring)."""
    from . import postprocess
    _mask(moving_mask, "moving_mask")
    _mask(fixed_mask, "fixed_mask")
    (msp, morg), (fsp, forg) = _frame(moving_spacing, moving_origin, "moving_"), _frame(fixed_spacing, fixed_origin, "fixed_")
    if isinstance(init, str):
        if init != "centroid":
            raise ValueError(f"registration: init must be 'centroid' or a float64 [4,4] tensor, got {init!r}")
    elif init is not None:
        init = _check_init(init, moving_mask.device)
    _lib.check_device(_ON_GPU.format("the masks"), moving_mask, fixed_mask)
    if moving_mask.device != fixed_mask.device:
        raise ValueError("registration: the two masks must live on the same device")
    points = surface_points(moving_mask, msp, morg)
    if points.shape[0] < 1:
        raise ValueError("registration: the moving mask is empty")
    fixed = fixed_mask != 0
    fixed_index = torch.nonzero(fixed)
    if fixed_index.shape[0] < 1:
        raise ValueError("registration: the fixed mask is empty")
    field = postprocess.distance_transform_edt(~fixed, sampling=fsp)
    if isinstance(init, str):
        cm = _world(torch.nonzero(moving_mask != 0), msp, morg).mean(0)
        cf = _world(fixed_index, fsp, forg).mean(0)
        init = torch.eye(4, dtype=torch.float64, device=points.device)
        init[:3, 3] = cf - cm
    return register_points(points, field, spacing=fsp, origin=forg, init=init, iterations=iterations,
                           max_distance=max_distance)
