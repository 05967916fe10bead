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
Shear and affine fits, intensity metrics, pyramids, subsampling and random warps are out of scope
(DESIGN.md); isotropic scale is the similarity model below.

A ``register_points`` call is ``1 + 2 (iterations + 1)`` launches on one stream (the mean of the points and the start
state; then accumulate and update per iteration): no host synchronisation, no float atomics, no allocation besides the
result and the workspace (``workspace_bytes(P)``; pass ``workspace=`` to bring your own), so it can be captured into a graph,
and two calls are bit-equal.  ``RegistrationResult.report()`` is the one read-back.

Principal-axes starts
---------------------

    r = register(skull, atlas, moving_spacing=(0.8, 0.45, 0.45), fixed_spacing=1.0, init="moments")

A scan that arrives turned (prone, feet first, a swapped axis, a strongly tilted gantry) sends the iteration from the centroid
start into a wrong basin, and the rms it reports there looks plausible.  ``init="moments"`` runs the chosen optimiser (rigid or
similarity, symmetric or not, unchanged) from five starts and keeps the best; the surface points and the distance fields are
computed once.  ``principal_frame(mask, spacing, origin)`` gives ``(centroid [3], axes [3,3], extent [3])``, float64 on the
device, from ``postprocess.region_properties`` of the binary mask (one pass of ``ctu_region_moments``; the rule of the axes, their
signs and their right-handedness is pinned there).  With ``A_m`` / ``A_f`` the frames and ``c_m`` / ``c_f`` the centroids of the
moving and the fixed mask, start ``k < 4`` is the proper rotation ``R = A_f diag(s_k) A_m^T``, ``s`` = (+,+,+), (+,-,-), (-,+,-),
(-,-,+), with the translation ``c_f - R c_m``; start 4 is the identity rotation with ``c_f - c_m``: the centroid start, its
centroids taken from the moments.  Selection, on the device and without a synchronisation, from the last history row of
every start: among the starts whose final inlier count is at least half the largest final inlier count, the lowest final
cost / P; the lowest index wins a tie.  The inlier condition matters: with ``max_distance=None`` a point thrown outside the
fixed field costs nothing.  ``RegistrationResult.candidate`` holds the chosen index.  A region with nearly equal extents has
ill-defined axes: nothing is promised then beyond the centroid start, and thanks to the fifth start nothing is lost.
Reflections are not tried.  The cost is five optimiser runs and two passes over the masks.

Similarity registration with the symmetric chamfer cost
-------------------------------------------------------

    r = register(skull, atlas, moving_spacing=(0.8, 0.45, 0.45), fixed_spacing=1.0, model="similarity", max_distance=4.0)

Heads differ in size by several percent, which six rigid parameters cannot absorb.  ``register(..., model="similarity")``
fits a seventh, isotropic scale, and by default (``symmetric=True``) adds the reverse distance to the cost: the surface points
of the fixed mask (``surface_points(fixed_mask)``), pulled back through the inverse matrix, against the distance field of the
moving mask (``distance_transform_edt(moving == 0, sampling=moving_spacing)``).  With a hole in the moving skull pass a
``max_distance`` of a few mm: the atlas's points over the hole have no counterpart and must saturate.  The directed cost alone
(``symmetric=False``) does not collapse but recovers the scale 0.4-0.45 % too small on the analytic skull of the tests; the
symmetric cost is within 0.06 %.  ``model="rigid", symmetric=True`` runs the same kernels with six unknowns; the defaults
(``model="rigid"``, ``symmetric=None``) take the rigid path above, bit for bit.  ``register_similarity_points`` is the optimiser
itself, ``accumulate_similarity`` one accumulation read back (``ctu_similarity_*``; ``tests/similarity_ref.py`` restates the
rule).  ``history`` has six columns: (cost / (P + Q), inliers of both terms, lambda, flag, backward inliers,
scale = cbrt(det)), and ``report()`` adds ``scale`` and ``backward_inlier_fraction``.

The pinned rule, all float64, every operation rounded on its own; the sample, the inside test, ``v``, ``g`` and ``lerp`` are the
rigid rule's.  DOF is 6 (rigid) or 7 (similarity).

Forward term, every moving point ``p`` (float32 ``[P,3]``): ``q = M_c p``; inlier iff ``q`` is inside the fixed field ``F`` and
``v = F(q) <= max_distance``; ``d = q - pivot`` and the gradient ``g``.  Backward term, every fixed point ``y`` (float32 ``[Q,3]``,
fixed world; present when Q > 0): ``x = M_c^-1 y``; inlier iff ``x`` is inside the moving field ``G`` (distance in mm to the
moving object on the moving grid, with its own spacing and origin) and ``w = G(x) <= max_distance``; the residual is ``w``,
``d = y - pivot``, and the gradient in the fixed frame is ``h_a = -((g_0 Ainv[0][a] + g_1 Ainv[1][a]) + g_2 Ainv[2][a])`` with
``g`` the gradient of ``G`` at ``x`` and ``Ainv`` the 3x3 of ``M_c^-1`` (``M_c <- E M_c`` gives ``x = M_c^-1 E^-1 y``, hence
``dw/d delta = (-Ainv^T g) . (generator y)``).  Jacobian row of either term, ``g`` standing for ``g`` or ``h``:
``J = [d x g, g, (d_0 g_0 + d_1 g_1) + d_2 g_2]`` (the last entry only for DOF 7).  A non-inlier has ``r = max_distance`` (0
without a bound) and ``J = 0``.  ``cost``, ``H`` and ``b`` run over both terms with equal weight per point, forward points
first, then backward points; ``pivot = M_c mean(finite moving points)``.

Levenberg-Marquardt as above (``lambda`` from 1e-3, accept iff the cost is lower, ``/ 3`` down to 1e-9 or ``x 10`` up to 1e9,
damping ``lambda diag(H) + 1e-12 I``) with a Cholesky factorisation of size DOF and the increment
``E = [L, pivot - L pivot + delta_t]``, ``L = exp(delta_s) Rod(delta_w)`` for DOF 7 and ``Rod(delta_w)`` for DOF 6.

The inverse is formed by the adjugate: cofactors as differences of products
(``c_ij = a_(i+1)(j+1) a_(i+2)(j+2) - a_(i+1)(j+2) a_(i+2)(j+1)``, indices mod 3), ``det = (a00 c00 + a01 c01) + a02 c02``,
entries ``c_ji / det``, translation ``-((inv_a0 t_0 + inv_a1 t_1) + inv_a2 t_2)``.  It is written into the state for the
candidate, so the accumulation reads it, and into ``inverse`` for the accepted matrix.

A step is refused (flag -1, candidate kept, no NaN ever written) with fewer than DOF inliers in total, a Cholesky pivot that is
not positive, a non-finite candidate, or a candidate whose determinant is non-finite or not positive or whose inverse is not
finite.  An ``init`` with such a determinant refuses every step: the matrix stays ``init``, the backward points count as
non-inliers, ``inverse`` reads the identity and the scale column 0.

B-spline deformable registration (free-form deformation)
--------------------------------------------------------

    d = register_deformable(skull, atlas, moving_spacing=(0.8, 0.45, 0.45), fixed_spacing=1.0, max_distance=6.0)
    prior = resample.deformable_resample(atlas, d, skull.shape, spacing=1.0, out_spacing=(0.8, 0.45, 0.45),
                                         mode="label_linear", num_classes=2)               # the atlas on the patient's grid
    in_atlas = mesh.transform(patient_mesh, d)                                             # points and meshes go forward
    d.report()                                                                             # the one read-back

A matrix cannot take the atlas onto one particular head.  ``register_deformable`` runs ``register`` (or takes ``affine=``) and
then fits a displacement field on top of the frozen matrix; ``register_ffd_points`` is that optimiser itself, ``FFDPlan`` its
two halves (the binning, which synchronises once, and ``run()``, which does not and can be captured into a graph),
``accumulate_ffd`` one accumulation read back, ``transform_points`` the transform of points (``ctu_ffd_*`` of
``csrc/ffd.hip``; ``tests/ffd_ref.py`` restates the rule).

The transform, all float64, every operation rounded on its own: ``T(p) = q0 + u(q0)``, ``q0 = M p`` as above.  ``T`` maps
moving world to fixed world, so it PULLS a fixed-frame volume onto a moving-frame grid and PUSHES moving-frame points into
the fixed frame; the inverse field is out of scope.  ``u`` is a uniform cubic B-spline over control displacements ``c``
``[3,Gz,Gy,Gx]`` (mm, fixed frame) on a lattice over the fixed field's box ``[origin, origin + (n - 1) spacing]``: with
``control_spacing`` ``h`` (a number or a triple, mm), ``ncell_a = max(1, ceil(extent_a / h_a))``, ``G_a = ncell_a + 3`` (at most
64) and control index ``i`` at ``origin_a + (i - 1) h_a``.  ``t_a = (q0_a - origin_a) / h_a`` clamped into ``[0, ncell_a]`` (a
non-finite ``t_a`` takes 0), ``cell_a = min(floor(t_a), ncell_a - 1)``, ``f_a = t_a - cell_a``: the clamp extends ``u``
continuously beyond the box.  The weights ``B(f)`` are ``RandomSpatial``'s (``tests/spatial_ref.py::bspline``) and
``u_a = sum_lmn ((Bz_l By_m) Bx_n) c_a[cell_z + l, cell_y + m, cell_x + n]``, 64 terms added in the order l, m, n (x innermost)
from 0.  Derivative weights: ``dB = (-(1 - f)^2 / 2, (3 f^2 - 4 f) / 2, ((-3 f^2 + 2 f) + 1) / 2, f^2 / 2)``, taken as zero on an
axis whose ``t_a`` was clamped; ``D_ab = sum ((dBz_l By_m) Bx_n | (Bz_l dBy_m) Bx_n | (Bz_l By_m) dBx_n)_b c_a``,
``J = I + D_ab / h_b`` and ``det`` by the first row's cofactors, ``(J00 m0 - J01 m1) + J02 m2``.

The fit.  For every point ``q = T(p)``; the sample ``v``, the inside test, the gradient ``g`` and the inlier test
(``v <= max_distance``) are the rigid rule's at ``q``.  Data cost ``1/2 sum r^2`` (``r = v`` for an inlier, ``max_distance`` or 0
otherwise); regulariser ``1/2 w sum_edges |c_i - c_j|^2`` over the 6-neighbour lattice edges, ``w = stiffness P / (Gz Gy Gx)``.
With ``B_c = (Bz_l By_m) Bx_n`` the weight of control ``c`` at a point: ``grad_c = sum_inliers (v g) B_c + w (deg_c c - sum_nbrs c_j)``
(neighbours in the order -z, +z, -y, +y, -x, +x) and the majorising diagonal ``d_c = sum_inliers |g|^2 B_c + 2 w deg_c`` (the
weights are non-negative and sum to 1, so ``(g g^T) x (B B^T) <= |g|^2 I x diag(B)``).  State: controls ``c`` (``init_control`` or
0), ``cost = +inf``, ``lambda = 1e-3``, candidate ``c_c = c``.  For ``it`` in ``0..iterations``: accumulate at ``c_c``; accept iff the
total cost is lower (``lambda <- max(lambda / 3, 1e-9)``, else ``lambda <- min(10 lambda, 1e9)``); the next candidate is
``c - grad / ((1 + lambda) d + 1e-12)`` from the accepted state.  The step is refused (flag -1, the candidate stays) when the
accepted state has no inlier or an entry of the candidate is not finite; no NaN is ever written.  History row:
(total cost / P, data rms ``sqrt(sum r^2 / P)``, regulariser energy, inliers, lambda, flag).  The device sums a cell's points in
sorted order segment by segment, and a control's cells by a fixed tree, so two calls are bit-equal; only the order of the
sums differs from the restatement's.  Multi-resolution lattices, the inverse field, a symmetric FFD cost, intensity metrics
and bending energy are out of scope.
"""
from __future__ import annotations

import math
from numbers import Integral, Real
from typing import NamedTuple, Optional

import numpy as np
import torch

import ctypes as C

from . import _args, _lib

MAX_BLOCKS = 1024                      # CTU_REG_MAX_BLOCKS of ctunet_hip.h
_HEAD_DOUBLES = 128                    # the workspace head: 1024 bytes
_PIVOT_C = 62                          # the candidate's pivot in the head (layout: ctunet_hip.h)
_ROW = 32                              # doubles of a slab row
_SIM_PIVOT_C = 102                     # the same of the similarity state (layout: ctunet_hip.h)
_SIM_ROW = 40                          # doubles of a similarity slab row
_DOF = {"rigid": 6, "similarity": 7}


class RegistrationResult(NamedTuple):
    """``matrix`` / ``inverse`` device float64 [4,4] (moving world -> fixed world and back), ``history`` device float64
    [iterations + 1, 4] = (cost / P, inliers, lambda, 1 accepted / 0 rejected / -1 refused), ``num_points`` P.  From the
    similarity kernels the history has two more columns (backward inliers, scale), the first two count both terms, and
    ``num_fixed_points`` is Q.  ``candidate``: from ``register(init="moments")`` the device int64 scalar that holds the index
    of the chosen start (0..3 the principal-axes starts, 4 the centroid start), otherwise None."""
    matrix: torch.Tensor
    inverse: torch.Tensor
    history: torch.Tensor
    num_points: int = 0
    num_fixed_points: int = 0
    candidate: Optional[torch.Tensor] = None

    def report(self) -> dict:
        """Reads the history back (one synchronisation): ``rms`` distance in mm of the accepted matrix, ``inlier_fraction``,
        ``accepted`` steps and ``status`` (0, or -1 when the last step was refused: too few inliers to move at all); with a
        six-column history also ``scale`` and ``backward_inlier_fraction`` (of the Q fixed points), and ``inlier_fraction``
        is of P + Q."""
        h = self.history.cpu().numpy()
        last = h[-1]
        rep = dict(rms=float(np.sqrt(last[0])), inlier_fraction=float(last[1] / max(self.num_points + self.num_fixed_points, 1)),
                   accepted=int((h[:, 3] == 1).sum()), status=-1 if last[3] < 0 else 0, iterations=int(h.shape[0] - 1))
        if h.shape[1] >= 6:
            rep.update(scale=float(last[5]), backward_inlier_fraction=float(last[4] / max(self.num_fixed_points, 1)))
        return rep


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


def _check_inputs(points, field, names=("points", "field"), count: str = "P"):
    """A point set and the distance field it is sampled against: (points, field), or (fixed_points, moving_field)."""
    pn, fn = names
    if not isinstance(points, torch.Tensor) or not isinstance(field, torch.Tensor):
        raise TypeError(f"registration: {pn} and {fn} must be tensors")
    if points.dtype != torch.float32 or field.dtype != torch.float32:
        raise TypeError(f"registration: {pn} and {fn} must be float32, got {points.dtype} and {field.dtype}")
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError(f"registration: {pn} must be [{count},3] with {count} >= 1, got {tuple(points.shape)}")
    if field.dim() != 3:
        raise ValueError(f"registration: {fn} must be one [D,H,W] volume, got {tuple(field.shape)}")
    if min(field.shape) < 2:
        raise ValueError(f"registration: a field with a side of 1 has no gradient along it, got {tuple(field.shape)}")
    if field.numel() >= 1 << 31:
        raise ValueError(f"registration: the field must hold fewer than 2^31 voxels, got {tuple(field.shape)}")


def _iterations(iterations) -> int:
    if isinstance(iterations, bool) or not isinstance(iterations, Integral) or not 0 <= iterations <= 10000:
        raise ValueError(f"registration: iterations must be an integer in 0..10000, got {iterations!r}")
    return int(iterations)


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


def _workspace(need: int, device, workspace):
    if workspace is None:
        return torch.empty(need, dtype=torch.uint8, device=device)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != device \
            or not workspace.is_contiguous() or workspace.numel() < need or workspace.data_ptr() % 8:
        raise ValueError(f"registration: workspace must be a contiguous, 8-byte aligned uint8 tensor of at least {need} bytes "
                         f"on {device}")
    return workspace


def _optimise(family: str, dev, points_ptr, P: int, init, accumulate_args, update_head, iterations: int, columns: int, ws):
    """The launch loop of both optimisers -- ``ctu_<family>_init``, then accumulate and update per iteration -- into fresh
    (matrix, inverse, history) with ``columns`` history columns; ``update_head`` is what the update takes ahead of ``it``."""
    rows = iterations + 1
    out = torch.empty((32 + columns * rows,), dtype=torch.float64, device=dev)
    matrix, inverse, history = out[:16].view(4, 4), out[16:32].view(4, 4), out[32:].view(rows, columns)
    with _lib.on(dev) as run:
        run(f"ctu_{family}_init", points_ptr, P, None if init is None else init.data_ptr(), ws.data_ptr())
        for it in range(rows):
            run(f"ctu_{family}_accumulate", *accumulate_args, ws.data_ptr())
            run(f"ctu_{family}_update", *update_head, it, matrix.data_ptr(), inverse.data_ptr(), history.data_ptr(), rows,
                ws.data_ptr())
    return matrix, inverse, history


def _accumulate_once(family: str, dev, points_ptr, P: int, matrix, accumulate_args, ws, row: int, sums: int, counts: int,
                     pivot_at: int):
    """``ctu_<family>_init`` at ``matrix`` and one accumulation, read back: the first ``sums`` doubles of the slab rows (``row``
    doubles each) added in block order, the ``counts`` int64 counts behind them, the candidate's pivot (at ``pivot_at`` in the
    head) and the number of blocks."""
    with _lib.on(dev) as run:
        run(f"ctu_{family}_init", points_ptr, P, None if matrix is None else matrix.data_ptr(), ws.data_ptr())
        run(f"ctu_{family}_accumulate", *accumulate_args, ws.data_ptr())
    host = ws.cpu().numpy().view(np.float64)
    slab = host[_HEAD_DOUBLES:].reshape(-1, row)
    tot = np.zeros(sums)
    for r in slab:                                                     # block order
        tot += r[:sums]
    return tot, slab[:, sums:sums + counts].copy().view(np.int64).sum(0), host[pivot_at:pivot_at + 3].copy(), int(slab.shape[0])


def register_points(points: torch.Tensor, field: torch.Tensor, *, spacing=None, origin=None, init=None, iterations: int = 30,
                    max_distance=None, workspace=None) -> RegistrationResult:
    """Fit the rigid matrix that takes ``points`` (float32 [P,3], moving world) onto the zero set of ``field`` (float32
    [D,H,W] distances on the fixed grid of ``spacing`` / ``origin``) by the module docstring's rule."""
    _check_inputs(points, field)
    iterations = _iterations(iterations)
    bound = _bound(max_distance)
    sp, org = _frame(spacing, origin)
    _lib.check_device(_ON_GPU.format("points and field"), points, field)
    if points.device != field.device:
        raise ValueError(f"registration: points live on {points.device}, the field on {field.device}")
    dev = points.device
    init = _check_init(init, dev)
    pts, fld = points.contiguous(), field.contiguous()
    P = int(pts.shape[0])
    ws = _workspace(workspace_bytes(P), dev, workspace)
    args = (pts.data_ptr(), P, fld.data_ptr(), *fld.shape, _lib.double_array(sp), _lib.double_array(org), bound)
    return RegistrationResult(*_optimise("registration", dev, pts.data_ptr(), P, init, args, (P,), iterations, 4, ws), P)


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
    args = (pts.data_ptr(), P, fld.data_ptr(), *fld.shape, _lib.double_array(sp), _lib.double_array(org), bound)
    tot, counts, pivot, blocks = _accumulate_once("registration", dev, pts.data_ptr(), P, matrix, args,
                                                  _workspace(workspace_bytes(P), dev, None), _ROW, 28, 1, _PIVOT_C)
    return dict(H=tot[:21], b=tot[21:27], cost=float(tot[27]), count=int(counts[0]), pivot=pivot, blocks=blocks)


def similarity_workspace_bytes(P: int, Q: int = 0) -> int:
    """Device workspace (bytes) of a similarity registration of ``P`` moving and ``Q`` fixed points: the state (1024 bytes) and
    one slab row of 320 bytes per block of the accumulation over P + Q items, at most 1024 blocks; 0 for P < 1 or Q < 0."""
    return int(_lib.load().ctu_similarity_ws_bytes(int(P), int(Q)))


def _dof(model) -> int:
    if not isinstance(model, str) or model not in _DOF:
        raise ValueError(f"registration: model must be 'rigid' or 'similarity', got {model!r}")
    return _DOF[model]


class _SimilarityCall:
    """The checked arguments of the similarity entry points, shared by the optimiser and the inspection helper."""

    def __init__(self, points, field, fixed_points, moving_field, model, spacing, origin, moving_spacing, moving_origin,
                 max_distance, iterations=0):
        _check_inputs(points, field)
        self.dof = _dof(model)
        # the optional backward term: both or neither, and a moving frame only with a moving field
        if (fixed_points is None) != (moving_field is None):
            raise ValueError("registration: fixed_points and moving_field come together or not at all")
        if fixed_points is not None:
            _check_inputs(fixed_points, moving_field, ("fixed_points", "moving_field"), "Q")
        elif moving_spacing is not None or moving_origin is not None:
            raise ValueError("registration: moving_spacing and moving_origin describe moving_field, which was not given")
        self.iterations = _iterations(iterations)
        bound = _bound(max_distance)
        sp, org = _frame(spacing, origin)
        msp, morg = _frame(moving_spacing, moving_origin, "moving_")
        tensors = (points, field) if fixed_points is None else (points, field, fixed_points, moving_field)
        _lib.check_device(_ON_GPU.format("points and fields"), *tensors)
        self.dev = points.device
        for t in tensors:
            if t.device != self.dev:
                raise ValueError(f"registration: points live on {self.dev}, another argument on {t.device}")
        self.keep = [t.contiguous() for t in tensors]                          # alive until the launches are issued
        pts, fld = self.keep[:2]
        self.P, self.Q = int(pts.shape[0]), 0 if fixed_points is None else int(fixed_points.shape[0])
        back = (None, 0, None, 0, 0, 0) if fixed_points is None else \
            (self.keep[2].data_ptr(), self.Q, self.keep[3].data_ptr(), *self.keep[3].shape)
        self.points_ptr = pts.data_ptr()
        self.accumulate_args = (self.dof, pts.data_ptr(), self.P, fld.data_ptr(), *fld.shape, _lib.double_array(sp),
                                _lib.double_array(org), *back, _lib.double_array(msp), _lib.double_array(morg), bound)

    def workspace(self, workspace):
        return _workspace(similarity_workspace_bytes(self.P, self.Q), self.dev, workspace)


def register_similarity_points(points: torch.Tensor, field: torch.Tensor, *, fixed_points=None, moving_field=None,
                               model: str = "similarity", spacing=None, origin=None, moving_spacing=None, moving_origin=None,
                               init=None, iterations: int = 30, max_distance=None, workspace=None) -> RegistrationResult:
    """Fit the similarity (``model="similarity"``, 7 unknowns) or rigid (``"rigid"``, 6) matrix that takes ``points`` (float32
    [P,3], moving world) onto the zero set of ``field`` (float32 distances on the fixed grid of ``spacing`` / ``origin``) and,
    with ``fixed_points`` (float32 [Q,3], fixed world) and ``moving_field`` (float32 distances to the moving object on the
    moving grid of ``moving_spacing`` / ``moving_origin``), the fixed points back onto the moving object: the symmetric cost of
    the module docstring's rule.  The two come together or not at all.  Workspace: ``similarity_workspace_bytes(P, Q)``."""
    call = _SimilarityCall(points, field, fixed_points, moving_field, model, spacing, origin, moving_spacing, moving_origin,
                           max_distance, iterations)
    init = _check_init(init, call.dev)
    ws = call.workspace(workspace)
    return RegistrationResult(*_optimise("similarity", call.dev, call.points_ptr, call.P, init, call.accumulate_args,
                                         (call.dof, call.P, call.Q), call.iterations, 6, ws), call.P, call.Q)


def accumulate_similarity(points: torch.Tensor, field: torch.Tensor, matrix: torch.Tensor, *, fixed_points=None,
                          moving_field=None, model: str = "similarity", spacing=None, origin=None, moving_spacing=None,
                          moving_origin=None, max_distance=None) -> dict:
    """One accumulation of the similarity kernels at ``matrix`` (device float64 [4,4]; its inverse is the adjugate's), read
    back for inspection: ``H`` [DOF (DOF + 1) / 2] (upper triangle, row by row), ``b`` [DOF], ``cost``, ``count`` (both terms),
    ``count_backward`` and the ``pivot`` -- numpy float64, the slab rows summed in block order as the update kernel sums them."""
    call = _SimilarityCall(points, field, fixed_points, moving_field, model, spacing, origin, moving_spacing, moving_origin,
                           max_distance)
    matrix = _check_init(matrix, call.dev)
    nh = call.dof * (call.dof + 1) // 2
    na = nh + call.dof + 1
    tot, counts, pivot, blocks = _accumulate_once("similarity", call.dev, call.points_ptr, call.P, matrix, call.accumulate_args,
                                                  call.workspace(None), _SIM_ROW, na, 2, _SIM_PIVOT_C)
    return dict(H=tot[:nh], b=tot[nh:nh + call.dof], cost=float(tot[na - 1]), count=int(counts[0]), count_backward=int(counts[1]),
                pivot=pivot, blocks=blocks)


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


def principal_frame(mask: torch.Tensor, spacing=None, origin=None):
    """``(centroid [3], axes [3,3], extent [3])`` of the foreground of one bool / uint8 [D,H,W] mask, float64 on the device:
    the centroid in world units (z, y, x), the unit principal axes as columns (right-handed, signs as
    ``postprocess.region_properties`` pins them) and the variances along them in descending order.  A mask with nearly
    equal extents has ill-defined axes; fewer than 2 voxels give NaN."""
    from . import postprocess
    _mask(mask, "mask")
    sp, org = _frame(spacing, origin)
    _lib.check_device(_ON_GPU.format("the mask"), mask)
    p = postprocess.region_properties(mask if mask.dtype == torch.bool else mask != 0, 1, sampling=sp, origin=org)
    return p.centroid[0, 0], p.axes[0, 0], p.extent[0, 0]


_MOMENT_SIGNS = ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))


def _moment_starts(moving_frame, fixed_frame):
    """The five float64 [4,4] starts of ``init="moments"`` (module docstring), built on the device."""
    (cm, Am, _), (cf, Af, _) = moving_frame, fixed_frame
    starts = []
    for s in _MOMENT_SIGNS + (None,):
        M = torch.eye(4, dtype=torch.float64, device=cm.device)
        if s is not None:
            B = Af.clone()
            for j in range(3):
                if s[j] < 0:
                    B[:, j] = -B[:, j]
            M[:3, :3] = (B.unsqueeze(1) * Am.unsqueeze(0)).sum(-1)                # B Am^T
        M[:3, 3] = cf - (M[:3, :3] * cm).sum(-1)
        starts.append(M)
    return starts


def _best_of(results) -> RegistrationResult:
    """The selection rule of ``init="moments"`` over the last history rows, on the device."""
    last = torch.stack([r.history[-1] for r in results])
    cost, inliers = last[:, 0], last[:, 1]
    ok = (inliers >= 0.5 * inliers.max()) & ~torch.isnan(cost)
    k = torch.argmin(torch.where(ok, cost, torch.full_like(cost, math.inf)))       # the first of equal minima

    def pick(tensors):
        return torch.stack(tensors).index_select(0, k.reshape(1))[0]
    return results[0]._replace(matrix=pick([r.matrix for r in results]), inverse=pick([r.inverse for r in results]),
                          history=pick([r.history for r in results]), candidate=k)


def register(moving_mask: torch.Tensor, fixed_mask: torch.Tensor, *, moving_spacing=None, moving_origin=None,
             fixed_spacing=None, fixed_origin=None, iterations: int = 30, max_distance=None, init="centroid",
             model: str = "rigid", symmetric=None) -> RegistrationResult:
    """Register the binary ``moving_mask`` to ``fixed_mask`` (the atlas), each a bool / uint8 [D,H,W] volume on its own grid:
    the surface voxels of the moving mask against the exact distance field of the fixed one (module docstring).
    ``model="similarity"`` also fits an isotropic scale; ``symmetric`` (default: True for the similarity model, False for the
    rigid one) adds the fixed mask's surface voxels against the distance field of the moving mask.  The defaults are the
    rigid rule through ``register_points``; every other combination runs ``register_similarity_points``."""
    from . import postprocess
    _mask(moving_mask, "moving_mask")
    _mask(fixed_mask, "fixed_mask")
    (msp, morg), (fsp, forg) = _frame(moving_spacing, moving_origin, "moving_"), _frame(fixed_spacing, fixed_origin, "fixed_")
    if isinstance(init, str):
        if init not in ("centroid", "moments"):
            raise ValueError(f"registration: init must be 'centroid', 'moments' or a float64 [4,4] tensor, got {init!r}")
    elif init is not None:
        init = _check_init(init, moving_mask.device)
    _dof(model)
    if symmetric is None:
        symmetric = model == "similarity"
    elif not isinstance(symmetric, bool):
        raise ValueError(f"registration: symmetric must be None, True or False, got {symmetric!r}")
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
    starts = None
    if isinstance(init, str) and init == "moments":
        starts = _moment_starts(principal_frame(moving_mask, msp, morg), principal_frame(fixed, fsp, forg))
    elif isinstance(init, str):
        cm = _world(torch.nonzero(moving_mask != 0), msp, morg).mean(0)
        cf = _world(fixed_index, fsp, forg).mean(0)
        init = torch.eye(4, dtype=torch.float64, device=points.device)
        init[:3, 3] = cf - cm
    if model == "rigid" and not symmetric:
        def run(start):
            return register_points(points, field, spacing=fsp, origin=forg, init=start, iterations=iterations,
                                   max_distance=max_distance)
    else:
        half = {}
        if symmetric:
            half = dict(fixed_points=surface_points(fixed, fsp, forg), moving_spacing=msp, moving_origin=morg,
                        moving_field=postprocess.distance_transform_edt(moving_mask == 0, sampling=msp))

        def run(start):
            return register_similarity_points(points, field, model=model, spacing=fsp, origin=forg, init=start,
                                              iterations=iterations, max_distance=max_distance, **half)
    if starts is None:
        return run(init)
    return _best_of([run(start) for start in starts])


# ---- B-spline deformable registration -----------------------------------------------------------------------------------
FFD_SEGMENT = 256                      # CTU_FFD_SEGMENT of ctunet_hip.h
FFD_MAX_G = 64                         # CTU_FFD_MAX_G


class DeformableResult(NamedTuple):
    """``T(p) = M p + u(M p)``: ``matrix`` device float64 [4,4] (moving world -> fixed world), ``control`` device float64
    [3,Gz,Gy,Gx] (mm) on the lattice of ``control_spacing`` over the box ``box_origin`` .. ``box_origin + box_extent`` (host
    triples), ``history`` device float64 [iterations + 1, 6] = (total cost / P, data rms, regulariser energy, inliers, lambda,
    1 accepted / 0 rejected / -1 refused), ``num_points`` P and ``jacobian`` device float64 [P]: ``det(I + du/dq0)`` at the
    fitted points (None for a result put together by hand)."""
    matrix: torch.Tensor
    control: torch.Tensor
    control_spacing: tuple
    box_origin: tuple
    box_extent: tuple
    history: Optional[torch.Tensor] = None
    num_points: int = 0
    jacobian: Optional[torch.Tensor] = None

    def report(self) -> dict:
        """Reads history, controls and determinants back (the one synchronisation): ``rms_before`` / ``rms`` in mm (first and
        last history row), ``inlier_fraction``, ``accepted`` steps, ``status`` (-1 when the last step was refused),
        ``max_displacement`` (the longest control displacement, mm), ``min_jacobian`` and ``folded`` (points with
        ``det <= 0``)."""
        c = self.control.cpu().numpy()
        rep = dict(max_displacement=float(np.sqrt((c * c).sum(0)).max()))
        if self.history is not None:
            h = self.history.cpu().numpy()
            last = h[-1]
            rep.update(rms_before=float(h[0, 1]), rms=float(last[1]), inlier_fraction=float(last[3] / max(self.num_points, 1)),
                       accepted=int((h[:, 5] == 1).sum()), status=-1 if last[5] < 0 else 0, iterations=int(h.shape[0] - 1))
        if self.jacobian is not None:
            j = self.jacobian.cpu().numpy()
            rep.update(min_jacobian=float(j.min()), folded=int((j <= 0).sum()))
        return rep


def ffd_lattice(shape, spacing, origin, control_spacing):
    """(G, h, box_origin, box_extent) of the control lattice over the grid ``shape`` / ``spacing`` / ``origin`` (module
    docstring); refuses a ``G`` above 64."""
    sp, org = _frame(spacing, origin)
    sp, org = sp or (1.0, 1.0, 1.0), org or (0.0, 0.0, 0.0)
    h = _args.triple(control_spacing, _REAL_POSITIVE, what="control_spacing")
    if h is None:
        raise ValueError("registration: control_spacing must be positive and finite, got None")
    extent = tuple((int(n) - 1) * s for n, s in zip(shape, sp))
    G = tuple(max(1, math.ceil(e / ha)) + 3 for e, ha in zip(extent, h))
    if max(G) > FFD_MAX_G:
        raise ValueError(f"registration: control_spacing {h} gives a lattice of {G} control points, more than {FFD_MAX_G} "
                         "along an axis")
    return G, tuple(h), tuple(org), extent


def _lattice_args(G, h, box_origin):
    return _lib.array(C.c_int, G), _lib.double_array(h), _lib.double_array(box_origin)


def _check_control(control, G, device, what: str):
    if not isinstance(control, torch.Tensor) or control.dtype != torch.float64 or tuple(control.shape) != (3, *G):
        raise ValueError(f"registration: {what} must be a float64 [3,{G[0]},{G[1]},{G[2]}] tensor")
    if control.device != device:
        raise ValueError(f"registration: {what} lives on {control.device}, the points on {device}")
    return control.contiguous()


class FFDPlan:
    """The binning of a free-form fit, done once: the lattice cell of every point under the frozen ``matrix``, the points
    sorted by cell and cut into segments of at most 256, workspace and outputs.  Building it synchronises once (the number
    of segments); ``run()`` launches the fit without a synchronisation or an allocation and can be captured into a graph.
    Every ``run()`` writes the same output tensors."""

    def __init__(self, points, field, matrix, *, spacing=None, origin=None, control_spacing=10.0, stiffness=0.1,
                 iterations: int = 60, max_distance=None):
        _check_inputs(points, field)
        self.rows = _iterations(iterations) + 1
        if isinstance(stiffness, bool) or not isinstance(stiffness, Real) or not math.isfinite(stiffness) or stiffness < 0:
            raise ValueError(f"registration: stiffness must be a finite number >= 0, got {stiffness!r}")
        if not isinstance(matrix, torch.Tensor) or matrix.dtype != torch.float64 or tuple(matrix.shape) != (4, 4):
            raise ValueError("registration: the matrix must be a float64 [4,4] tensor (moving world -> fixed world)")
        self.bound = _bound(max_distance)
        self.sp, self.org = _frame(spacing, origin)
        self.G, self.h, self.box_origin, self.box_extent = ffd_lattice(field.shape, self.sp, self.org, control_spacing)
        _lib.check_device(_ON_GPU.format("points and field"), points, field)
        if points.device != field.device:
            raise ValueError(f"registration: points live on {points.device}, the field on {field.device}")
        dev = self.dev = points.device
        self.matrix = _check_init(matrix, dev)
        self.pts, self.fld = points.contiguous(), field.contiguous()
        P = self.P = int(self.pts.shape[0])
        g3 = self.G[0] * self.G[1] * self.G[2]
        self.weight = float(stiffness) * P / g3
        self.lat = _lattice_args(self.G, self.h, self.box_origin)
        cells = torch.empty(P, dtype=torch.int32, device=dev)
        with _lib.on(dev) as run:
            run("ctu_ffd_cells", self.pts.data_ptr(), P, self.matrix.data_ptr(), *self.lat, cells.data_ptr())
        ncells = (self.G[0] - 3) * (self.G[1] - 3) * (self.G[2] - 3)
        cells = cells.to(torch.int64)
        perm = torch.sort(cells, stable=True)[1]
        counts = torch.bincount(cells, minlength=ncells)
        cell_seg = torch.zeros(ncells + 1, dtype=torch.int64, device=dev)
        cell_seg[1:] = torch.cumsum((counts + (FFD_SEGMENT - 1)) // FFD_SEGMENT, 0)
        S = self.S = int(cell_seg[-1])                                         # the one synchronisation
        seg = torch.arange(S, device=dev)
        seg_cell = torch.searchsorted(cell_seg[1:].contiguous(), seg, right=True)
        first = FFD_SEGMENT * (seg - cell_seg[seg_cell])                        # of the segment within its cell's run
        seg_begin = (torch.cumsum(counts, 0) - counts)[seg_cell] + first
        seg_count = torch.clamp(counts[seg_cell] - first, max=FFD_SEGMENT)
        self.tables = tuple(t.to(torch.int32).contiguous() for t in (perm, seg_cell, seg_begin, seg_count, cell_seg))
        self.ws = torch.empty(int(_lib.load().ctu_ffd_ws_bytes(self.lat[0], S)), dtype=torch.uint8, device=dev)
        self.control = torch.empty((3, *self.G), dtype=torch.float64, device=dev)
        self.history = torch.empty((self.rows, 6), dtype=torch.float64, device=dev)
        self.jacobian = torch.empty(P, dtype=torch.float64, device=dev)

    def _accumulate(self, run):
        perm, seg_cell, seg_begin, seg_count, _ = self.tables
        run("ctu_ffd_accumulate", self.pts.data_ptr(), self.P, self.matrix.data_ptr(), self.fld.data_ptr(), *self.fld.shape,
            _lib.double_array(self.sp), _lib.double_array(self.org), *self.lat, self.bound, perm.data_ptr(), seg_cell.data_ptr(),
            seg_begin.data_ptr(), seg_count.data_ptr(), self.S, self.ws.data_ptr())

    def run(self, init_control=None) -> "DeformableResult":
        if init_control is not None:
            init_control = _check_control(init_control, self.G, self.dev, "init_control")
        with _lib.on(self.dev) as run:
            run("ctu_ffd_init", self.lat[0], self.S, None if init_control is None else init_control.data_ptr(), self.weight,
                self.ws.data_ptr(), self.control.data_ptr())
            for it in range(self.rows):
                self._accumulate(run)
                run("ctu_ffd_update", self.P, *self.lat, self.tables[4].data_ptr(), self.S, it, self.control.data_ptr(),
                    self.history.data_ptr(), self.rows, self.ws.data_ptr())
            run("ctu_ffd_transform_points", self.pts.data_ptr(), self.P, self.matrix.data_ptr(), self.control.data_ptr(),
                *self.lat, None, self.jacobian.data_ptr())
        return DeformableResult(self.matrix, self.control, self.h, self.box_origin, self.box_extent, self.history, self.P,
                                self.jacobian)


def register_ffd_points(points: torch.Tensor, field: torch.Tensor, matrix: torch.Tensor, *, spacing=None, origin=None,
                        control_spacing=10.0, stiffness=0.1, iterations: int = 60, max_distance=None,
                        init_control=None) -> DeformableResult:
    """Fit the B-spline displacement that, behind the frozen ``matrix`` (float64 [4,4], moving world -> fixed world), takes
    ``points`` (float32 [P,3], moving world) onto the zero set of ``field`` (float32 distances on the fixed grid of ``spacing``
    / ``origin``) by the module docstring's rule.  ``init_control`` warm-starts at the same lattice."""
    return FFDPlan(points, field, matrix, spacing=spacing, origin=origin, control_spacing=control_spacing, stiffness=stiffness,
                   iterations=iterations, max_distance=max_distance).run(init_control)


def accumulate_ffd(points: torch.Tensor, field: torch.Tensor, matrix: torch.Tensor, control: torch.Tensor, *, spacing=None,
                   origin=None, control_spacing=10.0, stiffness=0.1, max_distance=None) -> dict:
    """One accumulation of the free-form kernels at ``control``, read back for inspection: ``grad`` [3,Gz,Gy,Gx] and ``diag``
    [Gz,Gy,Gx] (regulariser included), ``cost`` (total), ``sum2`` (sum of r^2), ``regulariser``, ``count`` and ``segments`` --
    numpy float64, summed as the kernels sum them.  A cost that is not finite leaves ``grad`` and ``diag`` zero."""
    plan = FFDPlan(points, field, matrix, spacing=spacing, origin=origin, control_spacing=control_spacing, stiffness=stiffness,
                   iterations=0, max_distance=max_distance)
    plan.run(control)
    host = plan.ws.cpu().numpy()
    head = host[:48].view(np.float64)
    body = host[_HEAD_DOUBLES * 8:].view(np.float64)
    g3 = plan.G[0] * plan.G[1] * plan.G[2]
    return dict(grad=body[9 * g3:12 * g3].reshape(3, *plan.G).copy(), diag=body[12 * g3:13 * g3].reshape(plan.G).copy(),
                cost=float(head[0]), sum2=float(head[1]), regulariser=float(head[2]), count=int(head[5:6].view(np.int64)[0]),
                segments=plan.S)


def _check_result(result) -> DeformableResult:
    if not isinstance(result, DeformableResult):
        raise TypeError(f"registration: expected a DeformableResult, got {type(result).__name__}")
    m, c = result.matrix, result.control
    if not isinstance(m, torch.Tensor) or m.dtype != torch.float64 or tuple(m.shape) != (4, 4):
        raise ValueError("registration: a DeformableResult's matrix must be a float64 [4,4] tensor")
    if not isinstance(c, torch.Tensor) or c.dtype != torch.float64 or c.dim() != 4 or c.shape[0] != 3 \
            or min(c.shape[1:]) < 4 or max(c.shape[1:]) > FFD_MAX_G:
        raise ValueError(f"registration: a DeformableResult's control must be a float64 [3,Gz,Gy,Gx] tensor with every G in "
                         f"4..{FFD_MAX_G}")
    if c.device != m.device:
        raise ValueError(f"registration: the matrix lives on {m.device}, the control on {c.device}")
    h = _args.triple(result.control_spacing, _REAL_POSITIVE, what="control_spacing")
    org = _args.triple(result.box_origin, _REAL, what="box_origin")
    if h is None or org is None:
        raise ValueError("registration: a DeformableResult needs control_spacing and box_origin")
    return result._replace(matrix=m.contiguous(), control=c.contiguous(), control_spacing=tuple(h), box_origin=tuple(org))


def transform_points(points: torch.Tensor, result: DeformableResult, return_jacobian: bool = False):
    """``T(p)`` of float32 ``points`` [P,3] (moving world) in the fixed frame: float64 inside, rounded to float32 once; with
    ``return_jacobian`` also ``det(I + du/dq0)`` per point (float64 [P])."""
    r = _check_result(result)
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("registration: points must be a float32 [P,3] tensor")
    _lib.check_device(_ON_GPU.format("points"), points)
    if points.device != r.matrix.device:
        raise ValueError(f"registration: points live on {points.device}, the result on {r.matrix.device}")
    pts = points.contiguous()
    P = int(pts.shape[0])
    out = torch.empty_like(pts)
    jac = torch.empty(P, dtype=torch.float64, device=pts.device) if return_jacobian else None
    if P:
        with _lib.on(pts.device) as run:
            run("ctu_ffd_transform_points", pts.data_ptr(), P, r.matrix.data_ptr(), r.control.data_ptr(),
                *_lattice_args(tuple(r.control.shape[1:]), r.control_spacing, r.box_origin), out.data_ptr(),
                None if jac is None else jac.data_ptr())
    return (out, jac) if return_jacobian else out


def register_deformable(moving_mask: torch.Tensor, fixed_mask: torch.Tensor, *, moving_spacing=None, moving_origin=None,
                        fixed_spacing=None, fixed_origin=None, affine=None, model: str = "similarity", control_spacing=10.0,
                        stiffness=0.1, iterations: int = 60, max_distance=None) -> DeformableResult:
    """``register(..., model=model, max_distance=max_distance)`` unless ``affine`` (a float64 [4,4] tensor or a
    ``RegistrationResult``) is given, then the free-form fit of the moving mask's surface voxels against the fixed mask's
    distance field behind that matrix."""
    from . import postprocess
    _mask(moving_mask, "moving_mask")
    _mask(fixed_mask, "fixed_mask")
    (msp, morg), (fsp, forg) = _frame(moving_spacing, moving_origin, "moving_"), _frame(fixed_spacing, fixed_origin, "fixed_")
    ffd_lattice(fixed_mask.shape, fsp, forg, control_spacing)
    _lib.check_device(_ON_GPU.format("the masks"), moving_mask, fixed_mask)
    if isinstance(affine, RegistrationResult):
        affine = affine.matrix
    if affine is None:
        affine = register(moving_mask, fixed_mask, moving_spacing=msp, moving_origin=morg, fixed_spacing=fsp, fixed_origin=forg,
                          model=model, max_distance=max_distance).matrix
    else:
        affine = _check_init(affine, moving_mask.device)
    points = surface_points(moving_mask, msp, morg)
    if points.shape[0] < 1:
        raise ValueError("registration: the moving mask is empty")
    field = postprocess.distance_transform_edt(fixed_mask == 0, sampling=fsp)
    return register_ffd_points(points, field, affine, spacing=fsp, origin=forg, control_spacing=control_spacing,
                               stiffness=stiffness, iterations=iterations, max_distance=max_distance)
