"""Decimation of surface meshes on the GPU by vertex clustering on a uniform grid: the step between ``mesh.smooth`` and
``mesh.write_stl`` (``ctu_mesh_decimate_*`` of ``csrc/mesh_decimate.hip``); no CPU fallback.

    m = mesh.smooth(mesh.extract_surface(implant, spacing=(0.8, 0.45, 0.45)))
    small = simplify.decimate(m, 1.0)                        # 1 mm clusters; closed stays closed
    small, index = simplify.decimate(m, (1.6, 0.9, 0.9), return_map=True)      # index[i]: the output vertex of input vertex i
    mesh.write_stl("implant.stl", small)

``extract_surface`` gives triangles the size of a voxel; a plate whose curvature radius is a hundred voxels does not need
them.  All vertices in one cell of a uniform grid become one vertex at their mean, and the faces that no longer span
three cells go.  The result is a function of the rule below alone, two calls are bit-equal, and
``tests/simplify_ref.py`` restates the rule in numpy.

The pinned rule.  All arithmetic is float64 on the float32 inputs widened, every operation rounded on its own
(contraction is off on the device).

1. **Accepted input.**  A face with an index outside ``[0, V)`` or a vertex that is not finite is never read through; it is
   counted and the call raises ``ValueError``, as ``mesh.voxelize`` does.  A *member* is a vertex used by at least one face;
   unreferenced vertices (NaN ones too) influence nothing.  ``F == 0`` gives the empty mesh (``V' = F' = 0``) without a launch.
2. **Grid.**  Per axis a, ``lo_a`` and ``hi_a`` are the minimum and maximum over the members, ``n_a = floor((hi_a - lo_a) /
   cell_a) + 1``, the cell of a member is ``c_a = min(n_a - 1, floor((v_a - lo_a) / cell_a))`` and its id
   ``(c_z n_y + c_y) n_x + c_x``.  More than ``MAX_CELLS`` cells raise ``ValueError`` with a ``cell_size`` that fits; nothing
   is truncated.
3. **Faces.**  A face maps to the cell ids ``(g0, g1, g2)`` of its corners; if two of them are equal it is dropped.
4. **Cancellation** (``cancel=True``).  Each remaining face is rotated so that its smallest id comes first, ``(s, x, y)``; it
   is *positive* if ``x < y``, else *negative*, and its key is ``(s, min(x, y), max(x, y))``.  Of the faces that share a key,
   p positive and q negative: if ``p > q`` the ``p - q`` positive faces of lowest input index survive, if ``q > p`` the
   ``q - p`` negative ones of lowest input index, if ``p == q`` none.  This removes the back-to-back sheets that clustering
   makes of walls thinner than a cell, and keeps multiplicities, so invariant (a) holds.  With ``cancel=False`` every face
   of step 3 survives.
5. **Output faces.**  The survivors in input order, corner order unchanged, indices renumbered.
6. **Output vertices.**  One per cell that a surviving face uses, in ascending cell id.  A mesh that collapses entirely
   (all members in one cell, ``cell_size`` beyond the mesh's extent) gives ``V' = F' = 0``.
7. **Position.**  ``ext = max_a(hi_a - lo_a)``, ``e`` the binary exponent with ``ext = m 2^e``, ``0.5 <= m < 1`` (C ``frexp``),
   ``S = 2^(30 - e)``.  Every member of a used cell contributes ``q_a = (int64) rint((v_a - lo_a) * S)``, and the vertex is
   ``float32(lo_a + (double(sum q_a) / double(count)) / S)``.  The sums are integers (``q <= 2^30`` and fewer than 2^31
   members keep them inside int64), so they do not depend on the order of the members: the device adds them with integer
   atomics and the result is still a function of the rule.  The quantum ``ext * 2^-31`` is far below a float32 ulp at the
   mesh's scale; a cluster of one member returns that member to within the quantum, not necessarily bit for bit.
8. **Map** (``return_map=True``).  int32 ``[V]``: the output index of each input vertex's cluster, -1 for a vertex that is no
   member or whose cluster no surviving face uses.

Invariants, which follow from the rule (``tests/test_simplify_cpu.py`` checks them on the reference):

- (a) **Closed stays closed, as a chain.**  If in the input every directed edge (a -> b) occurs as often as (b -> a), the same
  holds in the output, with ``cancel`` on or off: the vertex map is simplicial, a collapsed triangle has zero boundary, and
  cancellation removes a face together with a reverse of it.  ``mesh.measure``'s volume and ``mesh.voxelize``'s winding
  numbers therefore stay meaningful, and the enclosed volume is the same with ``cancel`` on and off.  The output need
  *not* be a 2-manifold: where two sheets meet in one cell an edge can carry four faces.  In practice a ``cell_size`` below
  half the thinnest wall keeps it one.
- (b) **Nothing moves far.**  Every member lies within ``cell_a`` of its output vertex on every axis, up to rounding, so the
  one-sided Hausdorff distance from the input vertices to the output vertices is at most ``|cell_size|_2``.

Device: bounds of the members (integer ``atomicMax`` on an order-preserving image of the floats), the cells and a scan of
one byte per cell that numbers the occupied ones (from then on everything is sized by V and F), the faces bucketed by
their lowest cell (count, scan, fill; the order within a bucket depends on arrival and nothing else does), a lane per face
that walks its bucket for p, q and its own rank (no sort), scans of the used clusters and of the survivors, and the
integer sums.  **Bounded work:** a face whose bucket holds more than ``MAX_BUCKET`` faces does not walk it; the call then
raises ``ValueError`` ("more than 4096 surviving faces share their lowest cluster").  Meshes of ``extract_surface`` have
buckets of 6 to 22 faces.

**Two host synchronisations per call, both inherent:** the grid's size depends on the box of the members (the first read:
the box and the refused-face count) and the output's size on the data (the second: V', F' and the bucket flag).  A call
cannot be captured into a graph.  ``workspace_bytes(V, F, cells)`` is what a call allocates besides its result.

Limits: V and F < 2^31, at most ``MAX_CELLS`` = 2^28 cells; anything beyond raises, nothing is truncated.

Out of scope: quadric-error placement and edge-collapse simplification, a ``target_faces=`` search over ``cell_size``, a
manifold guarantee or mesh repair, per-vertex attributes beyond the returned map, batches, formats other than binary STL.
"""
from __future__ import annotations

import ctypes
import math
from numbers import Integral

import torch

from . import _args, _lib
from .mesh import _ON_GPU, Mesh, _check_mesh

MAX_CELLS = 1 << 28        # CTU_MESH_DECIMATE_MAX_CELLS
MAX_BUCKET = 4096          # CTU_MESH_DECIMATE_MAX_BUCKET
_CELL = _args.Triple(shape="simplify: cell_size must be a number or a (z, y, x) triple, got {v!r}",
                     value="simplify: cell_size must be positive and finite in float32, got {v!r}", sign=_args.POSITIVE,
                     optional=False, float32=True)


def workspace_bytes(V: int, F: int, cells: int) -> int:
    """The device memory (bytes) one ``decimate`` call on a contiguous mesh of V vertices and F >= 1 faces whose grid has
    ``cells`` cells allocates besides its result: the 256 bytes the bounds pass reports in (``ctu_mesh_decimate_ws_bytes(V,
    F, 0)``) and the workspace of the build (``ctu_mesh_decimate_ws_bytes(V, F, cells)``): 256 bytes, 49 per vertex, 24 per
    face, 5 per cell and 8 per scan chunk of 4096 of the largest of the three, each array rounded up to 256."""
    if any(isinstance(n, bool) or not isinstance(n, Integral) for n in (V, F, cells)) or V < 0 or F < 0 or V >= 1 << 31 \
            or F >= 1 << 31 or not 1 <= cells <= MAX_CELLS:
        raise ValueError(f"simplify: workspace_bytes takes 0 <= V < 2^31, 0 <= F < 2^31 and 1 <= cells <= {MAX_CELLS}, got "
                         f"{V!r}, {F!r}, {cells!r}")
    lib = _lib.load()
    return int(lib.ctu_mesh_decimate_ws_bytes(int(V), int(F), 0)) + int(lib.ctu_mesh_decimate_ws_bytes(int(V), int(F), int(cells)))


def _cells(lo, hi, cell):
    """The cells per axis of the rule's grid, as Python ints (float64 arithmetic on the float32 values, as the device's)."""
    return [int(math.floor((h - l) / c)) + 1 for l, h, c in zip(lo, hi, cell)]


def _fitting(lo, hi, cell):
    """A multiple of ``cell`` whose grid has at most MAX_CELLS cells."""
    k = 2.0
    while math.prod(_cells(lo, hi, [_f32(c * k) for c in cell])) > MAX_CELLS:
        k *= 2.0
    return tuple(_f32(c * k) for c in cell)


def _f32(x: float) -> float:
    return ctypes.c_float(x).value


def _empty(dev, V: int, return_map: bool):
    out = Mesh(torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev))
    return (out, torch.full((V,), -1, dtype=torch.int32, device=dev)) if return_map else out


def decimate(m: Mesh, cell_size, cancel: bool = True, return_map: bool = False):
    """The mesh decimated by vertex clustering on a grid of ``cell_size`` cells, by the module docstring's rule: ``Mesh(vertices
    float32 [V',3], faces int32 [F',3])`` on the mesh's device, and with ``return_map=True`` also int32 ``[V]``, the output
    vertex of every input vertex (-1: none).  ``m``: a ``mesh.Mesh`` on the GPU (views are made contiguous first; the
    input is left untouched).  ``cell_size``: a number or a (z, y, x) triple in the units of the vertices, positive, rounded
    to float32 once.  ``cancel``: remove faces that clustering laid back to back (step 4).  A mesh whose directed edges are
    balanced stays so; a cluster of one member returns that member to within ``extent * 2^-31``, not bit for bit.  The call
    synchronises with the host twice (the box of the mesh, then the size of the result); a face index outside ``[0, V)`` or
    a vertex of a face that is not finite raises, as do a ``cell_size`` that needs more than ``MAX_CELLS`` cells and a mesh
    with more than ``MAX_BUCKET`` surviving faces around one cluster.  A mesh without faces, and one that collapses
    entirely, give ``V' = F' = 0``."""
    v, f = _check_mesh(m, "decimate")
    V, F = v.shape[0], f.shape[0]
    if V >= 1 << 31 or F >= 1 << 31:
        raise ValueError(f"simplify: decimate takes V < 2^31 vertices and F < 2^31 faces, got V = {V}, F = {F}")
    cell = tuple(_f32(c) for c in _args.triple(cell_size, _CELL))
    if not isinstance(cancel, bool) or not isinstance(return_map, bool):
        raise ValueError(f"simplify: cancel and return_map must be booleans, got {cancel!r} and {return_map!r}")
    _lib.check_device(_ON_GPU.format("decimate"), v)
    dev = v.device
    if F == 0:
        return _empty(dev, V, return_map)
    lib = _lib.load()
    v, f = v.contiguous(), f.contiguous()
    c_cell = _lib.float_array(cell)
    with _lib.on(dev) as run:
        box = torch.empty(lib.ctu_mesh_decimate_ws_bytes(V, F, 0), dtype=torch.uint8, device=dev)
        run("ctu_mesh_decimate_bounds", v.data_ptr(), V, f.data_ptr(), F, box.data_ptr())
        head = box[:32].cpu()                                           # synchronisation 1: the refused count and the box
        bad = int(head[:8].view(torch.int64).item())
        if bad:
            raise ValueError(f"simplify: a face refers to a vertex that does not exist or is not finite ({bad} of {F} faces hold "
                             f"an index outside [0, {V}) or a NaN / infinite coordinate)")
        lo, hi = head[8:20].view(torch.float32).tolist(), head[20:32].view(torch.float32).tolist()
        if max(h - l for l, h in zip(lo, hi)) == 0.0:                   # all members coincide: one cluster, no face
            return _empty(dev, V, return_map)
        n = _cells(lo, hi, cell)
        cells = n[0] * n[1] * n[2]
        if cells > MAX_CELLS:
            raise ValueError(f"simplify: cell_size={cell_size!r} needs {n[0]} x {n[1]} x {n[2]} cells for this mesh, more than "
                             f"{MAX_CELLS}; cell_size={_fitting(lo, hi, cell)!r} fits")
        c_lo, c_hi = _lib.float_array(lo), _lib.float_array(hi)
        ws = torch.empty(lib.ctu_mesh_decimate_ws_bytes(V, F, cells), dtype=torch.uint8, device=dev)
        run("ctu_mesh_decimate_build", v.data_ptr(), V, f.data_ptr(), F, c_lo, c_hi, c_cell, cells, int(bool(cancel)), ws.data_ptr())
        nv, nf, overflow = ws[:24].view(torch.int64).tolist()           # synchronisation 2: the size of the result
        if overflow:
            raise ValueError(f"simplify: more than {MAX_BUCKET} surviving faces share their lowest cluster; choose a smaller "
                             f"cell_size or cancel=False")
        if nf == 0:
            return _empty(dev, V, return_map)
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        index = torch.empty(V, dtype=torch.int32, device=dev) if return_map else None
        run("ctu_mesh_decimate_emit", f.data_ptr(), V, F, nv, nf, c_lo, c_hi, vertices.data_ptr(), faces.data_ptr(),
            index.data_ptr() if return_map else None, ws.data_ptr())
    out = Mesh(vertices, faces)
    return (out, index) if return_map else out
