"""Surface meshes of label volumes and scalar fields on the GPU, their smoothing, their voxelisation back onto a grid, and
their export and import as binary STL: the last step of the segmentation-to-implant pipeline and the way back from it
(``ctu_mesh_count`` / ``ctu_mesh_emit`` / ``ctu_mesh_measure`` of ``csrc/mesh.hip``, ``ctu_mesh_adjacency_*`` /
``ctu_mesh_smooth`` of ``csrc/mesh_smooth.hip``, ``ctu_mesh_voxelize`` of ``csrc/mesh_voxelize.hip``, ``ctu_mesh_grid_*`` /
``ctu_mesh_distance`` of ``csrc/mesh_distance.hip``); no CPU fallback.

    m = mesh.extract_surface(implant, spacing=(0.8, 0.45, 0.45))      # Mesh: vertices [V,3] (z, y, x) in mm, faces [F,3]
    m = mesh.smooth(m)                                                # Taubin: the staircase goes, the volume stays
    area, volume = mesh.measure(m).tolist()
    mesh.write_stl("implant.stl", m)
    v = mesh.voxelize(mesh.smooth(m), scan.shape, spacing=(0.8, 0.45, 0.45))      # uint8 [D,H,W] on the scanner's grid
    metrics.surface_metrics(v, truth, ...)                            # the smoothed implant scored as a volume
    w = mesh.winding_number(m, scan.shape, spacing=(0.8, 0.45, 0.45))  # int32: outside {0, 1} where a mesh self-intersects
    other = mesh.read_stl("designed_elsewhere.stl")                    # host Mesh; move both fields with .to("cuda")
    moved = mesh.point_distance(mesh.smooth(m).vertices, m).max()      # mm: how far smoothing moved the surface
    sdf = mesh.distance_field(other, scan.shape, spacing=(0.8, 0.45, 0.45), max_distance=5.0, signed=True)   # mm, < 0 inside
    metrics.mesh_surface_metrics(m, other, tolerance=1.0)              # HD, HD95, ASSD, NSD between two meshes, in mm
    small = simplify.decimate(mesh.smooth(m), 1.0)                     # fewer, larger triangles: see ctunet_amd.simplify

``volume`` is one ``[D,H,W]`` tensor.  Meshes are ragged (V and F depend on the data), so a batch is a Python loop over its
items.  bool, uint8 and int64 volumes are masks or label maps: inside = ``v != 0``, or ``v == label`` with ``label=``;
float32 volumes are scalar fields (probabilities, or ``-signed_distance``): inside = ``v > level``.

The pinned rule (``tests/mesh_ref.py`` restates it in numpy): **marching tetrahedra on the Kuhn split, welded and closed**.

- **Padded grid.**  The grid is padded by one virtual layer of *outside* points on every face; padded point ``p`` is voxel
  ``p - 1``.  The cells are the (D+1)(H+1)(W+1) cubes of the padded grid, so the mesh is closed at the volume border too.
  A mask reads as 1 / 0 against level 0.5.  Virtual points hold ``fill_value``: 0 for masks, ``level - 1`` by default for
  float32, never above ``level``.
- **Tetrahedra.**  Every cell splits into the six tetrahedra around its diagonal (0,0,0)-(1,1,1): the paths ``c0`` = corner
  0, ``c1 = c0 + e_a``, ``c2 = c1 + e_b``, ``c3 = c2 + e_c`` for the permutations (a, b, c) of the axes (z, y, x) = (0, 1, 2)
  in lexicographic order.  The split is translation invariant, so neighbouring cells agree on every shared face.
- **Vertices** lie on the lattice edges whose ends differ in insideness.  An edge belongs to the cell at its lower end; a
  cell owns seven edges, in this order of (dz, dy, dx): (0,0,1), (0,1,0), (1,0,0), (0,1,1), (1,0,1), (1,1,0), (1,1,1).
  Vertex order: cells in C order of the padded grid, then owned crossing edges in that order.  With ``v0`` the value at
  the owner's corner 0 and ``v1`` at the far end, ``t = (level - v0) / (v1 - v0)`` in float32 (exactly 0.5 for masks), and the
  coordinate on axis i is ``origin_i + (float32(p_i - 1) + t * d_i) * spacing_i``, every float32 operation rounded on its own.
- **Faces.**  Order: cells in C order, then tetrahedra in order, then: with one or three corners inside, ``i`` the lone corner
  and ``o0 < o1 < o2`` the others in path order, one triangle (i-o0, i-o1, i-o2); with two inside, ``i0 < i1`` inside and
  ``o0 < o1`` outside, the quad a = i0-o0, b = i0-o1, c = i1-o1, d = i1-o0 as the triangles (a, b, c) and (a, c, d).  The
  first index of a triangle stays; the other two are swapped where needed so that the right-hand normal, computed in
  (x, y, z) (the vertex columns reversed), points from inside to outside.  On the device that winding is a table by
  (permutation, case), derived at compile time from the tetrahedron's geometry.
- **Degenerate values.**  A sample equal to ``level`` is outside.  Vertices may then coincide at a lattice point and give faces
  without area; the mesh stays combinatorially a closed 2-manifold.  Nothing is snapped or removed: the result is a function
  of the rule alone.  The field must be finite (a NaN sample is outside and makes the vertices on its edges NaN).

Every input gives a closed, consistently oriented 2-manifold, without ambiguous cases.  A known property of the Kuhn split:
two voxels that touch only across the (0,0,0)-(1,1,1) body diagonal are joined, across the other three body diagonals they
are not.

One host synchronisation per call is inherent, because the output size depends on the data: the count pass runs, the host
reads (V, F), allocates ``vertices`` and ``faces``, and the emit pass runs.  There is no other synchronisation and no atomic
operation: every output position comes from a fixed-order scan, so two calls are bit-equal (``measure`` too: block sums,
then one fixed-order sum).  A call cannot be captured into a graph.

Limits: every side <= 1024, (D+1)(H+1)(W+1) < 2^31, V and F < 2^31; anything beyond raises, nothing is truncated.

**Smoothing** (``adjacency`` / ``smooth``; ``tests/mesh_smooth_ref.py`` restates the rule in numpy).  The surface of a mask is
a staircase: every vertex sits at the midpoint of a lattice edge.  ``smooth`` moves the vertices and keeps the faces.

- **Neighbours.**  ``N(i)`` is the set of distinct vertices ``j != i`` that occur in a face together with ``i``, in ascending
  ``j``.  Both directions of every face edge count (an open or inconsistently wound mesh gets a symmetric table), duplicate
  faces add nothing, a face with a repeated index such as ``[1, 1, 2]`` contributes only its distinct pairs, and a vertex in
  no face has ``N(i)`` empty.  ``Adjacency(offsets int32 [V+1], neighbours int32 [E])`` holds the sets in vertex order:
  ``offsets[i+1] - offsets[i] = |N(i)|``.  For the closed oriented meshes ``extract_surface`` gives, ``E = 3F``; nothing relies
  on it.
- **One step with factor s** (float32, every operation rounded on its own, Jacobi: all reads come from the previous
  positions).  For a vertex with neighbours ``n_1 < n_2 < ...`` and ``fixed[i]`` false, per coordinate:
  ``acc = v[n_1]; acc = acc + v[n_2]; ...`` in ascending order, ``mean = acc / float32(|N(i)|)`` (a true division),
  ``v'_i = v_i + s * (mean - v_i)``.  A vertex without neighbours or with ``fixed[i]`` true keeps its bits; a fixed vertex
  still enters its neighbours' sums.
- **Iterations.**  One iteration is a step with ``lamb`` followed by a step with ``mu`` (Taubin's lambda|mu smoothing, which
  keeps the enclosed volume where plain Laplacian smoothing shrinks it); ``mu=None`` is Laplacian smoothing, one ``lamb`` step
  per iteration; ``iterations=0`` returns a bit-equal copy.  ``0 < lamb <= 1``; ``mu`` is finite with ``mu < -lamb`` (Taubin's
  ``0 < lambda < -mu``: the pass-band frequency ``1/lambda + 1/mu`` is positive); both are rounded to float32 once.
- **Bad indices.**  The build skips every face with an index outside ``[0, V)`` and counts it; ``adjacency`` then raises.  The
  smoothing kernel compares every offset against ``E`` and every neighbour against ``V`` before use, so a hand-made or
  corrupted ``Adjacency`` gives wrong positions, never an out-of-range read.
- **Synchronisation.**  ``adjacency`` synchronises with the host once, to read ``E`` (and the bad-face count) and size
  ``neighbours``; ``smooth(m)`` calls it; ``smooth(m, adjacency=a)`` neither synchronises nor builds.  The build uses integer
  atomics only where the final value does not depend on arrival order (counts, fill cursors) and sorts every neighbour
  list afterwards, so the table does not depend on the order of the faces and two calls are bit-equal.

Limits of smoothing: V < 2^31 and 6F < 2^31 (E and every offset fit an int32); anything beyond raises.

**Voxelisation** (``voxelize`` / ``winding_number``; ``tests/mesh_voxelize_ref.py`` restates the rule in numpy): the inverse of
``extract_surface``, mesh in, volume out, on any grid ``(shape, spacing, origin)``; the mesh need not come from that grid.
The centre of voxel (i, j, k) is ``origin + (i, j, k) * spacing`` per axis.  A voxel's value is the winding number of the
mesh around its centre, evaluated with rays along x, one per (z, y) row of the grid; ``voxelize`` is ``winding != 0``.  For
every mask ``M``, ``voxelize(extract_surface(M), M.shape) == M`` bit for bit, and a float field cut at ``level`` comes back as
``field > level``: the marching-tetrahedra surface separates the lattice points exactly by their insideness.

- **Arithmetic.**  float64; vertex coordinates are the float32 values widened; the centre n of axis a is
  ``double(origin_a) + n * double(spacing_a)`` (``spacing`` and ``origin`` are rounded to float32 once, as everywhere in this
  module); every product, difference, sum and division is rounded on its own (contraction is off on the device).
- **Faces that are skipped.**  A face with an index outside ``[0, V)`` or a vertex that is not finite is skipped on the
  device, never read through, and counted; the call then reads the count and raises ``ValueError``.  Otherwise a face with
  a repeated index contributes nothing, and neither does one whose projected doubled area
  ``A = (p1_z - p0_z)(p2_y - p0_y) - (p1_y - p0_y)(p2_z - p0_z)`` evaluates to 0 (``p0, p1, p2`` its corners in face order).
- **Rows of a face.**  A face is tested against the rows whose centre ``p = (z_i, y_j)`` lies in the closed bounding box of
  its three projected corners (exact float64 comparisons), and against no other.
- **Containment in projection.**  For each of the three edges (corner q to corner q+1), with ``a`` the endpoint of lower
  vertex index and ``b`` the other: ``E = (b_z - a_z)(p_y - a_y) - (b_y - a_y)(p_z - a_z)``, and the edge's sign is
  ``sign(E)``; where ``E == 0`` it is ``sign(-(b_y - a_y))`` and, where that is 0 too, ``sign(b_z - a_z)`` (the ray shifted by
  (+eps, +eps^2) in (z, y)); where all are 0 the edge projects to a point and the face contributes nothing.  The sign is
  negated if the face traverses the edge from ``b`` to ``a``.  Two faces that share an edge thereby see bit-identical
  arithmetic and opposite signs.  The ray crosses the face where the three signs agree, and that common sign is the
  crossing's weight: +1 where the ray enters through ``extract_surface``'s outward winding, -1 where it leaves.  Rays
  through vertices and edges are the main case, not an edge case: every vertex of a mask's mesh on an x-directed lattice
  edge projects exactly onto a row centre.
- **Depth.**  With ``e1 = p1 - p0``, ``e2 = p2 - p0``, ``n_z = e1_y e2_x - e1_x e2_y`` and ``n_y = e1_x e2_z - e1_z e2_x``:
  ``x_c = p0_x - (n_z (p_z - p0_z) + n_y (p_y - p0_y)) / A``.  The crossing weighs on every voxel of the row with
  ``x_k > x_c``, strictly, against the float64 centres above; one behind the row's last centre (or with ``x_c`` NaN) is
  dropped, one before the first weighs on the whole row.  The device estimates the first such ``k`` (a product with
  ``1 / spacing``), clamps the estimate in floating point (a vertex at 1e30 never reaches a float-to-int conversion) and
  corrects it by explicit comparison, so the estimate's rounding never shows.
- **Value.**  ``winding[i, j, k]`` = the sum of the weights of the row's crossings with ``x_c < x_k``.  A closed, consistently
  wound mesh without self-intersection gives 1 inside and 0 outside (-1 inside if wound inward); a smoothed mesh that
  self-intersects shows other values.  For a mesh that is not closed the result is defined by this rule, bounded, and reads
  or writes nothing out of range; it is not meaningful.
- **Device.**  One memset of an int32 delta volume, one scatter launch (a lane per face, integer ``atomicAdd`` of the weight at
  the crossing's first voxel; a face whose box holds more than 16 rows is walked by its whole wave), one scan launch
  (prefix sums along x).  Integer adds commute, so the result does not depend on the order of the faces or of arrival and
  two calls are bit-equal.  The read of the refused-face count is the call's one host synchronisation.  Workspace:
  ``voxelize_workspace_bytes``, 4 bytes per voxel and 256; processing the grid in slabs would shrink it and is the follow-up
  if 512^3 grids matter.  Limits: every side <= 1024, D*H*W < 2^31, V < 2^31, F < 2^31; anything beyond raises.

``read_stl`` is the host-side inverse of ``write_stl``: binary STL only, the stored corners welded where their three float32
values are bit-equal, vertices numbered in order of first appearance, faces in file order and winding, normals ignored.

**Distance to a mesh** (``build_face_grid`` / ``point_distance`` / ``distance_field``; ``tests/mesh_distance_ref.py`` restates
the rule in numpy as brute force over all faces): the missing inverse, mesh in, distance out, at any points or on any grid.

- **Distance from a point to a face.**  float64; ``p`` is the query widened (or a grid centre, formed as above), ``a, b, c``
  the face's corners in face order, float32 widened, all in (z, y, x); ``n = (b - a) x (c - a)``.  The squared distance to a
  segment ``u-v``: ``t = ((p - u) . (v - u)) / |v - u|^2`` clamped to [0, 1] (a segment of zero length is its endpoint, ``t = 0``),
  closest point ``q = u + t (v - u)``, ``|p - q|^2``.  The squared distance to the face is the minimum over its three edge segments
  ``a-b``, ``b-c``, ``c-a`` (the first wins a tie) and, where ``|n|^2 > 0`` and the three edge functions ``((b-a) x (p-a)) . n``,
  ``((c-b) x (p-b)) . n`` and ``((a-c) x (p-c)) . n`` are all >= 0, also the plane term ``((p-a) . n)^2 / |n|^2`` where it is
  smaller, with closest point ``p - (((p-a) . n) / |n|^2) n``.  Every product, difference, sum and division is rounded on its
  own (contraction is off on the device); a dot product is ``(x + y) + z``.  This form is continuous across the edge / interior
  classification, so a sliver that is classified one way or the other by rounding costs nothing; against the textbook
  region-based closest-point algorithm it agrees to 1e-16 of the scene's diagonal (``tests/test_mesh_distance_cpu.py``).
- **Degenerate faces.**  A face with a repeated index, or with collinear corners, is its segments; nothing is skipped for lack
  of area (``extract_surface`` gives such faces for samples equal to ``level``).
- **Distance from a point to a mesh.**  The minimum over the faces of the squared distance, ``sqrt`` in float64, rounded to
  float32 once.  The reported face is the lowest face index among those whose computed squared distance equals the minimum;
  the reported closest point is that face's closest point rounded to float32.
- **Refused input.**  A face with an index outside ``[0, V)`` or a vertex that is not finite is never read through; it is
  counted and the call raises ``ValueError``, as ``voxelize`` does.  A query that is not finite gives NaN, face -1, closest
  point NaN and touches no face.  With ``F == 0`` every distance is ``+inf`` and every face -1, without a launch of the kernels.
- **max_distance.**  A positive finite float32, or ``None``.  A query whose squared distance exceeds ``float64(max_distance)^2``
  gives ``+inf``, face -1 and closest point NaN (``distance_field`` stores ``max_distance`` there: a truncated field), and the
  search may stop there.  ``None`` is unbounded and exact at any distance; its cost grows with the distance of the query from
  the mesh.
- **Face grid.**  ``FaceGrid``: a uniform grid of cubic cells over the bounding box of the vertices the accepted faces use;
  ``floor(extent / cell_size) + 1`` cells per axis and one cell for an axis of zero extent (a planar mesh, a single triangle,
  coinciding vertices), at most ``min(2^24, max(65536, 64 F))`` cells.  Every face is listed in every cell its bounding box
  overlaps: count, scan, fill, with integer atomics only for the counts and the fill cursors, so the order of a cell's list
  depends on arrival and nothing else does.  One host synchronisation reads the pair count, the cell count and the
  refused-face count.
- **Search.**  A lane per query: from the query's cell, clamped into the grid, shells of cells outward.  A cell is skipped, and
  the search stops at a shell, only where a lower bound of the distance to it exceeds the best squared distance so far (or
  ``max_distance^2``), strictly; the bound is lowered by 2^-45 of the coordinates' magnitude before it is squared, which
  covers the rounding of the bound and of the cells' indices, so rounding can only lower it.  Every face that attains the
  minimum is therefore evaluated, each with the same arithmetic wherever it is met: the result is a function of the rule
  alone, does not depend on the cell size or on the order of a cell's list, and two calls are bit-equal.
- **Sign.**  Only grid centres get one: ``distance_field(signed=True)`` takes it from ``winding_number``.

Limits of the distance functions: V, F, Q and the face-cell pairs < 2^31; ``distance_field`` has ``voxelize``'s grid limits.

Out of scope: decimation, formats other than binary STL, marching cubes.
Out of scope of voxelisation: anti-aliased coverage, mesh repair.
Out of scope of the distance functions: the sign at arbitrary points, area-weighted or resampled surface metrics, a BVH.
"""
from __future__ import annotations

import ctypes
import math
from numbers import Integral, Real
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _args, _lib
from .metrics import parse_spacing

MAX_SIDE = 1024
SCAN_BLOCK = 1024          # CTU_MESH_SCAN_BLOCK: more cell rows, (D+1)(H+1), than this take the scan's second level
_MEASURE_WS = 16384        # CTU_MESH_MEASURE_WS
ADJ_SCAN_CHUNK = 4096      # CTU_MESH_ADJ_SCAN_CHUNK: more vertices than this take the adjacency scan's second level
MAX_ITERATIONS = 10000     # CTU_MESH_SMOOTH_MAX_ITERATIONS
MAX_CELLS = 1 << 24        # CTU_MESH_GRID_MAX_CELLS: no face grid has more cells
MIN_CELL_CAP = 1 << 16     # a grid of F faces has at most min(MAX_CELLS, max(MIN_CELL_CAP, 64 F)) cells
_MASK_DTYPES = (torch.bool, torch.uint8, torch.int64)
_DTYPES = _MASK_DTYPES + (torch.float32,)
assert (MAX_SIDE + 1) ** 3 < 1 << 31          # the side limit keeps the cells (D+1)(H+1)(W+1) of the padded grid below 2^31
_GRID = _args.Grid(shape="mesh: the shape must be a (D, H, W) triple, got {v!r}",
                   integers="mesh: the shape must be a (D, H, W) triple of integers, got {v!r}",
                   side=f"mesh: every side must lie in 1..{MAX_SIDE}, got {{vals}}", max_side=MAX_SIDE, max_voxels=None)
_ORIGIN = _args.Triple(shape="mesh: origin must be a number or a (z, y, x) triple, got {v!r}",
                       value="mesh: origin must be finite in float32, got {v!r}", float32=True)
_ON_GPU = "mesh: {} takes a mesh on the GPU; this path has no CPU fallback"


class Mesh(NamedTuple):
    """``vertices`` float32 [V,3] in (z, y, x) physical units, ``faces`` int32 [F,3]; both on the volume's device."""
    vertices: torch.Tensor
    faces: torch.Tensor


class Adjacency(NamedTuple):
    """The vertex -> neighbours table (CSR) of a mesh: ``offsets`` int32 [V+1], ``neighbours`` int32 [E], both on the mesh's
    device; the neighbours of vertex i are ``neighbours[offsets[i]:offsets[i+1]]``, ascending."""
    offsets: torch.Tensor
    neighbours: torch.Tensor


class FaceGrid(NamedTuple):
    """The uniform grid of face lists ``point_distance`` and ``distance_field`` search (CSR over the cells in C order):
    ``offsets`` int32 [cells+1] and ``faces`` int32 [pairs]: the faces whose bounding box overlaps cell c are
    ``faces[offsets[c]:offsets[c+1]]``, in no particular order; ``corners`` float32 [F,12]: the nine coordinates of every
    face (a, b, c in (z, y, x)) and three words of padding; ``frame`` float64 [6]: the lower corner of the grid and the
    cell size per axis; all on the mesh's device.  ``dims``: the cells per axis (nz, ny, nx), and ``cell_size``: the side of
    a cell, both on the host."""
    offsets: torch.Tensor
    faces: torch.Tensor
    corners: torch.Tensor
    frame: torch.Tensor
    dims: tuple
    cell_size: float


def _spacing(spacing):
    sp = parse_spacing(spacing, 1, "mesh: spacing")
    if sp is not None and len(sp) == 1 and isinstance(spacing, (list, tuple)) and len(spacing) == 1:
        raise ValueError(f"mesh: spacing must be a number or a (z, y, x) triple, got {spacing!r}")
    if sp is not None and any(not math.isfinite(v) or ctypes.c_float(v).value <= 0.0
                              or not math.isfinite(ctypes.c_float(v).value) for v in sp[0]):
        raise ValueError(f"mesh: spacing must be positive and finite in float32, got {spacing!r}")
    return None if sp is None else sp[0]


def _number(v, what: str) -> float:
    if isinstance(v, bool) or not isinstance(v, Real) or not math.isfinite(ctypes.c_float(float(v)).value):
        raise ValueError(f"mesh: {what} must be a finite real number, got {v!r}")
    return ctypes.c_float(float(v)).value


def _check_mesh(m, who: str):
    if not (isinstance(m, tuple) and len(m) == 2 and all(isinstance(t, torch.Tensor) for t in m)):
        raise ValueError(f"mesh: {who} takes a Mesh (vertices, faces), got {type(m).__name__}")
    v, f = m
    if v.dtype != torch.float32 or v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"mesh: vertices must be float32 [V,3], got {v.dtype} {tuple(v.shape)}")
    if f.dtype != torch.int32 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"mesh: faces must be int32 [F,3], got {f.dtype} {tuple(f.shape)}")
    if v.device != f.device:
        raise ValueError("mesh: vertices and faces must live on the same device")
    if f.shape[0] and not v.shape[0]:
        raise ValueError("mesh: faces without vertices")
    return v, f


def workspace_bytes(shape) -> int:
    """Device workspace (bytes) of one ``extract_surface`` call on a (D, H, W) volume: 5 bytes per cell of the padded grid
    (rows of W+1 cells rounded up to 16), 12 per cell row and 256; the only allocation besides the mesh itself."""
    return int(_lib.load().ctu_mesh_ws_bytes(*_args.grid(shape, _GRID)))


def extract_surface(volume: torch.Tensor, level: float = 0.5, spacing=None, origin=None, label: Optional[int] = None,
                    fill_value: Optional[float] = None) -> Mesh:
    """The closed triangle mesh of one ``[D,H,W]`` volume by the module docstring's rule.

    bool / uint8 / int64: the surface of ``volume != 0`` (``volume == label`` with ``label=``); ``level`` stays 0.5 and
    ``fill_value`` 0.  float32: the level set ``volume > level``, the virtual layer at ``fill_value`` (default ``level - 1``,
    at most ``level``).  ``spacing`` and ``origin`` are a number or a (z, y, x) triple (default 1 and 0).  A batch is a Python
    loop: meshes are ragged.  The call synchronises with the host once, to read (V, F) between its count and emit passes; a
    non-contiguous view is copied first.  Returns ``Mesh(vertices float32 [V,3] (z, y, x), faces int32 [F,3])`` on the
    volume's device; an empty surface gives V = F = 0."""
    if not isinstance(volume, torch.Tensor) or volume.dim() != 3:
        raise ValueError("mesh: volume must be one [D,H,W] tensor (loop over a batch: meshes are ragged)")
    if volume.dtype not in _DTYPES:
        raise ValueError(f"mesh: volume must be one of {', '.join(str(d) for d in _DTYPES)}, got {volume.dtype}")
    shape = _args.grid(tuple(volume.shape), _GRID)
    field = volume.dtype == torch.float32
    lev = _number(level, "level")
    sp, org = _spacing(spacing), _args.triple(origin, _ORIGIN)
    if field:
        if label is not None:
            raise ValueError("mesh: label belongs to bool / uint8 / int64 volumes; a float32 field is cut at level")
        fill = ctypes.c_float(lev - 1.0).value if fill_value is None else _number(fill_value, "fill_value")
        if fill > lev:
            raise ValueError(f"mesh: fill_value must not exceed level ({lev}), got {fill_value!r}")
        has_label, lab = 0, 0
    else:
        if lev != 0.5:
            raise ValueError(f"mesh: a mask is cut at level 0.5 (inside = 1, outside = 0), got level={level!r}")
        if fill_value is not None and _number(fill_value, "fill_value") != 0.0:
            raise ValueError(f"mesh: the virtual layer of a mask is 0, got fill_value={fill_value!r}")
        fill = 0.0
        if label is None:
            has_label, lab = 0, 0
        elif isinstance(label, bool) or not isinstance(label, Integral) or not -(1 << 63) <= label < (1 << 63):
            raise ValueError(f"mesh: label must be an integer of the map's range, got {label!r}")
        else:
            has_label, lab = 1, int(label)
    _lib.check_device("mesh: volume must live on the GPU; this path has no CPU fallback", volume)
    lib = _lib.load()
    src = _lib.as_bytes(volume)
    dt = _lib.DTYPE_CODE[src.dtype]
    dev = volume.device
    c_sp, c_org = _lib.float_array(sp), _lib.float_array(org)
    ws = torch.empty(lib.ctu_mesh_ws_bytes(*shape), dtype=torch.uint8, device=dev)
    with _lib.on(dev) as run:
        run("ctu_mesh_count", src.data_ptr(), dt, *shape, has_label, lab, lev, ws.data_ptr())
        nv, nf = ws[:16].view(torch.int64).tolist()                     # the call's one host synchronisation
        if nv >= 1 << 31 or nf >= 1 << 31:
            raise ValueError(f"mesh: the surface has {nv} vertices and {nf} faces; both must stay below 2^31")
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        run("ctu_mesh_emit", src.data_ptr(), dt, *shape, lev, fill, c_sp, c_org, nv, nf, vertices.data_ptr() if nv else None,
            faces.data_ptr() if nf else None, ws.data_ptr())
    return Mesh(vertices, faces)


def _measure(m, want_normals: bool, who: str):
    v, f = _check_mesh(m, who)
    _lib.check_device(_ON_GPU.format(who), v)
    v, f = v.contiguous(), f.contiguous()
    out = torch.empty(2, dtype=torch.float64, device=v.device)
    normals = torch.empty((f.shape[0], 3), dtype=torch.float32, device=v.device) if want_normals else None
    ws = torch.empty(_MEASURE_WS, dtype=torch.uint8, device=v.device)
    with _lib.on(v.device) as run:
        run("ctu_mesh_measure", v.data_ptr() if v.shape[0] else None, v.shape[0], f.data_ptr() if f.shape[0] else None,
            f.shape[0], out.data_ptr(), normals.data_ptr() if want_normals and f.shape[0] else None, ws.data_ptr())
    return out, normals


def measure(m: Mesh) -> torch.Tensor:
    """float64 device tensor [2] = (surface area, enclosed volume) in the units of the vertices: per-face area and signed
    volume term ``p0 . (p1 x p2) / 6`` in float64 from the float32 vertices, summed in a fixed order (two calls are
    bit-equal).  The volume is positive for the outward winding ``extract_surface`` gives.  No host synchronisation."""
    return _measure(m, False, "measure")[0]


def face_normals(m: Mesh) -> torch.Tensor:
    """float32 [F,3] unit normals in (z, y, x), right-handed in (x, y, z): outward for ``extract_surface``'s winding; the zero
    vector for a face without area."""
    return _measure(m, True, "face_normals")[1]


def _check_sizes(v, f, who: str):
    V, F = v.shape[0], f.shape[0]
    if V >= 1 << 31 or 6 * F >= 1 << 31:
        raise ValueError(f"mesh: {who} takes V < 2^31 vertices and 6F < 2^31, got V = {V}, F = {F}")
    return V, F


def adjacency(m: Mesh) -> Adjacency:
    """The vertex -> neighbours table of a mesh on the GPU, by the module docstring's rule.  The call synchronises with the
    host once, to read E between its build and emit passes; a face index outside ``[0, V)`` raises (such faces are skipped
    on the device, never read through).  An empty mesh gives all-zero offsets and E = 0 without any launch."""
    v, f = _check_mesh(m, "adjacency")
    V, F = _check_sizes(v, f, "adjacency")
    _lib.check_device(_ON_GPU.format("adjacency"), v)
    return _build_adjacency(f, V, F)


def _build_adjacency(f: torch.Tensor, V: int, F: int) -> Adjacency:
    dev = f.device
    if V == 0 or F == 0:
        return Adjacency(torch.zeros(V + 1, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev))
    lib = _lib.load()
    f = f.contiguous()
    ws = torch.empty(lib.ctu_mesh_adjacency_ws_bytes(V, F), dtype=torch.uint8, device=dev)
    offsets = torch.empty(V + 1, dtype=torch.int32, device=dev)
    with _lib.on(dev) as run:
        run("ctu_mesh_adjacency_build", f.data_ptr(), V, F, offsets.data_ptr(), ws.data_ptr())
        ne, bad = ws[:16].view(torch.int64).tolist()                    # the call's one host synchronisation
        if bad:
            raise ValueError(f"mesh: a face refers to a vertex that does not exist ({bad} of {F} faces hold an index outside [0, {V}))")
        neighbours = torch.empty(ne, dtype=torch.int32, device=dev)
        run("ctu_mesh_adjacency_emit", V, F, ne, offsets.data_ptr(), neighbours.data_ptr() if ne else None, ws.data_ptr())
    return Adjacency(offsets, neighbours)


def smooth_workspace_bytes(V: int, F: int) -> int:
    """The most device memory (bytes) one ``smooth`` call on a contiguous mesh of V vertices and F faces allocates besides its
    result: the two staged position buffers (16 bytes per vertex each), which is all a call with ``adjacency=`` allocates,
    and the adjacency it builds otherwise: the build's workspace (``ctu_mesh_adjacency_ws_bytes``), ``offsets`` and at most
    6F ``neighbours``."""
    if any(isinstance(n, bool) or not isinstance(n, Integral) for n in (V, F)) or V < 0 or F < 0 or V >= 1 << 31 or 6 * F >= 1 << 31:
        raise ValueError(f"mesh: smooth_workspace_bytes takes 0 <= V < 2^31 and 0 <= 6F < 2^31, got {V!r}, {F!r}")
    lib = _lib.load()
    return int(lib.ctu_mesh_smooth_ws_bytes(V)) + int(lib.ctu_mesh_adjacency_ws_bytes(V, F)) + 4 * (int(V) + 1) + 24 * int(F)


def _factor(x, what: str) -> float:
    if isinstance(x, bool) or not isinstance(x, Real) or not math.isfinite(float(x)):
        raise ValueError(f"mesh: {what} must be a finite real number, got {x!r}")
    return ctypes.c_float(float(x)).value


def smooth(m: Mesh, iterations: int = 10, lamb: float = 0.5, mu: Optional[float] = -0.53, fixed: Optional[torch.Tensor] = None,
           adjacency: Optional[Adjacency] = None) -> Mesh:
    """``Mesh(new vertices, m.faces)`` after ``iterations`` of Taubin smoothing (``mu=None``: Laplacian) by the module
    docstring's rule; ``m.vertices`` is left untouched and ``faces`` is the same tensor.  ``fixed``: a bool / uint8 ``[V]``
    tensor on the mesh's device, true where a vertex must keep its position.  ``adjacency``: the table of ``adjacency(m)`` to
    reuse; with it the call neither synchronises nor allocates anything besides the result and
    ``ctu_mesh_smooth_ws_bytes(V)``; without it the table is built first (one synchronisation)."""
    v, f = _check_mesh(m, "smooth")
    V, F = _check_sizes(v, f, "smooth")
    if isinstance(iterations, bool) or not isinstance(iterations, Integral) or not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"mesh: iterations must be an integer in 0..{MAX_ITERATIONS}, got {iterations!r}")
    lam = _factor(lamb, "lamb")
    if not 0.0 < lam <= 1.0:
        raise ValueError(f"mesh: lamb must lie in (0, 1], got {lamb!r}")
    mu32 = None if mu is None else _factor(mu, "mu")
    if mu32 is not None and not (math.isfinite(mu32) and mu32 < -lam):
        raise ValueError(f"mesh: mu must be None or finite with mu < -lamb (Taubin's 0 < lambda < -mu), got mu={mu!r}, lamb={lamb!r}")
    if fixed is not None:
        if not isinstance(fixed, torch.Tensor) or fixed.dtype not in (torch.bool, torch.uint8) or tuple(fixed.shape) != (V,):
            raise ValueError(f"mesh: fixed must be a bool or uint8 [V] tensor with V = {V}, got "
                             f"{getattr(fixed, 'dtype', type(fixed).__name__)} {tuple(getattr(fixed, 'shape', ()))}")
        if fixed.device != v.device:
            raise ValueError("mesh: fixed must live on the mesh's device")
    if adjacency is not None:
        if not (isinstance(adjacency, tuple) and len(adjacency) == 2 and all(isinstance(t, torch.Tensor) for t in adjacency)):
            raise ValueError(f"mesh: adjacency must be an Adjacency (offsets, neighbours), got {type(adjacency).__name__}")
        off, nb = adjacency
        if off.dtype != torch.int32 or nb.dtype != torch.int32 or off.dim() != 1 or nb.dim() != 1:
            raise ValueError(f"mesh: offsets and neighbours must be int32 vectors, got {off.dtype} {tuple(off.shape)} and "
                             f"{nb.dtype} {tuple(nb.shape)}")
        if off.shape[0] != V + 1:
            raise ValueError(f"mesh: offsets must have V + 1 = {V + 1} entries, got {off.shape[0]}")
        if nb.shape[0] >= 1 << 31:
            raise ValueError(f"mesh: neighbours must have fewer than 2^31 entries, got {nb.shape[0]}")
        if off.device != v.device or nb.device != v.device:
            raise ValueError("mesh: the adjacency must live on the mesh's device")
    _lib.check_device(_ON_GPU.format("smooth"), v)
    off, nb = adjacency if adjacency is not None else _build_adjacency(f, V, F)
    lib = _lib.load()
    src, off, nb = v.contiguous(), off.contiguous(), nb.contiguous()
    fx = None
    if fixed is not None:
        fx = _lib.as_bytes(fixed)
    out = torch.empty((V, 3), dtype=torch.float32, device=v.device)
    ws = torch.empty(lib.ctu_mesh_smooth_ws_bytes(V), dtype=torch.uint8, device=v.device)
    with _lib.on(v.device) as run:
        run("ctu_mesh_smooth", src.data_ptr() if V else None, V, off.data_ptr(), nb.data_ptr() if nb.shape[0] else None,
            nb.shape[0], fx.data_ptr() if fx is not None and V else None, int(iterations), lam, int(mu32 is not None),
            0.0 if mu32 is None else mu32, out.data_ptr() if V else None, ws.data_ptr())
    return Mesh(out, f)


def voxelize_workspace_bytes(shape) -> int:
    """Device workspace (bytes) of one ``voxelize`` or ``winding_number`` call onto a (D, H, W) grid: the int32 delta volume
    (4 bytes per voxel, rounded up to 256) and 256 for the refused-face count; the only allocation besides the result and
    contiguous copies of non-contiguous inputs."""
    return int(_lib.load().ctu_mesh_voxelize_ws_bytes(*_args.grid(shape, _GRID)))


def _voxelize(m, shape, spacing, origin, winding: bool, who: str) -> torch.Tensor:
    v, f = _check_mesh(m, who)
    V, F = v.shape[0], f.shape[0]
    if V >= 1 << 31 or F >= 1 << 31:
        raise ValueError(f"mesh: {who} takes V < 2^31 vertices and F < 2^31 faces, got V = {V}, F = {F}")
    shape = _args.grid(shape, _GRID)
    sp, org = _spacing(spacing), _args.triple(origin, _ORIGIN)
    _lib.check_device(_ON_GPU.format(who), v)
    dev = v.device
    dtype = torch.int32 if winding else torch.uint8
    if F == 0:
        return torch.zeros(shape, dtype=dtype, device=dev)
    lib = _lib.load()
    v, f = v.contiguous(), f.contiguous()
    out = torch.empty(shape, dtype=dtype, device=dev)
    ws = torch.empty(lib.ctu_mesh_voxelize_ws_bytes(*shape), dtype=torch.uint8, device=dev)
    with _lib.on(dev) as run:
        run("ctu_mesh_voxelize", v.data_ptr(), V, f.data_ptr(), F, *shape, _lib.float_array(sp), _lib.float_array(org),
            int(winding), out.data_ptr(), ws.data_ptr())
        bad = int(ws[:8].view(torch.int64).item())                      # the call's one host synchronisation
    if bad:
        raise ValueError(f"mesh: a face refers to a vertex that does not exist or is not finite ({bad} of {F} faces hold an "
                         f"index outside [0, {V}) or a NaN / infinite coordinate)")
    return out


def voxelize(m: Mesh, shape, spacing=None, origin=None) -> torch.Tensor:
    """uint8 ``[D,H,W]`` on the mesh's device: 1 where the winding number of the mesh around the voxel's centre
    ``origin + (i, j, k) * spacing`` is not 0, by the module docstring's rule; the inverse of ``extract_surface``.  ``shape``,
    ``spacing`` and ``origin`` describe the target grid with ``extract_surface``'s conventions (a number or a (z, y, x) triple,
    default 1 and 0); the grid need not be the one the mesh was extracted on.  One host synchronisation (the refused-face
    count); a face index outside ``[0, V)`` or a vertex that is not finite raises.  An empty mesh gives zeros without a
    launch of the kernels."""
    return _voxelize(m, shape, spacing, origin, False, "voxelize")


def winding_number(m: Mesh, shape, spacing=None, origin=None) -> torch.Tensor:
    """int32 ``[D,H,W]``: the winding numbers ``voxelize`` thresholds, through the same device path: 0 / 1 for a closed
    outward-wound mesh, 0 / -1 for an inward-wound one, other values where a (smoothed) mesh intersects itself."""
    return _voxelize(m, shape, spacing, origin, True, "winding_number")


def _max_cells(F: int) -> int:
    return min(MAX_CELLS, max(MIN_CELL_CAP, 64 * int(F)))


def _cell_size(cell_size):
    if cell_size is None:
        return 0.0
    c = ctypes.c_float(float(cell_size)).value if isinstance(cell_size, Real) and not isinstance(cell_size, bool) else None
    if c is None or not (math.isfinite(c) and c > 0.0):
        raise ValueError(f"mesh: cell_size must be None or positive and finite in float32, got {cell_size!r}")
    return c


def distance_workspace_bytes(V: int, F: int, cell_size=None) -> int:
    """The most device memory (bytes) one ``build_face_grid`` call on a contiguous mesh of V vertices and F faces allocates
    besides the ``FaceGrid`` it returns: the build's workspace ``ctu_mesh_grid_ws_bytes(F, max_cells)``, where ``max_cells =
    min(2^24, max(65536, 64 F))`` caps the cells of the grid: 256 bytes, 64 per block of 256 faces, 8 per cell of the cap and
    8 per scan chunk of 4096 cells, each array rounded up to 256.  It does not depend on V or on ``cell_size`` (the cap
    holds for every size), which are validated and otherwise unused.  The ``FaceGrid`` itself holds 48 bytes per face,
    4 per cell and 4 per face-cell pair.  ``point_distance`` and ``distance_field`` with ``grid=`` allocate their results
    and nothing else; without it they build the grid first."""
    if any(isinstance(n, bool) or not isinstance(n, Integral) for n in (V, F)) or V < 0 or F < 0 or V >= 1 << 31 or F >= 1 << 31:
        raise ValueError(f"mesh: distance_workspace_bytes takes 0 <= V < 2^31 and 0 <= F < 2^31, got {V!r}, {F!r}")
    _cell_size(cell_size)
    if F == 0:
        return 0
    return int(_lib.load().ctu_mesh_grid_ws_bytes(int(F), _max_cells(F)))


def _empty_grid(dev) -> FaceGrid:
    return FaceGrid(torch.zeros(2, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                    torch.empty((0, 12), dtype=torch.float32, device=dev),
                    torch.tensor([0.0, 0.0, 0.0, 1.0, 1.0, 1.0], dtype=torch.float64, device=dev), (1, 1, 1), 1.0)


def build_face_grid(m: Mesh, cell_size: Optional[float] = None) -> FaceGrid:
    """The ``FaceGrid`` of a mesh on the GPU, by the module docstring's rule: what ``point_distance`` and ``distance_field``
    search, reusable for any number of queries against the same mesh (it holds the faces' coordinates: rebuild it when the
    vertices move).  ``cell_size``: the side of a cell in the units of the vertices, rounded to float32; ``None``: twice the
    mean largest extent of a face, which lists a few faces per cell for the meshes ``extract_surface`` gives, doubled until
    the grid has at most ``min(2^24, max(65536, 64 F))`` cells.  A given ``cell_size`` that needs more cells than that, or any
    that lists 2^31 face-cell pairs or more, raises ``ValueError`` (a face is listed in every cell its bounding box
    overlaps, so a cell far smaller than the faces multiplies the pairs).  The result of a query does not depend on
    ``cell_size``; its speed does.  The call synchronises with the host once, to read the pair count, the cell count and the
    refused-face count; a face index outside ``[0, V)`` or a vertex that is not finite raises (such faces are listed
    nowhere and never read through).  A mesh without faces gives an empty one-cell grid without any launch."""
    v, f = _check_mesh(m, "build_face_grid")
    V, F = v.shape[0], f.shape[0]
    if V >= 1 << 31 or F >= 1 << 31:
        raise ValueError(f"mesh: build_face_grid takes V < 2^31 vertices and F < 2^31 faces, got V = {V}, F = {F}")
    size = _cell_size(cell_size)
    _lib.check_device(_ON_GPU.format("build_face_grid"), v)
    dev = v.device
    if F == 0:
        return _empty_grid(dev)
    lib = _lib.load()
    v, f = v.contiguous(), f.contiguous()
    cap = _max_cells(F)
    corners = torch.empty((F, 12), dtype=torch.float32, device=dev)
    ws = torch.empty(lib.ctu_mesh_grid_ws_bytes(F, cap), dtype=torch.uint8, device=dev)
    with _lib.on(dev) as run:
        run("ctu_mesh_grid_build", v.data_ptr(), V, f.data_ptr(), F, size, cap, corners.data_ptr(), ws.data_ptr())
        head = ws[:104].cpu()                                           # the call's one host synchronisation
        pairs, bad, cells, overflow, nz, ny, nx = head[:56].view(torch.int64).tolist()
        lo_h = head[56:104].view(torch.float64).tolist()
        if bad:
            raise ValueError(f"mesh: a face refers to a vertex that does not exist or is not finite ({bad} of {F} faces hold an "
                             f"index outside [0, {V}) or a NaN / infinite coordinate)")
        if overflow:
            raise ValueError(f"mesh: cell_size={cell_size!r} needs more than {cap} cells for this mesh; choose a larger cell_size")
        if pairs >= 1 << 31:
            raise ValueError(f"mesh: the face grid lists {pairs} face-cell pairs; they must stay below 2^31: choose a larger cell_size")
        offsets = torch.empty(cells + 1, dtype=torch.int32, device=dev)
        items = torch.empty(pairs, dtype=torch.int32, device=dev)
        frame = ws[56:104].view(torch.float64).clone()
        run("ctu_mesh_grid_emit", corners.data_ptr(), F, cap, cells, pairs, offsets.data_ptr(),
            items.data_ptr() if pairs else None, ws.data_ptr())
    return FaceGrid(offsets, items, corners, frame, (nz, ny, nx), lo_h[3])


def _check_grid(grid, F: int, dev) -> FaceGrid:
    if not (isinstance(grid, tuple) and len(grid) == 6 and all(isinstance(t, torch.Tensor) for t in grid[:4])):
        raise ValueError(f"mesh: grid must be a FaceGrid (the result of build_face_grid), got {type(grid).__name__}")
    off, items, corners, frame, dims, _ = grid
    if off.dtype != torch.int32 or items.dtype != torch.int32 or off.dim() != 1 or items.dim() != 1:
        raise ValueError(f"mesh: the grid's offsets and faces must be int32 vectors, got {off.dtype} {tuple(off.shape)} and "
                         f"{items.dtype} {tuple(items.shape)}")
    if corners.dtype != torch.float32 or tuple(corners.shape) != (F, 12):
        raise ValueError(f"mesh: the grid belongs to another mesh: corners must be float32 [{F}, 12], got {corners.dtype} "
                         f"{tuple(corners.shape)}")
    if frame.dtype != torch.float64 or tuple(frame.shape) != (6,):
        raise ValueError(f"mesh: the grid's frame must be float64 [6], got {frame.dtype} {tuple(frame.shape)}")
    try:
        dims = tuple(dims)
    except TypeError:
        dims = ()
    if len(dims) != 3 or any(isinstance(n, bool) or not isinstance(n, Integral) or n < 1 for n in dims) \
            or dims[0] * dims[1] * dims[2] > MAX_CELLS or off.shape[0] != dims[0] * dims[1] * dims[2] + 1:
        raise ValueError(f"mesh: the grid's dims must be three positive integers with at most {MAX_CELLS} cells and "
                         f"offsets one entry per cell and one, got dims {grid[4]!r} and {off.shape[0]} offsets")
    if items.shape[0] >= 1 << 31:
        raise ValueError(f"mesh: the grid must list fewer than 2^31 face-cell pairs, got {items.shape[0]}")
    if any(t.device != dev for t in (off, items, corners, frame)):
        raise ValueError("mesh: the grid must live on the mesh's device")
    return FaceGrid(off.contiguous(), items.contiguous(), corners.contiguous(), frame.contiguous(), tuple(int(n) for n in dims), grid[5])


def _max_distance(max_distance, who: str, required: bool) -> float:
    if max_distance is None and not required:
        return 0.0
    md = None
    if isinstance(max_distance, Real) and not isinstance(max_distance, bool):
        md = ctypes.c_float(float(max_distance)).value
    if md is None or not (math.isfinite(md) and md > 0.0):
        raise ValueError(f"mesh: {who} takes a max_distance that is positive and finite in float32"
                         f"{'' if required else ', or None'}, got {max_distance!r}")
    return md


def _query(g: FaceGrid, F: int, points, shape, sp, org, md: float, far: float, want_faces: bool, want_points: bool, dev):
    Q = points.shape[0] if points is not None else shape[0] * shape[1] * shape[2]
    dist = torch.empty(Q, dtype=torch.float32, device=dev)
    faces = torch.empty(Q, dtype=torch.int32, device=dev) if want_faces else None
    closest = torch.empty((Q, 3), dtype=torch.float32, device=dev) if want_points else None
    if Q == 0:
        return dist, faces, closest
    if F == 0:                                                          # no face: every finite query is infinitely far
        dist.fill_(far)
        if points is not None:
            dist[~torch.isfinite(points).all(dim=1)] = float("nan")
        if faces is not None:
            faces.fill_(-1)
        if closest is not None:
            closest.fill_(float("nan"))
        return dist, faces, closest
    with _lib.on(dev) as run:
        run("ctu_mesh_distance", g.corners.data_ptr(), F, g.offsets.data_ptr(), g.faces.data_ptr() if g.faces.shape[0] else None,
            g.faces.shape[0], g.frame.data_ptr(), *g.dims, points.data_ptr() if points is not None else None,
            Q if points is not None else 0, *(shape if points is None else (0, 0, 0)), _lib.float_array(sp),
            _lib.float_array(org), md, far, dist.data_ptr(), faces.data_ptr() if want_faces else None,
            closest.data_ptr() if want_points else None)
    return dist, faces, closest


def point_distance(points: torch.Tensor, m: Mesh, max_distance: Optional[float] = None, return_faces: bool = False,
                   return_points: bool = False, grid: Optional[FaceGrid] = None, cell_size: Optional[float] = None):
    """float32 ``[Q]``: the exact distance from every point to the surface of the mesh, by the module docstring's rule.
    ``points``: float32 ``[Q,3]`` in (z, y, x) on the mesh's device; ``Q == 0`` works.  ``return_faces``: also int32 ``[Q]``,
    the lowest index among the nearest faces; ``return_points``: also float32 ``[Q,3]``, that face's closest point; the
    result is then a tuple in that order.  ``max_distance`` (positive, rounded to float32): a point farther away gets
    ``inf``, face -1 and closest point NaN, and its search stops there; ``None`` is exact at any distance, at a cost that
    grows with the distance of the point from the mesh (the search visits the cells of the grid shell by shell until a
    shell lies farther than the best face found).  A point that is not finite gets NaN, -1, NaN; a mesh without faces
    gives ``inf`` everywhere.  ``grid``: the ``FaceGrid`` of ``build_face_grid(m)`` to reuse; with it the call neither
    synchronises nor allocates anything besides its results.  Without it the grid is built first (one synchronisation),
    with ``cell_size``, which changes the speed and never the result."""
    v, f = _check_mesh(m, "point_distance")
    V, F = v.shape[0], f.shape[0]
    if V >= 1 << 31 or F >= 1 << 31:
        raise ValueError(f"mesh: point_distance takes V < 2^31 vertices and F < 2^31 faces, got V = {V}, F = {F}")
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"mesh: points must be a float32 [Q,3] tensor, got {getattr(points, 'dtype', type(points).__name__)} "
                         f"{tuple(getattr(points, 'shape', ()))}")
    if points.shape[0] >= 1 << 31:
        raise ValueError(f"mesh: point_distance takes Q < 2^31 points, got {points.shape[0]}")
    if points.device != v.device:
        raise ValueError(f"mesh: the points live on {points.device}, the mesh on {v.device}")
    md = _max_distance(max_distance, "point_distance", False)
    if grid is not None and cell_size is not None:
        raise ValueError("mesh: cell_size belongs to the build; give grid= or cell_size=, not both")
    _cell_size(cell_size)
    if grid is not None:
        grid = _check_grid(grid, F, v.device)
    _lib.check_device(_ON_GPU.format("point_distance"), v)
    g = grid if grid is not None else build_face_grid(m, cell_size)
    dist, faces, closest = _query(g, F, points.contiguous(), None, None, None, md, float("inf"), bool(return_faces),
                                  bool(return_points), v.device)
    out = (dist,) + ((faces,) if return_faces else ()) + ((closest,) if return_points else ())
    return out[0] if len(out) == 1 else out


_REQUIRED = object()


def distance_field(m: Mesh, shape, spacing=None, origin=None, max_distance=_REQUIRED, signed: bool = False,
                   grid: Optional[FaceGrid] = None) -> torch.Tensor:
    """float32 ``[D,H,W]`` on the mesh's device: the distance from the centre ``origin + (i, j, k) * spacing`` of every voxel
    to the surface of the mesh, truncated at ``max_distance``, by the module docstring's rule.  ``shape``, ``spacing`` and
    ``origin`` describe the grid with ``voxelize``'s conventions and limits; the centres are formed in float64 in the kernel
    as ``voxelize`` forms them, and no list of points is materialised.  ``max_distance`` is required (a whole grid has far
    voxels, and the search of each stops there): voxels farther away hold ``max_distance``, not ``inf``.  ``signed=True``
    multiplies by -1 where ``winding_number(m, shape, spacing, origin) != 0``: positive outside, negative inside, the
    convention of ``postprocess.signed_distance``; it costs that call, its workspace and its synchronisation.  ``grid``: a
    prebuilt ``FaceGrid``; with it and ``signed=False`` the call neither synchronises nor allocates anything besides the
    result.  A mesh without faces gives ``max_distance`` everywhere."""
    v, f = _check_mesh(m, "distance_field")
    V, F = v.shape[0], f.shape[0]
    if V >= 1 << 31 or F >= 1 << 31:
        raise ValueError(f"mesh: distance_field takes V < 2^31 vertices and F < 2^31 faces, got V = {V}, F = {F}")
    shape = _args.grid(shape, _GRID)
    sp, org = _spacing(spacing), _args.triple(origin, _ORIGIN)
    if max_distance is _REQUIRED:
        raise ValueError("mesh: distance_field takes a max_distance (a whole grid has far voxels; the field is truncated there)")
    md = _max_distance(max_distance, "distance_field", True)
    if grid is not None:
        grid = _check_grid(grid, F, v.device)
    _lib.check_device(_ON_GPU.format("distance_field"), v)
    g = grid if grid is not None else build_face_grid(m)
    dist, _, _ = _query(g, F, None, shape, sp, org, md, md, False, False, v.device)
    out = dist.view(shape)
    if signed:
        out = torch.where(winding_number(m, shape, spacing, origin) != 0, -out, out)
    return out


def transform(m: Mesh, matrix) -> Mesh:
    """The mesh with every vertex moved through ``matrix`` (float64 [3,4] or [4,4] on the mesh's device, acting on (z, y, x)
    column vectors: ``registration``'s ``matrix`` / ``inverse``): ``R v + t`` in float64, rounded to float32 once.  The faces
    are shared, not copied; a matrix with a negative determinant flips the surface's orientation and is not corrected.
    A ``registration.DeformableResult`` in place of the matrix pushes the vertices through ``registration.transform_points``."""
    v, f = _check_mesh(m, "transform")
    from . import registration
    if isinstance(matrix, registration.DeformableResult):
        return Mesh(registration.transform_points(v, matrix), f)
    if not isinstance(matrix, torch.Tensor) or matrix.dtype != torch.float64 or tuple(matrix.shape) not in ((3, 4), (4, 4)):
        raise ValueError("mesh: transform takes a float64 matrix [3,4] or [4,4]")
    if matrix.device != v.device:
        raise ValueError(f"mesh: the matrix lives on {matrix.device}, the mesh on {v.device}")
    moved = v.to(torch.float64) @ matrix[:3, :3].T + matrix[:3, 3]
    return Mesh(moved.to(torch.float32), f)


def stl_bytes(vertices, faces, header: bytes = b"") -> bytes:
    """The binary STL of host arrays ``vertices [V,3]`` (z, y, x) and ``faces [F,3]``: the 80-byte header, the uint32 count and
    50 bytes per triangle: normal and three corners as little-endian float32 in (x, y, z), then a zero uint16.  The winding
    is kept, so the stored right-hand normal points outward."""
    if not isinstance(header, (bytes, bytearray)) or len(header) > 80:
        raise ValueError(f"mesh: an STL header is at most 80 bytes, got {header!r}")
    if bytes(header[:5]).lower() == b"solid":
        raise ValueError("mesh: a binary STL header must not begin with 'solid' (readers take it for the ASCII form)")
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32)[:, ::-1])
    f = np.asarray(faces, dtype=np.int64)
    if len(f) >= 1 << 32:
        raise ValueError("mesh: binary STL counts its triangles in a uint32")
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("mesh: a face refers to a vertex that does not exist")
    rec = np.zeros(len(f), dtype=np.dtype([("n", "<f4", 3), ("p", "<f4", (3, 3)), ("a", "<u2")]))
    p = v[f] if len(f) else np.zeros((0, 3, 3), dtype=np.float32)
    n = np.cross(p[:, 1].astype(np.float64) - p[:, 0], p[:, 2].astype(np.float64) - p[:, 0])
    length = np.sqrt((n * n).sum(axis=1, keepdims=True))
    rec["n"] = np.divide(n, length, out=np.zeros_like(n), where=length > 0)
    rec["p"] = p
    return bytes(header).ljust(80, b"\0") + np.uint32(len(f)).astype("<u4").tobytes() + rec.tobytes()


def write_stl(path, m: Mesh, header: bytes = b"") -> None:
    """Write the mesh as binary STL (``stl_bytes``); the mesh may live on the GPU or on the host (it is copied to the host
    either way: this is file output)."""
    v, f = _check_mesh(m, "write_stl")
    data = stl_bytes(v.detach().cpu().numpy(), f.detach().cpu().numpy(), header)
    with open(path, "wb") as fh:
        fh.write(data)


def read_stl(source) -> Mesh:
    """The ``Mesh`` of a binary STL file, on the host: ``source`` is a path or a bytes object.  The stored corners are taken as
    they are (the stored normals are ignored), returned as (z, y, x) columns, and welded where their three float32 values
    are bit-equal (so -0.0 and 0.0 stay apart); vertices are numbered in order of first appearance, faces keep the file's
    order and winding.  For a mesh without unreferenced or duplicate vertices ``read_stl(stl_bytes(v, f))`` gives the same
    triangles back (``v[f]``, bit for bit), and ``(v, f)`` itself where ``v`` is numbered in that order.  A truncated file, a triangle count that does not match the length and the ASCII form raise ``ValueError``."""
    if isinstance(source, (bytes, bytearray, memoryview)):
        data = bytes(source)
    else:
        with open(source, "rb") as fh:
            data = fh.read()
    if len(data) < 84:
        if data[:5].lower() == b"solid":
            raise ValueError("mesh: read_stl reads binary STL only; this is the ASCII form (it begins with 'solid')")
        raise ValueError(f"mesh: a binary STL has an 80-byte header and a 4-byte count; this one is truncated at {len(data)} bytes")
    nf = int(np.frombuffer(data, dtype="<u4", count=1, offset=80)[0])
    if len(data) != 84 + 50 * nf:
        if data[:5].lower() == b"solid":
            raise ValueError("mesh: read_stl reads binary STL only; this is the ASCII form (it begins with 'solid')")
        if len(data) < 84 + 50 * nf:
            raise ValueError(f"mesh: the STL counts {nf} triangles ({84 + 50 * nf} bytes) and is truncated at {len(data)} bytes")
        raise ValueError(f"mesh: the STL counts {nf} triangles ({84 + 50 * nf} bytes) and holds {len(data)} bytes")
    rec = np.frombuffer(data, dtype=np.dtype([("n", "<f4", 3), ("p", "<f4", (3, 3)), ("a", "<u2")]), count=nf, offset=84)
    corners = np.ascontiguousarray(rec["p"].reshape(-1, 3)[:, ::-1]).astype(np.float32)            # (z, y, x)
    if nf == 0:
        return Mesh(torch.zeros((0, 3), dtype=torch.float32), torch.zeros((0, 3), dtype=torch.int32))
    keys = corners.view(np.uint32).reshape(-1, 3)
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                            # unique rows in order of first appearance
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    vertices = corners[first[order]]
    faces = rank[inverse.reshape(-1)].reshape(-1, 3).astype(np.int32)
    return Mesh(torch.from_numpy(np.ascontiguousarray(vertices)), torch.from_numpy(faces))
