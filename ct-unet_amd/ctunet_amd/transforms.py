"""Flap-reconstruction augmentation on the MI355X: the reference's ``flap_rec_transform`` (ctunet/pytorch/transforms.py:
131-134) = ``SkullRandomHole(double_output=True)`` then ``SaltAndPepper(p=.5, noise_density=.05)``, for batches of binary
skulls on the device, in three kernel launches (csrc/augment.hip) with no host sync, so it can be captured in a graph.

Semantics (reference line numbers in ctunet/pytorch/transforms.py unless noted):

SkullRandomHole, per sample (13-95 and random_blank_patch, 241-300):
  * the hole is drawn iff u < p (the reference's ``p >= r``: p = 1 always, p = 0 never, up to measure zero);
  * a voxel's value is its uint8 cast (truncation; float inputs are expected in [0, 256)) and it is bone iff that is
    nonzero (``np.argwhere(image > 0)`` on the uint8 copy, 66-69 and 246);
  * no bone, or the hole not drawn: image unchanged (its uint8 cast), flap all zero (298-300);
  * centre = ``argwhere(bone)[k]``, k uniform in [0, count), C order (z, y, x) (249-251);
  * ``size = randint(min_r, max_r)``, high exclusive, ``min_r = min(D,H,W)//5 - 1``,
    ``max_r = max(min_r, max(D,H,W)//3.5)`` (float floor division, 262-264); an empty range raises ValueError on the host
    as NumPy does -- for any real shape max(D,H,W)//3.5 >= min(D,H,W)//5 > min_r, so it is never empty in practice;
  * shape uniform over {sphere, box, flap} (or over the ``shapes=`` list, in its order) (266-270);
      sphere: dz^2 + dy^2 + dx^2 <= size^2 in integers (size >= 0) == the float64 ``norm(., 2) <= size`` of
              utilities.shape_3d (utilities.py:140-144,168-175);
      box:    max(|dz|, |dy|, |dx|) <= size == ``norm(., inf) <= size``;
      flap:   UNPINNED.  utilities.py:145-165 builds it with raster_geometry (not available here), whose sub-voxel
              conventions cannot be checked.  Restated as the union of a cube of side ``size`` about the centre,
              2|dz|, 2|dy|, 2|dx| <= size, and two z-axis cylinders of height ``size`` (2|dz| <= size) and radius
              ``c_diam = U(0.25, 1) size / 4`` centred at (cz, cy - size/2, cx -/+ size/2):
              (2y - 2cy + size)^2 + (2x - 2cx +/- size)^2 <= (2 c_diam)^2, the right side rounded to float32;
  * image = bone and not inside, flap = bone and inside, full skull = bone (taken before the hole and the noise).

SaltAndPepper (13-47), on the image only (``apply_to=(True, False)``):
  * per sample nd' = U(0, noise_density) -- and, as the reference does (line 31), nd' is stored back as the density, so
    the module singleton's density decays geometrically over a process: nd_i = U_i nd_{i-1}.  ``decay=True`` (default)
    mirrors this with the density kept on the device (replays decay too); ``decay=False`` leaves it alone;
  * with probability p per sample: zero the voxel where u1 <= nd' (1 - salt_ratio), then set it to 1 where
    u2 <= nd' salt_ratio (both thresholds float32 products);  output values are then 0 / 1;
  * a batch of N is N consecutive single-sample calls (one nd' per sample, in order; the reference draws one per call).

RNG: Philox4x32-10, key = the instance's 64-bit seed (lo, hi), counter = (c0, stream, seq lo, seq hi) with seq the
instance's device sample counter (+ n for sample n of a batch).  Uniform floats u = (r >> 8) 2^-24, integers
lo + (r (hi - lo)) >> 32.  Stream 0 holds the per-sample scalars:
  hole:  c0 = 0 -> (u_apply, k over count, size, shape index),  c0 = 1 -> (u for c_diam, -, -, -)
  noise: c0 = 0 -> (u_apply, U for nd', -, -)
Streams 1 and 2 are the noise fields u1 and u2: c0 = (z H + y) ceil(W/4) + x // 4, voxel x uses word x % 4.
Arithmetic: c_diam = ((0.25 + 0.75 u) size) 0.25 and nd' = U nd, every float32 operation rounded separately.

Results are float32: the network input [N, C, D, H, W] (channel 1 = atlas when given) and one-hot targets
[N, 2, D, H, W] (full skull, flap; or the flap alone) -- the reference's sample schema after its dataset's one_hot
(ctunet/pytorch/datasets.py:195-235).

RandomSpatial (csrc/spatial.hip; tests/spatial_ref.py restates it): the random flip, slight elastic deformation and random
zoom / shift / rotation that the docstring of the reference's ``cranioplasty_transform`` (173-228) lists before the flap
extraction, as ONE nearest-neighbour gather with fill 0.  The parameters carry torchio's names; the rule is this package's
own (torchio's random streams and resampling cannot be reproduced here, and no parity with it is claimed).  Axes are
(z, y, x); all C channels of a sample share one warp.  For output voxel o of a sample, in float64, every operation rounded
on its own (no contraction), with n the grid (D, H, W) and sp the spacing in mm:
  1. world:   w_a = o_a sp_a
  2. affine:  s_a = ((M_a0 w_0 + M_a1 w_1) + M_a2 w_2) + M_a3       (resample.affine_resample's form, origins 0)
              M = [L | c - L c + t],  L = Rz(az) Ry(ay) Rx(ax) diag(scale),  c_a = ((n_a - 1) 0.5) sp_a, where, on vectors
              (z, y, x) and with the angle in radians = degrees * 0.017453292519943295,
                Rz = [[1,0,0],[0,cos,-sin],[0,sin,cos]]  Ry = [[cos,0,sin],[0,1,0],[-sin,0,cos]]  Rx = [[cos,-sin,0],[sin,cos,0],[0,0,1]]
              every 3x3 product entry is ((a_0 b_0 + a_1 b_1) + a_2 b_2), L = ((Rz Ry) Rx) with column j times scale_j, and
              M_a3 = (c_a - ((L_a0 c_0 + L_a1 c_1) + L_a2 c_2)) + t_a.  Not applied: M is the exact identity.
  3. elastic: q = s + e(s) (not applied: q = s).  Per axis, G control points, m = G - 3:
                g = (s / (n sp)) m, then g = g if g >= 0 else 0 (NaN -> 0), then g = g if g <= m else m
                i = min(floor(g), m - 1),  f = g - i,  f2 = f f,  f3 = f2 f,  h = 1 - f
                B0 = ((h h) h) / 6   B1 = ((3 f3 - 6 f2) + 4) / 6   B2 = ((((-3 f3) + 3 f2) + 3 f) + 1) / 6   B3 = f3 / 6
              e_c = sum over l, then m, then n (x innermost) from 0, one accumulator per component c, of
                    ((Bz_l By_m) Bx_n) phi_c[iz + l, iy + m, ix + n]
  4. flip:    for each flipped axis  q_a = ((n_a - 1) sp_a) - q_a
  5. sample:  u_a = q_a / sp_a,  k_a = floor(u_a + 0.5);  out = x[k] where every 0 <= k_a < n_a, else 0 (a non-finite u
              fails the comparison, and every read sits behind it).
This is the pull form of "flip, then elastic, then affine" applied to the image.
Draws: Philox as above, key = the instance's seed, seq = its device sample counter + n.  All draws are consumed whether or
not a step is applied; step X is applied iff u_X < p_X (float64 comparison of the exact u).  Stream 0, (c0 -> words):
  0 -> (u_flip z, u_flip y, u_flip x, u_affine)      axis a flips iff a is in flip_axes and u_flip a < flip_p
  1 -> (u_elastic, scale z, scale y, scale x)        scale = lo + u (hi - lo)
  2 -> (angle z, angle y, angle x, -)                angle = (2 u - 1) degrees_a     (degrees, about axis a)
  3 -> (t z, t y, t x, -)                            t = (2 u - 1) translation_a     (mm)
Stream 1: c0 = the control point's flat index (iz Gy + iy) Gx + ix, words 0..2 = its z, y, x displacement
phi_c = (2 u - 1) max_displacement_c; the ``locked_borders`` outer layers on every side are 0.
The draw kernel records, per sample, float64 [26]: 0-2 flip flags, 3 affine applied, 4 elastic applied, 5-7 scales, 8-10
angles, 11-13 translations, 14-25 M row-major -- and the control grid [N, 3, Gz, Gy, Gx]; M uses the device's sin / cos, so
the restatement takes the recorded M for the voxel rule and tests bound M against NumPy's separately.

SkullRandomDefect (csrc/defect.hip; tests/defect_ref.py restates it): the "complex craniectomy defects" that the same
docstring lists, as a union of at most MAX_BALLS = 12 balls with a rough surface, in millimetres.  The rule is this
package's own.  All arithmetic is float64, every operation rounded on its own (no contraction); sp is the spacing, n the
grid (D, H, W), axes are (z, y, x).
Host, per call shape: (lo, hi) = size_range(n), s = min(sp); ``radius=None`` -> ((0.75 lo) s, (0.75 hi) s) mm;
``roughness=None`` (the amplitude amp, mm) -> 0.15 radius[0]; ``roughness_scale=None`` (the lattice pitch scale, mm) ->
1.5 radius[0]; lattice points per axis G_a = floor((n_a sp_a) / scale) + 2.  ValueError for G_a > 64, balls outside
1 <= lo <= hi <= 12, spread < 0, shrink outside 0 < lo <= hi <= 1, amp < 0, radius outside 0 < lo <= hi, scale <= 0.
Draws: Philox as above, key = the instance's seed, seq = its device sample counter + n, u = (r >> 8) 2^-24 as a double,
integers by draw_int.  All draws are consumed whether or not the defect is cut.  Stream 0, (c0 -> words):
  0        -> (u_apply, k over the bone count, u_r0, K = balls_lo + draw over (balls_hi - balls_lo + 1))
  16 + 2 j -> (parent i uniform in [0, j), u_shrink, -, -)          j = 1 .. K - 1
  17 + 2 j -> (u_z, u_y, u_x, -)
The centre voxel is the k-th bone voxel in C order (SkullRandomHole's rule and search).  Ball 0: c_0,a = float64(centre_a)
sp_a, r_0 = radius_lo + u_r0 (radius_hi - radius_lo).  Ball j: r_j = (shrink_lo + u_shrink (shrink_hi - shrink_lo)) r_i,
c_j,a = c_i,a + (((2 u_a) - 1) spread) r_i.  No transcendental is involved.
Stream 1 is the roughness lattice: c0 = the lattice point's flat index (iz Gy + iy) Gx + ix, word 0 -> nu = 2 u - 1, stored
as float64 [N, Gz, Gy, Gx].
Box (inclusive, per axis; the apply kernel may skip the shape test outside it):
  lo_a = max(0, min_j floor((c_j,a - (r_j + amp)) / sp_a) - 1),  hi_a = min(n_a - 1, max_j ceil((c_j,a + (r_j + amp)) / sp_a) + 1)
Voxel o: w_a = float64(o_a) sp_a;  g_a = w_a / scale, i_a = floor(g_a) (<= G_a - 2 by the choice of G), f_a = g_a - i_a;
nu(o) = the trilinear interpolation of the lattice, x first, then y, then z, each lerp a + f (b - a);  rho_j = r_j + amp nu;
the voxel is inside iff some j < K has rho_j > 0 and ((d_z d_z + d_y d_y) + d_x d_x) <= rho_j rho_j with d_a = w_a - c_j,a.
Outputs as for the hole: image = bone and not inside, flap = bone and inside, full = bone; not drawn (u_apply >= p) or no
bone: image unchanged (its uint8 cast), flap zero.  Without bone the record holds no chain: centre -1, balls zero, box
lo 0 and hi -1.
The draw kernel records, per sample, float64 [64]: 0 drawn, 1 bone count, 2 k, 3-5 centre, 6 K, 7 cut, 8-10 box lo, 11-13
box hi, 14-15 zero, 16 + 4 j .. 19 + 4 j ball j = (c_z, c_y, c_x, r).

RandomDilate (csrc/defect.hip): the "dilations prior to the craniectomy generation" of that docstring (the reference draws
only dilation, 119-120).  Sample n is dilated iff u < p, u = word 0 of stream 0, c0 = 0 of its own seed and counter + n; a
dilated sample equals ``scipy.ndimage.binary_dilation(bone, generate_binary_structure(3, 1), iterations, border_value=0)``
(``iterations`` steps of the 6-neighbour cross = the L1 ball of that radius, one gather pass), any other sample is ``bone``.
"""
from __future__ import annotations

import math
import os
from numbers import Real
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _args, _lib, ops

SHAPES = ("sphere", "box", "flap")
_RECORD_FIELDS = ("apply", "count", "k", "cz", "cy", "cx", "size", "shape", "c_diam", "cut", "noise_applied", "nd")


def randint_bounds(low, high) -> Tuple[int, int]:
    """The integer range ``np.random.randint(low, high)`` draws from, or its ValueError."""
    lo, hi = int(low), int(high)
    if lo >= hi:
        raise ValueError("low >= high")
    return lo, hi


def size_range(image_size: Sequence[int]) -> Tuple[int, int]:
    """[lo, hi) of the hole size for a volume of ``image_size`` (random_blank_patch, transforms.py:262-264)."""
    min_r = min(image_size) // 5 - 1
    max_r = max(min_r, max(image_size) // 3.5)
    return randint_bounds(min_r, max_r)


def _check_p(p, name):
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"{name} must be a probability in [0, 1], got {p!r}")
    return float(p)


def _seed(seed) -> int:
    if seed is None:                 # fresh entropy: never consumes torch's or NumPy's global generators
        return int.from_bytes(os.urandom(8), "little")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    return seed


class _DeviceRng:
    """An instance's device state: the sample counter (int64 [1]) and, for the noise, the density (float32 [1])."""

    def __init__(self, seed, density: Optional[float] = None):
        self.seed = _seed(seed)
        self._counter0, self._density0 = 0, density
        self.counter: Optional[torch.Tensor] = None
        self.density: Optional[torch.Tensor] = None

    def to(self, device) -> None:
        device = torch.device(device)
        if self.counter is not None and self.counter.device == device:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ctunet_amd: call the transform once, or .to(device), before capturing it in a graph")
        c, d = self.state()
        self.counter = torch.tensor([c], dtype=torch.int64, device=device)
        if d is not None:
            self.density = torch.tensor([d], dtype=torch.float32, device=device)

    def state(self):
        if self.counter is None:
            return self._counter0, self._density0
        return int(self.counter.item()), (None if self.density is None else float(self.density.item()))

    def load(self, counter: int, density: Optional[float]) -> None:
        self._counter0, self._density0 = int(counter), density
        if self.counter is not None:
            self.counter.fill_(int(counter))
            if density is not None:
                self.density.fill_(float(density))


def _decode(params: torch.Tensor) -> List[Dict]:
    rec = params.view(-1, ops.FLAP_RECORD).cpu()
    flt = rec.view(torch.float32)
    out = []
    for r, f in zip(rec.tolist(), flt.tolist()):
        d = dict(zip(_RECORD_FIELDS[:8], r[:8]))
        d["apply"], d["cut"], d["noise_applied"] = bool(r[0]), bool(r[9]), bool(r[10])
        d["centre"] = (r[3], r[4], r[5])
        d["shape"] = SHAPES[r[7]]
        d["c_diam"], d["nd"], d["thresholds"] = f[8], f[11], (f[12], f[13])
        d["noise_seq"] = (r[14] & 0xFFFFFFFF) | ((r[15] & 0xFFFFFFFF) << 32)
        out.append(d)
    return out


class _Recorded:
    _params: Optional[torch.Tensor] = None

    @property
    def last_params(self) -> List[Dict]:
        """Per-sample records of the last call (syncs): apply, count, k, centre, size, shape, c_diam, cut (the hole was
        cut: drawn and bone present), noise_applied, nd (the density nd' of that sample), thresholds (zero, salt) and
        noise_seq (the noise sample's sequence number)."""
        if self._params is None:
            raise RuntimeError("ctunet_amd: the transform has not been called yet")
        return _decode(self._params)


def _batch(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"Expected 'torch.Tensor'. Got {type(t)}.")
    if t.dim() != 5 or t.shape[1] != 1:
        raise ValueError(f"ctunet_amd: {name} must be a [N,1,D,H,W] batch, got {tuple(t.shape)}")
    if not t.is_cuda:
        raise RuntimeError(f"ctunet_amd: {name} must live on the GPU (MI355X); this path has no CPU fallback")
    if t.dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"ctunet_amd: {name} must be float32 or uint8, got {t.dtype}")
    return t.contiguous()


def _out(t: Optional[torch.Tensor], shape, device, name) -> torch.Tensor:
    if t is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != device:
        raise ValueError(f"ctunet_amd: {name} must be a contiguous float32 {tuple(shape)} tensor on {device}")
    return t


def _run(hole, noise: Optional["SaltAndPepper"], skulls: torch.Tensor,
         atlas: Optional[torch.Tensor], x: Optional[torch.Tensor], targets: Optional[Sequence[torch.Tensor]]):
    """The fused pass of ``hole`` (a SkullRandomHole, a SkullRandomDefect or None) and ``noise`` (or None) on a batch."""
    skulls = _batch(skulls, "skulls")
    dev = skulls.device
    n, _, d, h, w = skulls.shape
    mode = (ops.FLAP_HOLE if hole else 0) | (ops.FLAP_NOISE if noise else 0)
    for t in (hole, noise):
        if t is not None:
            t._rng.to(dev)
    if atlas is not None:
        if not atlas.is_cuda or atlas.dtype != torch.float32 or atlas.numel() != d * h * w or atlas.device != dev:
            raise ValueError(f"ctunet_amd: the atlas must be a float32 [{d},{h},{w}] tensor on {dev}")
        atlas = atlas.contiguous()
    x = _out(x, (n, 2 if atlas is not None else 1, d, h, w), dev, "x")
    full = flap = None
    if hole is not None:
        nt = 2 if hole.double_output else 1
        if targets is not None and len(targets) != nt:
            raise ValueError(f"ctunet_amd: {nt} target tensor(s) expected, got {len(targets)}")
        tg = [_out(None if targets is None else targets[i], (n, 2, d, h, w), dev, "target") for i in range(nt)]
        full, flap = (tg[0], tg[1]) if nt == 2 else (None, tg[0])
    counts = None
    params = torch.empty((n, ops.FLAP_RECORD), dtype=torch.int32, device=dev)
    if hole is not None:
        counts = torch.empty((n, -(-d * h * w // ops.FLAP_CHUNK)), dtype=torch.int32, device=dev)
        ops.flap_count(skulls, counts)
    hs = hole._rng if hole is not None else None
    ns = noise._rng if noise is not None else None
    if isinstance(hole, SkullRandomDefect):
        geo = hole.geometry((d, h, w))
        record, lattice = hole._buffers(n, geo["lattice"], dev)
        ops.defect_draw(skulls, counts, hole.spacing, hs.counter, hs.seed, hole.p,
                        geo["radius"] + (hole.spread,) + hole.shrink + (geo["roughness"],), hole.balls, geo["lattice"],
                        record, lattice)
        if noise is not None:                       # the noise scalars: the hole's draw kernel in noise-only mode
            ops.flap_draw(skulls, None, ops.FLAP_NOISE, None, 0, 0.0, (0, 1), 0, ns.counter, ns.density, ns.seed, noise.p,
                          noise.salt_ratio, noise.decay, params)
            noise._params = params
        ops.defect_apply(skulls, atlas, hole.spacing, record, lattice, geo["lattice"], geo["roughness_scale"],
                         geo["roughness"], params if noise is not None else None, mode, hs.counter, ns and ns.counter,
                         ns and ns.density, ns.seed if ns else 0, bool(noise and noise.decay), x, full, flap)
        hole._params = params if noise is not None else None
        return x, [full, flap] if full is not None else [flap]
    ops.flap_draw(skulls, counts, mode, hs and hs.counter, hs.seed if hs else 0, hole.p if hole else 0.0,
                  size_range((d, h, w)) if hole else (0, 1), hole._shape_code if hole else 0,
                  ns and ns.counter, ns and ns.density, ns.seed if ns else 0, noise.p if noise else 0.0,
                  noise.salt_ratio if noise else 0.0, bool(noise and noise.decay), params)
    ops.flap_apply(skulls, atlas, params, mode, hs and hs.counter, ns and ns.counter, ns and ns.density,
                   ns.seed if ns else 0, bool(noise and noise.decay), x, full, flap)
    for t in (hole, noise):
        if t is not None:
            t._params = params
    return x, ([full, flap] if full is not None else [flap]) if hole is not None else []


class SkullRandomHole(_Recorded):
    """Cut a random sphere / box / flap out of binary skulls (transforms.py:50-95).  ``sample`` dicts behave as the
    reference's (uint8 image, uint8 target(s)); ``apply`` is the device batch form with float32 one-hot targets."""

    def __init__(self, p=1, double_output=False, shapes: Optional[Sequence[str]] = None, seed: Optional[int] = None):
        self.p = _check_p(p, "p")
        self.double_output = bool(double_output)
        shapes = SHAPES if shapes is None else tuple(shapes)
        if not shapes or len(shapes) > 3 or any(s not in SHAPES for s in shapes):
            raise ValueError(f"shapes must be a non-empty list of at most 3 of {SHAPES}, got {shapes!r}")
        self.shapes = shapes
        self._shape_code = len(shapes) | sum(SHAPES.index(s) << (2 + 2 * i) for i, s in enumerate(shapes))
        self._rng = _DeviceRng(seed)

    @property
    def seed(self) -> int:
        return self._rng.seed

    def to(self, device) -> "SkullRandomHole":
        self._rng.to(device)
        return self

    def state_dict(self) -> Dict:
        c, _ = self._rng.state()
        return {"seed": self._rng.seed, "counter": c}

    def load_state_dict(self, sd: Dict) -> None:
        self._rng.seed = _seed(sd["seed"])
        self._rng.load(sd["counter"], None)

    def apply(self, skulls: torch.Tensor, x: Optional[torch.Tensor] = None,
              targets: Optional[Sequence[torch.Tensor]] = None):
        """skulls [N,1,D,H,W] float32 / uint8 on the GPU -> (x [N,1,D,H,W], [full, flap] or [flap] one-hot
        [N,2,D,H,W]), float32; x / targets: caller-supplied outputs."""
        return _run(self, None, skulls, None, x, targets)

    def __call__(self, sample: Dict) -> Dict:
        img = sample["image"]
        if not isinstance(img, torch.Tensor):
            raise TypeError(f"Expected 'torch.Tensor'. Got {type(img)}.")
        is_batch = img.dim() == 4
        b = (img if is_batch else img.unsqueeze(0)).unsqueeze(1)
        b = b.to("cuda") if not b.is_cuda else b
        x, tg = self.apply(b if b.dtype in (torch.float32, torch.uint8) else b.float())
        lab = [t[:, 1].to(torch.uint8) for t in tg]
        image = x[:, 0].to(torch.uint8)
        if not is_batch:
            image, lab = image[0], [t[0] for t in lab]
        return {"image": image, "target": tuple(lab) if self.double_output else lab[0]}


class SaltAndPepper(_Recorded):
    """Random zeroed ("pepper") and set ("salt") voxels (transforms.py:13-47), with the reference's density decay."""

    def __init__(self, p=1, noise_density=0.2, salt_ratio=0.1, keyws=("image", "target"), apply_to=(True, False),
                 decay: bool = True, seed: Optional[int] = None):
        self.p = _check_p(p, "p")
        _check_p(noise_density, "noise_density")
        self.salt_ratio = _check_p(salt_ratio, "salt_ratio")
        if len(keyws) != len(apply_to):
            raise ValueError("keyws and apply_to must have the same length")
        self.keyws, self.apply_to = tuple(keyws), tuple(bool(a) for a in apply_to)
        self.decay = bool(decay)
        self._rng = _DeviceRng(seed, float(torch.tensor(float(noise_density), dtype=torch.float32)))

    @property
    def seed(self) -> int:
        return self._rng.seed

    @property
    def noise_density(self) -> float:
        """The current density (syncs when it lives on the device)."""
        return self._rng.state()[1]

    @noise_density.setter
    def noise_density(self, v: float) -> None:
        _check_p(v, "noise_density")
        self._rng.load(self._rng.state()[0], float(v))

    def to(self, device) -> "SaltAndPepper":
        self._rng.to(device)
        return self

    def state_dict(self) -> Dict:
        c, d = self._rng.state()
        return {"seed": self._rng.seed, "counter": c, "noise_density": d}

    def load_state_dict(self, sd: Dict) -> None:
        self._rng.seed = _seed(sd["seed"])
        self._rng.load(sd["counter"], float(sd["noise_density"]))

    def apply(self, images: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """images [N,1,D,H,W] float32 / uint8 on the GPU -> float32 [N,1,D,H,W] (out: caller-supplied; may be images)."""
        return _run(None, self, images, None, out, None)[0]

    def __call__(self, sample: Dict) -> Dict:
        for keyw, on in zip(self.keyws, self.apply_to):
            if not on:
                continue
            img = sample[keyw]
            is_batch = img.dim() == 4
            b = (img if is_batch else img.unsqueeze(0)).unsqueeze(1)
            b = b.to("cuda") if not b.is_cuda else b
            out = self.apply(b if b.dtype in (torch.float32, torch.uint8) else b.float())[:, 0]
            sample[keyw] = out if is_batch else out[0]
        return sample


_REAL = _args.Triple(shape="RandomSpatial: {what} must be a number or a (z, y, x) triple, got {v!r}",
                     value="RandomSpatial: {what} must be finite, got {v!r}", shape_error=TypeError)
_REAL_POSITIVE = _REAL._replace(value="RandomSpatial: {what} must be positive and finite, got {v!r}", sign=_args.POSITIVE)


def _triple_nonneg(v, what: str) -> Tuple[float, float, float]:
    t = _args.triple(v, _REAL, what=what)
    if t is None or any(s < 0 for s in t):
        raise ValueError(f"RandomSpatial: {what} must be a non-negative number or (z, y, x) triple, got {v!r}")
    return t


class RandomSpatial:
    """Random flip, elastic deformation and affine map of a batch in one gather pass on the device (module docstring, the
    "RandomSpatial" rule).  ``apply`` is the device batch form; ``sample`` dicts get "image" (and "target" where present)
    warped by the same draw.  Two launches per call, no host sync: it can be captured in a graph after one warm call."""

    def __init__(self, flip_axes=(0,), flip_p=0.5, scales=(0.9, 1.1), degrees=15, translation=(10, 10, 15), affine_p=0.5,
                 num_control_points=7, max_displacement=7.5, locked_borders=2, elastic_p=0.5, spacing=(1, 1, 1),
                 seed: Optional[int] = None):
        axes = (flip_axes,) if isinstance(flip_axes, int) and not isinstance(flip_axes, bool) else tuple(flip_axes)
        if any(isinstance(a, bool) or not isinstance(a, int) or not 0 <= a <= 2 for a in axes) or len(set(axes)) != len(axes):
            raise ValueError(f"RandomSpatial: flip_axes must be distinct axes out of (0, 1, 2) = (z, y, x), got {flip_axes!r}")
        self.flip_axes = axes
        self.flip_p, self.affine_p = _check_p(flip_p, "flip_p"), _check_p(affine_p, "affine_p")
        self.elastic_p = _check_p(elastic_p, "elastic_p")
        try:
            lo, hi = scales
        except (TypeError, ValueError):
            raise TypeError(f"RandomSpatial: scales must be a (low, high) pair, got {scales!r}") from None
        if any(isinstance(v, bool) or not isinstance(v, Real) for v in (lo, hi)):
            raise TypeError(f"RandomSpatial: scales must be a (low, high) pair of numbers, got {scales!r}")
        if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo <= hi):
            raise ValueError(f"RandomSpatial: scales must satisfy 0 < low <= high < inf, got {scales!r}")
        self.scales = (float(lo), float(hi))
        self.degrees = _triple_nonneg(degrees, "degrees")
        self.translation = _triple_nonneg(translation, "translation")
        self.max_displacement = _triple_nonneg(max_displacement, "max_displacement")
        g = num_control_points
        g = (g, g, g) if isinstance(g, int) and not isinstance(g, bool) else g
        try:
            g = tuple(g)
        except TypeError:
            raise TypeError(f"RandomSpatial: num_control_points must be an int or a (z, y, x) triple, got {g!r}") from None
        if len(g) != 3 or any(isinstance(v, bool) or not isinstance(v, int) for v in g):
            raise TypeError(f"RandomSpatial: num_control_points must be an int or a (z, y, x) triple of ints, got {g!r}")
        if any(not ops.SPATIAL_MIN_POINTS <= v <= ops.SPATIAL_MAX_POINTS for v in g):
            raise ValueError(f"RandomSpatial: num_control_points must lie in {ops.SPATIAL_MIN_POINTS}.."
                             f"{ops.SPATIAL_MAX_POINTS} per axis, got {g!r}")
        self.num_control_points = g
        if isinstance(locked_borders, bool) or locked_borders not in (0, 1, 2):
            raise ValueError(f"RandomSpatial: locked_borders must be 0, 1 or 2, got {locked_borders!r}")
        if any(2 * locked_borders >= v for v in g):
            raise ValueError(f"RandomSpatial: locked_borders={locked_borders} leaves no free control point of {g}")
        self.locked_borders = int(locked_borders)
        self.spacing = _args.triple(spacing, _REAL_POSITIVE, what="spacing")
        if self.spacing is None:
            raise TypeError("RandomSpatial: spacing must be a number or a (z, y, x) triple")
        self._rng = _DeviceRng(seed)
        self._record: Optional[torch.Tensor] = None
        self._control: Optional[torch.Tensor] = None

    @property
    def seed(self) -> int:
        return self._rng.seed

    def to(self, device) -> "RandomSpatial":
        self._rng.to(device)
        return self

    def state_dict(self) -> Dict:
        c, _ = self._rng.state()
        return {"seed": self._rng.seed, "counter": c}

    def load_state_dict(self, sd: Dict) -> None:
        self._rng.seed = _seed(sd["seed"])
        self._rng.load(sd["counter"], None)

    def _buffers(self, n: int, device: torch.device):
        """The record and the control grid of a batch of n: kept between calls, so a steady call allocates nothing."""
        if self._record is None or self._record.shape[0] != n or self._record.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ctunet_amd: call the transform once with this batch size before capturing it in a graph")
            self._record = torch.empty((n, ops.SPATIAL_RECORD), dtype=torch.float64, device=device)
            self._control = torch.empty((n, 3) + self.num_control_points, dtype=torch.float64, device=device)
        return self._record, self._control

    def apply(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [N,C,D,H,W] uint8 / float32 on the GPU -> the warped batch, same dtype and shape (out: caller-supplied, not x)."""
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"RandomSpatial: expected a torch.Tensor, got {type(x).__name__}")
        if x.dim() != 5 or x.numel() == 0:
            raise ValueError(f"RandomSpatial: x must be a non-empty [N,C,D,H,W] batch, got {tuple(x.shape)}")
        if x.dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"RandomSpatial: x must be uint8 or float32, got {x.dtype}")
        if out is not None:
            if not isinstance(out, torch.Tensor):
                raise TypeError(f"RandomSpatial: out must be a tensor, got {type(out).__name__}")
            if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
                raise ValueError(f"RandomSpatial: out must be a contiguous {x.dtype} tensor of shape {tuple(x.shape)} on "
                                 f"{x.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        _lib.check_device("RandomSpatial: x must live on the GPU (MI355X); this path has no CPU fallback", x)
        x = x.contiguous()
        nbytes = x.numel() * x.element_size()
        if out is not None and out.data_ptr() < x.data_ptr() + nbytes and x.data_ptr() < out.data_ptr() + nbytes:
            raise ValueError("RandomSpatial: out overlaps x; the gather cannot run in place")
        n, _, d, h, w = x.shape
        self._rng.to(x.device)
        record, control = self._buffers(n, x.device)
        if out is None:
            out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            ops.spatial_draw(n, (d, h, w), self.spacing, self._rng.counter, self._rng.seed,
                             sum(1 << a for a in self.flip_axes), self.flip_p, self.affine_p, self.elastic_p,
                             self.scales + self.degrees + self.translation + self.max_displacement,
                             self.num_control_points, self.locked_borders, record, control)
            ops.spatial_warp(x, out, self.spacing, self.num_control_points, record, control, self._rng.counter)
        return out

    @property
    def last_params(self) -> List[Dict]:
        """Per-sample records of the last call (one read-back): flip (z, y, x), affine, elastic (the steps applied), scales,
        degrees, translation (the drawn values, used or not) and matrix (M, float64 [3, 4])."""
        if self._record is None:
            raise RuntimeError("ctunet_amd: the transform has not been called yet")
        out = []
        for r in self._record.cpu():
            out.append({"flip": tuple(bool(v) for v in r[0:3]), "affine": bool(r[3]), "elastic": bool(r[4]),
                        "scales": tuple(r[5:8].tolist()), "degrees": tuple(r[8:11].tolist()),
                        "translation": tuple(r[11:14].tolist()), "matrix": r[14:26].reshape(3, 4).clone()})
        return out

    @property
    def last_control(self) -> torch.Tensor:
        """The control displacements (mm) of the last call, float64 [N, 3, Gz, Gy, Gx] on the host (one read-back)."""
        if self._control is None:
            raise RuntimeError("ctunet_amd: the transform has not been called yet")
        return self._control.cpu()

    def __call__(self, sample: Dict) -> Dict:
        img = sample["image"]
        if not isinstance(img, torch.Tensor):
            raise TypeError(f"Expected 'torch.Tensor'. Got {type(img)}.")
        is_batch = img.dim() == 4
        tg = sample.get("target")
        tgs = [] if tg is None else (list(tg) if isinstance(tg, (tuple, list)) else [tg])
        vols = [img] + tgs                                   # one channel each: the same draw warps them all
        kind = torch.uint8 if all(v.dtype in (torch.uint8, torch.bool) for v in vols) else torch.float32
        b = torch.stack([(v if is_batch else v.unsqueeze(0)).to("cuda").to(kind) for v in vols], 1)
        out = self.apply(b)
        res = [out[:, i].to(v.dtype) if is_batch else out[0, i].to(v.dtype) for i, v in enumerate(vols)]
        sample["image"] = res[0]
        if tg is not None:
            sample["target"] = tuple(res[1:]) if isinstance(tg, (tuple, list)) else res[1]
        return sample


MAX_BALLS = ops.DEFECT_MAX_BALLS


def _pair(v, what: str) -> Tuple[float, float]:
    try:
        lo, hi = v
    except (TypeError, ValueError):
        raise TypeError(f"SkullRandomDefect: {what} must be a (low, high) pair, got {v!r}") from None
    if any(isinstance(t, bool) or not isinstance(t, Real) or not math.isfinite(t) for t in (lo, hi)):
        raise TypeError(f"SkullRandomDefect: {what} must be a (low, high) pair of finite numbers, got {v!r}")
    return float(lo), float(hi)


def _scalar(v, what: str) -> float:
    if isinstance(v, bool) or not isinstance(v, Real) or not math.isfinite(v):
        raise TypeError(f"SkullRandomDefect: {what} must be a finite number, got {v!r}")
    return float(v)


class SkullRandomDefect:
    """Cut an irregular craniectomy defect -- a union of ``balls`` rough balls around a random bone voxel, sized in
    millimetres -- out of binary skulls (module docstring, the "SkullRandomDefect" rule).  A sibling of SkullRandomHole with
    the same calling forms: ``apply`` on device batches, ``sample`` dicts as the reference's.  Three launches per call (four
    with noise fused in by FlapRecTransform), no host sync: it can be captured in a graph after one warm call."""

    def __init__(self, p=1, double_output=False, spacing=(1, 1, 1), radius=None, balls=(3, 8), spread=0.9,
                 shrink=(0.5, 0.9), roughness=None, roughness_scale=None, seed: Optional[int] = None):
        self.p = _check_p(p, "p")
        self.double_output = bool(double_output)
        self.spacing = _args.triple(spacing, _REAL_POSITIVE._replace(
            shape="SkullRandomDefect: {what} must be a number or a (z, y, x) triple, got {v!r}",
            value="SkullRandomDefect: {what} must be positive and finite, got {v!r}"), what="spacing")
        if self.spacing is None:
            raise TypeError("SkullRandomDefect: spacing must be a number or a (z, y, x) triple")
        self.radius = None if radius is None else _pair(radius, "radius")
        if self.radius is not None and not 0 < self.radius[0] <= self.radius[1]:
            raise ValueError(f"SkullRandomDefect: radius must satisfy 0 < low <= high (mm), got {radius!r}")
        try:
            blo, bhi = balls
        except (TypeError, ValueError):
            raise TypeError(f"SkullRandomDefect: balls must be a (low, high) pair of ints, got {balls!r}") from None
        if any(isinstance(b, bool) or not isinstance(b, int) for b in (blo, bhi)):
            raise TypeError(f"SkullRandomDefect: balls must be a (low, high) pair of ints, got {balls!r}")
        if not 1 <= blo <= bhi <= MAX_BALLS:
            raise ValueError(f"SkullRandomDefect: balls must satisfy 1 <= low <= high <= {MAX_BALLS}, got {balls!r}")
        self.balls = (blo, bhi)
        self.spread = _scalar(spread, "spread")
        if self.spread < 0:
            raise ValueError(f"SkullRandomDefect: spread must not be negative, got {spread!r}")
        self.shrink = _pair(shrink, "shrink")
        if not 0 < self.shrink[0] <= self.shrink[1] <= 1:
            raise ValueError(f"SkullRandomDefect: shrink must satisfy 0 < low <= high <= 1, got {shrink!r}")
        self.roughness = None if roughness is None else _scalar(roughness, "roughness")
        if self.roughness is not None and self.roughness < 0:
            raise ValueError(f"SkullRandomDefect: roughness must not be negative, got {roughness!r}")
        self.roughness_scale = None if roughness_scale is None else _scalar(roughness_scale, "roughness_scale")
        if self.roughness_scale is not None and self.roughness_scale <= 0:
            raise ValueError(f"SkullRandomDefect: roughness_scale must be positive, got {roughness_scale!r}")
        self._rng = _DeviceRng(seed)
        self._params: Optional[torch.Tensor] = None            # the fused noise's records of the last call
        self._record: Optional[torch.Tensor] = None
        self._lattice: Optional[torch.Tensor] = None

    @property
    def seed(self) -> int:
        return self._rng.seed

    def to(self, device) -> "SkullRandomDefect":
        self._rng.to(device)
        return self

    def state_dict(self) -> Dict:
        c, _ = self._rng.state()
        return {"seed": self._rng.seed, "counter": c}

    def load_state_dict(self, sd: Dict) -> None:
        self._rng.seed = _seed(sd["seed"])
        self._rng.load(sd["counter"], None)

    def geometry(self, shape: Sequence[int]) -> Dict:
        """What a volume of ``shape`` = (D, H, W) resolves the defaults to, on the host: radius (lo, hi), roughness and
        roughness_scale in mm and the lattice size (Gz, Gy, Gx); ValueError where the rule refuses them."""
        lo, hi = size_range(shape)
        s = min(self.spacing)
        radius = self.radius if self.radius is not None else ((0.75 * lo) * s, (0.75 * hi) * s)
        if not 0 < radius[0] <= radius[1]:
            raise ValueError(f"SkullRandomDefect: a {tuple(shape)} volume gives the radius range {radius}; it must satisfy "
                             "0 < low <= high")
        amp = self.roughness if self.roughness is not None else 0.15 * radius[0]
        scale = self.roughness_scale if self.roughness_scale is not None else 1.5 * radius[0]
        lattice = tuple(math.floor((n * sp) / scale) + 2 for n, sp in zip(shape, self.spacing))
        if any(g > ops.DEFECT_MAX_LATTICE for g in lattice):
            raise ValueError(f"SkullRandomDefect: roughness_scale {scale} mm needs a {lattice} lattice on a {tuple(shape)} "
                             f"volume (at most {ops.DEFECT_MAX_LATTICE} points per axis)")
        return {"radius": radius, "roughness": amp, "roughness_scale": scale, "lattice": lattice}

    def _buffers(self, n: int, lattice: Tuple[int, int, int], device: torch.device):
        """The record and the lattice of a batch of n: kept between calls, so a steady call allocates neither."""
        if self._record is None or self._record.shape[0] != n or self._record.device != device \
                or tuple(self._lattice.shape[1:]) != lattice:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ctunet_amd: call the transform once with this batch shape before capturing it in a graph")
            self._record = torch.empty((n, ops.DEFECT_RECORD), dtype=torch.float64, device=device)
            self._lattice = torch.empty((n,) + lattice, dtype=torch.float64, device=device)
        return self._record, self._lattice

    def apply(self, skulls: torch.Tensor, x: Optional[torch.Tensor] = None,
              targets: Optional[Sequence[torch.Tensor]] = None):
        """skulls [N,1,D,H,W] float32 / uint8 on the GPU -> (x [N,1,D,H,W], [full, flap] or [flap] one-hot
        [N,2,D,H,W]), float32; x / targets: caller-supplied outputs."""
        return _run(self, None, skulls, None, x, targets)

    __call__ = SkullRandomHole.__call__        # the sample-dict form needs only ``apply`` and ``double_output``

    @property
    def last_params(self) -> List[Dict]:
        """Per-sample records of the last call (one read-back): apply, cut (drawn and bone present), count, k, centre,
        n_balls, balls (n_balls tuples (cz, cy, cx, r) in mm; none without bone), box ((lo_z, lo_y, lo_x), (hi_z, hi_y,
        hi_x)), and the fused noise's noise_applied, nd, thresholds and noise_seq (False / 0 without noise)."""
        if self._record is None:
            raise RuntimeError("ctunet_amd: the transform has not been called yet")
        noise = _decode(self._params) if self._params is not None else [None] * self._record.shape[0]
        out = []
        for r, nz in zip(self._record.cpu().tolist(), noise):
            k = int(r[6])
            d = {"noise_applied": False, "nd": 0.0, "thresholds": (0.0, 0.0), "noise_seq": 0} if nz is None else \
                {f: nz[f] for f in ("noise_applied", "nd", "thresholds", "noise_seq")}
            d.update(apply=bool(r[0]), cut=bool(r[7]), count=int(r[1]), k=int(r[2]), centre=tuple(int(v) for v in r[3:6]),
                     n_balls=k, balls=[tuple(r[16 + 4 * j:20 + 4 * j]) for j in range(k if r[1] > 0 else 0)],
                     box=(tuple(int(v) for v in r[8:11]), tuple(int(v) for v in r[11:14])))
            out.append(d)
        return out

    @property
    def last_lattice(self) -> torch.Tensor:
        """The roughness lattice of the last call, float64 [N, Gz, Gy, Gx] on the host (one read-back)."""
        if self._lattice is None:
            raise RuntimeError("ctunet_amd: the transform has not been called yet")
        return self._lattice.cpu()


class RandomDilate:
    """Thicken a random share ``p`` of a batch of binary skulls by ``iterations`` steps of the 6-neighbour cross (module
    docstring, the "RandomDilate" rule): one gather launch, the per-sample choice drawn on the device, so a replayed graph
    draws afresh."""

    def __init__(self, p=0.3, iterations=1, seed: Optional[int] = None):
        self.p = _check_p(p, "p")
        if isinstance(iterations, bool) or not isinstance(iterations, int) or not 1 <= iterations <= ops.DILATE_MAX_ITERATIONS:
            raise ValueError(f"RandomDilate: iterations must be an int in 1..{ops.DILATE_MAX_ITERATIONS}, got {iterations!r}")
        self.iterations = iterations
        self._rng = _DeviceRng(seed)

    @property
    def seed(self) -> int:
        return self._rng.seed

    def to(self, device) -> "RandomDilate":
        self._rng.to(device)
        return self

    def state_dict(self) -> Dict:
        c, _ = self._rng.state()
        return {"seed": self._rng.seed, "counter": c}

    def load_state_dict(self, sd: Dict) -> None:
        self._rng.seed = _seed(sd["seed"])
        self._rng.load(sd["counter"], None)

    def apply(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [N,1,D,H,W] uint8 / float32 on the GPU -> uint8 0 / 1, the same shape (out: caller-supplied, not x)."""
        x = _batch(x, "x")
        if out is None:
            out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != x.shape or out.device != x.device \
                or not out.is_contiguous():
            raise ValueError(f"RandomDilate: out must be a contiguous uint8 tensor of shape {tuple(x.shape)} on {x.device}")
        nbytes = x.numel() * x.element_size()
        if out.data_ptr() < x.data_ptr() + nbytes and x.data_ptr() < out.data_ptr() + out.numel():
            raise ValueError("RandomDilate: out overlaps x; the gather cannot run in place")
        self._rng.to(x.device)
        with torch.cuda.device(x.device):
            ops.random_dilate(x, out, self.iterations, self._rng.counter, self._rng.seed, self.p)
        return out

    def __call__(self, sample: Dict) -> Dict:
        img = sample["image"]
        if not isinstance(img, torch.Tensor):
            raise TypeError(f"Expected 'torch.Tensor'. Got {type(img)}.")
        is_batch = img.dim() == 4
        b = (img if is_batch else img.unsqueeze(0)).unsqueeze(1).to("cuda")
        out = self.apply(b if b.dtype in (torch.float32, torch.uint8) else b.float())[:, 0]
        sample["image"] = out if is_batch else out[0]
        return sample


class FlapRecTransform(_Recorded):
    """``hole`` then ``noise`` in ONE fused pass, bit-equal to applying them in sequence (each keeps its own seed, counter
    and density); ``atlas`` [D,H,W] float32 becomes channel 1 of the network input, as the shape-prior datasets append it.
    ``hole`` is a SkullRandomHole or a SkullRandomDefect; ``spatial`` warps and then ``dilate`` thickens the skulls first."""

    def __init__(self, hole, noise: Optional[SaltAndPepper] = None, atlas: Optional[torch.Tensor] = None,
                 spatial: Optional[RandomSpatial] = None, dilate: Optional[RandomDilate] = None):
        if not isinstance(hole, (SkullRandomHole, SkullRandomDefect)) or not (noise is None or isinstance(noise, SaltAndPepper)) \
                or not (spatial is None or isinstance(spatial, RandomSpatial)) \
                or not (dilate is None or isinstance(dilate, RandomDilate)):
            raise TypeError("FlapRecTransform(hole: SkullRandomHole | SkullRandomDefect, noise: SaltAndPepper | None, "
                            "atlas=None, spatial: RandomSpatial | None, dilate: RandomDilate | None)")
        if noise is not None and (noise.keyws[:1] != ("image",) or noise.apply_to != (True,) + (False,) * (len(noise.apply_to) - 1)):
            raise ValueError("FlapRecTransform: the fused noise applies to the image only (apply_to=(True, False))")
        self.hole, self.noise, self.spatial, self.dilate = hole, noise, spatial, dilate
        self.atlas = None if atlas is None else atlas.float().contiguous()
        self._warped: Optional[torch.Tensor] = None
        self._dilated: Optional[torch.Tensor] = None

    def to(self, device) -> "FlapRecTransform":
        self.hole.to(device)
        if self.noise is not None:
            self.noise.to(device)
        if self.atlas is not None:
            self.atlas = self.atlas.to(device)
        if self.spatial is not None:
            self.spatial.to(device)
        if self.dilate is not None:
            self.dilate.to(device)
        return self

    def state_dict(self) -> Dict:
        sd = {"hole": self.hole.state_dict(), "noise": None if self.noise is None else self.noise.state_dict()}
        if self.spatial is not None:
            sd["spatial"] = self.spatial.state_dict()
        if self.dilate is not None:
            sd["dilate"] = self.dilate.state_dict()
        return sd

    def load_state_dict(self, sd: Dict) -> None:
        self.hole.load_state_dict(sd["hole"])
        if self.noise is not None:
            self.noise.load_state_dict(sd["noise"])
        if self.spatial is not None and sd.get("spatial") is not None:
            self.spatial.load_state_dict(sd["spatial"])
        if self.dilate is not None and sd.get("dilate") is not None:
            self.dilate.load_state_dict(sd["dilate"])

    def _warp(self, skulls: torch.Tensor) -> torch.Tensor:
        """The skulls' uint8 casts warped by ``spatial`` into a uint8 buffer kept between calls."""
        skulls = _batch(skulls, "skulls")
        if skulls.dtype != torch.uint8:
            skulls = skulls.to(torch.uint8)                 # the value of a voxel is its uint8 cast (truncation)
        if self._warped is None or self._warped.shape != skulls.shape or self._warped.device != skulls.device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ctunet_amd: call the transform once with this shape before capturing it in a graph")
            self._warped = torch.empty_like(skulls)
        return self.spatial.apply(skulls, out=self._warped)

    def _thicken(self, skulls: torch.Tensor) -> torch.Tensor:
        """The skulls' bone dilated by ``dilate`` into a uint8 buffer kept between calls."""
        skulls = _batch(skulls, "skulls")
        if self._dilated is None or self._dilated.shape != skulls.shape or self._dilated.device != skulls.device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ctunet_amd: call the transform once with this shape before capturing it in a graph")
            self._dilated = torch.empty(skulls.shape, dtype=torch.uint8, device=skulls.device)
        return self.dilate.apply(skulls, out=self._dilated)

    def apply(self, skulls: torch.Tensor, x: Optional[torch.Tensor] = None,
              targets: Optional[Sequence[torch.Tensor]] = None):
        """skulls [N,1,D,H,W] -> (x [N,C,D,H,W], one-hot targets), float32, written into x / targets when given (e.g.
        ``GraphedTrainStep.x`` / ``.targets``).  With ``spatial`` the skulls are warped first, with ``dilate`` then
        thickened; the full-skull target is the warped, dilated skull and the atlas channel is not warped."""
        if self.spatial is not None:
            skulls = self._warp(skulls)
        if self.dilate is not None:
            skulls = self._thicken(skulls)
        if self.atlas is not None and self.atlas.device != skulls.device:
            self.atlas = self.atlas.to(skulls.device)
        return _run(self.hole, self.noise, skulls, self.atlas, x, targets)

    @property
    def _params(self) -> Optional[torch.Tensor]:
        return self.hole._params            # the records of the last call of its hole (fused or not)

    @property
    def last_params(self) -> List[Dict]:
        """The records of the last call of its hole (fused or not): ``hole.last_params``."""
        return self.hole.last_params

    def __call__(self, sample: Dict) -> Dict:
        """The reference's Compose([hole, noise]) on a sample dict: float32 image, uint8 target(s); no atlas.  With
        ``spatial`` the image is warped first, with ``dilate`` then thickened."""
        if self.spatial is not None:
            sample = dict(sample, image=self.spatial({"image": sample["image"]})["image"])
        if self.dilate is not None:
            sample = dict(sample, image=self.dilate({"image": sample["image"]})["image"])
        sample = self.hole(sample)
        img = sample["image"]
        if self.noise is not None:
            sample = self.noise(sample)
        else:
            sample["image"] = img.float()
        return sample


flap_rec_transform = FlapRecTransform(SkullRandomHole(double_output=True), SaltAndPepper(p=.5, noise_density=.05))

cranioplasty_transform = FlapRecTransform(SkullRandomHole(p=0.9, double_output=True), SaltAndPepper(p=1, noise_density=.05),
                                          spatial=RandomSpatial(flip_axes=(0,)))
"""The pipeline the docstring of the reference's ``cranioplasty_transform`` (ctunet/pytorch/transforms.py:173-228)
describes, with its numbers: flip of axis 0 (p = .5), elastic deformation (7 control points, 7.5 mm, 2 locked layers,
p = .5), affine (scales .9-1.1, 15 degrees, translation (10, 10, 15) mm, p = .5), the flap extraction (p = .9) and salt and
pepper noise (p = 1, density .05).  Differences: no erode / dilate step (``realistic_cranioplasty_transform`` has the
dilation); the warp follows this module's RandomSpatial rule,
not torchio's; voxel spacing is (1, 1, 1) mm unless a RandomSpatial with another ``spacing`` is used; and the reference's
function itself cannot run (it calls ``erode_dilate`` and ``skull_random_hole``, which do not exist, and uses the
``SaltAndPepper`` class as a function), so there is no behaviour to match, only this described pipeline."""

realistic_cranioplasty_transform = FlapRecTransform(SkullRandomDefect(p=0.9, double_output=True),
                                                    SaltAndPepper(p=1, noise_density=.05),
                                                    spatial=RandomSpatial(flip_axes=(0,)), dilate=RandomDilate(p=0.3))
"""``cranioplasty_transform`` with the two augmentations that docstring lists besides: the skull is thickened by one step of
the 6-neighbour cross with p = .3 after the warp, and the hole is an irregular defect (SkullRandomDefect: 3-8 rough balls,
radii from the hole's size range in mm) instead of a sphere, box or idealised flap.  Spacing (1, 1, 1) mm unless the
members are built with another."""
