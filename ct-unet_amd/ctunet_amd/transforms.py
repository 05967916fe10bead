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
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops

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


def _run(hole: Optional["SkullRandomHole"], noise: Optional["SaltAndPepper"], skulls: torch.Tensor,
         atlas: Optional[torch.Tensor], x: Optional[torch.Tensor], targets: Optional[Sequence[torch.Tensor]]):
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


class FlapRecTransform(_Recorded):
    """``hole`` then ``noise`` in ONE fused pass, bit-equal to applying them in sequence (each keeps its own seed, counter
    and density); ``atlas`` [D,H,W] float32 becomes channel 1 of the network input, as the shape-prior datasets append it."""

    def __init__(self, hole: SkullRandomHole, noise: Optional[SaltAndPepper] = None, atlas: Optional[torch.Tensor] = None):
        if not isinstance(hole, SkullRandomHole) or not (noise is None or isinstance(noise, SaltAndPepper)):
            raise TypeError("FlapRecTransform(hole: SkullRandomHole, noise: SaltAndPepper | None, atlas=None)")
        if noise is not None and (noise.keyws[:1] != ("image",) or noise.apply_to != (True,) + (False,) * (len(noise.apply_to) - 1)):
            raise ValueError("FlapRecTransform: the fused noise applies to the image only (apply_to=(True, False))")
        self.hole, self.noise = hole, noise
        self.atlas = None if atlas is None else atlas.float().contiguous()

    def to(self, device) -> "FlapRecTransform":
        self.hole.to(device)
        if self.noise is not None:
            self.noise.to(device)
        if self.atlas is not None:
            self.atlas = self.atlas.to(device)
        return self

    def state_dict(self) -> Dict:
        return {"hole": self.hole.state_dict(), "noise": None if self.noise is None else self.noise.state_dict()}

    def load_state_dict(self, sd: Dict) -> None:
        self.hole.load_state_dict(sd["hole"])
        if self.noise is not None:
            self.noise.load_state_dict(sd["noise"])

    def apply(self, skulls: torch.Tensor, x: Optional[torch.Tensor] = None,
              targets: Optional[Sequence[torch.Tensor]] = None):
        """skulls [N,1,D,H,W] -> (x [N,C,D,H,W], one-hot targets), float32, written into x / targets when given (e.g.
        ``GraphedTrainStep.x`` / ``.targets``)."""
        if self.atlas is not None and self.atlas.device != skulls.device:
            self.atlas = self.atlas.to(skulls.device)
        return _run(self.hole, self.noise, skulls, self.atlas, x, targets)

    @property
    def _params(self) -> Optional[torch.Tensor]:
        return self.hole._params            # the records of the last call of its hole (fused or not)

    def __call__(self, sample: Dict) -> Dict:
        """The reference's Compose([hole, noise]) on a sample dict: float32 image, uint8 target(s); no atlas."""
        sample = self.hole(sample)
        img = sample["image"]
        if self.noise is not None:
            sample = self.noise(sample)
        else:
            sample["image"] = img.float()
        return sample


flap_rec_transform = FlapRecTransform(SkullRandomHole(double_output=True), SaltAndPepper(p=.5, noise_density=.05))
