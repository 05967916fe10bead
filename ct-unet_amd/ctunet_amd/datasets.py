"""Synthetic patch source with the reference datasets' sample schema.

The reference's datasets read NIfTI volumes with SimpleITK and cut random flaps with raster_geometry on the CPU
(/root/reference/ctunet/pytorch/datasets.py:89-112,195-235; transforms.py) -- I/O and augmentation are out of scope.
What the training step consumes is only their OUTPUT contract, reproduced here for synthetic binary skulls generated
on the GPU:

    sample = {"image":  float32 [C, D, H, W]   skull with the flap removed (+ atlas channel when append_atlas),
              "target": float32 one-hot [2, D, H, W]                      (single-output handlers), or
                        (full_skull one-hot, flap one-hot)                 (FlapRec...DoubleOut handlers),
              "filepath": str}

with ``one_hot(label.long(), 2).movedim(-1, 0).float()`` targets (datasets.py:107-110, 212-217; done by
``ctu_one_hot``) and ``full_skull = image + flap`` (datasets.py:228).  ``torch.utils.data.DataLoader``'s default
collate turns the target tuple into the list ``Model.forward_pass`` expects (Model.py:344-349).
Inputs are binary masks cast to float like the reference's (datasets.py:92-94): a hollow ellipsoid shell ("skull"),
a spherical bite out of it ("flap"); geometry is drawn from ``torch.Generator(seed + idx)`` so every rank / epoch can
address its own deterministic items (rank r takes idx = r, r + world, ...).

The in-memory training sets below (FlapRecWShapePrior2OTrainDataset, FlapRec2OTrainDataset) produce the same schema from
real binary skulls through the on-device flap_rec_transform (transforms.py).
"""
from __future__ import annotations

import torch
from torch.utils.data import Dataset

from . import ops


class SyntheticFlapDataset(Dataset):
    def __init__(self, n_items: int, size: int = 128, seed: int = 1234, double_out: bool = True,
                 append_atlas: bool = True, device="cuda"):
        if size % 16:
            raise ValueError("ctunet_amd: patch size must be divisible by 16 (4 pooling levels)")
        self.n, self.size, self.seed = int(n_items), int(size), int(seed)
        self.double_out, self.append_atlas = bool(double_out), bool(append_atlas)
        self.device = torch.device(device)
        ax = torch.linspace(-1.0, 1.0, self.size, device=self.device)
        self._zz, self._yy, self._xx = torch.meshgrid(ax, ax, ax, indexing="ij")
        self._atlas = self._shell(torch.tensor([0.0, 0.0, 0.0]), torch.tensor([0.72, 0.8, 0.66]), 0.07)

    def __len__(self):
        return self.n

    def _shell(self, centre, radii, thick):
        c, r = centre.tolist(), radii.tolist()
        q = ((self._zz - c[0]) / r[0]) ** 2 + ((self._yy - c[1]) / r[1]) ** 2 + ((self._xx - c[2]) / r[2]) ** 2
        return ((q <= 1.0) & (q >= (1.0 - thick / min(r)) ** 2)).float()

    def __getitem__(self, idx: int):
        if not 0 <= idx < self.n:
            raise IndexError(idx)
        g = torch.Generator().manual_seed(self.seed + idx)
        u = torch.rand(10, generator=g)
        centre = (u[0:3] - 0.5) * 0.16
        radii = torch.tensor([0.72, 0.8, 0.66]) * (0.9 + 0.2 * u[3:6])
        skull = self._shell(centre, radii, 0.06 + 0.04 * float(u[6]))
        # flap: the part of the shell inside a sphere centred on the upper half of the shell surface
        th, ph = float(u[7]) * 6.2832, 0.25 + 0.9 * float(u[8])
        fc = centre + radii * torch.tensor([torch.cos(torch.tensor(ph)), torch.sin(torch.tensor(ph)) * torch.sin(torch.tensor(th)),
                                            torch.sin(torch.tensor(ph)) * torch.cos(torch.tensor(th))])
        fr = 0.22 + 0.2 * float(u[9])
        fcl = fc.tolist()
        ball = ((self._zz - fcl[0]) ** 2 + (self._yy - fcl[1]) ** 2 + (self._xx - fcl[2]) ** 2) <= fr * fr
        flap = skull * ball.float()
        image = skull - flap                                        # binary {0, 1}, float
        full = ops.one_hot((image + flap).unsqueeze(0).contiguous(), 2)[0]          # datasets.py:228-230
        flap_oh = ops.one_hot(flap.unsqueeze(0).contiguous(), 2)[0]
        img = image.unsqueeze(0)
        if self.append_atlas:                                       # load_atlas_and_append_at_axis(image, 0)
            img = torch.cat((img, self._atlas.unsqueeze(0)), 0)
        target = (full, flap_oh) if self.double_out else flap_oh
        return {"image": img.contiguous(), "target": target, "filepath": f"synthetic://{self.seed}/{idx}"}


class FlapRecWShapePrior2OTrainDataset(Dataset):
    """In-memory binary skulls through the flap-reconstruction transform on the GPU (the reference's class of the same
    name, ctunet/pytorch/datasets.py:152-235, minus its NIfTI I/O): item idx is

        {"image":  float32 [2, D, H, W]  broken, noisy skull + atlas   ([1, D, H, W] without the atlas),
         "target": (full skull one-hot [2, D, H, W], flap one-hot [2, D, H, W]),
         "filepath": "memory://<idx>"}

    skulls: a list of [D,H,W] tensors or one [M,D,H,W] tensor, float32 or uint8, on the host or the device (host items
    are copied to the device per item); atlas: [D,H,W].  transform: a ``transforms.FlapRecTransform`` (default: the
    module's ``flap_rec_transform``, with the reference's decaying noise density); its hole must be double-output.
    The transform runs as ONE fused pass per item (after the warp of its ``spatial`` step and the thickening of its
    ``dilate`` step, when it has them, as ``transforms.realistic_cranioplasty_transform`` does); every call advances its
    device sample counters."""

    def __init__(self, skulls, atlas=None, transform=None, append_atlas: bool = True, device="cuda"):
        from . import transforms as T
        self.skulls = skulls
        if len(skulls) == 0 or any(s.dim() != 3 for s in (skulls[i] for i in range(len(skulls)))):
            raise ValueError("ctunet_amd: skulls must be a non-empty list of [D,H,W] tensors or an [M,D,H,W] tensor")
        self.device = torch.device(device)
        base = T.flap_rec_transform if transform is None else transform
        if not isinstance(base, T.FlapRecTransform) or not base.hole.double_output:
            raise ValueError("ctunet_amd: transform must be a FlapRecTransform whose hole has double_output=True")
        self.append_atlas = bool(append_atlas)
        if self.append_atlas and atlas is None:
            raise ValueError("ctunet_amd: append_atlas needs an atlas [D,H,W]")
        self.atlas = atlas.to(self.device, torch.float32).contiguous() if self.append_atlas else None
        self.transform = T.FlapRecTransform(base.hole, base.noise, self.atlas, base.spatial, base.dilate)   # shares their state

    def __len__(self):
        return len(self.skulls)

    def __getitem__(self, idx: int):
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        s = self.skulls[idx]
        s = s.to(self.device, non_blocking=True)
        if s.dtype not in (torch.float32, torch.uint8):
            s = s.float()
        x, (full, flap) = self.transform.apply(s.contiguous().view(1, 1, *s.shape))
        return {"image": x[0], "target": (full[0], flap[0]), "filepath": f"memory://{idx}"}


class FlapRec2OTrainDataset(FlapRecWShapePrior2OTrainDataset):
    """FlapRecDoubleOut's training set (datasets.py:238-250): the same without the atlas channel."""

    def __init__(self, skulls, transform=None, device="cuda"):
        super().__init__(skulls, None, transform, append_atlas=False, device=device)


class FlapRecPatchDataset(Dataset):
    """Random class-balanced patches of in-memory binary skulls through the flap-reconstruction transform, all on the GPU
    (BASELINE config 4, "skull volumes tiled to 192^3 patches"; ``sampling`` pins the draw).  Item idx is one patch of
    skull idx // patches_per_volume, centred on bone with the sampler's class share and jitter, anywhere otherwise:

        {"image":  float32 [2, pd, ph, pw]  broken, noisy skull patch + the atlas window   ([1, ...] without an atlas),
         "target": (full skull one-hot [2, pd, ph, pw], flap one-hot [2, pd, ph, pw]),
         "filepath": "memory://<skull>#<patch>",
         "coords": int32 [4] = (skull, z0, y0, x0) on the device}

    the schema of FlapRecWShapePrior2OTrainDataset at the patch size, plus ``coords``.  skulls: a list of [D,H,W] tensors
    of one shape or an [M,D,H,W] tensor; they are kept on the device as their uint8 casts (a voxel's value, as the
    transform reads it) and indexed once.  sampler: a ``sampling.PatchSampler`` with ``classes=None`` (bone = nonzero).
    atlas: [D,H,W], cropped at the same window as float32.  transform: as FlapRecWShapePrior2OTrainDataset's; it runs on
    the patch and shares the base transform's state.  Every item advances the sampler's and the transform's counters."""

    def __init__(self, skulls, sampler, atlas=None, transform=None, patches_per_volume: int = 1, device="cuda"):
        from . import sampling
        from . import transforms as T
        if not isinstance(sampler, sampling.PatchSampler) or sampler.classes is not None:
            raise ValueError("ctunet_amd: sampler must be a sampling.PatchSampler with classes=None (bone = nonzero)")
        if isinstance(patches_per_volume, bool) or not isinstance(patches_per_volume, int) or patches_per_volume < 1:
            raise ValueError(f"ctunet_amd: patches_per_volume must be a positive integer, got {patches_per_volume!r}")
        items = [skulls[i] for i in range(len(skulls))]
        if not items or any(s.dim() != 3 or s.shape != items[0].shape for s in items):
            raise ValueError("ctunet_amd: skulls must be a non-empty list of [D,H,W] tensors of one shape or an [M,D,H,W] tensor")
        base = T.flap_rec_transform if transform is None else transform
        if not isinstance(base, T.FlapRecTransform) or not base.hole.double_output:
            raise ValueError("ctunet_amd: transform must be a FlapRecTransform whose hole has double_output=True")
        self.device = torch.device(device)
        self.sampler, self.per = sampler, patches_per_volume
        vols = torch.stack([s.to(self.device) for s in items])
        self.skulls = vols if vols.dtype == torch.uint8 else vols.to(torch.uint8)    # [M,D,H,W]: the uint8 casts
        m, d, h, w = self.skulls.shape
        if atlas is not None and tuple(atlas.shape) != (d, h, w):
            raise ValueError(f"ctunet_amd: the atlas must be [{d},{h},{w}], got {tuple(atlas.shape)}")
        self.atlas = None if atlas is None else atlas.to(self.device, torch.float32).contiguous().view(1, 1, d, h, w)
        self.index = sampler.index(self.skulls)                                      # built once
        self._item = torch.arange(m, dtype=torch.int32, device=self.device)
        self._base = base

    def __len__(self):
        return self.skulls.shape[0] * self.per

    def __getitem__(self, idx: int):
        from . import sampling
        from . import transforms as T
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        m = idx // self.per
        coords = self.sampler.draw(self.index, items=self._item[m:m + 1])
        vols = self.skulls
        patch = sampling.crop(vols.view(vols.shape[0], 1, *vols.shape[1:]), coords, self.sampler.patch)
        ap = None if self.atlas is None else sampling.crop(self.atlas, coords, self.sampler.patch)[0, 0]
        b = self._base
        x, (full, flap) = T.FlapRecTransform(b.hole, b.noise, ap, b.spatial, b.dilate).apply(patch)   # shares their state
        return {"image": x[0], "target": (full[0], flap[0]), "filepath": f"memory://{m}#{idx % self.per}",
                "coords": coords[0]}


class FlapRecTrainDataset(Dataset):
    """Not provided: in the reference (datasets.py:136-149 with 89-112) flap_rec_transform's (full skull, flap) tuple
    target reaches ``sample['target'].long()`` (datasets.py:107-110) and raises, so this class cannot produce a sample."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("FlapRecTrainDataset crashes in the reference: flap_rec_transform's tuple target "
                                  "reaches .long() (ctunet/pytorch/datasets.py:107-110); use FlapRec2OTrainDataset")


class FlapRecWShapePriorTrainDataset(Dataset):
    """Not provided: the reference's version (datasets.py:253-270) runs cranioplasty_transform, whose elastic and affine
    steps come from torchio -- outside this package."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("FlapRecWShapePriorTrainDataset needs torchio's elastic and affine transforms "
                                  "(cranioplasty_transform); use FlapRecWShapePrior2OTrainDataset")
