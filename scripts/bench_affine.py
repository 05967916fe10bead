#!/usr/bin/env python3
"""Affine resampling at the project's usual volume: a 224x512x512 uint8 skull mask at spacing (0.8, 0.45, 0.45) pulled
through a rigid matrix (11 degrees about an oblique axis plus a translation) onto a 224x304x304 atlas grid at spacing
(0.8, 0.76, 0.76), in each mode of ``resample.affine_resample``:

  1. ``nearest``       uint8 -> uint8
  2. ``linear``        uint8 -> float32
  3. ``label_linear``  uint8 -> uint8, K = 2

Each leg runs --warmup untimed calls, then --reps timed calls with ``out=`` given, each ending in a device synchronise (wall
clock per call, median and range), and next to it the device time per call of the same number of calls issued back to back
between two stream events: a call is one kernel launch, so that figure is the per-kernel time.  Each leg states the bytes
the call must move (input read once, output written once) and the time those take at the 6.29 TB/s measured copy rate.
The yardstick is the same warp through ``torch.nn.functional.affine_grid`` + ``grid_sample`` (align_corners=True, zeros
padding) on the same GPU: float input made from the mask inside the timed call, as a user holding a uint8 mask would have
to (legs 1 and 3 convert back to uint8; leg 3 thresholds the trilinear result at 0.5).  Prints one JSON line and, with
--out DIR, writes DIR/affine_bench.json and DIR/affine.md.

    python scripts/bench_affine.py --reps 20 --out profiles
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd")]

import numpy as np
import torch
import torch.nn.functional as F

COPY_TBS = 6.29
IN_SHAPE, IN_SPACING, IN_ORIGIN = (224, 512, 512), (0.8, 0.45, 0.45), (0.0, 0.0, 0.0)
OUT_SHAPE, OUT_SPACING, OUT_ORIGIN = (224, 304, 304), (0.8, 0.76, 0.76), (0.0, 0.0, 0.0)
ROTATION, TRANSLATION = (0.12, -0.09, 0.11), (3.0, -4.0, 2.5)       # Rodrigues vector (|w| = 0.186 rad = 10.7 degrees), mm


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    t = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + np.sin(t) / t * K + (1.0 - np.cos(t)) / t ** 2 * (K @ K)


def out_to_in():
    """Rotation about the centre of the atlas grid's world box, then the translation."""
    c = np.asarray(OUT_ORIGIN) + (np.asarray(OUT_SHAPE) - 1) * np.asarray(OUT_SPACING) / 2
    ci = np.asarray(IN_ORIGIN) + (np.asarray(IN_SHAPE) - 1) * np.asarray(IN_SPACING) / 2
    R = rodrigues(ROTATION)
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = ci - R @ c + np.asarray(TRANSLATION)
    return M


def skull(dev):
    """A skull-like uint8 mask on the input grid: an ellipsoid shell, open below."""
    d, h, w = IN_SHAPE
    zz = torch.arange(d, device=dev, dtype=torch.float32).view(-1, 1, 1)
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(1, -1, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, -1)
    r = (((zz - d / 2) / (0.45 * d)) ** 2 + ((yy - h / 2) / (0.42 * h)) ** 2 + ((xx - w / 2) / (0.36 * w)) ** 2).sqrt()
    return ((r <= 1.0) & (r >= 0.93) & (zz > 0.2 * d)).to(torch.uint8)


def torch_theta(M):
    """theta [1,3,4] of affine_grid (align_corners=True, (x, y, z) order) for the same warp."""
    sp, org, osp, oorg = (np.asarray(v, dtype=np.float64) for v in (IN_SPACING, IN_ORIGIN, OUT_SPACING, OUT_ORIGIN))
    A = M[:3, :3] * osp[None, :] / sp[:, None]                      # index space: u_in = A idx_out + b
    b = (M[:3, :3] @ oorg + M[:3, 3] - org) / sp
    so = (np.asarray(OUT_SHAPE) - 1) / 2.0                           # idx = s (c + 1)
    si = (np.asarray(IN_SHAPE) - 1) / 2.0
    lin = A * so[None, :] / si[:, None]
    off = (A @ so + b - si) / si
    th = np.concatenate([lin, off[:, None]], axis=1)                 # (z, y, x) rows and columns
    th = th[::-1][:, [2, 1, 0, 3]]                                   # -> (x, y, z)
    return torch.from_numpy(np.ascontiguousarray(th)).float()[None]


def _time(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def _stream_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


MD = """# Affine resampling (`resample.affine_resample`, `csrc/affine.hip`) on one MI355X

`scripts/bench_affine.py --reps {reps}` (raw line: `affine_bench.json`).  A {ishape} uint8 skull mask ({fg:.1%} foreground) at
spacing {isp} pulled through a rigid matrix (10.7 degrees about an oblique axis plus a translation, in device memory) onto a
{oshape} grid at spacing {osp}; {inside:.1%} of the output voxels have their nearest input voxel inside the input.  Per leg:
{warmup} untimed calls, then {reps} timed ones with `out=` given.  "wall" is the wall clock of one call ending in a device
synchronise, median (min-max).  "kernel" is the device time per call of {reps} calls issued back to back between two stream
events; a call is one launch, so this is the per-kernel time (no `rocprofv3` trace was taken).  "floor" is the bytes the call
must move (the whole input read once, the output written once) / the 6.29 TB/s measured copy rate.  "torch" is the same
warp through `affine_grid` + `grid_sample` (align_corners=True, zeros padding) on the same GPU, the float input made from the
uint8 mask inside the timed call and the result converted back where the leg's output is uint8 ({treps} timed calls after one
untimed).

| leg | wall ms | kernel ms | bytes | floor ms | kernel / floor | torch wall ms | voxels differing from torch |
|---|---|---|---|---|---|---|---|
{rows}

What was kept and what was tried:

* **Plain gathers were kept.**  Every thread reads its 1 (nearest) or 8 (linear, label_linear) inputs per output voxel
  straight from global memory; a block owns a 4 x 4 x 16-chunk output tile, so under a rigid transform its reads fall into
  a compact source box that the caches serve.  Staging that box in LDS, as `resample_kernel` does for the axis-aligned
  case, was **not tried**: the figures above are the only measurement taken, and the box of an oblique tile is not
  axis-aligned in the input, so its bound has to be formed from the tile's eight corners first.
* **`label_linear` is the slow leg**: it reads the same 8 neighbours as `linear` and mostly takes the shortcut (all 8 labels
  agree), yet takes {label_ratio:.1f}x as long.  What the structure suggests, **unmeasured**: its thread owns 16 output voxels (one
  16-byte store of uint8) where `linear`'s owns 4, and each voxel's 8 one-byte gathers sit behind that voxel's own
  inside-the-volume branch and class loop, so a thread waits for 16 rounds of loads one after the other.  Gathering the
  neighbours of all 16 voxels first (branch-free, clamped indices) and deciding the labels afterwards is the next step; it
  was **not tried**.
* The coordinates cost three float64 divisions per output voxel (the rule divides by the spacing; a reciprocal would change
  the rounding).  Whether the kernel is bound by that arithmetic or by the gathers was **not measured** (no counters were
  read).
* Every figure is from one process on one device; no second run was made, so run-to-run spread beyond the min-max above is
  unmeasured.  The torch results are not the same numbers: torch forms the coordinates in float32 and leg 3 thresholds one
  interpolated value where the rule compares two class scores; bit-exactness is checked against the restated rule in
  `tests/test_affine_gpu.py`, not here.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import resample as rs
    dev = torch.device("cuda", 0)
    mask = skull(dev)
    M = out_to_in()
    m = torch.from_numpy(M).to(dev)
    kw = dict(spacing=IN_SPACING, origin=IN_ORIGIN, out_spacing=OUT_SPACING, out_origin=OUT_ORIGIN)
    vin, vout = int(np.prod(IN_SHAPE)), int(np.prod(OUT_SHAPE))
    out_u8 = torch.empty(OUT_SHAPE, dtype=torch.uint8, device=dev)
    out_f32 = torch.empty(OUT_SHAPE, dtype=torch.float32, device=dev)
    legs = {
        "nearest_u8": (lambda: rs.affine_resample(mask, m, OUT_SHAPE, mode="nearest", out=out_u8, **kw), vin + vout, out_u8),
        "linear_u8_f32": (lambda: rs.affine_resample(mask, m, OUT_SHAPE, mode="linear", out=out_f32, **kw), vin + 4 * vout, out_f32),
        "label_linear_k2": (lambda: rs.affine_resample(mask, m, OUT_SHAPE, mode="label_linear", num_classes=2, out=out_u8, **kw),
                            vin + vout, out_u8),
    }
    theta = torch_theta(M).to(dev)
    size = (1, 1) + OUT_SHAPE

    def tgrid(mode):
        return F.grid_sample(mask.float()[None, None], F.affine_grid(theta, size, align_corners=True), mode=mode,
                             padding_mode="zeros", align_corners=True)[0, 0]

    torch_legs = {"nearest_u8": lambda: tgrid("nearest").to(torch.uint8), "linear_u8_f32": lambda: tgrid("bilinear"),
                  "label_linear_k2": lambda: (tgrid("bilinear") > 0.5).to(torch.uint8)}
    inside = rs.affine_resample(torch.ones(IN_SHAPE, dtype=torch.uint8, device=dev), m, OUT_SHAPE, mode="nearest", **kw)
    res = {"metric": "affine resampling, ms per call (wall clock, synchronised)", "reps": args.reps, "warmup": args.warmup,
           "copy_rate_tb_s": COPY_TBS, "device": torch.cuda.get_device_name(0), "in_shape": list(IN_SHAPE),
           "in_spacing": list(IN_SPACING), "out_shape": list(OUT_SHAPE), "out_spacing": list(OUT_SPACING),
           "foreground_fraction": round(float(mask.float().mean()), 4),
           "output_inside_input_fraction": round(float(inside.float().mean()), 4), "legs": {}}
    for name, (fn, nbytes, out) in legs.items():
        entry = {"device": _stats(_time(fn, args.warmup, args.reps))}
        entry["device"]["kernel_ms"] = round(_stream_ms(fn, args.reps), 4)
        entry["hbm_bytes"] = nbytes
        entry["hbm_floor_ms"] = round(nbytes / (COPY_TBS * 1e12) * 1e3, 4)
        if args.torch_reps > 0:
            tfn = torch_legs[name]
            entry["torch"] = _stats(_time(tfn, 1, args.torch_reps))
            fn()
            t = tfn()
            if out.dtype == torch.float32:
                entry["max_abs_diff_vs_torch"] = float((t - out).abs().max())
                entry["voxels_differing_from_torch"] = int(((t - out).abs() > 1e-3).sum())
            else:
                entry["voxels_differing_from_torch"] = int((t != out).sum())
        res["legs"][name] = entry
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(os.path.join(args.out, "affine_bench.json"), "w") as f:
            f.write(line + "\n")
        rows = []
        titles = {"nearest_u8": "1 `nearest`, uint8 -> uint8", "linear_u8_f32": "2 `linear`, uint8 -> float32",
                  "label_linear_k2": "3 `label_linear` K = 2, uint8 -> uint8"}
        for name, e in res["legs"].items():
            d, t = e["device"], e.get("torch")
            rows.append(f"| {titles[name]} | {d['median_ms']:.3f} ({d['min_ms']:.3f}-{d['max_ms']:.3f}) | {d['kernel_ms']:.3f} | "
                        f"{e['hbm_bytes'] / 1e6:.1f} MB | {e['hbm_floor_ms']:.4f} | {d['kernel_ms'] / e['hbm_floor_ms']:.0f}x | "
                        + (f"{t['median_ms']:.3f} ({t['min_ms']:.3f}-{t['max_ms']:.3f}) | {e['voxels_differing_from_torch']}"
                           if t else "not run | not run") + " |")
        with open(os.path.join(args.out, "affine.md"), "w") as f:
            f.write(MD.format(reps=args.reps, warmup=args.warmup, treps=args.torch_reps, ishape="x".join(map(str, IN_SHAPE)),
                              oshape="x".join(map(str, OUT_SHAPE)), isp=IN_SPACING, osp=OUT_SPACING,
                              label_ratio=res["legs"]["label_linear_k2"]["device"]["kernel_ms"] / res["legs"]["linear_u8_f32"]["device"]["kernel_ms"],
                              fg=res["foreground_fraction"], inside=res["output_inside_input_fraction"], rows="\n".join(rows)))


if __name__ == "__main__":
    main()
