#!/usr/bin/env python3
"""Random spatial augmentation at the project's usual skull volume, 224x304x304 uint8, N = 1, C = 1:

  1. ``warp_nothing``:     ``RandomSpatial.apply`` with every probability 0 (the identity gather: draw + warp launches);
  2. ``warp_affine``:      affine only (probability 1);
  3. ``warp_all``:         flip, elastic (7 control points) and affine, all with probability 1;
  4. ``warp_all_g12``:     the same with 12 control points per axis (the largest LDS grid, 41.5 KB per block);
  5. ``preset``:           ``cranioplasty_transform``-like fused transform end to end (warp, hole, noise, float32 input and
                           two one-hot targets), probabilities 1 so that every call does all the work;
  6. ``affine_resample``:  ``resample.affine_resample(mode="nearest")`` on the same volume through a recorded matrix.

Each leg runs --warmup untimed calls, then --reps timed calls with the outputs preallocated, each ending in a device
synchronise (wall clock per call, median and range), and next to it the device time per call of the same number of calls
issued back to back between two stream events.  Each leg states the bytes the call must move (input read once, output
written once) and the time those take at the 6.29 TB/s measured copy rate.  Prints one JSON line and, with --out DIR, writes
DIR/spatial_bench.json.

    python scripts/bench_spatial.py --reps 20 --out profiles
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd")]

import torch

COPY_TBS = 6.29
SHAPE = (224, 304, 304)


def _skull(dev):
    """A hollow ellipsoid shell, uint8 0 / 1."""
    d, h, w = SHAPE
    zz = torch.arange(d, device=dev, dtype=torch.float32).view(-1, 1, 1)
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(1, -1, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, -1)
    r = (((zz - d / 2) / (0.45 * d)) ** 2 + ((yy - h / 2) / (0.46 * h)) ** 2 + ((xx - w / 2) / (0.44 * w)) ** 2).sqrt()
    return ((r <= 1.0) & (r >= 0.93)).to(torch.uint8).view(1, 1, d, h, w)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import resample
    from ctunet_amd.transforms import FlapRecTransform, RandomSpatial, SaltAndPepper, SkullRandomHole
    dev = torch.device("cuda", 0)
    skull = _skull(dev)
    vox = skull.numel()
    out = torch.empty_like(skull)
    off = dict(flip_p=0.0, affine_p=0.0, elastic_p=0.0)
    on = dict(flip_p=1.0, affine_p=1.0, elastic_p=1.0)
    nothing, affine = RandomSpatial(seed=1, **off), RandomSpatial(seed=2, **dict(off, affine_p=1.0))
    all7, all12 = RandomSpatial(seed=3, **on), RandomSpatial(seed=4, num_control_points=12, **on)
    preset = FlapRecTransform(SkullRandomHole(p=1, double_output=True, seed=5), SaltAndPepper(p=1, noise_density=.05, decay=False, seed=6),
                              spatial=RandomSpatial(seed=7, **on))
    x = torch.empty(skull.shape, dtype=torch.float32, device=dev)
    targets = [torch.empty((1, 2) + SHAPE, dtype=torch.float32, device=dev) for _ in range(2)]
    affine.apply(skull, out=out)
    m = affine.last_params[0]["matrix"].to(dev)
    vol, rout = skull[0, 0], torch.empty(SHAPE, dtype=torch.uint8, device=dev)
    legs = {
        "warp_nothing": (lambda: nothing.apply(skull, out=out), 2 * vox),
        "warp_affine": (lambda: affine.apply(skull, out=out), 2 * vox),
        "warp_all": (lambda: all7.apply(skull, out=out), 2 * vox),
        "warp_all_g12": (lambda: all12.apply(skull, out=out), 2 * vox),
        # warp: 1 + 1 bytes; count: 1; apply: 1 read, 4 (x) + 16 (two one-hot targets) written
        "preset": (lambda: preset.apply(skull, x=x, targets=targets), (2 + 1 + 1 + 20) * vox),
        "affine_resample": (lambda: resample.affine_resample(vol, m, SHAPE, mode="nearest", out=rout), 2 * vox),
    }
    res = {"metric": "random spatial augmentation, ms per call (wall clock, synchronised)", "reps": args.reps,
           "warmup": args.warmup, "copy_rate_tb_s": COPY_TBS, "device": torch.cuda.get_device_name(0), "shape": list(SHAPE),
           "dtype": "uint8", "legs": {}}
    for name, (fn, nbytes) in legs.items():
        entry = {"device": _stats(_time(fn, args.warmup, args.reps))}
        entry["device"]["back_to_back_ms"] = round(_stream_ms(fn, args.reps), 4)
        entry["hbm_bytes"] = nbytes
        entry["hbm_floor_ms"] = round(nbytes / (COPY_TBS * 1e12) * 1e3, 4)
        entry["device_over_floor"] = round(entry["device"]["back_to_back_ms"] / entry["hbm_floor_ms"], 1)
        res["legs"][name] = entry
    ref = res["legs"]["affine_resample"]["device"]["back_to_back_ms"]
    for name in ("warp_nothing", "warp_affine", "warp_all", "warp_all_g12"):
        res["legs"][name]["over_affine_resample"] = round(res["legs"][name]["device"]["back_to_back_ms"] / ref, 2)
    affine.apply(skull, out=out)
    m2 = affine.last_params[0]["matrix"].to(dev)
    res["affine_voxels_differing_from_affine_resample"] = int(
        (resample.affine_resample(vol, m2, SHAPE, mode="nearest") != out[0, 0]).sum())
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(os.path.join(args.out, "spatial_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
