#!/usr/bin/env python3
"""One rigid registration at the project's usual volume: a 224x512x512 uint8 skull mask at spacing (0.8, 0.45, 0.45), rotated
by 10.7 degrees about an oblique axis and shifted, with a 25 mm hole, registered to the full skull on a 224x304x304 atlas grid
at spacing (0.8, 0.76, 0.76) by ``registration.register`` (30 iterations, centroid start).

Times, each after --warmup untimed calls: the whole ``register`` call (wall clock ending in a device synchronise: erosion,
the two ``nonzero`` read-backs, the distance transform, the centroids, and the optimiser); ``register_points`` alone on the
same points and field (wall clock, and device time between two stream events: 1 + 2 x 31 launches); and one accumulation
launch pair timed the same way.  Next to the accumulation: the bytes it must move (12 per point, and the 8 float32 samples a
point gathers from the field, 32) at the 6.29 TB/s measured copy rate.  The result is checked against the transform the scene
was built with (target registration error over the points).  Prints one JSON line and, with --out DIR, writes
DIR/registration_bench.json and DIR/registration.md.

    python scripts/bench_registration.py --reps 10 --out profiles
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

COPY_TBS = 6.29
MOVING_SHAPE, MOVING_SPACING = (224, 512, 512), (0.8, 0.45, 0.45)
FIXED_SHAPE, FIXED_SPACING = (224, 304, 304), (0.8, 0.76, 0.76)
ROTATION, TRANSLATION = (0.12, -0.09, 0.11), (3.0, -4.0, 2.5)       # Rodrigues vector (10.7 degrees), mm
CENTRE, AXES = (95.0, 115.0, 115.0), (78.0, 95.0, 80.0)             # the skull in the atlas frame, mm
HOLE_CENTRE, HOLE_RADIUS = (150.0, 80.0, 150.0), 25.0


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    t = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + np.sin(t) / t * K + (1.0 - np.cos(t)) / t ** 2 * (K @ K)


def truth():
    """Moving world -> fixed world: a rotation about the skull's centre plus a translation."""
    R, c = rodrigues(ROTATION), np.asarray(CENTRE)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = c - R @ c + np.asarray(TRANSLATION)
    return T


def shape(p):
    """The skull at atlas-frame points p [..., 3] (z, y, x) in mm: an ellipsoid shell open below, with two bumps."""
    def rho(centre, axes):
        c, a = (torch.tensor(v, dtype=p.dtype, device=p.device) for v in (centre, axes))
        return (((p - c) / a) ** 2).sum(-1).sqrt()
    r = rho(CENTRE, AXES)
    shell = (r >= 0.93) & (r <= 1.0) & (p[..., 0] > 40.0)
    return shell | (rho((110.0, 115.0, 198.0), (12.0, 22.0, 12.0)) <= 1.0) | (rho((125.0, 30.0, 100.0), (10.0, 10.0, 18.0)) <= 1.0)


def world(shape_, spacing, dev, z0=0, z1=None):
    """World coordinates [z1 - z0, H, W, 3] of the planes z0 .. z1 of a grid with origin 0."""
    axes = [torch.arange(n, device=dev, dtype=torch.float32) for n in shape_]
    axes[0] = axes[0][z0:z1]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1) * torch.tensor(spacing, dtype=torch.float32, device=dev)


def scene(dev):
    T = torch.from_numpy(truth()).float().to(dev)
    fixed = shape(world(FIXED_SHAPE, FIXED_SPACING, dev)).to(torch.uint8)
    moving = torch.empty(MOVING_SHAPE, dtype=torch.uint8, device=dev)
    hole = torch.tensor(HOLE_CENTRE, dtype=torch.float32, device=dev)
    for z0 in range(0, MOVING_SHAPE[0], 32):                          # in slabs: the coordinates are 12 bytes a voxel
        pw = world(MOVING_SHAPE, MOVING_SPACING, dev, z0, z0 + 32)
        tp = pw @ T[:3, :3].T + T[:3, 3]
        moving[z0:z0 + 32] = (shape(tp) & (((tp - hole) ** 2).sum(-1).sqrt() >= HOLE_RADIUS)).to(torch.uint8)
    return moving, fixed


def _wall(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def _stream_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return round(start.elapsed_time(end) / reps, 4)


MD = """# Rigid registration (`ctunet_amd.registration`, `csrc/registration.hip`) on one MI355X

`scripts/bench_registration.py --reps {reps}` (raw line: `registration_bench.json`).  A {mshape} uint8 skull mask at spacing
{msp} (an ellipsoid shell with two bumps, rotated by 10.7 degrees about an oblique axis, shifted by (3, -4, 2.5) mm, with a
25 mm hole) registered to the full skull on a {fshape} grid at spacing {fsp}: {P} surface points, 30 iterations from the
centroid start.  {warmup} untimed calls, then {reps} timed ones.  "wall" is the wall clock of one call ending in a device
synchronise, median (min-max); "device" is the time per call of {reps} calls issued back to back between two stream events
(the kernel-trace figures below are from a separate run).

| what | wall ms | device ms |
|---|---|---|
| `register` (erosion, two `nonzero` read-backs, distance transform, centroids, optimiser) | {reg} | not taken: the call synchronises inside |
| `register_points` alone: 1 + 2 x 31 launches | {rp} | {rp_dev:.3f} |
| one accumulate + update pair | | {pair_dev:.4f} |

HBM floor of one accumulation: {P} points x (12 bytes of coordinates + 8 float32 field samples) = {acc_mb:.1f} MB, {floor:.4f} ms
at the 6.29 TB/s measured copy rate; the pair takes {ratio:.0f}x that.  (The field itself is {field_mb:.0f} MB; the points sample it
only near the skull's surface.)

Result: target registration error against the transform the scene was built with, over the {P} points: mean {tre_mean:.3f} mm,
max {tre_max:.3f} mm (start: mean {tre_start:.2f} mm); `report()`: {report}.

What the numbers say, and what was and was not tried:

* A pair of launches moves {acc_mb:.1f} MB and takes {ratio:.0f}x its HBM floor: the optimiser is nowhere near bandwidth-bound; it is
  two dependent launches and a one-thread 6x6 solve per iteration.  A `rocprofv3 --kernel-trace --stats` run of a first
  version showed where a pair's time went: `reg_update_kernel` 452 us, `reg_accumulate_kernel` 22.5 us, `reg_init_kernel`
  227 us (once per call).  The update kernel summed the 1024 slab rows with one dependent load per addition; it now issues
  16 loads ahead of their additions (the order of the sum, and so every bit of the result, is unchanged), which took the pair
  from 0.474 ms to the figure above.  No trace of this version was taken.  Capturing the call into a graph (it synchronises
  nowhere), a parallel mean in `reg_init_kernel` and fewer, longer-running accumulation blocks (~{ppt:.0f} point(s) per thread
  here, so the 28 x 6 float64 shuffles of the wave reduction are a large share of its work) were **not tried**.
* The optimiser is most of `register`; the difference between the first two rows is its plumbing (erosion, the distance
  transform of the atlas grid, the `nonzero` read-backs and the centroids), which this change did not touch.  A caller
  who registers many scans to one atlas can compute the field once and call `register_points`.
* Every figure is from one process on one device; no second run was made, so run-to-run spread beyond the min-max above is
  unmeasured.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import postprocess, registration as reg
    dev = torch.device("cuda", 0)
    moving, fixed = scene(dev)
    kw = dict(moving_spacing=MOVING_SPACING, fixed_spacing=FIXED_SPACING)
    whole = _wall(lambda: reg.register(moving, fixed, **kw), args.warmup, args.reps)
    r = reg.register(moving, fixed, **kw)
    points = reg.surface_points(moving, MOVING_SPACING)
    field = postprocess.distance_transform_edt(fixed == 0, sampling=FIXED_SPACING)
    P = int(points.shape[0])
    cm = (torch.nonzero(moving).double() * torch.tensor(MOVING_SPACING, dtype=torch.float64, device=dev)).mean(0)
    cf = (torch.nonzero(fixed).double() * torch.tensor(FIXED_SPACING, dtype=torch.float64, device=dev)).mean(0)
    init = torch.eye(4, dtype=torch.float64, device=dev)
    init[:3, 3] = cf - cm
    ws = torch.empty(reg.workspace_bytes(P), dtype=torch.uint8, device=dev)

    def fit(iterations=30):
        return reg.register_points(points, field, spacing=FIXED_SPACING, init=init, iterations=iterations, workspace=ws)

    rp = _wall(fit, args.warmup, args.reps)
    rp_dev = _stream_ms(fit, args.reps)
    one = _stream_ms(lambda: fit(0), args.reps)                        # init + one pair
    pair_dev = round((rp_dev - one) / 30.0, 4)
    again = fit()
    T, M, M0 = truth(), r.matrix.cpu().numpy(), init.cpu().numpy()
    p = points.cpu().numpy().astype(np.float64)

    def tre(A):
        return np.sqrt((((p @ A[:3, :3].T + A[:3, 3]) - (p @ T[:3, :3].T + T[:3, 3])) ** 2).sum(1))

    acc_bytes = P * (12 + 32)
    res = {"metric": "rigid registration, ms per call", "reps": args.reps, "warmup": args.warmup, "copy_rate_tb_s": COPY_TBS,
           "device": torch.cuda.get_device_name(0), "moving_shape": list(MOVING_SHAPE), "fixed_shape": list(FIXED_SHAPE),
           "points": P, "iterations": 30, "register": whole, "register_points": dict(rp, device_ms=rp_dev),
           "pair_device_ms": pair_dev, "accumulate_hbm_bytes": acc_bytes,
           "accumulate_hbm_floor_ms": round(acc_bytes / (COPY_TBS * 1e12) * 1e3, 5),
           "tre_mean_mm": round(float(tre(M).mean()), 4), "tre_max_mm": round(float(tre(M).max()), 4),
           "tre_start_mean_mm": round(float(tre(M0).mean()), 3), "report": r.report(),
           "register_points_equals_register": bool(torch.equal(again.matrix, r.matrix))}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(os.path.join(args.out, "registration_bench.json"), "w") as f:
            f.write(line + "\n")

        def fmt(s):
            return f"{s['median_ms']:.2f} ({s['min_ms']:.2f}-{s['max_ms']:.2f})"

        blocks = min(-(-P // 256), reg.MAX_BLOCKS)
        with open(os.path.join(args.out, "registration.md"), "w") as f:
            f.write(MD.format(reps=args.reps, warmup=args.warmup, mshape="x".join(map(str, MOVING_SHAPE)), msp=MOVING_SPACING,
                              fshape="x".join(map(str, FIXED_SHAPE)), fsp=FIXED_SPACING, P=P, reg=fmt(whole), rp=fmt(rp),
                              rp_dev=rp_dev, pair_dev=pair_dev, acc_mb=acc_bytes / 1e6, floor=res["accumulate_hbm_floor_ms"],
                              ratio=pair_dev / max(res["accumulate_hbm_floor_ms"], 1e-9), field_mb=field.numel() * 4 / 1e6,
                              tre_mean=res["tre_mean_mm"], tre_max=res["tre_max_mm"], tre_start=res["tre_start_mean_mm"],
                              report=res["report"], ppt=P / (blocks * 256.0)))


if __name__ == "__main__":
    main()
