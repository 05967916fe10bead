#!/usr/bin/env python3
"""One similarity registration with the symmetric chamfer cost at the project's usual volume: the scene of
``scripts/bench_registration.py`` (a 224x512x512 uint8 skull mask at spacing (0.8, 0.45, 0.45), rotated by 10.7 degrees,
shifted, with a 25 mm hole, against the full skull on a 224x304x304 atlas grid at spacing (0.8, 0.76, 0.76)) with the moving
skull also 6 % smaller: truth = rigid @ scale_about(centre, 1.06).  ``registration.register(model="similarity")``, 30
iterations from the centroid start, ``max_distance`` --bound mm (the atlas's points over the hole have no counterpart).

Times, each after --warmup untimed calls: the whole ``register`` call (wall clock ending in a device synchronise: two
erosions, the ``nonzero`` read-backs, two distance transforms, the centroids, the optimiser);
``register_similarity_points`` alone on the same points and fields (wall clock, and device time between two stream events);
one accumulate + update pair of the similarity kernels (P + Q items, 7 unknowns), and -- the yardstick -- one pair of the
rigid kernels on the same moving points and fixed field in the same run.  The result is checked against the transform the
scene was built with (target registration error over the moving points, and the scale).  Prints one JSON line and, with
--out DIR, writes DIR/registration_similarity_bench.json and DIR/registration_similarity.md.

    python scripts/bench_similarity.py --reps 10 --out profiles
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd"), os.path.join(ROOT, "scripts")]

import numpy as np
import torch

import bench_registration as B

SCALE = 1.06
ITERATIONS = 30


def truth():
    """Moving world -> fixed world: the rigid scene's transform after a scale about the skull's centre."""
    c = np.asarray(B.CENTRE)
    S = np.eye(4)
    S[:3, :3] *= SCALE
    S[:3, 3] = c - SCALE * c
    return B.truth() @ S


def scene(dev):
    """bench_registration.scene with the scaled truth."""
    T = torch.from_numpy(truth()).float().to(dev)
    fixed = B.shape(B.world(B.FIXED_SHAPE, B.FIXED_SPACING, dev)).to(torch.uint8)
    moving = torch.empty(B.MOVING_SHAPE, dtype=torch.uint8, device=dev)
    hole = torch.tensor(B.HOLE_CENTRE, dtype=torch.float32, device=dev)
    for z0 in range(0, B.MOVING_SHAPE[0], 32):
        tp = B.world(B.MOVING_SHAPE, B.MOVING_SPACING, dev, z0, z0 + 32) @ T[:3, :3].T + T[:3, 3]
        moving[z0:z0 + 32] = (B.shape(tp) & (((tp - hole) ** 2).sum(-1).sqrt() >= B.HOLE_RADIUS)).to(torch.uint8)
    return moving, fixed


MD = """# Similarity registration with the symmetric chamfer cost (`ctunet_amd.registration`, `csrc/registration.hip`) on one MI355X

`scripts/bench_similarity.py --reps {reps} --bound {bound}` (raw line: `registration_similarity_bench.json`).  The scene of
`registration.md` ({mshape} uint8 mask at spacing {msp}, 10.7 degrees, (3, -4, 2.5) mm, a 25 mm hole; atlas grid {fshape} at
{fsp}) with the moving skull 6 % smaller (true scale {scale}): P = {P} moving surface points, Q = {Q} fixed surface points,
{iterations} iterations from the centroid start, `max_distance` {bound} mm.  {warmup} untimed calls, then {reps} timed ones.  "wall"
is the wall clock of one call ending in a device synchronise, median (min-max); "device" is the time per call of {reps} calls
issued back to back between two stream events.

| what | wall ms | device ms |
|---|---|---|
| `register(model="similarity")` (two erosions, `nonzero` read-backs, two distance transforms, centroids, optimiser) | {reg} | not taken: the call synchronises inside |
| `register_similarity_points` alone: 1 + 2 x {rows} launches | {sp} | {sp_dev:.3f} |
| one similarity accumulate + update pair ({items} items, 7 unknowns, 36 sums) | | {pair:.4f} |
| one rigid accumulate + update pair, same run ({P} points, 6 unknowns, 28 sums) | | {rigid_pair:.4f} |

Ratio of the pairs: {ratio:.2f}; (P + Q) / P = {items_ratio:.2f}.  {verdict}

Result: target registration error against the transform the scene was built with, over the {P} moving points: mean
{tre_mean:.3f} mm, max {tre_max:.3f} mm (start: mean {tre_start:.2f} mm); scale {scale_got:.5f} against {scale}
({scale_err:+.3%}); `report()`: {report}.  The rigid fit of the same pair (`register` with its defaults and the same
`max_distance`): mean {rigid_mean:.3f} mm, max {rigid_max:.3f} mm.

What was and was not measured:

* The pair is timed as the difference of a {iterations}-iteration and a 0-iteration call over {iterations}, for both kernels the same
  way; no kernel trace of the new kernels was taken, so the split between accumulate and update is not known here.
* The accumulation kernel holds 36 + 2 sums per thread (160 VGPRs, 3 waves per SIMD, no scratch) against 28 + 1 (122 VGPRs,
  4 waves) for the rigid one, and its wave reduction is 38 x 6 shuffles of 64-bit values against 29 x 6.
* Every figure is from one process on one device; run-to-run spread beyond the min-max above is unmeasured.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bound", type=float, default=6.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import postprocess, registration as reg
    dev = torch.device("cuda", 0)
    moving, fixed = scene(dev)
    kw = dict(moving_spacing=B.MOVING_SPACING, fixed_spacing=B.FIXED_SPACING, iterations=ITERATIONS, max_distance=args.bound)
    whole = B._wall(lambda: reg.register(moving, fixed, model="similarity", **kw), args.warmup, args.reps)
    r = reg.register(moving, fixed, model="similarity", **kw)
    rigid = reg.register(moving, fixed, **kw)
    points = reg.surface_points(moving, B.MOVING_SPACING)
    fpoints = reg.surface_points(fixed, B.FIXED_SPACING)
    field = postprocess.distance_transform_edt(fixed == 0, sampling=B.FIXED_SPACING)
    mfield = postprocess.distance_transform_edt(moving == 0, sampling=B.MOVING_SPACING)
    P, Q = int(points.shape[0]), int(fpoints.shape[0])
    cm = (torch.nonzero(moving).double() * torch.tensor(B.MOVING_SPACING, dtype=torch.float64, device=dev)).mean(0)
    cf = (torch.nonzero(fixed).double() * torch.tensor(B.FIXED_SPACING, dtype=torch.float64, device=dev)).mean(0)
    init = torch.eye(4, dtype=torch.float64, device=dev)
    init[:3, 3] = cf - cm
    ws = torch.empty(reg.similarity_workspace_bytes(P, Q), dtype=torch.uint8, device=dev)

    def fit(iterations=ITERATIONS):
        return reg.register_similarity_points(points, field, fixed_points=fpoints, moving_field=mfield, spacing=B.FIXED_SPACING,
                                              moving_spacing=B.MOVING_SPACING, init=init, iterations=iterations,
                                              max_distance=args.bound, workspace=ws)

    def fit_rigid(iterations=ITERATIONS):
        return reg.register_points(points, field, spacing=B.FIXED_SPACING, init=init, iterations=iterations,
                                   max_distance=args.bound, workspace=ws)

    sp = B._wall(fit, args.warmup, args.reps)
    sp_dev = B._stream_ms(fit, args.reps)
    pair = round((sp_dev - B._stream_ms(lambda: fit(0), args.reps)) / ITERATIONS, 4)
    for _ in range(args.warmup):
        fit_rigid()
    rigid_dev = B._stream_ms(fit_rigid, args.reps)
    rigid_pair = round((rigid_dev - B._stream_ms(lambda: fit_rigid(0), args.reps)) / ITERATIONS, 4)
    again = fit()
    T, M, M0, Mr = truth(), r.matrix.cpu().numpy(), init.cpu().numpy(), rigid.matrix.cpu().numpy()
    p = points.cpu().numpy().astype(np.float64)

    def tre(A):
        return np.sqrt((((p @ A[:3, :3].T + A[:3, 3]) - (p @ T[:3, :3].T + T[:3, 3])) ** 2).sum(1))

    scale_got = float(np.cbrt(np.linalg.det(M[:3, :3])))
    res = {"metric": "similarity registration with the symmetric chamfer cost, ms per call", "reps": args.reps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "moving_shape": list(B.MOVING_SHAPE),
           "fixed_shape": list(B.FIXED_SHAPE), "points": P, "fixed_points": Q, "iterations": ITERATIONS,
           "max_distance": args.bound, "true_scale": SCALE, "register": whole,
           "register_similarity_points": dict(sp, device_ms=sp_dev), "pair_device_ms": pair,
           "rigid_register_points_device_ms": rigid_dev, "rigid_pair_device_ms": rigid_pair,
           "pair_ratio": round(pair / max(rigid_pair, 1e-9), 3), "items_ratio": round((P + Q) / P, 3),
           "tre_mean_mm": round(float(tre(M).mean()), 4), "tre_max_mm": round(float(tre(M).max()), 4),
           "tre_start_mean_mm": round(float(tre(M0).mean()), 3), "scale": round(scale_got, 6),
           "scale_error": round(scale_got / SCALE - 1.0, 6), "rigid_tre_mean_mm": round(float(tre(Mr).mean()), 4),
           "rigid_tre_max_mm": round(float(tre(Mr).max()), 4), "report": r.report(),
           "points_call_equals_register": bool(torch.equal(again.matrix, r.matrix))}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(os.path.join(args.out, "registration_similarity_bench.json"), "w") as f:
            f.write(line + "\n")

        def fmt(s):
            return f"{s['median_ms']:.2f} ({s['min_ms']:.2f}-{s['max_ms']:.2f})"

        verdict = ("The expectation was about (P + Q) / P of the rigid pair or less: met." if res["pair_ratio"] <= res["items_ratio"]
                   else "The expectation was about (P + Q) / P of the rigid pair or less: NOT met; no trace was taken, so where "
                        "the extra time goes is not known.")
        with open(os.path.join(args.out, "registration_similarity.md"), "w") as f:
            f.write(MD.format(reps=args.reps, warmup=args.warmup, bound=args.bound, mshape="x".join(map(str, B.MOVING_SHAPE)),
                              msp=B.MOVING_SPACING, fshape="x".join(map(str, B.FIXED_SHAPE)), fsp=B.FIXED_SPACING, scale=SCALE,
                              P=P, Q=Q, iterations=ITERATIONS, rows=ITERATIONS + 1, items=P + Q, reg=fmt(whole), sp=fmt(sp),
                              sp_dev=sp_dev, pair=pair, rigid_pair=rigid_pair, ratio=res["pair_ratio"],
                              items_ratio=res["items_ratio"], verdict=verdict, tre_mean=res["tre_mean_mm"],
                              tre_max=res["tre_max_mm"], tre_start=res["tre_start_mean_mm"], scale_got=scale_got,
                              scale_err=res["scale_error"], report=res["report"], rigid_mean=res["rigid_tre_mean_mm"],
                              rigid_max=res["rigid_tre_max_mm"]))


if __name__ == "__main__":
    main()
