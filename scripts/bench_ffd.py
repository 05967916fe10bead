#!/usr/bin/env python3
"""One B-spline deformable registration at the project's usual volume: the scene of ``bench_registration.py`` (a 224x512x512
uint8 skull mask at spacing (0.8, 0.45, 0.45) with a 25 mm hole, the full skull on a 224x304x304 atlas grid at (0.8, 0.76,
0.76)) with the moving head also deformed: a 3-4 % anisotropic stretch and a 6 mm smooth bump.  ``register_deformable``
(similarity matrix, then 60 free-form iterations on a 10 mm lattice, ``max_distance`` 6 mm) and the pull of the atlas onto
the patient's grid by ``deformable_resample``.

Times, each after --warmup untimed calls: the whole ``register_deformable`` call and the binning of ``FFDPlan`` (wall clock
ending in a device synchronise); ``FFDPlan.run`` (wall clock, and device time between two stream events); one free-form
iteration (accumulate + update: the difference of a 60- and a 0-iteration run over 60) next to one similarity
accumulate + update pair over the same P points, timed the same way; ``deformable_resample`` next to ``affine_resample`` on
the same volumes.  Prints one JSON line and, with --out DIR, writes DIR/registration_ffd_bench.json and
DIR/registration_ffd.md.

    python scripts/bench_ffd.py --reps 10 --out profiles
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd"), os.path.join(ROOT, "scripts")]

import torch

from bench_registration import (CENTRE, FIXED_SHAPE, FIXED_SPACING, HOLE_CENTRE, HOLE_RADIUS, MOVING_SHAPE, MOVING_SPACING, _stream_ms,
                                _wall, shape, truth, world)

STRETCH = (1.04, 0.97, 1.03)
BUMP, BUMP_CENTRE, BUMP_SIGMA = (6.0, -4.0, 5.0), (140.0, 130.0, 140.0), 30.0
CONTROL_SPACING, STIFFNESS, ITERATIONS, BOUND = 10.0, 0.1, 60, 6.0


def phi(q):
    t = lambda v: torch.tensor(v, dtype=q.dtype, device=q.device)                                        # noqa: E731
    d = q - t(BUMP_CENTRE)
    return t(CENTRE) + t(STRETCH) * (q - t(CENTRE)) + t(BUMP) * torch.exp(-(d * d).sum(-1, keepdim=True) / (2.0 * BUMP_SIGMA ** 2))


def scene(dev):
    """(moving with the hole, moving without it, fixed)."""
    T = torch.from_numpy(truth()).float().to(dev)
    fixed = shape(world(FIXED_SHAPE, FIXED_SPACING, dev)).to(torch.uint8)
    moving = torch.empty(MOVING_SHAPE, dtype=torch.uint8, device=dev)
    full = torch.empty(MOVING_SHAPE, dtype=torch.uint8, device=dev)
    hole = torch.tensor(HOLE_CENTRE, dtype=torch.float32, device=dev)
    for z0 in range(0, MOVING_SHAPE[0], 16):
        pw = world(MOVING_SHAPE, MOVING_SPACING, dev, z0, z0 + 16)
        tp = pw @ T[:3, :3].T + T[:3, 3]
        s = shape(phi(tp))
        full[z0:z0 + 16] = s.to(torch.uint8)
        moving[z0:z0 + 16] = (s & (((tp - hole) ** 2).sum(-1).sqrt() >= HOLE_RADIUS)).to(torch.uint8)
    return moving, full, fixed


def dice(a, b):
    return float(2.0 * (a & b).sum() / (a.sum() + b.sum()))


MD = """# B-spline deformable registration (`ctunet_amd.registration`, `csrc/ffd.hip`) on one MI355X

`scripts/bench_ffd.py --reps {reps}` (raw line: `registration_ffd_bench.json`).  The scene of `registration.md` ({mshape} uint8
mask at spacing {msp}, 10.7 degrees, (3, -4, 2.5) mm, a 25 mm hole; atlas grid {fshape} at {fsp}) with the moving head also
deformed by a 3-4 % anisotropic stretch and a 6 mm smooth bump: P = {P} surface points, lattice {G} at {h} mm ({S} segments of
at most 256 points over {cells} occupied cells), {it} iterations behind the similarity matrix, `max_distance` {bound} mm.
{warmup} untimed calls, then {reps} timed ones.  "wall" is the wall clock of one call ending in a device synchronise, median
(min-max); "device" is the time per call of {reps} calls issued back to back between two stream events.

| what | wall ms | device ms |
|---|---|---|
| `register_deformable` (`register(model="similarity")`, erosion, distance transform, binning, fit) | {whole} | not taken: the call synchronises inside |
| `FFDPlan(...)`: cells kernel, stable sort, segment tables, one read-back | {plan} | |
| `FFDPlan.run()`: 1 + 3 x {rows} launches, the finish and the Jacobian launch | {run} | {run_dev:.3f} |
| one free-form iteration (accumulate + reduce + step, {P} points) | | {iter_dev:.4f} |
| one similarity accumulate + update pair over the same {P} points (forward term only), same run | | {sim_dev:.4f} |
| `deformable_resample`, uint8 `label_linear`, {fshape} -> {mshape} | {dl} | {dl_dev:.3f} |
| `affine_resample`, the same call through the matrix alone | {al} | {al_dev:.3f} |
| `deformable_resample`, float32 `linear`, the same grids | {df} | {df_dev:.3f} |
| `affine_resample`, float32 `linear` | {af} | {af_dev:.3f} |

Ratios: one free-form iteration is {r_sim:.2f}x the similarity pair at the same P measured here, and {r_prof:.2f}x the 0.0616 ms
of `registration_similarity.md` (586216 items).  `deformable_resample` is {r_l:.2f}x (`label_linear`) and {r_f:.2f}x (`linear`)
`affine_resample`; `RandomSpatial`'s elastic warp is 1.0 ms on its own volume (`spatial.md`), and the `label_linear` pull here
is {r_sp:.2f}x that.  No target was set for these times.

Result: `report()`: {report}.  Dice of the atlas pulled onto the patient's grid against the hole-free moving skull:
{d0:.4f} through the similarity matrix alone, {d1:.4f} through the free-form result.

Kernel resources (`hipcc -Rpass-analysis=kernel-resource-usage`; no kernel uses scratch):

| kernel | VGPRs | LDS bytes / block | waves / SIMD |
|---|---|---|---|
| `ffd_accumulate_kernel` | 78 | 37376 | 4 (LDS: four blocks of 256 a CU) |
| `ffd_reduce_kernel` (one block of 1024) | 38 | 24576 | 8 |
| `ffd_step_kernel` | 38 | 0 | 8 |
| `ffd_transform_kernel` with / without the determinant | 128 / 90 | 0 | 4 / 5 |
| `ffd_resample_kernel` nearest / linear / label_linear | 96 / 98 / 98 | 40 | 5 / 4 / 4 |

What was and was not measured:

* The iteration is timed as the difference of a {it}-iteration and a 0-iteration run over {it}; no kernel trace was taken, so
  the split between the three launches is not known here.
* The 64-term sums were first unrolled completely: the accumulation then took 256 VGPRs (one wave a SIMD).  Keeping the
  outer loop of four rolled gives the figures above; nothing else was tuned.  Staging the controls of `deformable_resample`
  in LDS was **not tried**: they are read from global memory (a {G} lattice is {ctl_kb:.0f} KiB and stays in L2).
* Every figure is from one process on one device; run-to-run spread beyond the min-max above is unmeasured.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import postprocess, registration as reg, resample
    dev = torch.device("cuda", 0)
    moving, full, fixed = scene(dev)
    kw = dict(moving_spacing=MOVING_SPACING, fixed_spacing=FIXED_SPACING, max_distance=BOUND, control_spacing=CONTROL_SPACING,
              stiffness=STIFFNESS, iterations=ITERATIONS)
    whole = _wall(lambda: reg.register_deformable(moving, fixed, **kw), args.warmup, args.reps)
    d = reg.register_deformable(moving, fixed, **kw)
    report = d.report()
    affine = d.matrix.clone()
    points = reg.surface_points(moving, MOVING_SPACING)
    field = postprocess.distance_transform_edt(fixed == 0, sampling=FIXED_SPACING)
    P = int(points.shape[0])
    pk = dict(spacing=FIXED_SPACING, control_spacing=CONTROL_SPACING, stiffness=STIFFNESS, max_distance=BOUND)
    plan_t = _wall(lambda: reg.FFDPlan(points, field, affine, iterations=ITERATIONS, **pk), args.warmup, args.reps)
    plan = reg.FFDPlan(points, field, affine, iterations=ITERATIONS, **pk)
    plan0 = reg.FFDPlan(points, field, affine, iterations=0, **pk)
    run = _wall(plan.run, args.warmup, args.reps)
    run_dev = _stream_ms(plan.run, args.reps)
    run0_dev = _stream_ms(plan0.run, args.reps)
    iter_dev = round((run_dev - run0_dev) / ITERATIONS, 4)

    def sim(iterations):
        return reg.register_similarity_points(points, field, spacing=FIXED_SPACING, init=affine, iterations=iterations,
                                              max_distance=BOUND)

    sim(30)
    sim_dev = round((_stream_ms(lambda: sim(30), args.reps) - _stream_ms(lambda: sim(0), args.reps)) / 30.0, 4)

    rk = dict(spacing=FIXED_SPACING, out_spacing=MOVING_SPACING)
    lab = dict(mode="label_linear", num_classes=2, **rk)
    lin = dict(mode="linear", **rk)
    out_l = torch.empty(MOVING_SHAPE, dtype=torch.uint8, device=dev)
    out_f = torch.empty(MOVING_SHAPE, dtype=torch.float32, device=dev)
    calls = {"dl": lambda: resample.deformable_resample(fixed, d, MOVING_SHAPE, out=out_l, **lab),
             "al": lambda: resample.affine_resample(fixed, affine, MOVING_SHAPE, out=out_l, **lab),
             "df": lambda: resample.deformable_resample(field, d, MOVING_SHAPE, out=out_f, **lin),
             "af": lambda: resample.affine_resample(field, affine, MOVING_SHAPE, out=out_f, **lin)}
    times = {k: dict(_wall(fn, args.warmup, args.reps), device_ms=_stream_ms(fn, args.reps)) for k, fn in calls.items()}
    truth_mask = full != 0
    d0 = dice(resample.affine_resample(fixed, affine, MOVING_SHAPE, **lab) != 0, truth_mask)
    d1 = dice(resample.deformable_resample(fixed, d, MOVING_SHAPE, **lab) != 0, truth_mask)
    cells = int((plan.tables[4][1:] > plan.tables[4][:-1]).sum())
    res = {"metric": "B-spline deformable registration, ms per call", "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "moving_shape": list(MOVING_SHAPE), "fixed_shape": list(FIXED_SHAPE),
           "points": P, "lattice": list(plan.G), "segments": plan.S, "occupied_cells": cells, "iterations": ITERATIONS,
           "register_deformable": whole, "plan": plan_t, "run": dict(run, device_ms=run_dev), "run0_device_ms": run0_dev,
           "iteration_device_ms": iter_dev, "similarity_pair_device_ms": sim_dev, "resample": times, "report": report,
           "dice_affine": round(d0, 4), "dice_ffd": round(d1, 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(os.path.join(args.out, "registration_ffd_bench.json"), "w") as f:
            f.write(line + "\n")

        def fmt(s):
            return f"{s['median_ms']:.2f} ({s['min_ms']:.2f}-{s['max_ms']:.2f})"

        x = lambda s: "x".join(map(str, s))                                                              # noqa: E731
        with open(os.path.join(args.out, "registration_ffd.md"), "w") as f:
            f.write(MD.format(reps=args.reps, warmup=args.warmup, mshape=x(MOVING_SHAPE), msp=MOVING_SPACING, fshape=x(FIXED_SHAPE),
                              fsp=FIXED_SPACING, P=P, G=x(plan.G), h=CONTROL_SPACING, S=plan.S, cells=cells, it=ITERATIONS,
                              rows=ITERATIONS + 1, bound=BOUND, whole=fmt(whole), plan=fmt(plan_t), run=fmt(run), run_dev=run_dev,
                              iter_dev=iter_dev, sim_dev=sim_dev, dl=fmt(times["dl"]), al=fmt(times["al"]), df=fmt(times["df"]),
                              af=fmt(times["af"]), dl_dev=times["dl"]["device_ms"], al_dev=times["al"]["device_ms"],
                              df_dev=times["df"]["device_ms"], af_dev=times["af"]["device_ms"], r_sim=iter_dev / max(sim_dev, 1e-9),
                              r_prof=iter_dev / 0.0616, r_l=times["dl"]["device_ms"] / times["al"]["device_ms"],
                              r_f=times["df"]["device_ms"] / times["af"]["device_ms"], r_sp=times["dl"]["device_ms"] / 1.0,
                              report=report, d0=d0, d1=d1, ctl_kb=3 * plan.G[0] * plan.G[1] * plan.G[2] * 8 / 1024))


if __name__ == "__main__":
    main()
