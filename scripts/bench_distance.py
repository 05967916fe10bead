#!/usr/bin/env python3
"""Distance transform and ball morphology on a whole CT-sized mask: ``postprocess.distance_transform_edt`` (with and
without indices), ``signed_distance`` and ``ball_opening(r = 2 mm)`` on a 224x512x512 uint8 skull shell built on the
device (the scene of scripts/bench_morphology.py) with the scanner's spacing (0.8, 0.45, 0.45), against
``scipy.ndimage.distance_transform_edt`` / ``binary_opening`` with the ball structure on the host on the same array, and
next to the existing ``binary_opening(iterations=4)`` for scale.

Each device leg runs --warmup untimed calls, then --reps timed calls, each ending in a device synchronise; wall clock per
call (allocation of the output and the workspace included), median and range, and next to it the device time per call of
the same number of calls issued back to back between two stream events.  "bytes_per_voxel_at_copy_rate" is that
back-to-back time x the 6.29 TB/s measured copy rate / voxels: what the call would have moved had it run at HBM speed,
an upper bound on its traffic, not a counter.  scipy is timed --scipy-reps times.  Prints one JSON line and, with
--out DIR, writes DIR/distance_bench.json.

    python scripts/bench_distance.py --reps 10 --out profiles
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd"), os.path.join(ROOT, "scripts")]

import torch

from bench_morphology import COPY_TBS, _host, _scene, _stream_ms, _time

SPACING = (0.8, 0.45, 0.45)
RADIUS = 2.0


def _ball(radius, spacing):
    import numpy as np
    ax = [np.arange(-int(radius // s), int(radius // s) + 1, dtype=np.float64) * s for s in spacing]
    zz, yy, xx = np.meshgrid(*ax, indexing="ij")
    return np.sqrt(zz * zz + yy * yy + xx * xx) <= radius


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scipy-reps", type=int, default=1)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import postprocess as pp
    dev = torch.device("cuda", 0)
    shape = (224, args.side, args.side)
    v = shape[0] * shape[1] * shape[2]
    full, _ = _scene(shape, dev)
    calls = {
        "edt_unit": lambda: pp.distance_transform_edt(full),
        "edt": lambda: pp.distance_transform_edt(full, sampling=SPACING),
        "edt_indices": lambda: pp.distance_transform_edt(full, sampling=SPACING, return_indices=True),
        "signed_distance": lambda: pp.signed_distance(full, sampling=SPACING),
        "ball_opening_2mm": lambda: pp.ball_opening(full, RADIUS, sampling=SPACING),
        "binary_opening_x4": lambda: pp.binary_opening(full, iterations=4),
    }
    res = {"metric": "distance transform / ball morphology, ms per call (wall clock, synchronised)", "reps": args.reps,
           "warmup": args.warmup, "copy_rate_tb_s": COPY_TBS, "device": torch.cuda.get_device_name(0), "shape": list(shape),
           "voxels": v, "spacing": list(SPACING), "radius": RADIUS,
           "foreground_fraction": round(float(full.float().mean()), 4),
           "workspace_mb": {"edt": round(pp.distance_workspace_bytes(1, shape) / 1e6, 2),
                            "edt_indices": round(pp.distance_workspace_bytes(1, shape, True) / 1e6, 2)},
           "device_ms": {}, "scipy_ms": {}}
    for name, fn in calls.items():
        ms = _time(fn, args.warmup, args.reps)
        b2b = _stream_ms(fn, args.reps)
        res["device_ms"][name] = {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
                                  "max_ms": round(max(ms), 3), "back_to_back_ms": round(b2b, 3),
                                  "bytes_per_voxel_at_copy_rate": round(b2b * 1e-3 * COPY_TBS * 1e12 / v, 1)}
        torch.cuda.empty_cache()
    if args.scipy_reps > 0:
        import numpy as np
        from scipy import ndimage as ndi
        hf = full.cpu().numpy() != 0
        st = _ball(RADIUS, SPACING)
        keep = {}

        def edt():
            keep["edt"] = ndi.distance_transform_edt(hf, sampling=SPACING)

        def signed():
            keep["signed"] = ndi.distance_transform_edt(~hf, sampling=SPACING) - ndi.distance_transform_edt(hf, sampling=SPACING)

        def opening():
            keep["opening"] = ndi.binary_opening(hf, st)

        for name, fn in (("edt", edt), ("signed_distance", signed), ("ball_opening_2mm", opening)):
            res["scipy_ms"][name] = round(statistics.median(_host(fn, args.scipy_reps)), 1)
        res["ball_structure_voxels"] = int(st.sum())
        d = pp.distance_transform_edt(full, sampling=SPACING).cpu().numpy()
        res["edt_max_rel_err_vs_scipy"] = float(np.max(np.abs(d - keep["edt"]) / np.maximum(keep["edt"], 1e-30) * (keep["edt"] > 0)))
        s = pp.signed_distance(full, sampling=SPACING).cpu().numpy()
        res["signed_max_rel_err_vs_scipy"] = float(np.max(np.abs(s - keep["signed"]) / np.abs(keep["signed"])))
        res["ball_opening_matches_scipy"] = bool(np.array_equal(pp.ball_opening(full, RADIUS, sampling=SPACING).cpu().numpy() != 0,
                                                                keep["opening"]))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(os.path.join(args.out, "distance_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
