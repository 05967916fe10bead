#!/usr/bin/env python3
"""Voxelisation at a scan's own grid: ``mesh.voxelize`` onto 224x304x304 at spacing (0.8, 0.45, 0.45) of (a) the extracted
and Taubin-smoothed surface of a skull-like shell on that grid (millions of sub-voxel faces: the per-lane scatter path) and
(b) a 12-triangle cube spanning most of the grid (every face covers about 5 * 10^4 rows: the wave-cooperative path).

Times are HIP events around the call on the current stream (--warmup untimed calls, then --reps timed ones, the median
reported); the call reads its refused-face count, so each figure includes that one round trip to the host.  By construction a
call moves 4 bytes per voxel for the clear, 4 for the scan's read and 1 for its write (4 for ``winding_number``): the 9 bytes
per voxel floor, reported at the 6.29 TB/s measured copy rate and at the 8 TB/s peak; the scatter reads 12 bytes per face and
its gathered vertices and adds one int32 per crossing.  Per-kernel times come from a kernel trace of this script in a run of
its own (``rocprofv3 --kernel-trace --stats -- python scripts/bench_voxelize.py --reps 3 --warmup 1``).  Prints one JSON
line and, with --out DIR, writes DIR/voxelize_bench.json.

    python scripts/bench_voxelize.py --reps 20 --out profiles
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd")]

import torch

PEAK_TBS, COPY_TBS = 8.0, 6.29
SHAPE, SPACING = (224, 304, 304), (0.8, 0.45, 0.45)


def _time(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def shell(dev):
    """The ellipsoidal shell 0.93 <= r <= 1 of scripts/bench_mesh.py on SHAPE, uint8."""
    d, h, w = SHAPE
    zz = torch.arange(d, device=dev, dtype=torch.float32).view(-1, 1, 1)
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(1, -1, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, -1)
    r = (((zz - d / 2) / (0.45 * d)) ** 2 + ((yy - h / 2) / (0.46 * h)) ** 2 + ((xx - w / 2) / (0.44 * w)) ** 2).sqrt()
    return ((r <= 1.0) & (r >= 0.93)).to(torch.uint8)


def cube(dev):
    """12 triangles, corners a tenth of the grid's extent from its border, wound outward."""
    from ctunet_amd import mesh
    lo = [0.1 * (n - 1) * s for n, s in zip(SHAPE, SPACING)]
    hi = [0.9 * (n - 1) * s for n, s in zip(SHAPE, SPACING)]
    v = torch.tensor([[(lo, hi)[z][0], (lo, hi)[y][1], (lo, hi)[x][2]] for z in (0, 1) for y in (0, 1) for x in (0, 1)],
                     dtype=torch.float32, device=dev)
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3)]
    f = torch.tensor([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=torch.int32, device=dev)
    return mesh.Mesh(v, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import mesh
    dev = torch.device("cuda", 0)
    vol = shell(dev)
    raw = mesh.extract_surface(vol, spacing=SPACING)
    smoothed = mesh.smooth(raw)
    box = cube(dev)
    voxels = SHAPE[0] * SHAPE[1] * SHAPE[2]
    res = {"metric": "mesh voxelisation, ms per call (HIP events, median)", "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "spacing": list(SPACING), "voxels": voxels,
           "V": raw.vertices.shape[0], "F": raw.faces.shape[0], "workspace_bytes": mesh.voxelize_workspace_bytes(SHAPE),
           "floor_bytes_9_per_voxel": 9 * voxels,
           "floor_ms_at_copy_rate": round(9 * voxels / (COPY_TBS * 1e12) * 1e3, 4),
           "floor_ms_at_peak": round(9 * voxels / (PEAK_TBS * 1e12) * 1e3, 4)}
    # what the round trip must give, checked at the size that is timed
    back = mesh.voxelize(raw, SHAPE, spacing=SPACING)
    res["round_trip_equal"] = bool(torch.equal(back, vol))
    w = mesh.winding_number(smoothed, SHAPE, spacing=SPACING)
    res["smoothed_winding_min_max"] = [int(w.min()), int(w.max())]
    res["smoothed_voxels"], res["mask_voxels"] = int((w != 0).sum()), int(vol.sum())
    res["cube_voxels"] = int(mesh.voxelize(box, SHAPE, spacing=SPACING).sum())
    del back, w
    res["extracted_shell"] = _time(lambda: mesh.voxelize(raw, SHAPE, spacing=SPACING), args.warmup, args.reps)
    res["smoothed_shell"] = _time(lambda: mesh.voxelize(smoothed, SHAPE, spacing=SPACING), args.warmup, args.reps)
    res["smoothed_shell_winding"] = _time(lambda: mesh.winding_number(smoothed, SHAPE, spacing=SPACING), args.warmup, args.reps)
    res["cube_12_triangles"] = _time(lambda: mesh.voxelize(box, SHAPE, spacing=SPACING), args.warmup, args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(os.path.join(args.out, "voxelize_bench.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
