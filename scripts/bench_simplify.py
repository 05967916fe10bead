#!/usr/bin/env python3
"""Mesh decimation at the project's usual volume: ``simplify.decimate`` on the smoothed surface of the skull-like shell of
224x512x512 voxels at spacing (0.8, 0.45, 0.45) (the uint8 mask of ``scripts/bench_mesh.py``), with cells of 1, 2 and 3
voxels (``cell_size = k * spacing``).

Times are HIP events around the whole call on the current stream (--warmup untimed calls, then --reps timed ones, the
median reported); a call synchronises with the host twice and allocates its workspace, and the figure includes both.  Per
cell size the script reports V and F before and after, the bytes of the binary STL (84 + 50 F), the change of the
enclosed volume (``mesh.measure``) and HD / ASSD between the decimated and the undecimated mesh
(``metrics.mesh_surface_metrics``).  There is no earlier timing to compare with, so each time is set against two
baselines: the numpy restatement ``tests/simplify_ref.py`` on the same mesh on the host (one run, wall clock), and the time
to stream the call's algorithmic bytes once (vertices and faces in, vertices and faces out: 12 V + 12 F + 12 V' + 12 F')
at the 8 TB/s HBM peak and at the 6.29 TB/s a device-to-device copy reaches.  Which pass dominates is read from a kernel
trace of this script taken in a run of its own (``rocprofv3 --kernel-trace --stats -- python scripts/bench_simplify.py
--reps 5 --no-reference``); nothing here is read from hardware counters.  Prints one JSON line and, with --out DIR, writes
it to DIR/simplify_bench.json; ``profiles/simplify.md`` is written from it.

    python scripts/bench_simplify.py --reps 20 --out profiles
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import torch

from bench_mesh import SHAPE, SPACING, _radius

PEAK_TBS, COPY_TBS = 8.0, 6.29


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cells", type=float, nargs="+", default=[1.0, 2.0, 3.0], help="cell sizes in voxels")
    ap.add_argument("--no-reference", action="store_true", help="skip the numpy restatement on the host (tens of seconds)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import mesh, metrics, simplify
    dev = torch.device("cuda", 0)
    r = _radius(dev)
    vol = ((r <= 1.0) & (r >= 0.93)).to(torch.uint8)
    del r
    m = mesh.smooth(mesh.extract_surface(vol, spacing=SPACING))
    del vol
    V, F = m.vertices.shape[0], m.faces.shape[0]
    area0, vol0 = mesh.measure(m).tolist()
    grid0 = mesh.build_face_grid(m)
    res = {"metric": "mesh decimation, ms per call (HIP events, median; two host synchronisations inside)", "reps": args.reps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "spacing": list(SPACING),
           "V": V, "F": F, "stl_bytes": 84 + 50 * F, "area_mm2": area0, "volume_mm3": vol0, "cells": []}
    if not args.no_reference:
        import simplify_ref
        hv, hf = m.vertices.cpu().numpy(), m.faces.cpu().numpy()
    for k in args.cells:
        cell = tuple(k * s for s in SPACING)
        out, index = simplify.decimate(m, cell, return_map=True)
        nv, nf = out.vertices.shape[0], out.faces.shape[0]
        lo, hi = m.vertices.min(dim=0).values.tolist(), m.vertices.max(dim=0).values.tolist()
        n = simplify._cells(lo, hi, [simplify._f32(c) for c in cell])
        row = {"voxels": k, "cell_size_mm": [round(c, 4) for c in cell], "grid": n, "V_out": nv, "F_out": nf,
               "stl_bytes": 84 + 50 * nf, "stl_ratio": round((84 + 50 * F) / (84 + 50 * nf), 2),
               "workspace_bytes": simplify.workspace_bytes(V, F, n[0] * n[1] * n[2])}
        row["call"] = _time(lambda: simplify.decimate(m, cell), args.warmup, args.reps)
        row["call_with_map"] = _time(lambda: simplify.decimate(m, cell, return_map=True), args.warmup, args.reps)
        row["call_cancel_off"] = _time(lambda: simplify.decimate(m, cell, cancel=False), args.warmup, args.reps)
        nf_off = simplify.decimate(m, cell, cancel=False).faces.shape[0]
        row["faces_cancelled"] = nf_off - nf
        stream_bytes = 12 * V + 12 * F + 12 * nv + 12 * nf
        row["stream_bytes"] = stream_bytes
        row["stream_ms_at_8_tb_s"] = round(stream_bytes / (PEAK_TBS * 1e12) * 1e3, 5)
        row["stream_ms_at_copy_rate"] = round(stream_bytes / (COPY_TBS * 1e12) * 1e3, 5)
        row["call_over_stream_at_copy_rate"] = round(row["call"]["median_ms"] / row["stream_ms_at_copy_rate"], 1)
        area1, vol1 = mesh.measure(out).tolist()
        row["area_ratio"], row["volume_ratio"] = round(area1 / area0, 5), round(vol1 / vol0, 6)
        sm = metrics.mesh_surface_metrics(out, m, grid_b=grid0)
        row["hd_mm"], row["hd95_mm"], row["assd_mm"] = (round(float(sm[key]), 4) for key in ("hd", "hd_p", "assd"))
        d = mesh.point_distance(m.vertices, out)
        row["input_vertices_to_output_surface_max_mm"] = round(float(d.max()), 4)
        if not args.no_reference:
            t0 = time.perf_counter()
            rv, rf, rmap = simplify_ref.decimate(hv, hf, cell)
            row["numpy_reference_s"] = round(time.perf_counter() - t0, 2)
            row["numpy_over_call"] = round(row["numpy_reference_s"] * 1e3 / row["call_with_map"]["median_ms"], 1)
            row["bit_equal_to_reference"] = bool((out.vertices.cpu().numpy().view("u4") == rv.view("u4")).all()
                                                 and (out.faces.cpu().numpy() == rf).all() and (index.cpu().numpy() == rmap).all())
        print(json.dumps(row), file=sys.stderr, flush=True)
        res["cells"].append(row)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(os.path.join(args.out, "simplify_bench.json"), "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
