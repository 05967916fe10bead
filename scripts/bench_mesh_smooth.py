#!/usr/bin/env python3
"""Mesh smoothing at the project's usual volume: ``mesh.adjacency`` and ``mesh.smooth`` on the surface of a skull-like shell
of 224x512x512 voxels at spacing (0.8, 0.45, 0.45) (the uint8 mask of ``scripts/bench_mesh.py``).

Times are HIP events around the calls on the current stream (--warmup untimed calls, then --reps timed ones, the median
reported).  ``adjacency`` synchronises once inside the call, so its figure includes that round trip.  The time per step is
the difference between a 10-iteration and a 1-iteration Taubin call over their 18 extra steps, which leaves out the staging
pass and the launch of the call itself.  A step moves by construction 16 V bytes of staged positions in, 4 (V + 1) + 4 E
bytes of table in and 16 V out (12 V for the last step); the neighbour gathers are counted once (16 V, the cache's part),
not per use.  The issue's floor of about 48 V bytes (12 V + 4 E + 12 V at E = 6 V, packed positions) at the 8 TB/s peak is
reported next to it.  Nothing here is read from hardware counters.

The comparison is the same rule written with torch on the same device, as a user would otherwise write it: the directed
edge list from the faces, made unique, ``index_add_`` of the neighbour positions and a division by the degree (float32, but
the sum order is not fixed, so it is not bit-equal).  Prints one JSON line and, with --out DIR, writes DIR/mesh_smooth.md.

    python scripts/bench_mesh_smooth.py --reps 20 --out profiles
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd"), os.path.join(ROOT, "scripts")]

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


def torch_edges(m):
    """(src, dst, degree) of the unique directed edges: the table a user would build with torch."""
    f = m.faces.long()
    V = m.vertices.shape[0]
    a = torch.cat([f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2], f[:, 0]])
    b = torch.cat([f[:, 1], f[:, 0], f[:, 2], f[:, 1], f[:, 0], f[:, 2]])
    key = torch.unique(a * V + b)
    src, dst = key // V, key % V
    return src, dst, torch.bincount(src, minlength=V).to(torch.float32).clamp_(min=1).unsqueeze(1)


def torch_smooth(v, src, dst, deg, iterations, lamb, mu):
    for _ in range(iterations):
        for s in (lamb, mu):
            acc = torch.zeros_like(v).index_add_(0, src, v[dst])
            v = v + s * (acc / deg - v)
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import mesh
    dev = torch.device("cuda", 0)
    r = _radius(dev)
    vol = ((r <= 1.0) & (r >= 0.93)).to(torch.uint8)
    del r
    m = mesh.extract_surface(vol, spacing=SPACING)
    del vol
    V, F = m.vertices.shape[0], m.faces.shape[0]
    adj = mesh.adjacency(m)
    E = adj.neighbours.shape[0]
    deg = (adj.offsets[1:] - adj.offsets[:-1])
    res = {"metric": "mesh smoothing, ms (HIP events, median)", "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "spacing": list(SPACING), "V": V, "F": F, "E": E,
           "valence_min_max": [int(deg.min()), int(deg.max())],
           "adjacency_workspace_bytes": int(mesh._lib.load().ctu_mesh_adjacency_ws_bytes(V, F)),
           "smooth_workspace_bytes": int(mesh._lib.load().ctu_mesh_smooth_ws_bytes(V))}
    res["adjacency"] = _time(lambda: mesh.adjacency(m), args.warmup, args.reps)
    res["smooth_10_prebuilt"] = _time(lambda: mesh.smooth(m, adjacency=adj), args.warmup, args.reps)
    res["smooth_1_prebuilt"] = _time(lambda: mesh.smooth(m, 1, adjacency=adj), args.warmup, args.reps)
    res["smooth_10_with_build"] = _time(lambda: mesh.smooth(m), args.warmup, args.reps)
    step_ms = (res["smooth_10_prebuilt"]["median_ms"] - res["smooth_1_prebuilt"]["median_ms"]) / 18.0
    step_bytes = 16 * V + 4 * (V + 1) + 4 * E + 16 * V + 16 * V
    res["step"] = {"ms": round(step_ms, 5), "bytes_by_construction": step_bytes,
                   "achieved_tb_s": round(step_bytes / (step_ms * 1e-3) / 1e12, 3),
                   "floor_48V_bytes": 48 * V, "floor_ms_at_8_tb_s": round(48 * V / (PEAK_TBS * 1e12) * 1e3, 5),
                   "ms_at_measured_copy_rate": round(step_bytes / (COPY_TBS * 1e12) * 1e3, 5)}
    src, dst, tdeg = torch_edges(m)
    res["torch_index_add"] = {"edges": _time(lambda: torch_edges(m), 1, max(3, args.reps // 4)),
                              "smooth_10": _time(lambda: torch_smooth(m.vertices, src, dst, tdeg, 10, 0.5, -0.53), args.warmup, args.reps)}
    ours, theirs = mesh.smooth(m, adjacency=adj).vertices, torch_smooth(m.vertices, src, dst, tdeg, 10, 0.5, -0.53)
    res["torch_index_add"]["max_abs_difference_mm"] = float((ours - theirs).abs().max())
    res["torch_index_add"]["smooth_10_over_ours"] = round(res["torch_index_add"]["smooth_10"]["median_ms"] / res["smooth_10_prebuilt"]["median_ms"], 2)
    (a0, v0), (a1, v1) = mesh.measure(m).tolist(), mesh.measure(mesh.Mesh(ours, m.faces)).tolist()
    res["area_ratio"], res["volume_ratio"] = round(a1 / a0, 5), round(v1 / v0, 5)
    line = json.dumps(res)
    print(line)
    if args.out:
        st, ti = res["step"], res["torch_index_add"]
        with open(os.path.join(args.out, "mesh_smooth.md"), "w") as fh:
            fh.write(f"""# Mesh smoothing on the MI355X (`scripts/bench_mesh_smooth.py`)

Surface of the skull-like shell mask of `scripts/bench_mesh.py`, {SHAPE[0]}x{SHAPE[1]}x{SHAPE[2]} at spacing {SPACING}: V = {V},
F = {F}, E = {E} (= 3F: {E == 3 * F}), valence {res['valence_min_max'][0]}..{res['valence_min_max'][1]}.  HIP events, {args.warmup} warm-up calls,
median of {args.reps} (min .. max).  Device: {res['device']}.

| call | median ms | min .. max |
|---|---|---|
| `adjacency(m)` (build, one host synchronisation, emit) | {res['adjacency']['median_ms']} | {res['adjacency']['min_ms']} .. {res['adjacency']['max_ms']} |
| `smooth(m, adjacency=a)`, 10 iterations = 20 steps + staging | {res['smooth_10_prebuilt']['median_ms']} | {res['smooth_10_prebuilt']['min_ms']} .. {res['smooth_10_prebuilt']['max_ms']} |
| `smooth(m, 1, adjacency=a)`, 2 steps + staging | {res['smooth_1_prebuilt']['median_ms']} | {res['smooth_1_prebuilt']['min_ms']} .. {res['smooth_1_prebuilt']['max_ms']} |
| `smooth(m)`, table built inside | {res['smooth_10_with_build']['median_ms']} | {res['smooth_10_with_build']['min_ms']} .. {res['smooth_10_with_build']['max_ms']} |
| torch `index_add_` form, 10 iterations (edge list prebuilt) | {ti['smooth_10']['median_ms']} | {ti['smooth_10']['min_ms']} .. {ti['smooth_10']['max_ms']} |
| torch edge list (`cat`, `unique`, `bincount`) | {ti['edges']['median_ms']} | {ti['edges']['min_ms']} .. {ti['edges']['max_ms']} |

One step: {st['ms']} ms ((10 iterations - 1 iteration) / 18).  By construction it moves {st['bytes_by_construction']} bytes (staged
positions 16 V in and out, the gathers counted once as 16 V, the table 4 (V + 1) + 4 E): {st['achieved_tb_s']} TB/s achieved; the
same bytes at the measured copy rate of {COPY_TBS} TB/s take {st['ms_at_measured_copy_rate']} ms.  The floor of 48 V = {st['floor_48V_bytes']}
bytes at the 8 TB/s peak is {st['floor_ms_at_8_tb_s']} ms.  The torch form takes {ti['smooth_10_over_ours']} times as long for 10 iterations and differs by at
most {ti['max_abs_difference_mm']:.3g} mm (its sum order is not fixed).  After 10 iterations the area is {res['area_ratio']} and the
enclosed volume {res['volume_ratio']} of the unsmoothed mesh's.

Workspace: adjacency build {res['adjacency_workspace_bytes']} bytes, smoothing {res['smooth_workspace_bytes']} bytes.

Not read from counters, hence unmeasured: the cache hit rate of the neighbour gathers, the bytes that actually reach HBM,
and the per-kernel split of `adjacency` (count, scans, fill, sort, emit).
""")


if __name__ == "__main__":
    main()
