#!/usr/bin/env python3
"""Region properties at the project's usual volume, 224x512x512, against the existing one-pass integer reduction
(``preprocess.histogram``) on a tensor of the same byte size, and ``registration.register(init="moments")`` against the
centroid start.

Legs (``--legs``):
  mask     uint8 skull mask (an ellipsoid shell), R = 1                      | histogram of a uint8 tensor, same bytes
  labels   int32 map from ``label()`` of a noisy prediction, R = 4096        | histogram of a float32 tensor, same bytes
  classes  int64 class map (shell 1, inside 2, a ball 3), R = 3              | histogram of a float32 tensor, same bytes
  noise    int32 map of independent labels 0..4096, R = 4096: the spill path (no yardstick)
  register ``register`` on the skull / atlas pair of scripts/bench_registration.py with init="centroid" and init="moments"
           (wall clock: the call synchronises inside), ``principal_frame`` of both masks, and the two
           ``nonzero().mean(0)`` centroids that the moments pass replaces

Timing of the first four: each call is captured into a graph (it synchronises nowhere) and a round times --reps replays
between two events; the two legs of a pair take turns round by round; reported: the median round, the fastest and slowest,
and GB/s of the label map's bytes at the median.  Prints one JSON line.

    python scripts/bench_regionprops.py --reps 50 --rounds 9
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd"), os.path.join(ROOT, "scripts")]

import numpy as np
import torch

DIMS = (224, 512, 512)


def _rho(dev):
    z, y, x = (torch.arange(n, device=dev, dtype=torch.float32) for n in DIMS)
    q = ((z - (DIMS[0] - 1) / 2) / (0.45 * DIMS[0]))[:, None, None] ** 2 + ((y - (DIMS[1] - 1) / 2) / (0.45 * DIMS[1]))[None, :, None] ** 2 \
        + ((x - (DIMS[2] - 1) / 2) / (0.45 * DIMS[2]))[None, None, :] ** 2
    return q.sqrt()


def _graph(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    return g, keep


def _round(g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _summary(ms, nbytes):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "GB_per_s_at_median": round(nbytes / med / 1e6, 1)}


def _pair(calls, nbytes, reps, rounds):
    graphs = {k: _graph(fn) for k, fn in calls.items()}
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k in calls:
            ms[k].append(_round(graphs[k][0], reps))
    return {k: _summary(v, nbytes) for k, v in ms.items()}


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
    return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--legs", default="mask,labels,classes,noise,register")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_regionprops.py measures on the GPU; there is no CPU leg"
    from ctunet_amd import postprocess, preprocess, registration as reg
    dev = torch.device("cuda", 0)
    legs = args.legs.split(",")
    V = int(np.prod(DIMS))
    res = {"metric": "region_properties, ms per call (graph replays)", "shape": list(DIMS), "reps": args.reps,
           "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    rho = _rho(dev)
    shell = (rho <= 1.0) & (rho > 0.88)
    if "mask" in legs:
        mask = shell.to(torch.uint8)
        other = torch.randint(0, 256, DIMS, dtype=torch.uint8, device=dev)
        hist = torch.empty(256, dtype=torch.int64, device=dev)
        res["mask_foreground_share"] = round(float(mask.float().mean()), 4)
        res["mask"] = _pair({"region_properties": lambda: postprocess.region_properties(mask, 1),
                             "histogram": lambda: preprocess.histogram(other, 256, (0, 256), out=hist)}, V, args.reps, args.rounds)
    if "labels" in legs:
        noisy = shell | (torch.rand(DIMS, device=dev) < 2e-5)                # a prediction with stray islands
        labels, num = postprocess.label(noisy, connectivity=3)
        res["labels_components"] = int(num.item())
        other = torch.rand(DIMS, device=dev)
        hist = torch.empty(256, dtype=torch.int64, device=dev)
        p = postprocess.region_properties(labels, 4096)
        res["labels_overflow"] = int(p.overflow.item())
        res["labels"] = _pair({"region_properties": lambda: postprocess.region_properties(labels, 4096),
                               "histogram": lambda: preprocess.histogram(other, 256, (0.0, 1.0), out=hist)}, 4 * V, args.reps,
                              args.rounds)
        del labels, other, noisy
    if "classes" in legs:
        classes = torch.where(shell, 1, 0) + torch.where(rho <= 0.88, 2, 0)
        classes[100:130, 200:260, 200:260] = 3
        classes = classes.to(torch.int64)
        other = torch.rand((2,) + DIMS, device=dev)
        hist = torch.empty(256, dtype=torch.int64, device=dev)
        res["classes"] = _pair({"region_properties": lambda: postprocess.region_properties(classes, 3),
                                "histogram": lambda: preprocess.histogram(other, 256, (0.0, 1.0), out=hist)}, 8 * V, args.reps,
                               args.rounds)
        del classes, other
    if "noise" in legs:
        noise = torch.randint(0, 4097, DIMS, dtype=torch.int32, device=dev)
        res["noise"] = _pair({"region_properties": lambda: postprocess.region_properties(noise, 4096)}, 4 * V,
                             max(args.reps // 10, 2), args.rounds)
        del noise
    del rho, shell
    if "register" in legs:
        import bench_registration as B
        moving, fixed = B.scene(dev)
        kw = dict(moving_spacing=B.MOVING_SPACING, fixed_spacing=B.FIXED_SPACING)
        out = {}
        for init in ("centroid", "moments"):
            out[init] = _wall(lambda: reg.register(moving, fixed, init=init, **kw), 2, 7)
        r = reg.register(moving, fixed, init="moments", **kw)
        out["candidate"] = int(r.candidate)
        out["report"] = r.report()
        T, p = B.truth(), reg.surface_points(moving, B.MOVING_SPACING).cpu().numpy().astype(np.float64)
        for init in ("centroid", "moments"):
            M = reg.register(moving, fixed, init=init, **kw).matrix.cpu().numpy()
            out[f"tre_max_mm_{init}"] = round(float(np.sqrt((((p @ M[:3, :3].T + M[:3, 3]) - (p @ T[:3, :3].T + T[:3, 3])) ** 2)
                                                            .sum(1)).max()), 4)
        sm = torch.tensor(B.MOVING_SPACING, dtype=torch.float64, device=dev)
        sf = torch.tensor(B.FIXED_SPACING, dtype=torch.float64, device=dev)
        out["nonzero_mean_both_masks"] = _wall(lambda: ((torch.nonzero(moving != 0).to(torch.float64) * sm).mean(0),
                                                        (torch.nonzero(fixed != 0).to(torch.float64) * sf).mean(0)), 2, 7)
        out["principal_frame_both_masks"] = _wall(lambda: (reg.principal_frame(moving, B.MOVING_SPACING),
                                                           reg.principal_frame(fixed, B.FIXED_SPACING)), 2, 7)
        res["register"] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
