#!/usr/bin/env python3
"""Whole-volume sliding-window inference: ``predict_volume`` on a 224x512x512 two-channel volume with UNetSP, patch 192,
overlap 48, batch 2 (2 x 4 x 4 = 32 tiles), Gaussian blend, labels on.

Legs: fp32 / bf16, eager / graph=True.  Each leg runs one untimed call first (code objects, packed weights, and for the
graph leg the capture), then --reps timed calls, each ending in a device synchronise; wall clock per call.  Peak device
memory is torch.cuda.max_memory_allocated over one call, less what was allocated before it (the model and the volume).
Prints one JSON line.

    python scripts/bench_predict.py --reps 3
    python scripts/bench_predict.py --legs bf16-eager --reps 1      # (the leg a kernel-trace run profiles)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(224, 512, 512))
    ap.add_argument("--patch", type=int, default=192)
    ap.add_argument("--overlap", type=int, default=48)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="fp32-eager,fp32-graph,bf16-eager,bf16-graph")
    args = ap.parse_args()
    import ctunet_amd as A
    from ctunet_amd.inference import tile_grid
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = A.UNetSP().to(dev)
    shape = tuple(args.shape)
    vol = torch.randn((2,) + shape, generator=torch.Generator().manual_seed(1)).to(dev)
    nvox = shape[0] * shape[1] * shape[2]
    tiles = tile_grid(shape, (args.patch,) * 3, (args.overlap,) * 3).shape[0]
    res = {"metric": "predict_volume UNetSP, ms per call", "shape": list(shape), "patch": args.patch,
           "overlap": args.overlap, "batch": args.batch, "tiles": tiles, "reps": args.reps, "legs": {}}
    for leg in args.legs.split(","):
        prec, mode = leg.split("-")
        net.set_precision(prec)
        graph = mode == "graph"

        def call():
            return A.predict_volume(net, vol, patch=args.patch, overlap=args.overlap, batch=args.batch, graph=graph)
        out = call()
        del out
        torch.cuda.synchronize()
        ms = []
        peak = 0
        for _ in range(args.reps):
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            out = call()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            peak = max(peak, torch.cuda.max_memory_allocated() - base)
            del out
        med = statistics.median(ms)
        res["legs"][leg] = {"ms": [round(m, 2) for m in ms], "median_ms": round(med, 2),
                            "voxels_per_s": round(nvox / (med / 1e3)), "ms_per_tile": round(med / tiles, 3),
                            "peak_mb": round(peak / 1e6, 1)}
        net.__dict__.pop("_window_graph", None)          # free the leg's capture before the next leg
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
