#!/usr/bin/env python3
"""Mirrored passes, ensembles and uncertainty maps of ``predict_volume``: what the new kernels and the extra passes cost.

Workload of profiles/sliding_window.md: UNetSP, a 2 x 224 x 512 x 512 float32 volume on the GPU, patch 192, overlap 48,
batch 2 (32 tiles in 16 batches), Gaussian blend.

kernels   device-event time per launch of every variant of one kernel family, interleaved in one process: a round times
          --launches back-to-back launches of each variant in turn, --rounds rounds.  Launch i of a round works on batch
          i mod 16 of the plan (its tiles, its box), so consecutive launches touch different memory as they do inside a
          call.  Bytes are what the algorithm moves, computed from the shapes here.
            extract:    extract_patches_kernel (the tiler's gather) | the flip kernel at mask 0 | mask x | zyx
            accumulate: window_accumulate_kernel<2> | the flip kernel at mask 0 | x | zyx | + S2 | + SH | + S2 + SH
            finalize:   window_finalize_kernel<2> | the statistics kernel without statistics | each statistic | all
calls     wall clock per whole call (ending in a device synchronise) and peak memory above model + volume for 1, 2 and 8
          passes, fp32 and bf16, and for 2 passes with all three statistics; one untimed call first.

--ring N keeps the last N extraction outputs alive, so consecutive launches write different blocks (N x 113 MB; from 3
on that is more than the 256 MiB Infinity Cache) instead of the one block the caching allocator would hand back.

Prints one JSON line.

    python scripts/bench_tta.py
    python scripts/bench_tta.py --parts extract --ring 8 --launches 512      # extraction with cold writes, 17 - 60 ms windows
    python scripts/bench_tta.py --parts kernels --rounds 3 --launches 8      # (what a kernel-trace run profiles)
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

HBM_COPY_TBS = 6.3        # float4 copy on an MI355X (MI355X_MICROARCH: achievable HBM bandwidth)


def time_variants(variants, rounds, launches):
    """variants: name -> fn(i).  us per launch of each, a list over rounds; the variants alternate inside every round."""
    for fn in variants.values():                 # warm every variant on every batch: code objects, allocator
        for i in range(launches):
            fn(i)
    torch.cuda.synchronize()
    out = {n: [] for n in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(launches):
                fn(i)
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / launches)
    return out


def report(times, nbytes):
    res = {}
    for name, us in times.items():
        med = statistics.median(us)
        res[name] = {"us": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2), "mb": round(nbytes[name] / 1e6, 1),
                     "tb_per_s": round(nbytes[name] / med / 1e6, 3), "of_copy": round(nbytes[name] / med / 1e6 / HBM_COPY_TBS, 3)}
    return res


def bench_kernels(args, dev):
    from ctunet_amd import ops
    from ctunet_amd.inference import WEIGHT_FLOOR, plan_batches, tile_grid, window_tables
    shape, patch, b, k, c = tuple(args.shape), (args.patch,) * 3, args.batch, 2, 2
    tiles = tile_grid(shape, patch, (args.overlap,) * 3)
    bp = plan_batches(tiles, b, shape, patch)
    metas = torch.from_numpy(bp.meta()).to(dev)
    nb = metas.shape[0]
    coords = [metas[i, :3 * b].view(b, 3) for i in range(nb)]
    valid = [metas[i, 3 * b:4 * b] for i in range(nb)]
    box = [metas[i, 4 * b:] for i in range(nb)]
    flips = {m: torch.full((1,), m, dtype=torch.int32, device=dev) for m in (0, 1, 7)}
    g = torch.Generator().manual_seed(1)
    vol = torch.randn((c,) + shape, generator=g).to(dev)
    pv, v = patch[0] * patch[1] * patch[2], shape[0] * shape[1] * shape[2]
    res = {}

    # ---- extraction: the volume window in, the patches out
    ring = [None] * args.ring

    def keep(i, out):
        ring[i % args.ring] = out

    ext = {"extract_patches_kernel": lambda i: keep(i, ops.extract_patches(vol, coords[i % nb], patch))}
    for m, nm in ((0, "0"), (1, "x"), (7, "zyx")):
        ext[f"extract_flip_kernel mask {nm}"] = lambda i, m=m: keep(i, ops.extract_patches_flip(vol, coords[i % nb], patch,
                                                                                             flips[m]))
    if "extract" in args.parts:
        res["extract"] = report(time_variants(ext, args.rounds, args.launches), {n: 2 * b * c * pv * 4 for n in ext})
    ring[:] = [None] * args.ring
    if "accumulate" not in args.parts and "finalize" not in args.parts:
        return res

    # ---- accumulation: K + 1 accumulators read and written over the batch's box, both patches' values read
    ys = torch.softmax(torch.randn((b, k) + patch, generator=g), 1).to(dev)
    tabs = tuple(torch.from_numpy(t).to(dev) for t in window_tables(patch, "gaussian", 0.125))
    num, ws = torch.zeros((k,) + shape, device=dev), torch.zeros(shape, device=dev)
    sq, sh = torch.zeros_like(num), torch.zeros_like(ws)
    hi = np.minimum(bp.coords.max(1) + np.asarray(patch), np.asarray(shape))
    vox = float(np.prod(hi - bp.box, axis=1).mean())                                # voxels of a batch's box, mean over batches
    base = (k + 1) * 2 * 4 * vox + b * k * pv * 4

    def acc(i, m=None, s2=None, s_h=None):
        j = i % nb
        if m is None:
            ops.window_accumulate(ys, coords[j], valid[j], box[j], tabs, WEIGHT_FLOOR, bp.extent, num, ws)
        else:
            ops.window_accumulate_flip(ys, coords[j], valid[j], box[j], flips[m], tabs, WEIGHT_FLOOR, bp.extent, num, ws, s2, s_h)

    accs = {"window_accumulate_kernel<2>": (lambda i: acc(i), base),
            "accumulate_flip_kernel<2> mask 0": (lambda i: acc(i, 0), base),
            "accumulate_flip_kernel<2> mask x": (lambda i: acc(i, 1), base),
            "accumulate_flip_kernel<2> mask zyx": (lambda i: acc(i, 7), base),
            "accumulate_flip_kernel<2> mask x + S2": (lambda i: acc(i, 1, sq), base + k * 2 * 4 * vox),
            "accumulate_flip_kernel<2> mask x + SH": (lambda i: acc(i, 1, None, sh), base + 2 * 4 * vox),
            "accumulate_flip_kernel<2> mask x + S2 + SH": (lambda i: acc(i, 1, sq, sh), base + (k + 1) * 2 * 4 * vox)}
    if "accumulate" in args.parts:
        res["accumulate"] = report(time_variants({n: f for n, (f, _) in accs.items()}, args.rounds, args.launches),
                                   {n: nb_ for n, (_, nb_) in accs.items()})
        res["accumulate_box_voxels"] = vox
    if "finalize" not in args.parts:
        return res

    # ---- finalize: num and wsum in, probabilities and labels out, plus what each statistic reads and writes
    probs, lab = torch.empty_like(num), torch.empty(shape, dtype=torch.uint8, device=dev)
    var, ent, mi = torch.empty_like(num), torch.empty_like(ws), torch.empty_like(ws)
    fb = (2 * k + 1) * 4 * v + v
    fins = {"window_finalize_kernel<2>": (lambda i: ops.window_finalize(num, ws, probs, lab), fb),
            "finalize_stats_kernel<2> no statistic": (lambda i: ops.window_finalize_stats(num, ws, probs, lab), fb),
            "finalize_stats_kernel<2> entropy": (lambda i: ops.window_finalize_stats(num, ws, probs, lab, ent=ent), fb + 4 * v),
            "finalize_stats_kernel<2> variance": (lambda i: ops.window_finalize_stats(num, ws, probs, lab, sq=sq, var=var),
                                                  fb + 2 * k * 4 * v),
            "finalize_stats_kernel<2> mutual information": (lambda i: ops.window_finalize_stats(num, ws, probs, lab, sh=sh, mi=mi),
                                                            fb + 2 * 4 * v),
            "finalize_stats_kernel<2> all three": (lambda i: ops.window_finalize_stats(num, ws, probs, lab, sq, sh, var, ent, mi),
                                                   fb + (2 * k + 3) * 4 * v)}
    res["finalize"] = report(time_variants({n: f for n, (f, _) in fins.items()}, args.rounds, max(2, args.launches // 4)),
                             {n: nb_ for n, (_, nb_) in fins.items()})
    return res


def bench_calls(args, dev):
    import ctunet_amd as A
    torch.manual_seed(0)
    net = A.UNetSP().to(dev)
    shape = tuple(args.shape)
    vol = torch.randn((2,) + shape, generator=torch.Generator().manual_seed(1)).to(dev)
    stats = ("entropy", "variance", "mutual_information")
    legs = {"1 pass": dict(), "2 passes (x)": dict(flips=("x",)), "8 passes (all)": dict(flips="all"),
            "2 passes (x) + all statistics": dict(flips=("x",), uncertainty=stats),
            "1 pass + all statistics": dict(uncertainty=stats)}
    res = {}
    for prec in args.precisions.split(","):
        net.set_precision(prec)
        for name, kw in legs.items():
            def call():
                return A.predict_volume(net, vol, patch=args.patch, overlap=args.overlap, batch=args.batch, **kw)
            out = call()
            del out
            torch.cuda.synchronize()
            ms, peak = [], 0
            for _ in range(args.reps):
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                out = call()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
                peak = max(peak, torch.cuda.max_memory_allocated() - base)
                del out
            res[f"{prec} {name}"] = {"ms": [round(m, 2) for m in ms], "median_ms": round(statistics.median(ms), 2),
                                     "peak_mb": round(peak / 1e6, 1)}
            torch.cuda.empty_cache()
    net.set_precision("fp32")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(224, 512, 512))
    ap.add_argument("--patch", type=int, default=192)
    ap.add_argument("--overlap", type=int, default=48)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--parts", default="kernels,calls", help="of extract, accumulate, finalize (kernels = all three), calls")
    ap.add_argument("--ring", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precisions", default="fp32,bf16")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    res = {"metric": "predict_volume mirrored passes and statistics, UNetSP", "shape": list(args.shape), "patch": args.patch,
           "overlap": args.overlap, "batch": args.batch, "rounds": args.rounds, "launches": args.launches, "reps": args.reps}
    parts = args.parts.split(",")
    if "kernels" in parts:
        parts += ["extract", "accumulate", "finalize"]
    args.parts = parts
    res["ring"] = args.ring
    if any(p in parts for p in ("extract", "accumulate", "finalize")):
        res["kernels"] = bench_kernels(args, dev)
    if "calls" in parts:
        res["calls"] = bench_calls(args, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
