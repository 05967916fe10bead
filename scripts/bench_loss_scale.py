#!/usr/bin/env python3
"""Cost of dynamic loss scaling: the UNet() 128^3 float16 train step replayed from a HIP graph, static vs dynamic scale.

Timed as bench.py times its graph leg: the same synthetic batch copied in and replayed each step, one device->host read of
the logged loss per step, wall clock over the timed region.  The two legs are interleaved (static, dynamic, static, ...)
so that clock drift hits both alike.  Prints one JSON line.

    python scripts/bench_loss_scale.py --steps 100 --warmup 20 --rounds 3
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd")]

import torch

from bench import synth_batch


def build(loss_scale, size, dev):
    import ctunet_amd
    from ctunet_amd import optim
    from ctunet_amd.graph import GraphedTrainStep
    torch.manual_seed(0)
    net = ctunet_amd.UNet().to(dev).train().set_precision("fp16", loss_scale=loss_scale)
    opt = optim.Adam(net.parameters(), lr=1e-4, weight_decay=0, amsgrad=True).guard(net)
    x, targets = synth_batch(size, 0, dev)
    return net, GraphedTrainStep(net, opt, x, targets, 1.0, 1.0, input_requires_grad=True), x, targets


def timed(gstep, x, targets, steps, warmup):
    for _ in range(warmup):
        gstep(x, targets).tolist()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        gstep(x, targets).tolist()[-1]
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    legs = {"static": build(None, args.size, dev), "dynamic": build("dynamic", args.size, dev)}
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, (_, gstep, x, targets) in legs.items():
            ms[name].append(timed(gstep, x, targets, args.steps, args.warmup))
    sc = legs["dynamic"][0].loss_scaler
    print(json.dumps({"metric": f"UNet() {args.size}^3 fp16 graphed train step, ms", "steps": args.steps,
                      "rounds": args.rounds, "static_ms": ms["static"], "dynamic_ms": ms["dynamic"],
                      "static_min_ms": min(ms["static"]), "dynamic_min_ms": min(ms["dynamic"]),
                      "dynamic_final_scale": sc.get_scale(), "dynamic_skipped_steps": sc.skipped_steps(),
                      "static_overflowed": legs["static"][0].overflowed()}))


if __name__ == "__main__":
    main()
