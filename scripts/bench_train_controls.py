#!/usr/bin/env python3
"""Cost of the device-resident train controls: the UNet() 128^3 fp32 train step replayed from a HIP graph in five legs.

    a  optim.Adam as today (device_lr=False): the step bench.py measures
    b  device_lr=True
    c  b + max_grad_norm clipping
    d  c + lr_scheduler.ReduceLROnPlateau stepped inside the graph
    h  a + torch.optim.lr_scheduler.ReduceLROnPlateau stepped per batch on the host (what users have today: the schedule
       edits group["lr"], which the captured step never reads, and float(loss) waits for the device every step)

Timed as bench.py times its graph leg: the same synthetic batch copied in and replayed each step, one device->host read of
the logged loss per step, wall clock over the timed region.  The legs alternate (a, b, c, d, h, a, ...) so that clock drift
hits all alike; per leg the median and the spread (max - min) over the rounds are reported.  Prints one JSON line and,
with --md, writes the table.

    python scripts/bench_train_controls.py --steps 100 --warmup 20 --rounds 5 --md profiles/train_controls.md
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

from bench import synth_batch

LEGS = {"a": "device_lr=False (today's step)", "b": "device_lr", "c": "device_lr + clipping",
        "d": "device_lr + clipping + in-graph plateau scheduler", "h": "today's step + torch ReduceLROnPlateau on the host"}


def build(leg, size, dev):
    import ctunet_amd
    from ctunet_amd import lr_scheduler, optim
    from ctunet_amd.graph import GraphedTrainStep
    torch.manual_seed(0)
    net = ctunet_amd.UNet().to(dev).train()
    kw = {} if leg in "ah" else dict(device_lr=True)
    if leg in "cd":
        kw["max_grad_norm"] = 1.0
    opt = optim.Adam(net.parameters(), lr=1e-4, weight_decay=0, amsgrad=True, **kw)
    sched = lr_scheduler.ReduceLROnPlateau(opt) if leg == "d" else None
    x, targets = synth_batch(size, 0, dev)
    gstep = GraphedTrainStep(net, opt, x, targets, 1.0, 1.0, input_requires_grad=True, scheduler=sched)
    host = torch.optim.lr_scheduler.ReduceLROnPlateau(opt) if leg == "h" else None
    return gstep, x, targets, host


def timed(gstep, x, targets, host, steps, warmup):
    def one():
        values = gstep(x, targets)
        if host is not None:
            host.step(values[-1])                  # float(loss): the per-batch host sync of the reference's loop
        return values.tolist()[-1]
    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--legs", default="abcdh")
    ap.add_argument("--md", default=None, help="write the table to this markdown file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    legs = {k: build(k, args.size, dev) for k in args.legs}
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, leg in legs.items():
            ms[name].append(timed(*leg, args.steps, args.warmup))
    res = {"metric": f"UNet() {args.size}^3 fp32 graphed train step, ms", "steps": args.steps, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0)}
    for k, v in ms.items():
        res[k] = {"what": LEGS[k], "ms": [round(t, 4) for t in v], "median_ms": round(statistics.median(v), 4),
                  "spread_ms": round(max(v) - min(v), 4)}
    print(json.dumps(res))
    if args.md:
        base = res.get("a")
        rows = ["| leg | variant | median ms | spread (max - min) ms | median - a, ms |", "|---|---|---|---|---|"]
        for k in ms:
            d = "" if base is None or k == "a" else f"{res[k]['median_ms'] - base['median_ms']:+.4f}"
            rows.append(f"| {k} | {LEGS[k]} | {res[k]['median_ms']:.4f} | {res[k]['spread_ms']:.4f} | {d} |")
        with open(args.md, "w") as f:
            f.write(f"# Device-resident train controls: {res['metric']}\n\n`scripts/bench_train_controls.py --steps {args.steps} "
                    f"--warmup {args.warmup} --rounds {args.rounds}` on {res['device']}; legs alternate within each round.\n\n"
                    + "\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
