#!/usr/bin/env python3
"""Optimizer step alone on UNet()'s parameter set: optim.SGD / optim.RMSprop against torch.optim's foreach path.

Every parameter gets a fixed random gradient; nothing else runs.  Two ways of issuing the step are timed with device
events around `--steps` steps: eagerly (what a hand-written loop pays: host work included, whichever of host and device is
slower) and replayed from a captured graph (the device time of the launches alone; torch.optim.RMSprop needs
capturable=True for that).  The legs alternate within each round; per leg the median per-step time and the spread
(max - min) over the rounds are reported.  Prints one JSON line and, with --md, writes the table.

    python scripts/bench_optimizers.py --steps 200 --warmup 20 --rounds 7 --md profiles/optimizers.md
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd")]

import torch

LEGS = {
    "sgd": ("optim.SGD(momentum=0.9)", lambda O, ps: O.SGD(ps, lr=1e-3, momentum=0.9)),
    "sgd_torch": ("torch.optim.SGD(momentum=0.9, foreach=True)",
                  lambda O, ps: torch.optim.SGD(ps, lr=1e-3, momentum=0.9, foreach=True)),
    "rms": ("optim.RMSprop(momentum=0.9)", lambda O, ps: O.RMSprop(ps, lr=1e-3, momentum=0.9)),
    "rms_torch": ("torch.optim.RMSprop(momentum=0.9, foreach=True, capturable=True)",
                  lambda O, ps: torch.optim.RMSprop(ps, lr=1e-3, momentum=0.9, foreach=True, capturable=True)),
    "adam": ("optim.Adam(amsgrad=True), for scale", lambda O, ps: O.Adam(ps, lr=1e-3, amsgrad=True)),
}


def build(leg, dev):
    import ctunet_amd
    from ctunet_amd import optim
    torch.manual_seed(0)
    ps = [p.detach().clone().requires_grad_(True) for p in ctunet_amd.UNet().to(dev).parameters()]
    g = torch.Generator(device=dev).manual_seed(1)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g, device=dev) * 1e-3
    opt = LEGS[leg][1](optim, ps)
    for _ in range(3):                                  # state, step counter: in place before the capture
        opt.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):
            opt.step()
    except Exception as e:                             # reported as "not measured"
        print(f"{leg}: no graph ({type(e).__name__}: {e})", file=sys.stderr)
        graph = None
    return opt, graph, ps


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps * 1e3              # microseconds per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--md", default=None, help="write the table to this markdown file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_optimizers.py measures on the GPU; there is none")
    dev = torch.device("cuda", 0)
    legs = {k: build(k, dev) for k in args.legs.split(",")}
    eager, graphed = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, (opt, graph, _) in legs.items():
            eager[k].append(timed(opt.step, args.steps, args.warmup))
        for k, (opt, graph, _) in legs.items():
            if graph is not None:
                graphed[k].append(timed(graph.replay, args.steps, args.warmup))
    ps = next(iter(legs.values()))[2]
    n, floats = len(ps), sum(p.numel() for p in ps)
    res = {"metric": "optimizer step on UNet()'s parameters, microseconds per step", "tensors": n, "floats": floats,
           "steps": args.steps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "fused_launches_per_step": 1 + -(-n // 64)}

    def stat(v):
        return None if not v else {"us": [round(t, 2) for t in v], "median_us": round(statistics.median(v), 2),
                                   "spread_us": round(max(v) - min(v), 2)}
    for k in legs:
        res[k] = {"what": LEGS[k][0], "eager": stat(eager[k]), "graph": stat(graphed[k])}
    print(json.dumps(res))
    if args.md:
        def cell(s):
            return "not measured | " if s is None else f"{s['median_us']:.2f} | {s['spread_us']:.2f}"
        rows = ["| leg | optimizer | eager median us | eager spread us | graph median us | graph spread us |",
                "|---|---|---|---|---|---|"]
        rows += [f"| {k} | {LEGS[k][0]} | {cell(res[k]['eager'])} | {cell(res[k]['graph'])} |" for k in legs]
        with open(args.md, "w") as f:
            f.write(f"# Optimizer step alone: {n} tensors, {floats} floats (UNet())\n\n`scripts/bench_optimizers.py --steps "
                    f"{args.steps} --warmup {args.warmup} --rounds {args.rounds}` on {res['device']}; device events around "
                    f"{args.steps} steps, legs alternate within each round, spread = max - min over the rounds.\n\n"
                    + "\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
