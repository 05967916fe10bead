#!/usr/bin/env python3
"""Forward + backward time of the loss kernels on one [1,2,S,S,S] map: the plain CE + Dice pair (ctu_loss_fwd / ctu_loss_bwd)
against the loss family (ctu_seg_loss_fwd / ctu_seg_loss_bwd) with class weights alone, weights + focal, + Tversky, + the
boundary map.

Per case: ``--warmup`` untimed forward + backward pairs, then ``--rounds`` windows of ``--reps`` pairs issued back to back
between two stream events; the figure is the device time per pair, median (min - max) over the windows.  The cases are
interleaved inside each round, so that a drift of the machine hits all of them alike.  The output buffers are allocated once
outside the windows (``out=`` for the gradient; the workspace and the terms are small torch.empty calls inside).  Bytes are
the ones the algorithm needs: 16 B / voxel forward (20 with the map), 24 B / voxel backward (28).  Needs a GPU.

    python scripts/bench_loss_family.py [--sizes 128 256] [--out profiles]      # one JSON line per case and size
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ct-unet_amd"))

CASES = ("plain", "weights", "weights_focal", "weights_focal_tversky", "all_with_phi")


def make_case(name, ops, p, t, phi, g, sm):
    if name == "plain":
        def run():
            _, ws = ops.loss_fwd(p, t, 1.0, 1.0, sm)
            ops.loss_bwd(p, t, 1.0, 1.0, sm, ws, None, None, g)
        return run
    lam = dict(weights=(1.0, 1.0, 0.0, 0.0), weights_focal=(1.0, 1.0, 0.0, 0.0), weights_focal_tversky=(1.0, 1.0, 1.0, 0.0),
               all_with_phi=(1.0, 1.0, 1.0, 0.1))[name]
    kw = dict(class_weight=(0.2, 0.8), focal_gamma=0.0 if name == "weights" else 2.0, tversky_ab=(0.3, 0.7),
              boundary=phi if lam[3] else None)

    def run():
        _, ws = ops.seg_loss_fwd(p, t, lam, sm, **kw)
        ops.seg_loss_bwd(p, t, lam, sm, ws, out=g, **kw)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--softmax-view", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_loss_family: needs a GPU")
    from ctunet_amd import ops
    sm = bool(a.softmax_view)
    lines = []
    for s in a.sizes:
        gen = torch.Generator().manual_seed(s)
        v = s ** 3
        p = (torch.randn(1, 2, s, s, s, generator=gen) * 2.0).cuda()
        m = (torch.rand(1, s, s, s, generator=gen) < 0.01).long()
        t = torch.nn.functional.one_hot(m, 2).movedim(4, 1).float().contiguous().cuda()
        phi = (torch.randn(1, s, s, s, generator=gen) * 5.0).cuda()
        g = torch.empty_like(p)
        runs = {name: make_case(name, ops, p, t, phi, g, sm) for name in CASES}
        for run in runs.values():
            for _ in range(a.warmup):
                run()
        torch.cuda.synchronize()
        ms = {name: [] for name in CASES}
        for _ in range(a.rounds):
            for name, run in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    run()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.reps)
        for name in CASES:
            nbytes = v * ((16 + 24) + (8 if name == "all_with_phi" else 0))
            med = statistics.median(ms[name])
            lines.append(dict(case=name, size=s, softmax_view=sm, ms_median=round(med, 5), ms_min=round(min(ms[name]), 5),
                              ms_max=round(max(ms[name]), 5), bytes=nbytes, tb_per_s=round(nbytes / med / 1e9, 3),
                              reps=a.reps, rounds=a.rounds))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "loss_family_bench.json"), "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
