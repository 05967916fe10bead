#!/usr/bin/env python3
"""Irregular defects and random dilation: GPU time per call of the fused defect pass against the hole pass it sits beside,
and of RandomDilate against postprocess.binary_dilation, at 224x304x304.

Legs (``--legs``), uint8 ellipsoid-shell skulls [N,1,D,H,W], N = 1 and 4:
  hole    FlapRecTransform(SkullRandomHole(double_output=True), SaltAndPepper(p=.5, noise_density=.05)) = flap_rec_transform
  defect  the same with SkullRandomDefect(double_output=True): count, draw, noise draw, fused apply
  dilate  RandomDilate(p=1, iterations=k) and postprocess.binary_dilation(iterations=k), k = 1, 2, 3, N = 1
Both transform legs write x [N,1,D,H,W] and two one-hot targets [N,2,D,H,W] into kept buffers and draw the same noise (same
seed).  Algorithmic bytes: the skull read twice (count, apply) + 5 float32 channels written = 22 B per voxel; dilate:
1 B read + 1 B written = 2 B per voxel.

Timing: one untimed call per leg, then --rounds rounds; a round times --reps calls of each leg between two events, the legs
taking turns, so the legs of one run see the same machine.  Reported per leg: the median round, the fastest and slowest
round (the spread) in ms per call, and GB/s at the median.  ``--legs hole`` needs nothing this module's siblings lack, so
the same script times an older checkout of the package (put it first on PYTHONPATH).  Prints one JSON line.

    python scripts/bench_defect.py --reps 20 --rounds 7
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[len(sys.path):] = [ROOT, os.path.join(ROOT, "ct-unet_amd")]      # after PYTHONPATH: an older package may shadow

import numpy as np

DIMS = (224, 304, 304)


def _skull(dims, n):
    """n binary ellipsoid shells (semi-axes 0.45 n, 12 % thick), uint8."""
    z, y, x = np.ogrid[:dims[0], :dims[1], :dims[2]]
    q = ((z - (dims[0] - 1) / 2) / (0.45 * dims[0])) ** 2 + ((y - (dims[1] - 1) / 2) / (0.45 * dims[1])) ** 2 + \
        ((x - (dims[2] - 1) / 2) / (0.45 * dims[2])) ** 2
    return np.repeat(((q <= 1.0) & (q > 0.88 ** 2)).astype(np.uint8)[None, None], n, 0)


def _timed(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _summary(ms, nbytes):
    med = statistics.median(ms)
    return {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
            "algorithmic_GB": round(nbytes / 1e9, 4), "GB_per_s_at_median": round(nbytes / med / 1e6, 1)}


def transform_legs(legs, reps, rounds):
    import torch
    from ctunet_amd import transforms as T
    out = {}
    for n in (1, 4):
        sk = torch.from_numpy(_skull(DIMS, n)).cuda()
        calls = {}
        for leg in legs:
            hole = T.SkullRandomHole(double_output=True, seed=1) if leg == "hole" else \
                T.SkullRandomDefect(double_output=True, seed=1)
            t = T.FlapRecTransform(hole, T.SaltAndPepper(p=.5, noise_density=.05, seed=2))
            x, tg = t.apply(sk)
            calls[leg] = (lambda t=t, x=x, tg=tg: t.apply(sk, x=x, targets=tg))
            if leg == "defect":
                recs = t.last_params
                box = [np.prod([h - l + 1 for l, h in zip(*r["box"])]) / np.prod(DIMS) for r in recs]
                out[f"defect_box_share_N{n}"] = [round(float(b), 4) for b in box]
        torch.cuda.synchronize()
        ms = {leg: [] for leg in legs}
        for _ in range(rounds):
            for leg in legs:
                ms[leg].append(_timed(calls[leg], reps))
        for leg in legs:
            out[f"{leg}_N{n}"] = _summary(ms[leg], 22 * n * int(np.prod(DIMS)))
    return out


def dilate_legs(reps, rounds):
    import torch
    from ctunet_amd import postprocess
    from ctunet_amd.transforms import RandomDilate
    sk = torch.from_numpy(_skull(DIMS, 1)).cuda()
    out = {}
    for k in (1, 2, 3):
        t = RandomDilate(p=1, iterations=k, seed=3)
        buf = t.apply(sk)
        ref = postprocess.binary_dilation(sk[0, 0], iterations=k)
        assert torch.equal(buf[0, 0], ref.to(torch.uint8)), k
        calls = {"random_dilate": lambda t=t: t.apply(sk, out=buf),
                 "binary_dilation": lambda k=k: postprocess.binary_dilation(sk[0, 0], iterations=k)}
        ms = {leg: [] for leg in calls}
        for _ in range(rounds):
            for leg, fn in calls.items():
                ms[leg].append(_timed(fn, reps))
        for leg in calls:
            out[f"{leg}_k{k}"] = _summary(ms[leg], 2 * int(np.prod(DIMS)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", default="hole,defect,dilate")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_defect.py measures on the GPU; there is no CPU leg"
    legs = args.legs.split(",")
    res = {"metric": "defect / hole pass and dilation, ms per call", "shape": list(DIMS), "reps": args.reps,
           "rounds": args.rounds}
    tl = [leg for leg in legs if leg in ("hole", "defect")]
    if tl:
        res.update(transform_legs(tl, args.reps, args.rounds))
    if "dilate" in legs:
        res.update(dilate_legs(args.reps, args.rounds))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
