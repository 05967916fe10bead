#!/usr/bin/env python3
"""Flap-reconstruction augmentation: GPU time per sample of the fused transform (``FlapRecTransform`` with an atlas,
float32 skull, batch 1 -> float32 input [1,2,D,H,W] + two one-hot targets), against a NumPy restatement of the
reference's host transform (np.argwhere over the skull, the float64 np.indices grid and 2-norm of utilities.shape_3d,
two float64 uniform noise fields), and the UNetSP bf16 train step at 224x304x304 for scale.

GPU legs: one untimed call, then --reps calls between two events; per-call time = elapsed / reps (kernel-bound, the host
enqueue of three launches overlaps).  GB/s over the algorithmic bytes: the skull read twice (count, apply), the atlas
read once, x (2 channels) and both targets written once = 36 B per voxel for a float32 skull.
CPU legs ("port": this restatement, not the reference's code): one sample in one process, and --procs processes
working on --procs samples at once (time per sample = wall / samples).  Prints one JSON line.

    python scripts/bench_augment.py --reps 20 --procs 16
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd")]

import numpy as np

SIZES = [(64, 128, 128), (224, 304, 304), (224, 512, 512)]


def host_transform(skull, seed):
    """The reference's flap_rec_transform restated in NumPy for one sample (sphere hole, noise always applied)."""
    rng = np.random.RandomState(seed)
    img = skull.astype(np.uint8)
    pixels = np.argwhere(img > 0)
    centre = pixels[rng.choice(pixels.shape[0])]
    min_r = np.min(img.shape) // 5 - 1
    size = rng.randint(min_r, np.max([min_r, np.max(img.shape) // 3.5]))
    dist = np.linalg.norm(np.subtract(np.indices(img.shape).T, np.asarray(centre)), axis=3, ord=2)
    shape_np = (1 - np.ones(img.shape).T * (dist <= size)).T
    brk = np.logical_and(img, shape_np).astype(np.uint8)
    flap = np.logical_and(img, 1 - shape_np).astype(np.uint8)
    nd = rng.uniform(0, 0.05)
    black = (rng.uniform(0, 1, brk.shape) > nd * 0.9).astype(np.uint8)
    white = 1 - (rng.uniform(0, 1, brk.shape) > nd * 0.1).astype(np.uint8)
    out = np.logical_or(np.logical_and(brk, black), white).astype(np.float32)
    return out, img, flap


def _skull(dims, seed=0):
    """A binary ellipsoid shell, about 8 % bone."""
    z, y, x = np.ogrid[:dims[0], :dims[1], :dims[2]]
    q = ((z - dims[0] / 2) / (0.45 * dims[0])) ** 2 + ((y - dims[1] / 2) / (0.45 * dims[1])) ** 2 + \
        ((x - dims[2] / 2) / (0.45 * dims[2])) ** 2
    return ((q <= 1.0) & (q >= 0.75)).astype(np.float32)


def _host_one(args):
    dims, seed = args
    sk = _skull(dims)
    t0 = time.perf_counter()
    host_transform(sk, seed)
    return time.perf_counter() - t0


def gpu_legs(reps):
    import torch
    from ctunet_amd.transforms import FlapRecTransform, SaltAndPepper, SkullRandomHole
    out = {}
    for dims in SIZES:
        sk = torch.from_numpy(_skull(dims)).cuda().view(1, 1, *dims)
        atlas = torch.from_numpy(_skull(dims, 1)).cuda()
        t = FlapRecTransform(SkullRandomHole(double_output=True, seed=1), SaltAndPepper(p=.5, noise_density=.05, seed=2),
                             atlas)
        x, tg = t.apply(sk)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            t.apply(sk, x=x, targets=tg)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        nbytes = 36 * int(np.prod(dims))
        out["x".join(map(str, dims))] = {"ms_per_sample": round(ms, 4), "algorithmic_GB": round(nbytes / 1e9, 4),
                                         "GB_per_s": round(nbytes / ms / 1e6, 1)}
    return out


def cpu_legs(procs):
    out = {}
    for dims in SIZES:
        key = "x".join(map(str, dims))
        single = _host_one((dims, 0))
        leg = {"s_per_sample_1proc": round(single, 3)}
        if dims[1] <= 304:           # the 224x512x512 grid needs ~5 GB per process: single process only
            ctx = mp.get_context("spawn")
            with ctx.Pool(procs) as pool:
                t0 = time.perf_counter()
                pool.map(_host_one, [(dims, s) for s in range(procs)])
                wall = time.perf_counter() - t0
            leg["s_per_sample_%dproc" % procs] = round(wall / procs, 3)
        else:
            leg["s_per_sample_%dproc" % procs] = "not measured"
        out[key] = leg
    return out


def train_step_leg(reps):
    import torch
    import ctunet_amd as A
    from ctunet_amd import optim
    from ctunet_amd.graph import GraphedTrainStep
    dims = (224, 304, 304)
    torch.manual_seed(0)
    net = A.UNetSP().cuda().set_precision("bf16")
    sk = torch.from_numpy(_skull(dims)).cuda().view(1, 1, *dims)
    t = A.FlapRecTransform(A.SkullRandomHole(double_output=True, seed=1), A.SaltAndPepper(p=.5, noise_density=.05, seed=2),
                           torch.from_numpy(_skull(dims, 1)).cuda())
    x, tg = t.apply(sk)
    gs = GraphedTrainStep(net, optim.Adam(net.parameters(), lr=1e-4, amsgrad=True), x, tg, 1.0, 1.0, warmup=2)
    gs()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        gs()
    e1.record()
    torch.cuda.synchronize()
    step = e0.elapsed_time(e1) / reps
    e0.record()
    for _ in range(reps):
        t.apply(sk, x=gs.x, targets=gs.targets)
        gs()
    e1.record()
    torch.cuda.synchronize()
    return {"shape": list(dims), "graphed_step_ms": round(step, 3),
            "augment_plus_step_ms": round(e0.elapsed_time(e1) / reps, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--legs", default="gpu,cpu,step")
    args = ap.parse_args()
    res = {"metric": "flap_rec_transform per sample", "reps": args.reps}
    legs = args.legs.split(",")
    if "gpu" in legs:
        res["gpu_fused"] = gpu_legs(args.reps)
    if "step" in legs:
        res["unetsp_bf16_step"] = train_step_leg(args.reps)
    if "cpu" in legs:
        res["cpu_numpy_port"] = cpu_legs(args.procs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
