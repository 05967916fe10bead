#!/usr/bin/env python3
"""Binary morphology on whole CT-sized masks: ``postprocess.binary_erosion`` at 1, 2 and 4 iterations, ``binary_opening``
x2, ``binary_fill_holes`` and ``extract_implant`` on 224x304x304 and 224x512x512 uint8 skull shells built on the device
(the shell of scripts/bench_components.py; the defective skull is the shell with a sphere cut out), against scipy.ndimage
on the host on the same arrays.

Each device leg runs --warmup untimed calls, then --reps timed calls, each ending in a device synchronise; wall clock per
call (allocation of the output and the workspace included), median and range reported, and next to it the device time
per call of the same number of calls issued back to back between two stream events.  scipy is timed --scipy-reps times
per leg.  Each leg also states its HBM floor: the bytes the call has to move (input read once, output written once, for
fill-holes the complement image and the union-find arrays too) at the 6.29 TB/s measured copy rate.  Prints one JSON line
and, with --out DIR, writes DIR/morphology_bench.json.

    python scripts/bench_morphology.py --reps 20 --out profiles
    python scripts/bench_morphology.py --legs 512 --reps 3 --scipy-reps 0      # (the leg a kernel-trace run profiles)
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

COPY_TBS = 6.29


def _scene(shape, dev):
    d, h, w = shape
    zz = torch.arange(d, device=dev, dtype=torch.float32).view(-1, 1, 1)
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(1, -1, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, -1)
    r = (((zz - d / 2) / (0.45 * d)) ** 2 + ((yy - h / 2) / (0.46 * h)) ** 2 + ((xx - w / 2) / (0.44 * w)) ** 2).sqrt()
    shell = (r <= 1.0) & (r >= 0.93)
    hole = ((zz - d / 2) ** 2 + (yy - h / 2) ** 2 + (xx - 0.94 * w) ** 2) <= (0.2 * d) ** 2
    full = shell.to(torch.uint8)
    defective = (shell & ~hole).to(torch.uint8)
    g = torch.Generator().manual_seed(5)
    for i in range(40):                           # islands of 1 to 27 voxels anywhere off the shell
        z, y, x = (int(torch.randint(0, s - 3, (1,), generator=g)) for s in shape)
        e = 1 + i % 3
        box = full[z:z + e, y:y + e, x:x + e]
        if not bool(box.any()):
            box.fill_(1)
    return full, defective


def _time(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def _stream_ms(fn, reps):
    """Device time per call of `reps` calls issued back to back (events on the stream; no host gap between calls)."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def _host(fn, reps):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scipy-reps", type=int, default=1)
    ap.add_argument("--legs", default="304,512")
    ap.add_argument("--calls", default=None, help="comma-separated subset of the calls")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import postprocess as pp
    dev = torch.device("cuda", 0)
    res = {"metric": "binary morphology, ms per call (wall clock, synchronised)", "reps": args.reps, "warmup": args.warmup,
           "copy_rate_tb_s": COPY_TBS, "device": torch.cuda.get_device_name(0), "legs": {}}
    for leg in args.legs.split(","):
        shape = (224, int(leg), int(leg))
        v = shape[0] * shape[1] * shape[2]
        full, defective = _scene(shape, dev)
        # bytes per voxel over HBM: uint8 in + uint8 out; fill-holes adds the complement (write + 3 reads), parent (write,
        # merge / flatten / apply reads) and its own output pass; the implant call reads two maps and runs the filter
        calls = {
            "erosion_x1": (lambda: pp.binary_erosion(full), 2),
            "erosion_x2": (lambda: pp.binary_erosion(full, iterations=2), 2),
            "erosion_x4": (lambda: pp.binary_erosion(full, iterations=4), 2),
            "opening_x2": (lambda: pp.binary_opening(full, iterations=2), 2),
            "fill_holes": (lambda: pp.binary_fill_holes(full), 2 + 4 + 12),
            "extract_implant": (lambda: pp.extract_implant(full, defective), 3 + 2 + 12),
        }
        if args.calls:
            calls = {k: c for k, c in calls.items() if k in args.calls.split(",")}
        entry = {"shape": list(shape), "voxels": v, "foreground_fraction": round(float(full.float().mean()), 4),
                 "workspace_mb": round(pp.morphology_workspace_bytes(1, shape) / 1e6, 2), "device": {}, "scipy_ms": {}}
        for name, (fn, bpv) in calls.items():
            ms = _time(fn, args.warmup, args.reps)
            entry["device"][name] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                                     "max_ms": round(max(ms), 4),
                                     "back_to_back_ms": round(_stream_ms(fn, args.reps), 4), "hbm_bytes_per_voxel": bpv,
                                     "hbm_floor_ms": round(bpv * v / (COPY_TBS * 1e12) * 1e3, 4)}
        if args.scipy_reps > 0:
            from scipy import ndimage as ndi
            hf, hd = full.cpu().numpy() != 0, defective.cpu().numpy() != 0
            st3 = ndi.generate_binary_structure(3, 3)

            def implant():
                m = ndi.binary_opening(hf & ~hd)
                lab, n = ndi.label(m, st3)
                return lab == (1 + ndi.sum_labels(m, lab, range(1, n + 1)).argmax()) if n else m

            host = {"erosion_x1": lambda: ndi.binary_erosion(hf), "erosion_x2": lambda: ndi.binary_erosion(hf, iterations=2),
                    "erosion_x4": lambda: ndi.binary_erosion(hf, iterations=4),
                    "opening_x2": lambda: ndi.binary_opening(hf, iterations=2), "fill_holes": lambda: ndi.binary_fill_holes(hf),
                    "extract_implant": implant}
            for name, fn in host.items():
                if name not in calls:
                    continue
                entry["scipy_ms"][name] = round(statistics.median(_host(fn, args.scipy_reps)), 1)
        if args.scipy_reps > 0 and not args.calls:
            entry["opening_matches_scipy"] = bool(torch.equal(pp.binary_opening(full, iterations=2).cpu(),
                                                              torch.from_numpy(host["opening_x2"]().astype("uint8"))))
            entry["fill_holes_matches_scipy"] = bool(torch.equal(pp.binary_fill_holes(full).cpu(),
                                                                 torch.from_numpy(host["fill_holes"]().astype("uint8"))))
            entry["implant_matches_scipy"] = bool(torch.equal(pp.extract_implant(full, defective).cpu(),
                                                              torch.from_numpy(implant().astype("uint8"))))
        res["legs"][leg] = entry
        del full, defective
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(os.path.join(args.out, "morphology_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
