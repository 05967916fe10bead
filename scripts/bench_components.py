#!/usr/bin/env python3
"""Connected components on whole CT-sized label maps: ``postprocess.label`` and
``postprocess.keep_largest_connected_component`` on 224x304x304 and 224x512x512 uint8 maps with one and two foreground
classes (a skull shell, the second class a flap cut out of it, plus far islands of every class, built on the device),
against ``scipy.ndimage.label`` on the host on the same arrays (one call per foreground class for the two-class maps).

Each device leg runs one untimed call first, then --reps timed calls, each ending in a device synchronise; wall clock per
call.  scipy is timed once per leg (--scipy-reps).  Prints one JSON line and, with --out DIR, writes
DIR/components_bench.json.

    python scripts/bench_components.py --reps 5 --out profiles
    python scripts/bench_components.py --legs 512-1 --reps 2 --scipy-reps 0     # (the leg a kernel-trace run profiles)
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


def _labels(shape, classes, dev):
    d, h, w = shape
    zz = torch.arange(d, device=dev, dtype=torch.float32).view(-1, 1, 1)
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(1, -1, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, -1)
    r = (((zz - d / 2) / (0.45 * d)) ** 2 + ((yy - h / 2) / (0.46 * h)) ** 2 + ((xx - w / 2) / (0.44 * w)) ** 2).sqrt()
    shell = (r <= 1.0) & (r >= 0.93)
    lab = shell.to(torch.uint8)
    if classes == 2:
        lab[shell & (zz > d * 0.55) & (xx > w * 0.6)] = 2
    g = torch.Generator().manual_seed(5)
    for i in range(40):                           # islands of 1 to 27 voxels anywhere off the shell
        z, y, x = (int(torch.randint(0, s - 3, (1,), generator=g)) for s in shape)
        e = 1 + i % 3
        box = lab[z:z + e, y:y + e, x:x + e]
        if not bool(box.any()):
            box.fill_(1 + i % classes)
    return lab


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-reps", type=int, default=1)
    ap.add_argument("--legs", default="304-1,304-2,512-1,512-2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import postprocess
    dev = torch.device("cuda", 0)
    res = {"metric": "connected components, ms per call", "reps": args.reps, "legs": {}}
    for leg in args.legs.split(","):
        side, fg = leg.split("-")
        shape, fg = (224, int(side), int(side)), int(fg)
        v = shape[0] * shape[1] * shape[2]
        lab = _labels(shape, fg, dev)
        mask = lab > 0
        lab_ms = _time(lambda: postprocess.label(mask), args.reps)
        keep_ms = _time(lambda: postprocess.keep_largest_connected_component(lab), args.reps)
        _, num = postprocess.label(mask)
        kept = postprocess.keep_largest_connected_component(lab)
        entry = {"shape": list(shape), "foreground_classes": fg, "foreground_fraction": round(float(mask.float().mean()), 4),
                 "components": int(num[0]), "voxels_dropped_by_keep_largest": int((kept != lab).sum()),
                 "label_ms": [round(m, 3) for m in lab_ms], "label_median_ms": round(statistics.median(lab_ms), 3),
                 "keep_largest_ms": [round(m, 3) for m in keep_ms],
                 "keep_largest_median_ms": round(statistics.median(keep_ms), 3),
                 "workspace_mb": round(postprocess.workspace_bytes(1, shape) / 1e6, 1),
                 "workspace_bytes_per_voxel": round(postprocess.workspace_bytes(1, shape) / v, 3)}
        if args.scipy_reps > 0:
            from scipy import ndimage as ndi
            host = lab.cpu().numpy()
            st = ndi.generate_binary_structure(3, 3)
            sms = []
            for _ in range(args.scipy_reps):
                t0 = time.perf_counter()
                for c in range(1, fg + 1):
                    ndi.label(host == c, st)
                sms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            lab.cpu()
            entry["device_to_host_copy_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            entry["scipy_label_ms"] = [round(m, 1) for m in sms]
            entry["scipy_label_median_ms"] = round(statistics.median(sms), 1)
            entry["label_matches_scipy"] = bool(torch.equal(postprocess.label(mask)[0].cpu(),
                                                            torch.from_numpy(ndi.label(host > 0, st)[0])))
        res["legs"][leg] = entry
        del lab, mask, kept
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(os.path.join(args.out, "components_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
