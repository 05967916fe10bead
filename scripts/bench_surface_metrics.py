#!/usr/bin/env python3
"""Surface metrics on whole CT-sized label pairs: ``metrics.surface_metrics`` (HD, HD95, ASSD, NSD, Dice in one call,
anisotropic spacing) on 224x304x304 and 224x512x512 uint8 label maps with one and two foreground classes (skull shells
and a flap, built on the device), against the existing ``ops.hausdorff`` on the matching float one-hot tensors.

Each leg runs one untimed call first, then --reps timed calls, each ending in a device synchronise; wall clock per call.
Workspace is what ``ctu_surface_ws_bytes`` asks for.  ``model_bytes`` counts the HBM traffic the kernels need
(labels once per pair, per plane: edge byte + x-pass distance written, y and z passes read + write 4 B each, the
reduction reads the edge bytes, each of the 4 percentile passes reads them again).  Prints one JSON line.

    python scripts/bench_surface_metrics.py --reps 5
    python scripts/bench_surface_metrics.py --legs 512-1 --reps 1 --no-hausdorff      # (the leg a kernel-trace run profiles)
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

SPACING = (0.8, 0.45, 0.45)


def _labels(shape, classes, dev, shift):
    d, h, w = shape
    zz = torch.arange(d, device=dev, dtype=torch.float32).view(-1, 1, 1)
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(1, -1, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, -1)
    r = (((zz - d / 2 - shift) / (0.45 * d)) ** 2 + ((yy - h / 2) / (0.46 * h)) ** 2 +
         ((xx - w / 2 + shift) / (0.44 * w)) ** 2).sqrt()
    lab = ((r <= 1.0) & (r >= 0.93)).to(torch.uint8)
    if classes == 2:
        flap = (r <= 1.0) & (r >= 0.93) & (zz > d * 0.55 + shift) & (xx > w * 0.6)
        lab[flap] = 2
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
    ap.add_argument("--legs", default="304-1,304-2,512-1,512-2")
    ap.add_argument("--no-hausdorff", action="store_true")
    args = ap.parse_args()
    from ctunet_amd import metrics, ops
    dev = torch.device("cuda", 0)
    res = {"metric": "surface_metrics (hd, hd95, assd, nsd, dice), ms per call", "spacing": SPACING, "reps": args.reps,
           "legs": {}}
    for leg in args.legs.split(","):
        side, fg = leg.split("-")
        shape, fg = (224, int(side), int(side)), int(fg)
        v = shape[0] * shape[1] * shape[2]
        p, g = _labels(shape, fg, dev, 0), _labels(shape, fg, dev, 3)
        call = lambda: metrics.surface_metrics(p, g, fg + 1, spacing=SPACING, percentile=95.0, tolerance=1.0)
        out = call()
        ms = _time(call, args.reps)
        med = statistics.median(ms)
        planes = 2 * fg
        model = fg * 2 * v + planes * v * (1 + 4 + 8 + 8 + 1 + 4)
        entry = {"shape": list(shape), "foreground_classes": fg, "ms": [round(m, 3) for m in ms],
                 "median_ms": round(med, 3), "workspace_mb": round(metrics.workspace_bytes(1, fg, shape) / 1e6, 1),
                 "workspace_bytes_per_voxel_per_plane": round(metrics.workspace_bytes(1, fg, shape) / (planes * v), 3),
                 "model_bytes_gb": round(model / 1e9, 3), "model_gb_per_s_wall": round(model / 1e9 / (med / 1e3), 1),
                 "hd": out["hd"].flatten().tolist(), "hd_p": out["hd_p"].flatten().tolist(),
                 "assd": out["assd"].flatten().tolist(), "nsd": out["nsd"].flatten().tolist(),
                 "dice": out["dice"].flatten().tolist()}
        if not args.no_hausdorff:
            c = fg + 1
            pf = torch.nn.functional.one_hot(p.long(), c).movedim(-1, 0).unsqueeze(0).float().contiguous()
            gf = torch.nn.functional.one_hot(g.long(), c).movedim(-1, 0).unsqueeze(0).float().contiguous()
            hms = _time(lambda: ops.hausdorff(pf, gf), max(1, min(args.reps, 2)))
            entry["ops_hausdorff_ms"] = [round(m, 2) for m in hms]
            entry["ops_hausdorff_median_ms"] = round(statistics.median(hms), 2)
            unit = metrics.surface_metrics(p, g, c, percentile=None)["hd"]
            entry["hd_unit_spacing_equals_ops_hausdorff"] = bool(torch.equal(unit, ops.hausdorff(pf, gf)))
            del pf, gf
        res["legs"][leg] = entry
        del p, g, out
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
