#!/usr/bin/env python3
"""Volume resampling at the project's usual volume, three legs of one ``resample.Resampler``:

  1. ``linear``:        224x512x512 int16 at spacing (0.8, 0.45, 0.45) -> 1 mm (179x230x230 float32);
  2. ``label_linear``:  a uint8 label map on the 1 mm grid back up to 224x512x512, K = 2;
  3. ``nearest``:       the same map, nearest.

Each device leg runs --warmup untimed calls, then --reps timed calls with ``out=`` given, each ending in a device
synchronise (wall clock per call, median and range), and next to it the device time per call of the same number of calls
issued back to back between two stream events: one call is one kernel launch, so that figure is the per-kernel time.  Each
leg states the bytes the call must move (input read once, output written once) and the time those take at the 6.29 TB/s
measured copy rate.  Beside it: the same operation through ``torch.nn.functional.interpolate`` on the same GPU (leg 1:
``float() -> trilinear``; leg 2: ``one_hot -> trilinear per class -> argmax`` with its peak extra memory; leg 3:
``nearest-exact`` on the uint8 map) and ``scipy.ndimage.zoom`` on the host (order 1 / per-class order 1 + argmax / order 0).
Prints one JSON line and, with --out DIR, writes DIR/resample_bench.json.

    python scripts/bench_resample.py --reps 20 --out profiles
    python scripts/bench_resample.py --reps 3 --torch-reps 0 --scipy-reps 0      # (the legs a kernel-trace run profiles)
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
import torch.nn.functional as F

COPY_TBS = 6.29
SHAPE, SPACING, NEW_SPACING = (224, 512, 512), (0.8, 0.45, 0.45), 1.0


def _scene(dev):
    """A skull-like int16 CT (air -1000, soft tissue ~40 with noise, a bone shell ~1200) and its bone mask."""
    d, h, w = SHAPE
    zz = torch.arange(d, device=dev, dtype=torch.float32).view(-1, 1, 1)
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(1, -1, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, -1)
    r = (((zz - d / 2) / (0.45 * d)) ** 2 + ((yy - h / 2) / (0.46 * h)) ** 2 + ((xx - w / 2) / (0.44 * w)) ** 2).sqrt()
    g = torch.Generator(device=dev).manual_seed(5)
    ct = torch.full(SHAPE, -1000.0, device=dev)
    ct = torch.where(r <= 1.0, 40.0 + 20.0 * torch.randn(SHAPE, device=dev, generator=g), ct)
    ct = torch.where((r <= 1.0) & (r >= 0.93), torch.tensor(1200.0, device=dev), ct)
    return ct.round().to(torch.int16)


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
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def _peak_extra_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del y
    return round(peak / 1e6, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--scipy-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import resample as rs
    dev = torch.device("cuda", 0)
    ct = _scene(dev)
    r = rs.Resampler(SHAPE, in_spacing=SPACING, out_spacing=NEW_SPACING).to(dev)
    small = r.out_shape
    vin, vout = SHAPE[0] * SHAPE[1] * SHAPE[2], small[0] * small[1] * small[2]
    down = torch.empty(small, dtype=torch.float32, device=dev)
    r(ct, out=down)
    labels = (down > 600.0).to(torch.uint8)                       # the bone of the 1 mm volume
    up = torch.empty(SHAPE, dtype=torch.uint8, device=dev)
    legs = {
        "linear_down_int16": (lambda: r(ct, out=down), 2 * vin + 4 * vout),
        "label_linear_up_k2": (lambda: r.inverse(labels, mode="label_linear", num_classes=2, out=up), vout + vin),
        "nearest_up": (lambda: r.inverse(labels, mode="nearest", out=up), vout + vin),
    }
    torch_legs = {
        "linear_down_int16": lambda: F.interpolate(ct.float()[None, None], size=small, mode="trilinear", align_corners=False)[0, 0],
        "label_linear_up_k2": lambda: F.interpolate(F.one_hot(labels.long(), 2).movedim(3, 0).float()[None], size=SHAPE,
                                                     mode="trilinear", align_corners=False)[0].argmax(0).to(torch.uint8),
        "nearest_up": lambda: F.interpolate(labels[None, None], size=SHAPE, mode="nearest-exact")[0, 0],
    }
    res = {"metric": "volume resampling, ms per call (wall clock, synchronised)", "reps": args.reps, "warmup": args.warmup,
           "copy_rate_tb_s": COPY_TBS, "device": torch.cuda.get_device_name(0), "in_shape": list(SHAPE),
           "spacing": list(SPACING), "new_spacing": NEW_SPACING, "out_shape": list(small),
           "label_foreground_fraction": round(float(labels.float().mean()), 4), "legs": {}}
    for name, (fn, nbytes) in legs.items():
        entry = {"device": _stats(_time(fn, args.warmup, args.reps))}
        entry["device"]["kernel_ms"] = round(_stream_ms(fn, args.reps), 4)
        entry["hbm_bytes"] = nbytes
        entry["hbm_floor_ms"] = round(nbytes / (COPY_TBS * 1e12) * 1e3, 4)
        if args.torch_reps > 0:
            tfn = torch_legs[name]
            entry["torch"] = _stats(_time(tfn, 1, args.torch_reps))
            entry["torch"]["back_to_back_ms"] = round(_stream_ms(tfn, args.torch_reps), 4)
            entry["torch"]["peak_extra_mb"] = _peak_extra_mb(tfn)
            entry["torch_over_device"] = round(entry["torch"]["median_ms"] / entry["device"]["median_ms"], 1)
        res["legs"][name] = entry
    if args.torch_reps > 0:
        # how far the results are from torch's (float32 coordinates there, float64 tables here)
        res["linear_max_abs_diff_vs_torch"] = float((torch_legs["linear_down_int16"]() - down).abs().max())
        r.inverse(labels, mode="label_linear", num_classes=2, out=up)
        res["label_linear_voxels_differing_from_torch"] = int((torch_legs["label_linear_up_k2"]() != up).sum())
        r.inverse(labels, mode="nearest", out=up)
        res["nearest_voxels_differing_from_torch"] = int((torch_legs["nearest_up"]() != up).sum())
    if args.scipy_reps > 0:
        import numpy as np
        from scipy import ndimage as ndi
        hct, hl = ct.cpu().numpy(), labels.cpu().numpy()
        zd = [m / n for n, m in zip(SHAPE, small)]
        zu = [n / m for n, m in zip(SHAPE, small)]

        def host_label():
            s = [ndi.zoom((hl == c).astype(np.float32), zu, order=1, mode="nearest", grid_mode=True) for c in (0, 1)]
            return np.argmax(np.stack(s), axis=0).astype(np.uint8)

        host = {"linear_down_int16": lambda: ndi.zoom(hct.astype(np.float32), zd, order=1, mode="nearest", grid_mode=True),
                "label_linear_up_k2": host_label,
                "nearest_up": lambda: ndi.zoom(hl, zu, order=0, mode="nearest", grid_mode=True)}
        for name, fn in host.items():
            ms = []
            for _ in range(args.scipy_reps):
                t0 = time.perf_counter()
                fn()
                ms.append((time.perf_counter() - t0) * 1e3)
            res["legs"][name]["scipy_ms"] = round(statistics.median(ms), 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(os.path.join(args.out, "resample_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
