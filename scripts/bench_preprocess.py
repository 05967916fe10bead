#!/usr/bin/env python3
"""CT preprocessing at the project's usual volume, 224x512x512 int16 at spacing (0.8, 0.45, 0.45):

  1. ``gaussian``:   ``preprocess.gaussian_filter`` at sigma = 1 mm (radii 5, 9, 9 voxels), float32 out; beside it the same call
                     with the z sigma at 0, which is the x-y launch alone;
  2. ``histogram``:  256 bins over (-1024, 3072);
  3. ``binarize``:   ``> 300`` to a uint8 mask.

Each device leg runs --warmup untimed calls, then --reps timed calls with ``out=`` given, each ending in a device
synchronise (wall clock per call, median and range), and next to it the device time per call of the same number of calls
issued back to back between two stream events.  Each leg states the bytes the call must move (input read once, output
written once) and the time those take at the 6.29 TB/s measured copy rate.  Beside it: the same operation through torch on
the same GPU (leg 1: ``float()``, then three ``torch.nn.functional.conv3d`` calls on replicate-padded input; leg 2:
``torch.histc`` of ``float()``; leg 3: ``(x > 300).to(uint8)``) and scipy / numpy on the host.
Prints one JSON line and, with --out DIR, writes DIR/preprocess_bench.json.

    python scripts/bench_preprocess.py --reps 20 --out profiles
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
SHAPE, SPACING, SIGMA_MM = (224, 512, 512), (0.8, 0.45, 0.45), 1.0
HIST_RANGE, BINS, BONE_HU = (-1024, 3072), 256, 300


def _scene(dev):
    """A skull-like int16 CT: air -1000, soft tissue ~40 with noise, a bone shell ~1200."""
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


def _host_ms(fn, reps):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--scipy-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import preprocess as pp
    dev = torch.device("cuda", 0)
    ct = _scene(dev)
    vox = SHAPE[0] * SHAPE[1] * SHAPE[2]
    sig_vox = tuple(SIGMA_MM / s for s in SPACING)
    radii = tuple(int(4.0 * s + 0.5) for s in sig_vox)
    smooth = torch.empty(SHAPE, dtype=torch.float32, device=dev)
    counts = torch.empty(BINS, dtype=torch.int64, device=dev)
    mask = torch.empty(SHAPE, dtype=torch.uint8, device=dev)
    legs = {
        "gaussian_int16": (lambda: pp.gaussian_filter(ct, SIGMA_MM, spacing=SPACING, out=smooth), 2 * vox + 4 * vox),
        "gaussian_int16_xy_launch_only": (lambda: pp.gaussian_filter(ct, (0.0, SIGMA_MM, SIGMA_MM), spacing=SPACING, out=smooth),
                                          2 * vox + 4 * vox),
        "histogram_int16": (lambda: pp.histogram(ct, BINS, HIST_RANGE, out=counts), 2 * vox),
        "binarize_int16": (lambda: pp.binarize(ct, BONE_HU, out=mask), 2 * vox + vox),
    }
    kernels = [torch.from_numpy(pp.gaussian_weights(s)).to(dev) for s in sig_vox]
    kernels = [torch.cat([k.flip(0)[:-1], k]) for k in kernels]                      # w_R .. w_0 .. w_R

    def torch_gauss():
        v = ct.float()[None, None]
        for axis, (k, r) in enumerate(zip(kernels, radii)):                          # z, y, x: the order changes roundings only
            shape, pad = [1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0]
            shape[2 + axis] = k.numel()
            pad[2 * (2 - axis)] = pad[2 * (2 - axis) + 1] = r
            v = F.conv3d(F.pad(v, pad, mode="replicate"), k.view(shape))
        return v[0, 0]

    torch_legs = {
        "gaussian_int16": torch_gauss,
        "histogram_int16": lambda: torch.histc(ct.float(), BINS, HIST_RANGE[0], HIST_RANGE[1]),
        "binarize_int16": lambda: (ct > BONE_HU).to(torch.uint8),
    }
    res = {"metric": "CT preprocessing, ms per call (wall clock, synchronised)", "reps": args.reps, "warmup": args.warmup,
           "copy_rate_tb_s": COPY_TBS, "device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "spacing": list(SPACING),
           "sigma_mm": SIGMA_MM, "radii_zyx": list(radii), "bins": BINS, "range": list(HIST_RANGE), "legs": {}}
    for name, (fn, nbytes) in legs.items():
        entry = {"device": _stats(_time(fn, args.warmup, args.reps))}
        entry["device"]["back_to_back_ms"] = round(_stream_ms(fn, args.reps), 4)
        entry["hbm_bytes"] = nbytes
        entry["hbm_floor_ms"] = round(nbytes / (COPY_TBS * 1e12) * 1e3, 4)
        entry["achieved_tb_s"] = round(nbytes / (entry["device"]["back_to_back_ms"] * 1e-3) / 1e12, 3)
        entry["floor_over_device"] = round(entry["hbm_floor_ms"] / entry["device"]["back_to_back_ms"], 3)
        if args.torch_reps > 0 and name in torch_legs:
            tfn = torch_legs[name]
            entry["torch"] = _stats(_time(tfn, 1, args.torch_reps))
            entry["torch"]["back_to_back_ms"] = round(_stream_ms(tfn, args.torch_reps), 4)
            entry["torch_over_device"] = round(entry["torch"]["median_ms"] / entry["device"]["median_ms"], 1)
        res["legs"][name] = entry
    if args.torch_reps > 0:
        pp.gaussian_filter(ct, SIGMA_MM, spacing=SPACING, out=smooth)
        res["gaussian_max_abs_diff_vs_torch"] = float((torch_gauss() - smooth).abs().max())
        pp.histogram(ct, BINS, HIST_RANGE, out=counts)
        res["histogram_bins_differing_from_torch"] = int((torch_legs["histogram_int16"]().long() != counts).sum())
        pp.binarize(ct, BONE_HU, out=mask)
        res["binarize_voxels_differing_from_torch"] = int((torch_legs["binarize_int16"]() != mask).sum())
    if args.scipy_reps > 0:
        import numpy as np
        from scipy import ndimage as ndi
        hct = ct.cpu().numpy()
        host = {"gaussian_int16": lambda: ndi.gaussian_filter(hct.astype(np.float32), sig_vox, mode="nearest"),
                "histogram_int16": lambda: np.histogram(hct, bins=BINS, range=HIST_RANGE),
                "binarize_int16": lambda: (hct > BONE_HU).astype(np.uint8)}
        for name, fn in host.items():
            res["legs"][name]["host_ms"] = _host_ms(fn, args.scipy_reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(os.path.join(args.out, "preprocess_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
