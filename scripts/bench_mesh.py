#!/usr/bin/env python3
"""Surface extraction at the project's usual volume: ``mesh.extract_surface`` and ``mesh.measure`` on a skull-like shell of
224x512x512 voxels at spacing (0.8, 0.45, 0.45), as a uint8 mask and as a float32 field (the same shell as
``0.5 - |r - 0.965| / 0.035`` cut at 0, so the two surfaces are alike in size).

Per input: wall clock per call (--warmup untimed calls, then --reps calls, each ending in a device synchronise; the call
itself synchronises once to read V and F), V and F, the bytes each pass moves by construction and the time those take at the
6.29 TB/s measured copy rate.  Per-kernel times come from a kernel trace of this script in a run of its own
(``--reps 3 --host-reps 0`` under ``rocprofv3 --kernel-trace --stats``).  The only other implementation at hand is the numpy
restatement ``tests/mesh_ref.py`` on the host; it runs at --host-shape (a centred crop of the same shell) next to the
device on the same crop, and the ratio is reported.  Prints one JSON line and, with --out DIR, writes DIR/mesh_bench.json.

    python scripts/bench_mesh.py --reps 10 --out profiles
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd"), os.path.join(ROOT, "tests")]

import torch

COPY_TBS = 6.29
SHAPE, SPACING = (224, 512, 512), (0.8, 0.45, 0.45)


def _radius(dev):
    d, h, w = SHAPE
    zz = torch.arange(d, device=dev, dtype=torch.float32).view(-1, 1, 1)
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(1, -1, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, -1)
    return (((zz - d / 2) / (0.45 * d)) ** 2 + ((yy - h / 2) / (0.46 * h)) ** 2 + ((xx - w / 2) / (0.44 * w)) ** 2).sqrt()


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
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def pass_bytes(shape, itemsize, nv, nf):
    """Bytes each pass moves by construction (volume rows are shared by four cell rows: counted once, the cache's part)."""
    d, h, w = shape
    rows = (d + 1) * (h + 1)
    ncp = rows * (-(-(w + 1) // 16) * 16)
    return {"count": d * h * w * itemsize + 5 * ncp + 4 * rows,        # volume in; code + prefix out, row totals
            "scan": 12 * rows,
            "vertices": ncp + 12 * nv + (4 * nv if itemsize == 4 else 0),   # codes in; vertices out (+ ~2 samples per vertex)
            "faces": ncp + 12 * nf,                                    # codes in; faces out (neighbour look-ups: cache)
            "measure": 12 * nf + 12 * nv}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-shape", type=int, nargs=3, default=(56, 128, 128))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import mesh
    dev = torch.device("cuda", 0)
    r = _radius(dev)
    inputs = {"uint8": (((r <= 1.0) & (r >= 0.93)).to(torch.uint8), {}),
              "float32": ((0.5 - (r - 0.965).abs() / 0.035).contiguous(), dict(level=0.0))}
    del r
    res = {"metric": "surface extraction, ms per call (wall clock, synchronised)", "reps": args.reps, "warmup": args.warmup,
           "copy_rate_tb_s": COPY_TBS, "device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "spacing": list(SPACING),
           "workspace_bytes": mesh.workspace_bytes(SHAPE), "inputs": {}}
    for name, (vol, kw) in inputs.items():
        m = mesh.extract_surface(vol, spacing=SPACING, **kw)
        nv, nf = m.vertices.shape[0], m.faces.shape[0]
        entry = {"V": nv, "F": nf, "extract": _time(lambda: mesh.extract_surface(vol, spacing=SPACING, **kw), args.warmup, args.reps),
                 "measure": _time(lambda: mesh.measure(m), args.warmup, args.reps)}
        entry["area_mm2"], entry["volume_mm3"] = mesh.measure(m).tolist()
        entry["pass_bytes"] = pass_bytes(SHAPE, vol.element_size(), nv, nf)
        entry["pass_floor_ms"] = {k: round(b / (COPY_TBS * 1e12) * 1e3, 4) for k, b in entry["pass_bytes"].items()}
        entry["extract_floor_ms"] = round(sum(v for k, v in entry["pass_floor_ms"].items() if k != "measure"), 4)
        res["inputs"][name] = entry
        del m
    if args.host_reps > 0:
        import mesh_ref
        hs = tuple(args.host_shape)
        lo = [(n - c) // 2 for n, c in zip(SHAPE, hs)]
        crop = inputs["uint8"][0][lo[0]:lo[0] + hs[0], :hs[1], :hs[2]].contiguous()       # a corner of the shell's middle slab
        host = crop.cpu().numpy()
        ms = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            hv, hf = mesh_ref.extract(host, spacing=SPACING)
            ms.append((time.perf_counter() - t0) * 1e3)
        dm = mesh.extract_surface(crop, spacing=SPACING)
        same = bool((dm.faces.cpu().numpy() == hf).all() and (dm.vertices.cpu().numpy() == hv).all())
        dt = _time(lambda: mesh.extract_surface(crop, spacing=SPACING), args.warmup, args.reps)
        res["host_reference"] = {"shape": list(hs), "V": len(hv), "F": len(hf), "numpy_ms": round(statistics.median(ms), 1),
                                 "device": dt, "numpy_over_device": round(statistics.median(ms) / dt["median_ms"], 1),
                                 "bit_equal": same}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(os.path.join(args.out, "mesh_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
