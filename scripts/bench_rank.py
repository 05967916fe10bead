#!/usr/bin/env python3
"""Rank filters at the project's usual volume, one 224x512x512 int16 scan (and its float32 copy for the last leg):

  median 3^3, median 5^3, percentile 25 over (3, 5, 5), minimum and maximum at 3^3 and 7^3, float32 median 3^3.

Each device leg runs --warmup untimed calls, then --reps timed calls with ``out=`` given, each ending in a device
synchronise (wall clock per call, median and range), and next to it the device time per call of the same number of calls
issued back to back between two stream events.  Each leg states the bytes the call must move (input read once, output
written once) and the time those take at the 6.29 TB/s measured copy rate.
A/B on the same build: the legs whose kernel is the 3 x 3 x 3 register kernel or the separable one run again with
CTU_RANK_PATH=generic in the environment, which sends the call down the generic bit-search kernel.
Baselines: ``scipy.ndimage`` on the host on a 64x128x128 sub-volume, the time scaled by voxel count; and the simplest torch
formulation on the same GPU (replicate pad, three ``unfold``s, ``kthvalue``) on a sub-volume that fits, scaled likewise.
Prints one JSON line and, with --out DIR, writes DIR/rank_bench.json.

    python scripts/bench_rank.py --reps 10 --out profiles
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd"), os.path.join(ROOT, "scripts")]

import torch
import torch.nn.functional as F

from bench_preprocess import COPY_TBS, SHAPE, _scene, _stats, _stream_ms, _time

SUB = (64, 128, 128)             # scipy's sub-volume
TORCH_SUB = (32, 128, 128)       # torch's: the unfolded windows are n times the volume, as int16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--scipy-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import preprocess as pp
    dev = torch.device("cuda", 0)
    ct = _scene(dev)
    ctf = ct.float()
    vox = SHAPE[0] * SHAPE[1] * SHAPE[2]
    o16, o32 = torch.empty_like(ct), torch.empty_like(ctf)
    # name: (input, out, size, rank of n or "min" / "max", percentile for scipy / None)
    legs = {
        "median_3_int16": (ct, o16, (3, 3, 3), 13),
        "median_5_int16": (ct, o16, (5, 5, 5), 62),
        "percentile25_3x5x5_int16": (ct, o16, (3, 5, 5), pp.percentile_rank(25, 75)),
        "minimum_3_int16": (ct, o16, (3, 3, 3), 0),
        "maximum_3_int16": (ct, o16, (3, 3, 3), 26),
        "minimum_7_int16": (ct, o16, (7, 7, 7), 0),
        "maximum_7_int16": (ct, o16, (7, 7, 7), 342),
        "median_3_float32": (ctf, o32, (3, 3, 3), 13),
    }
    res = {"metric": "rank filters, ms per call (wall clock, synchronised)", "reps": args.reps, "warmup": args.warmup,
           "copy_rate_tb_s": COPY_TBS, "device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "tile": pp.TILE,
           "scipy_sub_volume": list(SUB), "torch_sub_volume": list(TORCH_SUB), "legs": {}}
    for name, (x, out, size, rank) in legs.items():
        fn = lambda: pp.rank_filter(x, rank, size, out=out)
        nbytes = 2 * vox * x.element_size()
        os.environ.pop("CTU_RANK_PATH", None)
        entry = {"path": pp.path_of(size, rank), "size": list(size), "rank": rank, "device": _stats(_time(fn, args.warmup, args.reps))}
        entry["device"]["back_to_back_ms"] = round(_stream_ms(fn, args.reps), 4)
        kept = out.clone()
        entry["hbm_bytes"] = nbytes
        entry["hbm_floor_ms"] = round(nbytes / (COPY_TBS * 1e12) * 1e3, 4)
        entry["device_over_floor"] = round(entry["device"]["back_to_back_ms"] / entry["hbm_floor_ms"], 2)
        if entry["path"] != "generic":
            os.environ["CTU_RANK_PATH"] = "generic"
            reps = max(2, args.reps // 3)
            entry["forced_generic"] = _stats(_time(fn, 1, reps))
            entry["forced_generic"]["back_to_back_ms"] = round(_stream_ms(fn, reps), 4)
            entry["forced_generic"]["bit_equal"] = bool(torch.equal(out, kept))
            entry["generic_over_device"] = round(entry["forced_generic"]["back_to_back_ms"] / entry["device"]["back_to_back_ms"], 2)
            os.environ.pop("CTU_RANK_PATH", None)
        if args.torch_reps > 0:
            d, h, w = TORCH_SUB
            sub = x[80:80 + d, 192:192 + h, 192:192 + w].contiguous()
            r = [s // 2 for s in size]

            def tfn():
                p = F.pad(sub[None, None].float(), (r[2], r[2], r[1], r[1], r[0], r[0]), mode="replicate")[0, 0].to(sub.dtype)
                win = p.unfold(0, size[0], 1).unfold(1, size[1], 1).unfold(2, size[2], 1).reshape(d, h, w, -1)
                return win.kthvalue(rank + 1, dim=-1).values
            try:
                entry["torch_sub_volume_scaled_ms"] = round(statistics.median(_time(tfn, 1, args.torch_reps)) * vox / (d * h * w), 1)
                entry["torch_equal_on_sub_volume"] = bool(torch.equal(tfn(), pp.rank_filter(sub, rank, size)))
                entry["torch_over_device"] = round(entry["torch_sub_volume_scaled_ms"] / entry["device"]["median_ms"], 1)
            except RuntimeError as e:                  # e.g. out of memory at 7^3: the baseline is reported as not run
                entry["torch_error"] = str(e).splitlines()[0][:200]
        if args.scipy_reps > 0:
            from scipy import ndimage as ndi
            d, h, w = SUB
            hsub = x[80:80 + d, 192:192 + h, 192:192 + w].contiguous().cpu().numpy()
            t0 = time.perf_counter()
            want = ndi.rank_filter(hsub, rank, size=size, mode="nearest")
            entry["scipy_sub_volume_scaled_ms"] = round((time.perf_counter() - t0) * 1e3 * vox / (d * h * w), 0)
            entry["scipy_equal_on_sub_volume"] = bool((pp.rank_filter(torch.tensor(hsub, device=dev), rank, size).cpu().numpy() == want).all())
            entry["scipy_over_device"] = round(entry["scipy_sub_volume_scaled_ms"] / entry["device"]["median_ms"], 0)
        res["legs"][name] = entry
        print(name, json.dumps(entry), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(os.path.join(args.out, "rank_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
