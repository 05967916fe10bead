#!/usr/bin/env python3
"""Local thickness on whole volumes: ``postprocess.local_thickness``, the ``distance_transform_edt(squared=True)`` call it
starts with on its own (so the search's share is visible) and ``thickness_summary``, on

- ``shell_unit`` / ``shell_aniso``: the 224x512x512 skull shell of scripts/bench_morphology.py at unit sampling and at the
  scanner's (0.8, 0.45, 0.45);
- ``plate``: an implant-like spherical cap about 6 voxels thick in the same grid;
- ``ball``: a solid ball of radius --ball-radius (60) in a cube of side 2 r + 8, where the cube of the radius bites.

Each leg runs --warmup untimed calls, then --reps timed calls, each ending in a device synchronise (wall clock per call,
allocations included), and the same number of calls back to back between two stream events.  The candidate counts are the
foreground voxels of the squared map (before) and the nonzero entries of the pruned map, the first plane of the search's
workspace (after).  ``--check`` compares the device result bit for bit with the unpruned numpy search of
tests/thickness_ref.py on a 48x64x64 crop of the shell, computed on that crop alone on both sides, at both samplings.
Prints one JSON line per input and, with --out DIR, merges them into DIR/thickness_bench.json.

    python scripts/bench_thickness.py --inputs shell_unit,shell_aniso,plate,ball --check --out profiles
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ct-unet_amd"), os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

import torch

from bench_morphology import _scene, _stream_ms, _time

SPACING = (0.8, 0.45, 0.45)
SHAPE = (224, 512, 512)
CROP = (slice(0, 48), slice(224, 288), slice(224, 288))      # the crown of the shell: 48x64x64


def _plate(shape, dev):
    """A spherical cap: the voxels between radius 300 and 306 around a centre below the volume, within 90 voxels of the axis."""
    d, h, w = shape
    zz = torch.arange(d, device=dev, dtype=torch.float32).view(-1, 1, 1)
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(1, -1, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, -1)
    r = ((zz - (d / 2 + 280)) ** 2 + (yy - h / 2) ** 2 + (xx - w / 2) ** 2).sqrt()
    lateral = ((yy - h / 2) ** 2 + (xx - w / 2) ** 2).sqrt()
    return ((r >= 300) & (r <= 306) & (lateral <= 90) & (zz < d / 2 + 280)).to(torch.uint8)


def _ball(radius, dev):
    side = 2 * radius + 8
    g = torch.arange(side, device=dev, dtype=torch.float32) - (side - 1) / 2
    return ((g.view(-1, 1, 1) ** 2 + g.view(1, -1, 1) ** 2 + g.view(1, 1, -1) ** 2) <= radius * radius).to(torch.uint8)


def _candidates(pp, mask, sampling):
    """(foreground voxels, candidates kept by the pruning): one call of the entry point on a workspace held here."""
    from ctunet_amd import _lib
    lib = _lib.load()
    d2 = pp.distance_transform_edt(mask, sampling=sampling, squared=True)
    shape = tuple(mask.shape)
    v = shape[0] * shape[1] * shape[2]
    is_float = int(d2.dtype == torch.float32)
    out = torch.empty(shape, dtype=torch.float32, device=mask.device)
    ws = torch.empty(lib.ctu_thickness_ws_bytes(1, *shape, is_float), dtype=torch.uint8, device=mask.device)
    with _lib.on(mask.device) as run:
        run("ctu_local_thickness", d2.data_ptr(), is_float, 1, *shape,
            _lib.float_array(sampling) if is_float else None, out.data_ptr(), ws.data_ptr())
    torch.cuda.synchronize()
    return int((d2 != 0).sum()), int((ws[:4 * v].view(torch.int32) != 0).sum())


def _leg(pp, mask, sampling, warmup, reps):
    shape = tuple(mask.shape)
    calls = {"local_thickness": lambda: pp.local_thickness(mask, sampling=sampling),
             "edt_squared": lambda: pp.distance_transform_edt(mask, sampling=sampling, squared=True)}
    res = {"shape": list(shape), "voxels": shape[0] * shape[1] * shape[2], "sampling": list(sampling) if sampling else None,
           "workspace_mb": round(pp.thickness_workspace_bytes(1, shape, sampling) / 1e6, 1), "device_ms": {}}
    for name, fn in calls.items():
        ms = _time(fn, warmup, reps)
        res["device_ms"][name] = {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
                                  "max_ms": round(max(ms), 3), "back_to_back_ms": round(_stream_ms(fn, reps), 3)}
        torch.cuda.empty_cache()
    t = pp.local_thickness(mask, sampling=sampling)
    ms = _time(lambda: pp.thickness_summary(t, 2.0), warmup, reps)
    res["device_ms"]["thickness_summary"] = {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
                                             "max_ms": round(max(ms), 3),
                                             "back_to_back_ms": round(_stream_ms(lambda: pp.thickness_summary(t, 2.0), reps), 3)}
    res["summary_count_min_max_mean_below2"] = [float(x) for x in pp.thickness_summary(t, 2.0).cpu()]
    del t
    before, after = _candidates(pp, mask, sampling)
    res["candidates"] = {"foreground": before, "kept": after}
    return res


def _check(pp, full):
    import numpy as np
    import thickness_ref as R
    crop = full[CROP].contiguous()
    out = {"crop": [48, 64, 64], "foreground": int(crop.sum())}
    for name, s in (("unit", None), ("aniso", SPACING)):
        d2 = pp.distance_transform_edt(crop, sampling=s, squared=True).cpu().numpy()
        ref = R.local_thickness(d2, s)
        got = pp.local_thickness(crop, sampling=s).cpu().numpy()
        out[name + "_bit_equal"] = bool(np.array_equal(got, ref))
        out[name + "_max"] = float(ref.max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--inputs", default="shell_unit,shell_aniso,plate,ball")
    ap.add_argument("--ball-radius", type=int, default=60)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ctunet_amd import postprocess as pp
    dev = torch.device("cuda", 0)
    res = {}
    for name in [n for n in args.inputs.split(",") if n]:
        if name in ("shell_unit", "shell_aniso"):
            mask, sampling = _scene(SHAPE, dev)[0], (None if name == "shell_unit" else SPACING)
        elif name == "plate":
            mask, sampling = _plate(SHAPE, dev), None
        elif name == "ball":
            mask, sampling = _ball(args.ball_radius, dev), None
            name = "ball_r%d" % args.ball_radius
        else:
            raise SystemExit(f"unknown input {name!r}")
        leg = _leg(pp, mask, sampling, args.warmup, args.reps)
        leg.update(reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
                   foreground_fraction=round(float(mask.float().mean()), 4))
        res[name] = leg
        print(json.dumps({name: leg}), flush=True)
        del mask
        torch.cuda.empty_cache()
    if args.check:
        res["check_vs_unpruned_reference"] = _check(pp, _scene(SHAPE, dev)[0])
        print(json.dumps({"check_vs_unpruned_reference": res["check_vs_unpruned_reference"]}), flush=True)
    if args.out:
        path = os.path.join(args.out, "thickness_bench.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.update(res)
        with open(path, "w") as f:
            f.write(json.dumps(old, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
