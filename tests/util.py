"""Shared helpers for the test-suite (test infrastructure, not product code)."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_npz(name):
    z = np.load(os.path.join(GOLDEN, name))
    return {k: z[k] for k in z.files}


def load_json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def sd_from(rec, prefix="sd."):
    return {k[len(prefix):]: torch.from_numpy(np.array(v)) for k, v in rec.items() if k.startswith(prefix)}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def onehot_target(shape, seed, p=0.3):
    """Same generator as tests/golden/make_golden.py::onehot_target."""
    n, _, d, h, w = shape
    m = (torch.rand(n, d, h, w, generator=gen(seed)) < p).long()
    return torch.nn.functional.one_hot(m, 2).movedim(4, 1).float().contiguous()


def summarize(t):
    """Same statistics as make_golden.summarize."""
    f = t.detach().flatten().double().cpu()
    idx = torch.linspace(0, f.numel() - 1, 16).long()
    return {"mean": f.mean().item(), "std": f.std().item(), "abs_sum": f.abs().sum().item(), "sample": f[idx].tolist()}


def close_summary(got, exp, rtol, atol):
    ok = abs(got["mean"] - exp["mean"]) <= atol + rtol * abs(exp["mean"])
    ok &= abs(got["std"] - exp["std"]) <= atol + rtol * abs(exp["std"])
    ok &= abs(got["abs_sum"] - exp["abs_sum"]) <= rtol * abs(exp["abs_sum"]) + atol
    ok &= bool(np.allclose(got["sample"], exp["sample"], rtol=rtol, atol=atol))
    return ok


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


CLASS_INPUT = {  # name -> (in_ch, size) as in make_golden.class_checksums
    "UNet": (1, 32), "UNet4b2i3o": (2, 32), "UNet5b2i3o": (2, 64), "UNet4b1i3o": (1, 32), "UNetSP": (2, 32),
    "UNetSPSmall": (2, 64), "UNetDO": (1, 32), "recAE_v2_fixed": (1, 32), "UNet4_2IC": (2, 32),
}


def fp64_rule_misses(checks, g64, full_size, report=None, floor=None):
    """The fp64 rule for gradients (test_models_gpu.oracle_train_check and the module-lifecycle tests share it).
    checks: [(name, got, ATen-CPU fp32 gradient, fp64 oracle gradient)]; g64: the fp64 oracle's gradients by parameter
    name; full_size: patch of at least 128^3; floor: the rule's floor as a fraction of the tensor's largest fp64 entry in place of
    the one full_size selects (tests/test_mask_stable_gpu.py: 1e-4, on states whose ReLU masks cannot flip).  Returns the list
    of misses (empty = pass)."""
    def err(a, b):
        return (a.detach().cpu().double() - b).abs().max().item()
    # One ReLU mask (or pooling arg-max) that flips on fp32 rounding noise changes a weight-gradient entry -- a sum of N
    # randomly signed terms, N = voxels of the layer -- by ~1/sqrt(N) of its magnitude: 5e-3 at 32^3, 1.6e-2 at the 16^3
    # level below, 7e-4 at 128^3; either implementation may flip, at different places (scripts/diag_grad_layers.py on
    # UNetDO: this path flips once in u_blocks.2 (5e-3), ATen-CPU once in u_blocks.1 (up to 6e-2); on other inputs
    # neither does; UNet4b1i3o seed 1234: 4.8e-2 on u_blocks.2.block.4.weight, a 16^3 layer, = three flips).  So the
    # floor of the rule is 2e-3 of scale where one flip stays below it (>= 128^3, the full-size tests); on the small
    # patches of the per-class runs it is a loose 6e-2, backed by the DIRECTION of every gradient tensor against the fp64
    # oracle (a handful of flips moves the cosine by ~1e-3; a wrong tap, stride or missing term moves it by far more).
    if floor is None:
        floor = 2e-3 if full_size else 6e-2
    misses = []
    for n_, got, c32, r64 in checks:
        scale = r64.abs().max().item()
        if report is not None:       # tests/arbitrate_fullsize.py: (tensor, scale, HIP vs fp64, ATen-CPU fp32 vs fp64, cosines)
            cs = lambda u: float(torch.dot(u.detach().cpu().double().flatten(), r64.flatten())
                                 / (u.detach().cpu().double().norm() * r64.norm() + 1e-300))
            report.append((n_, scale, err(got, r64), err(c32, r64), cs(got), cs(c32)))
        if err(got, r64) > max(5 * err(c32, r64), floor * scale) + 1e-7:
            misses.append((n_, err(got, r64), err(c32, r64), scale))
        a, b = got.detach().cpu().double().flatten(), r64.flatten()
        w64 = g64.get(n_[:-4] + "weight") if n_.endswith(".bias") else None
        if w64 is not None and w64.dim() == 5 and b.norm() < 1e-3 * w64.norm():
            continue                                   # conv bias in front of a BatchNorm: the true gradient is zero
        if float(torch.dot(a, b) / (a.norm() * b.norm())) < 0.995:
            misses.append((n_, "cosine", float(torch.dot(a, b) / (a.norm() * b.norm()))))
    return misses
