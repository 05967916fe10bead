"""The software pipelines of the fp32 ConvTranspose3d(k = 2, s = 2) kernels (csrc/convt.hip) at the smallest shapes at which they
can go wrong, through ops.convt_fwd / convt_bwd_data / convt_wgrad, against float64 autograd of F.conv_transpose3d.

convt2_kernel fetches the next weight stage and (data gradient) the next tap's gather into registers under the current
stage's MFMAs and reads the fragments of the next pair of 8-channel groups ahead of the current pair's MFMAs; what can break is a
stage swapped too early or too late, a fragment read that runs past the stage, and the group a pair does not cover.  So:
  reduction side (padded) .... 8 (one group), 24 (odd: three), 64 (even), 128 (four taps per weight stage at these volumes)
  output side (padded) ....... 8, 32, 128
  coarse volumes ............. 4 x 4 x 4 (exactly one 64-voxel block), 5 x 4 x 4 (a second, partial block), 2 x (8 x 8 x 8), and
                               D x 8 x 8 with D tiles = the weight gradient's planned grid.x + 3, so that three blocks of its
                               tile loop take one tile more than the others (the plan query gives grid.x)
Every case runs the forward and the weight gradient with and without the lazy-BatchNorm input transform, the forward with and
without bias, and the data gradient; one more case is the 128 -> 128 level at 16^3 (two taps per stage, 256 blocks) and one has
a concat input with padded holes.  Every operand is a channel slice at offset 8 of a buffer 16 channels wider (so the output's
voxel stride exceeds its padded channels), and the neighbours and the padded channels are checked as in
tests/test_convt_plans_gpu.py, whose helpers and gate this file uses: 1e-4 of max |ref| for the output, dx, dW and db.

Every case also asserts that the launch plans are what they were before the pipelines: ctu_convt2_plan and
ctu_convt2_wgrad_plan against the inline arithmetic kept in tests/test_convt_plans_cpu.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

import convt_ref
from test_convt_plans_cpu import Case, case_plans, cdiv, old_convt, old_convt_wgrad
from test_convt_plans_gpu import (HOLES, Data, _id, check_neighbours_and_padding, far_outside, from_slice, gate, sentinel_slice,
                                  to_slice)

pytestmark = pytest.mark.gpu

TOL = 1e-4
RIN = (8, 24, 64, 128)
NOUT = (8, 32, 128)


def uneven_volume(ci, co):
    """D x 8 x 8 (one 64-voxel tile per d plane) with three tiles more than the weight gradient's full grid.x."""
    pairs = cdiv(ci, 32 if ci > 16 else 16) * cdiv(co, 32 if co > 16 else 16)
    return (1, max(512 // pairs, 1) + 3, 8, 8)


def volumes(ci, co):
    return [(1, 4, 4, 4), (1, 5, 4, 4), (2, 8, 8, 8), uneven_volume(ci, co)]


CASES = [Case("fp32", ci, co, *v, None, ()) for ci in RIN for co in NOUT for v in volumes(ci, co)]
CASES.append(Case("fp32", 128, 128, 1, 16, 16, 16, None, ()))          # two taps per weight stage on a split grid of 256 blocks
CASES.append(Case("fp32", 14, 14, 2, 8, 8, 8, HOLES, ()))


class Refs:
    """float64 autograd of F.conv_transpose3d on the CPU, once per case and input transform."""

    def __init__(self, D, xf):
        a = (D.a if xf else D.x.double()).clone().requires_grad_(True)
        w = D.wt.double().clone().requires_grad_(True)
        b = D.b.double().clone().requires_grad_(True)
        self.out = F.conv_transpose3d(a, w, b, stride=2)
        self.out.backward(D.go.double())
        self.out = self.out.detach()
        self.out_nobias = self.out - D.b.double().view(1, -1, 1, 1, 1)
        self.dx, self.dw, self.db = a.grad, w.grad, b.grad


@functools.lru_cache(maxsize=1)
def setup(c):
    D = Data(c)
    return D, Refs(D, True), Refs(D, False)


def check_plans(c, cip, cop):
    """The launch plans of the case, which must be the inline arithmetic of the launchers before the plan functions."""
    nvox = c.N * c.D * c.H * c.W
    p = case_plans(c)
    ntt, gx, gy, tps, lds = old_convt(cip, cop, nvox)
    assert p.fwd == (f"convt2_kernel<{ntt}, 0>", gx, gy, tps, lds), p.fwd
    ntt, gx, gy, tps, lds = old_convt(cop, cip, nvox)
    assert p.dgrad == (f"convt2_kernel<{ntt}, 1>", gx, gy, tps, lds), p.dgrad
    mi, nj, gx, gy, ntiles = old_convt_wgrad(cip, cop, nvox)
    assert p.wgrad == (f"convt2_wgrad_kernel<{mi}, {nj}>", gx, gy, ntiles), p.wgrad
    return p


@pytest.mark.parametrize("c", [pytest.param(c, id=_id(c)) for c in CASES])
def test_convt_pipeline(c):
    from ctunet_amd import ops
    n, d, h, w = c.N, c.D, c.H, c.W
    D, ref_xf, ref_id = setup(c)
    cip, cop, pos = D.cip, D.cop, D.pos
    opos = list(range(c.Co))
    imap, cinv = D.maps()
    plan = check_plans(c, cip, cop)
    if (d, h, w) == uneven_volume(cip, cop)[1:] and c.segs is None:
        assert plan.wgrad[3] == plan.wgrad[1] + 3, plan.wgrad          # tiles = grid.x + 3: an uneven tile loop
    if cip == 128:
        assert plan.fwd[3] == (2 if d == 16 else 4), plan.fwd           # the 128-channel reduction side: more than one weight stage

    wp = ops.pack_convt_w(D.wt.cuda(), cinv, cip, cop, 0)
    gc = to_slice(D.go, opos, cop, "fp32")
    for xf, ref in ((True, ref_xf), (False, ref_id)):
        xc = to_slice(D.x, pos, cip, "fp32")
        if xf:
            xc = xc.with_xf(D.sc.cuda(), D.sh.cuda(), True)
        bias = D.b.cuda() if xf else None                               # transform with bias, no transform without
        out = sentinel_slice(n, 2 * d, 2 * h, 2 * w, cop, "fp32")
        ops.convt_fwd(xc, wp, bias, out)
        torch.cuda.synchronize()
        gate(c, f"output (xf {xf})", from_slice(out, opos), ref.out if xf else ref.out_nobias, TOL)
        check_neighbours_and_padding(c, out, opos, "output")

        ws = torch.full((ops.convt_wgrad_ws((n, d, h, w), cip, cop),), float("nan"), device="cuda")      # every slab must be written
        dw, db = ops.convt_wgrad(xc, gc, c.Ci, c.Co, imap, ws)
        torch.cuda.synchronize()
        gate(c, f"dW (xf {xf})", dw.cpu(), ref.dw, TOL)
        gate(c, f"db (xf {xf})", db.cpu(), ref.db, TOL)

    wpd = ops.pack_convt_w(D.wt.cuda(), cinv, cop, cip, 1)
    gin = sentinel_slice(n, d, h, w, cip, "fp32")
    ops.convt_bwd_data(gc, wpd, gin)
    torch.cuda.synchronize()
    gate(c, "dx", from_slice(gin, pos), ref_xf.dx, TOL)
    check_neighbours_and_padding(c, gin, pos, "dx")

    if c.segs is not None:          # a kernel that ignored the channel maps would produce these: they must miss the gate by far
        xb = torch.zeros(n, cip, d, h, w, dtype=torch.float64)
        xb[:, pos] = D.a
        far_outside(c, "output", convt_ref.forward(xb[:, :c.Ci], D.wt, D.b), ref_xf.out, TOL)
        far_outside(c, "dW", convt_ref.weight_gradient(xb[:, :c.Ci], D.go)[0], ref_xf.dw, TOL)
