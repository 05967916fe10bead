"""The direct input-gradient kernel of the first encoder convolution (first_bwd_data_kernel, csrc/conv3d_first.hip) through
its two entry points, ctu_conv3d_first_bwd_data and ctu_lp_conv3d_first_bwd_data, against float64 autograd of F.conv3d.

A lane pair of the kernel owns four consecutive w outputs of one (d, h) row of a 4 x 4 x 32 box; the even lane sums gradient
channels 0-3 and the odd lane 4-7.  The volumes are the smallest at which that mapping can go wrong:
  4 x 4 x 32 .......... exactly one box
  5 x 6 x 33 .......... ragged boxes in d, h and w, with a one-voxel w tail (odd W: the scalar stores)
  4 x 4 x 16 .......... narrower than a box
  2 x (8 x 8 x 64) .... several boxes per block, a batch boundary
with 1 and 2 input channels, 8 and 6 output channels (the two padded gradient channels hold a finite sentinel and must
contribute nothing), the gradient as a whole 8-channel buffer and as the upper half of a 16-channel one, and dx at an 8-byte
aligned and at an odd 4-byte address (paired resp. single stores).  The gradient's border voxels are pushed away from zero by
a fixed amount, so a halo that is dropped, or read where it should be zero, moves every border output by far more than the gate.

The 16-bit cases call the entry point itself: ops.conv_first_bwd_data sends volumes at least 32 wide to the matrix-pipe route.

Gates (those of test_ops_gpu.py::test_first_layer_direct_kernels and of the first-layer part of test_lowp_gpu.py):
  fp32 gradient ....... 1e-5 of max |ref|
  16-bit gradient ..... 2 ulp of the type times max |ref|, the gradient rounded to the type first (weights stay fp32)
dx sits inside a NaN-filled buffer with sentinel guards on both sides: every element must be written, nothing outside it."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
GATE = {"fp32": 1e-5, "bf16": 2 * 2.0 ** -8, "fp16": 2 * 2.0 ** -11}
SENT = 7.0
GUARD = 64                                   # floats on either side of dx
VOLUMES = [(1, 4, 4, 32), (1, 5, 6, 33), (1, 4, 4, 16), (2, 8, 8, 64)]
# (Co, voxel stride of the gradient, dx offset in floats past an aligned address): every pair of values occurs
LAYOUTS = [(8, 8, 0), (6, 16, 0), (8, 16, 1), (6, 8, 1)]


def _ops():
    from ctunet_amd import ops
    return ops


@functools.lru_cache(maxsize=None)
def problem(vol, cin, co):
    """(weights, gradient with its border pushed off zero, float64 dx per dtype) of a case; shared by dtypes and layouts."""
    n, d, h, w = vol
    g = torch.Generator().manual_seed(1000 * cin + 10 * co + d + h + w)
    wt = torch.randn(co, cin, 3, 3, 3, generator=g) * 0.3
    go = torch.randn(n, co, d, h, w, generator=g)
    border = torch.ones(d, h, w, dtype=torch.bool)
    border[1:-1, 1:-1, 1:-1] = False
    go = torch.where(border, go + torch.where(go >= 0, 2.0, -2.0), go)
    refs = {}
    for name, dt in DT.items():
        gr = go.to(dt).double()
        x = torch.zeros(n, cin, d, h, w, dtype=torch.float64, requires_grad=True)
        F.conv3d(x, wt.double(), None, 1, 1).backward(gr)
        refs[name] = x.grad
    return wt, go, refs


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"co{l[0]}-gcs{l[1]}-off{l[2]}")
@pytest.mark.parametrize("cin", [1, 2])
@pytest.mark.parametrize("vol", VOLUMES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("dt", ["fp32", "bf16", "fp16"])
def test_first_dx(dt, vol, cin, layout):
    ops = _ops()
    co, g_cs, off = layout
    n, d, h, w = vol
    wt, go, refs = problem(vol, cin, co)
    ref = refs[dt]
    c0 = g_cs - 8
    gbuf = torch.full((n, d, h, w, g_cs), SENT, dtype=DT[dt])
    gbuf[..., c0:c0 + co] = go.permute(0, 2, 3, 4, 1).to(DT[dt])
    gc = ops.CL(gbuf.cuda(), c0, 8)
    numel = n * cin * d * h * w
    flat = torch.full((GUARD + off + numel + GUARD,), SENT, device="cuda")
    flat[GUARD + off:GUARD + off + numel] = float("nan")
    ops._dual(gc.lp, "conv3d_first_bwd_data", gc.ptr, gc.cs, wt.cuda().data_ptr(), cin, co, ops._ptr(flat, GUARD + off), n, d, h, w,
              ops._stream())
    torch.cuda.synchronize()
    flat = flat.cpu()
    got = flat[GUARD + off:GUARD + off + numel].view(n, cin, d, h, w)
    assert torch.all(flat[:GUARD + off] == SENT) and torch.all(flat[GUARD + off + numel:] == SENT), "dx was written outside its planes"
    assert not torch.isnan(got).any(), f"{int(torch.isnan(got).sum())} elements of dx were not written"
    err = (got.double() - ref).abs()
    scale = ref.abs().max().item()
    print(f"{dt} {vol} cin {cin} {layout}: max |err| / max |ref| = {err.max().item() / scale:.3e} (gate {GATE[dt]:.3e})")
    i = [int(v) for v in torch.unravel_index(err.flatten().argmax(), err.shape)]
    assert err.max().item() <= GATE[dt] * scale, f"worst |err| {err.max().item():.3e} (max |ref| {scale:.3e}) at (n, ci, d, h, w) = {i}"
