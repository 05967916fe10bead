"""Per-op checks of the large-volume convolution routes against fp64 references.

The per-op suites (test_ops_gpu.py, test_lowp_gpu.py) use small volumes and so mostly reach the small-volume kernels.  The
cases here land on the routes the training sizes take -- the persistent kernels that loop over several boxes per block,
the wider channel tiles, the fused up-convolutions and first-layer kernels -- at two or more boxes per block and with
partial boxes, so the loop over a block's second box (prefetch, accumulator reset, the stats row one block writes for
several boxes) runs under a tight gate.  tests/test_routes_cpu.py checks, without a GPU, that each case still lands on the
route it names and that every route the shipped classes reach has a case.

Gates (the per-op suites' gates, references in fp64):
  fp32 outputs and data gradients ........ 1e-4 of max |ref|
  16-bit stored outputs .................. one 16-bit ulp of max |ref|, on inputs already rounded to 16 bits
  16-bit fused up-convolution ............ 6 ulps (the composite weights are rounded once more: test_lowp_gpu.py)
  weight gradients ....................... 1e-4 of max |ref| (fused up-convolution: 2e-4 fp32, 2e-3 16-bit, as per-op suites)
  raw-output gradients of the lazy path .. 2e-4 (fp32), 2 ulps (16-bit)
  first layer ............................ 1e-5 of max |ref| for fp32 outputs and every float32 data gradient (the 16-bit
                                           routes accumulate exact products in float32, like the fp32 kernel); 16-bit stored
                                           outputs one ulp and bit-equal to the rounded fp32 kernel's
A failure names the worst voxel, its box and the block that ran the box."""
import zlib

import pytest
import torch
import torch.nn.functional as F

from test_routes_cpu import Case, cdiv, pad8, route

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
SENT = 7.0

# (route, op, dtype, N, Ci, Co, D, H, W, k, transform, cs, c0): cs / c0 = channel stride and offset of the output (or of
# the gradient / raw-output buffers of the lazy path); 0 = the default (a slice at offset 8 of a buffer 8 channels wider).
# Up-convolution cases give the COARSE volume; Ci is the transposed conv's channel count.
CASES = [
    # ---- fp32 forward / data gradient (mode-1 packing through the same kernels)
    Case("conv3d_fwd_k3_persist<1, false>", "fwd", "fp32", 1, 14, 16, 36, 64, 136, 3, True, 0, 0),
    Case("conv3d_fwd_k3_persist<1, false>", "dgrad", "fp32", 1, 14, 28, 52, 60, 52, 3, False, 0, 0),
    Case("conv3d_fwd_k3_persist<2, false>", "fwd", "fp32", 1, 16, 28, 36, 60, 132, 3, True, 0, 0),
    Case("conv3d_fwd_k3_persist<2, false>", "dgrad", "fp32", 1, 28, 14, 44, 64, 36, 3, False, 0, 0),
    Case("conv3d_fwd_k3_persist<1, true>", "fwd", "fp32", 1, 14, 7, 44, 64, 68, 3, True, 0, 0),
    Case("conv3d_fwd_k3_persist<1, true>", "dgrad", "fp32", 1, 7, 14, 44, 64, 68, 3, False, 0, 0),
    Case("conv3d_fwd_k5_persist<1, true>", "fwd", "fp32", 1, 8, 7, 40, 52, 36, 5, True, 0, 0),
    Case("conv3d_fwd_kernel<5, 1, 4, 4, 16>", "fwd", "fp32", 1, 14, 28, 6, 128, 18, 5, True, 0, 0),
    Case("conv3d_fwd_kernel<5, 2, 4, 4, 16>", "dgrad", "fp32", 1, 56, 14, 6, 128, 18, 5, False, 0, 0),
    Case("conv3d_fwd_kernel<3, 1, 4, 8, 8>", "fwd", "fp32", 1, 32, 14, 64, 60, 10, 3, True, 0, 0),
    Case("conv3d_fwd_kernel<5, 1, 4, 8, 8>", "fwd", "fp32", 1, 32, 14, 64, 60, 10, 5, True, 0, 0),
    # ---- fp32 weight gradient
    Case("conv3d_wgrad_k3s_kernel<1, 1>", "wgrad", "fp32", 1, 14, 28, 6, 40, 100, 3, True, 0, 0),
    Case("conv3d_wgrad_k3s_kernel<1, 1>", "wgrad", "fp32", 2, 16, 16, 36, 36, 40, 3, True, 0, 0),
    Case("conv3d_wgrad_k3s_kernel<2, 1>", "wgrad", "fp32", 1, 7, 14, 6, 64, 132, 3, True, 0, 0),
    Case("conv3d_wgrad_k3s_kernel<1, 2>", "wgrad", "fp32", 1, 14, 7, 6, 64, 132, 3, True, 0, 0),
    Case("conv3d_wgrad_k3s_kernel<2, 2>", "wgrad", "fp32", 1, 7, 7, 44, 64, 36, 3, True, 0, 0),
    Case("conv3d_wgrad_k5s_kernel<2, 1>", "wgrad", "fp32", 1, 7, 14, 10, 48, 18, 5, True, 0, 0),
    Case("conv3d_wgrad_k5s_kernel<1, 2>", "wgrad", "fp32", 1, 14, 7, 10, 48, 18, 5, True, 0, 0),
    Case("conv3d_wgrad_k5s_kernel<2, 2>", "wgrad", "fp32", 1, 7, 7, 16, 52, 18, 5, True, 0, 0),
    Case("conv3d_wgrad_kernel<5, 1, 4, 4, 4>", "wgrad", "fp32", 1, 28, 14, 6, 52, 6, 5, True, 0, 0),
    Case("conv3d_wgrad_kernel<5, 1, 4, 8, 8>", "wgrad", "fp32", 1, 16, 14, 52, 28, 10, 5, True, 0, 0),
    Case("conv3d_wgrad_kernel<3, 3, 4, 8, 8>", "wgrad", "fp32", 1, 16, 14, 80, 104, 10, 3, True, 0, 0),
    Case("conv3d_wgrad_kernel<3, 3, 4, 4, 4>", "wgrad", "fp32", 1, 16, 14, 40, 104, 6, 3, True, 0, 0),
    # ---- fp32 weight gradient with the lazy BatchNorm + ReLU backward (volumes: multiples of the box)
    Case("conv3d_wgrad_k3s_kernel<1, 1>+LZ", "wgrad_bn", "fp32", 1, 14, 14, 16, 40, 104, 3, True, 32, 16),
    Case("conv3d_wgrad_k3s_kernel<2, 1>+LZ", "wgrad_bn", "fp32", 1, 7, 14, 16, 40, 104, 3, True, 16, 0),
    Case("conv3d_wgrad_k3s_kernel<1, 2>+LZ", "wgrad_bn", "fp32", 1, 14, 7, 16, 40, 104, 3, True, 16, 8),
    Case("conv3d_wgrad_k3s_kernel<2, 2>+LZ", "wgrad_bn", "fp32", 1, 7, 7, 20, 52, 128, 3, True, 8, 0),
    # ---- 16-bit forward / data gradient / weight gradient
    Case("lp_conv_fwd_p1_kernel<4x16>", "fwd", "bf16", 1, 28, 16, 64, 64, 52, 3, True, 0, 0),
    Case("lp_conv_fwd_p1_kernel<8x16>", "fwd", "fp16", 1, 14, 16, 64, 60, 120, 3, True, 0, 0),
    Case("lp_conv_fwd_p1_kernel<4x16>", "dgrad", "fp16", 1, 28, 28, 64, 64, 52, 3, False, 0, 0),
    Case("lp_conv_fwd_p1_kernel<8x16>", "dgrad", "bf16", 1, 14, 14, 64, 60, 120, 3, False, 0, 0),
    Case("lp_conv_fwd_pair_kernel", "fwd", "bf16", 1, 7, 8, 112, 112, 36, 3, True, 0, 0),
    Case("lp_conv_fwd_pair_kernel", "dgrad", "fp16", 1, 8, 7, 112, 112, 36, 3, False, 0, 0),
    Case("lp_wgrad8_kernel", "wgrad", "bf16", 1, 7, 8, 40, 104, 128, 3, True, 0, 0),
    Case("lp_wgrad16_kernel", "wgrad", "fp16", 1, 14, 28, 52, 40, 40, 3, True, 0, 0),
    Case("lp_conv_wgrad_kernel", "wgrad", "bf16", 1, 7, 14, 52, 60, 100, 3, True, 0, 0),
    Case("lp_wgrad8_kernel+LZ", "wgrad_bn", "fp16", 1, 7, 8, 40, 104, 128, 3, True, 16, 8),
    Case("lp_wgrad16_kernel+LZ", "wgrad_bn", "bf16", 1, 14, 14, 52, 40, 128, 3, True, 32, 0),
    Case("lp_conv_wgrad_kernel+LZ", "wgrad_bn", "bf16", 1, 7, 14, 52, 60, 128, 3, True, 16, 0),
    # ---- fp32 fused up-convolution (COARSE dims)
    Case("upconv_fused_fwd_kernel<8, 1>", "up_fwd", "fp32", 1, 8, 16, 40, 104, 18, 3, True, 0, 0),
    Case("upconv_fused_fwd_kernel<4, 1>", "up_fwd", "fp32", 1, 8, 16, 6, 40, 36, 3, True, 0, 0),
    Case("upconv_fused_fwd_kernel<4, 1, true>", "up_fwd", "fp32", 1, 8, 7, 40, 104, 18, 3, True, 0, 0),
    Case("upconv_fused_fwd_kernel<4, 2>", "up_fwd", "fp32", 1, 8, 28, 40, 52, 18, 3, True, 0, 0),
    Case("upconv_fused_fwd_kernel<2, 4>", "up_fwd", "fp32", 1, 8, 56, 20, 52, 18, 3, True, 0, 0),
    Case("upconv_fused_bwd_data_kernel<1>", "up_dgrad", "fp32", 1, 14, 16, 40, 104, 18, 3, False, 0, 0),
    Case("upconv_fused_bwd_data_kernel<2>", "up_dgrad", "fp32", 1, 28, 8, 44, 64, 36, 3, False, 0, 0),
    Case("upconv_fused_bwd_data_kernel<4>", "up_dgrad", "fp32", 1, 56, 8, 44, 64, 36, 3, False, 0, 0),
    Case("conv3d_wgrad_k3s_kernel<1, 1, 1>", "up_wgrad", "fp32", 1, 14, 16, 6, 6, 132, 3, True, 0, 0),
    Case("conv3d_wgrad_k3s_kernel<1, 1, 2>", "up_wgrad", "fp32", 1, 14, 7, 10, 60, 18, 3, True, 0, 0),
    Case("conv3d_wgrad_k3s_kernel<1, 1, 1>+LZ", "up_wgrad_bn", "fp32", 1, 14, 16, 4, 20, 104, 3, True, 16, 0),
    Case("conv3d_wgrad_k3s_kernel<1, 1, 2>+LZ", "up_wgrad_bn", "fp32", 1, 14, 7, 4, 40, 104, 3, True, 8, 0),
    # ---- 16-bit fused up-convolution (COARSE dims; 8 padded outputs, input channels a multiple of 32)
    Case("lp_upconv_fwd_kernel", "up_fwd", "bf16", 1, 28, 7, 40, 52, 18, 3, True, 0, 0),
    Case("lp_upconv_bwd_data_kernel<2>", "up_dgrad", "fp16", 1, 28, 7, 40, 52, 18, 3, False, 0, 0),
    Case("lp_upconv_bwd_data_kernel<4>", "up_dgrad", "bf16", 3, 64, 7, 6, 88, 18, 3, False, 0, 0),
    Case("lp_upwg4_kernel", "up_wgrad", "bf16", 1, 28, 7, 20, 52, 128, 3, True, 0, 0),
    Case("lp_upwg_kernel<16>", "up_wgrad", "fp16", 1, 28, 7, 40, 36, 18, 3, True, 0, 0),
    Case("lp_upwg_kernel<32>", "up_wgrad", "bf16", 1, 28, 7, 28, 28, 36, 3, True, 0, 0),
    Case("lp_upwg_kernel<16>+LZ", "up_wgrad_bn", "bf16", 1, 28, 7, 40, 80, 16, 3, True, 8, 0),
    Case("lp_upwg_kernel<32>+LZ", "up_wgrad_bn", "fp16", 1, 28, 7, 28, 28, 64, 3, True, 8, 0),
    # ---- fp32 first layer (C_in <= 2, NCDHW input)
    Case("first_fwd_kernel<1>", "first_fwd", "fp32", 1, 1, 7, 52, 64, 132, 3, False, 0, 0),
    Case("first_fwd_kernel<2>", "first_fwd", "fp32", 2, 2, 8, 44, 64, 68, 3, False, 0, 0),
    Case("first_bwd_data_kernel<1>", "first_dgrad", "fp32", 1, 1, 7, 100, 100, 36, 3, False, 0, 0),
    Case("first_bwd_data_kernel<2>", "first_dgrad", "fp32", 1, 2, 8, 52, 60, 100, 3, False, 0, 0),
    Case("first_wgrad_kernel<1>", "first_wgrad", "fp32", 1, 1, 7, 104, 104, 36, 3, False, 0, 0),
    Case("first_wgrad_kernel<2>", "first_wgrad", "fp32", 1, 2, 8, 104, 104, 36, 3, False, 0, 0),
    Case("first_wgrad_kernel<1>+LZ", "first_wgrad_bn", "fp32", 1, 1, 7, 104, 104, 36, 3, False, 16, 8),
    Case("first_wgrad_kernel<2>+LZ", "first_wgrad_bn", "fp32", 2, 2, 8, 96, 112, 36, 3, False, 8, 0),
    # ---- 16-bit first layer: the T = bf16 / half instantiations, the matrix-pipe data gradient with float32 planes (>= 32
    # wide) and the matrix-pipe weight gradient of large volumes (forced: first_wgrad_mfma).  Each volume is the smallest that
    # gives every block two boxes; outputs and gradients are a slice at offset 8 of a 16-channel sentinel-filled buffer.
    Case("first_fwd_kernel<1, T>", "first_fwd", "bf16", 1, 1, 7, 50, 62, 132, 3, False, 16, 8),
    Case("first_fwd_kernel<2, T>", "first_fwd", "fp16", 2, 2, 8, 44, 64, 68, 3, False, 16, 8),
    Case("lp_conv_fwd_pair_kernel<OUT32>", "first_dgrad", "fp16", 1, 1, 7, 110, 108, 36, 3, False, 16, 8),
    Case("lp_conv_fwd_pair_kernel<OUT32>", "first_dgrad", "bf16", 2, 2, 4, 54, 108, 36, 3, False, 16, 8),
    Case("first_bwd_data_kernel<2, T>", "first_dgrad", "fp16", 1, 2, 7, 100, 124, 24, 3, False, 16, 8),     # 16 <= W < 32
    Case("first_wgrad_kernel<1, T>", "first_wgrad", "bf16", 1, 1, 7, 104, 104, 36, 3, False, 16, 8),
    Case("first_wgrad_kernel<2, T>", "first_wgrad", "fp16", 2, 2, 8, 50, 106, 36, 3, False, 16, 8),
    Case("lp_wgrad8_kernel<first>", "first_wgrad_mfma", "bf16", 1, 2, 7, 40, 104, 128, 3, False, 16, 8),
    Case("lp_wgrad8_kernel<first>", "first_wgrad_mfma", "fp16", 2, 1, 4, 20, 104, 128, 3, False, 16, 8),
]


def _ops():
    from ctunet_amd import ops
    return ops


def _id(c):
    return f"{c.op}-{c.dtype}-{c.route}-{c.N}x{c.Ci}x{c.Co}x{c.D}x{c.H}x{c.W}"


def gen(c, salt=0):
    return torch.Generator().manual_seed((zlib.crc32(repr(tuple(c)).encode()) + salt) % (1 << 31))


def rnd(x, dt):
    return x.to(DT[dt]).float() if dt != "fp32" else x


def to_cl(x, cp, dt, cs=None, c0=0, fill=0.0):
    """NCDHW (CPU) -> channels-last GPU buffer of width cs with x at [c0, c0 + C), padding zeros, other channels = fill."""
    ops = _ops()
    n, c, d, h, w = x.shape
    cs = cs or cp
    buf = torch.full((n, d, h, w, cs), fill, dtype=DT[dt])
    v = torch.zeros(n, d, h, w, cp)
    v[..., :c] = x.permute(0, 2, 3, 4, 1)
    buf[..., c0:c0 + cp] = v.to(DT[dt])
    return ops.CL(buf.cuda(), c0, cp)


def from_cl(a, c):
    return a.buf[..., a.c0:a.c0 + c].float().permute(0, 4, 1, 2, 3).contiguous().cpu()


def xform(c, cp, x):
    """Input transform vectors (BatchNorm scale / shift + ReLU of the previous layer) and the transformed input."""
    g = gen(c, 7)
    sc = torch.zeros(cp)
    sh = torch.zeros(cp)
    sc[:c.Ci] = torch.rand(c.Ci, generator=g) * 1.5 - 0.25
    sh[:c.Ci] = torch.randn(c.Ci, generator=g) * 0.3
    return sc, sh, F.relu(x * sc[:c.Ci].view(1, -1, 1, 1, 1) + sh[:c.Ci].view(1, -1, 1, 1, 1))


def where(c, got, ref, scale=None, fine=False):
    """Worst voxel of got - ref, with the box and block (tiles are dealt to blocks in runs of tpb) that computed it."""
    err = (got.double() - ref.double()).abs()
    i = int(err.flatten().argmax())
    n, ch, d, h, w = [int(v) for v in torch.unravel_index(torch.tensor(i), err.shape)]
    msg = f"{_id(c)}: worst |err| {err.flatten()[i].item():.3e} (scale {scale if scale is not None else ref.abs().max().item():.3e}) " \
          f"at n={n} c={ch} d={d} h={h} w={w}"
    r = route(c)
    if r.persistent:
        if fine:
            d, h, w = d // 2, h // 2, w // 2
        bd, bh, bw = r.box
        tile = ((n * cdiv(c.D, bd) + d // bd) * cdiv(c.H, bh) + h // bh) * cdiv(c.W, bw) + w // bw
        msg += f"; box ({d // bd}, {h // bh}, {w // bw}) = tile {tile} of {r.boxes}, block {tile // r.tpb} ({r.tpb} boxes per block)"
    return msg


def check(c, got, ref, tol_rel, fine=False):
    scale = ref.abs().max().item()
    err = (got.double() - ref.double()).abs().max().item()
    assert err <= tol_rel * scale, where(c, got, ref, scale, fine)


def check_w(c, name, got, ref, tol_rel):
    err = (got.cpu().double() - ref).abs().max().item()
    assert err <= tol_rel * ref.abs().max().item(), f"{_id(c)} {name}: max |err| {err:.3e}, scale {ref.abs().max().item():.3e}"


def out_buffer(n, d, h, w, cp, dt, c):
    """A slice of cp channels at offset 8 of a buffer 8 channels wider, everything filled with the sentinel."""
    ops = _ops()
    return ops.CL(torch.full((n, d, h, w, cp + 8), SENT, dtype=DT[dt], device="cuda"), 8, cp)


def check_sentinel_and_padding(c, out, creal):
    assert torch.all(out.buf[..., :out.c0].float() == SENT), f"{_id(c)}: the neighbouring channels were written"
    if out.cp > creal:
        pad = out.buf[..., out.c0 + creal:out.c0 + out.cp].float()
        assert torch.all(pad == 0), f"{_id(c)}: padded channels hold {pad.abs().max().item()}"


def bn_setup(c, y, co, cop):
    """BatchNorm vectors [4, cop] (scale, shift, mean, invstd) of y with random gamma / beta."""
    g = gen(c, 11)
    gamma = torch.rand(co, generator=g) * 1.5 - 0.25
    beta = torch.randn(co, generator=g) * 0.2
    mean = y.double().mean(dim=(0, 2, 3, 4))
    invstd = (1.0 / torch.sqrt(y.double().var(dim=(0, 2, 3, 4), unbiased=False) + 1e-5)).float()
    vec = torch.zeros(4, cop)
    vec[0, :co] = gamma * invstd
    vec[1, :co] = beta - mean.float() * gamma * invstd
    vec[2, :co] = mean.float()
    vec[3, :co] = invstd
    return gamma, beta, vec.cuda()


def bn_relu_grad64(y, gamma, beta, ga):
    """fp64 autograd: gradient w.r.t. y of relu(batch_norm(y)) (train mode) given ga."""
    y64 = y.double().requires_grad_(True)
    F.relu(F.batch_norm(y64, None, None, gamma.double(), beta.double(), True, 0.1, 1e-5)).backward(ga.double())
    return y64.grad


# ------------------------------------------------------------------ convolutions: forward / data gradient
@pytest.mark.parametrize("c", [pytest.param(c, id=_id(c)) for c in CASES if c.op in ("fwd", "dgrad")])
def test_conv_forward_and_data_gradient(c):
    ops = _ops()
    dt, k, n, d, h, w = c.dtype, c.k, c.N, c.D, c.H, c.W
    g = gen(c)
    if c.op == "fwd":
        ci, co = c.Ci, c.Co
    else:                       # the data gradient is a forward of the gradient with the mode-1 packing
        ci, co = c.Co, c.Ci
    rin, nout = pad8(ci), pad8(co)
    x = rnd(torch.randn(n, ci, d, h, w, generator=g), dt)
    wt = rnd(torch.randn(c.Co, c.Ci, k, k, k, generator=g) * (2.0 / (c.Ci * k ** 3)) ** 0.5, dt)
    xc = to_cl(x, rin, dt)
    a = x
    if c.xf:
        sc, sh, a = xform(c._replace(Ci=ci), rin, x)
        a = rnd(a, dt)
        xc = xc.with_xf(sc.cuda(), sh.cuda(), True)
    if dt == "fp32":
        lay = ops.conv_layout(k, nout, w)
        wp = ops.pack_conv_w(wt.cuda(), None, rin, nout, 0 if c.op == "fwd" else 1, lay)
    else:
        lay = ops.conv_layout(k, nout, w, DT[dt], rin)
        wp = ops.pack_conv_w_lp(wt.cuda(), None, rin, nout, 0 if c.op == "fwd" else 1, DT[dt], None, lay)
    out = out_buffer(n, d, h, w, nout, dt, c)
    stats = None
    if c.op == "fwd":
        nb = ops.conv_num_blocks((n, d, h, w), nout, lay, k, DT[dt], rin)
        stats = torch.full((nb, 2, nout), float("nan"), device="cuda")       # every row must be written
    ops.conv3d_fwd(xc, wp, None, out, k, stats, None, lay)
    torch.cuda.synchronize()
    if c.op == "fwd":
        ref = F.conv3d(a.double(), wt.double(), None, 1, (k - 1) // 2)
    else:
        ref = torch.nn.grad.conv3d_input((n, c.Ci, d, h, w), wt.double(), a.double(), 1, (k - 1) // 2)
    got = from_cl(out, co)
    check(c, got, ref, 1e-4 if dt == "fp32" else ULP[dt])
    check_sentinel_and_padding(c, out, co)
    if stats is not None:
        s = stats.sum(0).cpu().double()
        assert not torch.isnan(s).any(), f"{_id(c)}: a stats row was not written"
        base = ref if dt == "fp32" else got.double()                         # 16-bit: sums of the ROUNDED outputs
        s1, s2 = base.sum((0, 2, 3, 4)), (base * base).sum((0, 2, 3, 4))
        assert torch.allclose(s[0, :co], s1, rtol=1e-4, atol=1e-3 * s2.max().sqrt().item()), f"{_id(c)}: channel sums"
        assert torch.allclose(s[1, :co], s2, rtol=1e-4), f"{_id(c)}: channel sums of squares"
        assert float(s[:, co:].abs().max()) == 0.0 if nout > co else True


# ------------------------------------------------------------------ convolutions: weight gradient (+ lazy BatchNorm)
@pytest.mark.parametrize("c", [pytest.param(c, id=_id(c)) for c in CASES if c.op in ("wgrad", "wgrad_bn")])
def test_conv_weight_gradient(c):
    ops = _ops()
    dt, k, n, d, h, w = c.dtype, c.k, c.N, c.D, c.H, c.W
    g = gen(c)
    cip, cop = pad8(c.Ci), pad8(c.Co)
    x = rnd(torch.randn(n, c.Ci, d, h, w, generator=g), dt)
    sc, sh, a = xform(c, cip, x)
    a = rnd(a, dt)
    xc = to_cl(x, cip, dt).with_xf(sc.cuda(), sh.cuda(), True)
    ws = torch.empty(ops.conv3d_wgrad_ws((n, d, h, w), k, cip, cop, DT[dt]), device="cuda")
    ga = rnd(torch.randn(n, c.Co, d, h, w, generator=g), dt)
    if c.op == "wgrad":
        gc = to_cl(ga, cop, dt)
        dw, _ = ops.conv3d_wgrad(xc, gc, c.Co, c.Ci, k, None, ws, False)
        torch.cuda.synchronize()
        check_w(c, "dW", dw, torch.nn.grad.conv3d_weight(a.double(), (c.Co, c.Ci, k, k, k), ga.double(), 1, (k - 1) // 2), 1e-4)
        return
    cs, c0 = c.cs, c.c0
    assert ops.conv3d_wgrad_bn_supported((n, d, h, w), k, cip, cop, DT[dt])
    y = rnd(torch.randn(n, c.Co, d, h, w, generator=g) * 1.3 + 0.3, dt)
    gamma, beta, vec = bn_setup(c, y, c.Co, cop)
    yc, gac = to_cl(y, cop, dt, cs, c0, SENT), to_cl(ga, cop, dt, cs, c0, SENT)
    part = torch.empty(ops.bn_bwd_partials_floats(n * d * h * w, cop), device="cuda")
    _, _, coef = ops.bn_relu_bwd(yc, gac, vec, gamma.cuda(), c.Co, part, lazy=True)
    gy = ops.CL(torch.full_like(gac.buf, SENT), c0, cop)
    dw = ops.conv3d_wgrad_bn(xc, gac, yc, vec, coef, gy, c.Co, c.Ci, k, None, ws)
    torch.cuda.synchronize()
    gy64 = bn_relu_grad64(y, gamma, beta, ga)
    gy_k = from_cl(gy, c.Co)
    check(c, gy_k, gy64, 2e-4 if dt == "fp32" else 2 * ULP[dt])
    if cs > cop:
        other = torch.ones(cs, dtype=torch.bool)
        other[c0:c0 + cop] = False
        assert torch.all(gy.buf[..., other.cuda()].float() == SENT), f"{_id(c)}: channels outside the slice were written"
    # fp32: dW against fp64 autograd of conv(relu(batch_norm(y))); 16-bit: the kernel rounds the raw-output gradient to the
    # storage type before it multiplies, so dW is held to fp64 of the gradient it wrote (checked against fp64 just above)
    gref = gy64 if dt == "fp32" else gy_k.double()
    check_w(c, "dW", dw, torch.nn.grad.conv3d_weight(a.double(), (c.Co, c.Ci, k, k, k), gref, 1, (k - 1) // 2), 1e-4)


# ------------------------------------------------------------------ fused up-convolution (ConvTranspose3d 2/2 -> Conv3d 3)
def _up_setup(c):
    g = gen(c)
    n, d, h, w = c.N, c.D, c.H, c.W
    C, co = c.Ci, c.Co
    x = rnd(torch.randn(n, C, d, h, w, generator=g), c.dtype)
    wt = torch.randn(C, C, 2, 2, 2, generator=g) * (1.0 / C) ** 0.5
    bt = torch.randn(C, generator=g) * 0.1
    w3 = torch.randn(co, C, 3, 3, 3, generator=g) * (2.0 / (27 * C)) ** 0.5
    return x, wt, bt, w3


def _up_ref(a, wt, bt, w3, op):
    """fp64 reference of the two unfused ops; autograd only on the tensors the op's check needs (the data gradient of the
    wide cases is the most expensive reference of this file)."""
    a64 = a.double().requires_grad_(op == "up_dgrad")
    wt64, bt64, w364 = (t.double().requires_grad_(op.startswith("up_wgrad")) for t in (wt, bt, w3))
    return a64, wt64, bt64, w364, F.conv3d(F.conv_transpose3d(a64, wt64, bt64, stride=2), w364, padding=1)


@pytest.mark.parametrize("c", [pytest.param(c, id=_id(c)) for c in CASES if c.op.startswith("up_")])
def test_fused_upconv(c):
    ops = _ops()
    dt, n, d, h, w = c.dtype, c.N, c.D, c.H, c.W
    lp = dt != "fp32"
    C, co = c.Ci, c.Co
    cp, cop = pad8(C), pad8(co)
    x, wt, bt, w3 = _up_setup(c)
    sc, sh, a = xform(c, cp, x)
    a = rnd(a, dt)
    xc = to_cl(x, cp, dt).with_xf(sc.cuda(), sh.cuda(), True)
    wp32, beff, pws = ops.upconv_fused_pack(wt.cuda(), bt.cuda(), w3.cuda(), None, cp, cop)
    a64, wt64, bt64, w364, ref = _up_ref(a, wt, bt, w3, c.op)
    ulps = 6 * ULP[dt] if lp else 1e-4
    if c.op == "up_fwd":
        out = ops.CL(torch.full((n, 2 * d, 2 * h, 2 * w, cop), float("nan"), dtype=DT[dt], device="cuda"), 0, cop)
        if lp:
            wp16 = ops.lp_upconv_fused_pack(wp32, cp, DT[dt])
            nb = ops.lp_upconv_fused_num_blocks((n, d, h, w))
            stats = torch.full((nb, 2, cop), float("nan"), device="cuda")
            ops.lp_upconv_fused_fwd(xc, wp16, beff, out, stats)
        else:
            nb = ops.upconv_fused_num_blocks((n, d, h, w), cop)
            stats = torch.full((nb, 2, cop), float("nan"), device="cuda")
            ops.upconv_fused_fwd(xc, wp32, beff, out, stats)
        torch.cuda.synchronize()
        got = from_cl(out, co)
        check(c, got, ref.detach(), ulps, fine=True)
        full = from_cl(out, cop)
        assert cop == co or float(full[:, co:].abs().max()) == 0.0, f"{_id(c)}: padded channels"
        s = stats.sum(0).cpu().double()
        assert not torch.isnan(s).any(), f"{_id(c)}: a stats row was not written"
        base = ref.detach() if not lp else got.double()
        s1, s2 = base.sum((0, 2, 3, 4)), (base * base).sum((0, 2, 3, 4))
        assert torch.allclose(s[0, :co], s1, rtol=1e-4, atol=1e-3 * s2.max().sqrt().item()), f"{_id(c)}: channel sums"
        assert torch.allclose(s[1, :co], s2, rtol=1e-4), f"{_id(c)}: channel sums of squares"
        return
    go = rnd(torch.randn(ref.shape, generator=gen(c, 3)), dt)
    if c.op == "up_dgrad":
        ref.backward(go.double())
        gin = ops.CL(torch.full((n, d, h, w, cp), float("nan"), dtype=DT[dt], device="cuda"), 0, cp)
        if lp:
            ops.lp_upconv_fused_bwd_data(to_cl(go, cop, dt), ops.lp_upconv_fused_pack(wp32, cp, DT[dt]), gin)
        else:
            ops.upconv_fused_bwd_data(to_cl(go, cop, dt), ops.upconv_fused_pack_bwd(wp32, cp, cop), gin)
        torch.cuda.synchronize()
        check(c, from_cl(gin, C), a64.grad, ulps)
        full = from_cl(gin, cp)
        assert cp == C or float(full[:, C:].abs().max()) == 0.0, f"{_id(c)}: padded channels"
        return
    wtol = 2e-3 if lp else 2e-4
    wgrad = ops.lp_upconv_fused_wgrad if lp else ops.upconv_fused_wgrad
    if c.op == "up_wgrad":
        ref.backward(go.double())
        got = wgrad(xc, to_cl(go, cop, dt), C, co, bt.cuda(), pws, None)
    else:                       # lazy BatchNorm + ReLU backward of the fused op's output
        y = rnd(torch.randn(ref.shape, generator=gen(c, 5)) * 1.2 - 0.2, dt)
        gamma, beta, vec = bn_setup(c, y, co, cop)
        yc, gac = to_cl(y, cop, dt, c.cs, c.c0), to_cl(go, cop, dt, c.cs, c.c0)
        part = torch.empty(ops.bn_bwd_partials_floats(yc.nvox, cop), device="cuda")
        _, _, coef = ops.bn_relu_bwd(yc, gac, vec, gamma.cuda(), co, part, lazy=True)
        gy = ops.CL(torch.full_like(gac.buf, SENT), c.c0, cop)
        got = wgrad(xc, gac, C, co, bt.cuda(), pws, None, (yc, vec, coef, gy))
        torch.cuda.synchronize()
        gy64 = bn_relu_grad64(y, gamma, beta, go)
        gy_k = from_cl(gy, co)
        check(c, gy_k, gy64, 2e-4 if not lp else 2 * ULP[dt], fine=True)
        ref.backward(gy64 if not lp else gy_k.double())
    torch.cuda.synchronize()
    for name, t, want in zip(("dWT", "dbT", "dW3"), got, (wt64.grad, bt64.grad, w364.grad)):
        check_w(c, name, t, want, wtol)


# ------------------------------------------------------------------ first layer (C_in <= 2, NCDHW input, 8 padded outputs)
def first_buffer(c, dt, n, d, h, w):
    """The 8-channel output slice of a first-layer case in a sentinel-filled buffer (default: offset 8 of 16 channels)."""
    cs, c0 = (c.cs, c.c0) if c.cs else (16, 8)
    return _ops().CL(torch.full((n, d, h, w, cs), SENT, dtype=DT[dt], device="cuda"), c0, 8)


def first_grad(c, ga, dt):
    """The gradient of a first-layer case as a channels-last slice (c.cs = 0: a plain 8-channel tensor)."""
    return to_cl(ga, 8, dt, c.cs or None, c.c0, SENT)


def check_first_fwd(c, out, stats, ref, co, tol_rel):
    """Output, neighbouring and padded channels and the BatchNorm partial rows of a first-layer forward.  16-bit: the sums are
    taken over the ROUNDED stored outputs."""
    got = from_cl(out, co)
    check(c, got, ref, tol_rel)
    check_sentinel_and_padding(c, out, co)
    assert torch.all(out.buf[..., out.c0 + 8:].float() == SENT), f"{_id(c)}: the channels behind the slice were written"
    s = stats.sum(0).cpu().double()
    assert not torch.isnan(s).any(), f"{_id(c)}: a stats row was not written"
    base = ref if c.dtype == "fp32" else got.double()
    s1, s2 = base.sum((0, 2, 3, 4)), (base * base).sum((0, 2, 3, 4))
    assert torch.allclose(s[0, :co], s1, rtol=1e-4, atol=1e-3 * s2.max().sqrt().item()), f"{_id(c)}: channel sums"
    assert torch.allclose(s[1, :co], s2, rtol=1e-4), f"{_id(c)}: channel sums of squares"
    assert co == 8 or float(s[:, co:].abs().max()) == 0.0, f"{_id(c)}: statistics of the padded channels"
    return got


@pytest.mark.parametrize("c", [pytest.param(c, id=_id(c)) for c in CASES if c.op.startswith("first_")])
def test_first_layer(c, monkeypatch):
    ops = _ops()
    dt, n, ci, co, d, h, w = c.dtype, c.N, c.Ci, c.Co, c.D, c.H, c.W
    lp = dt != "fp32"
    assert ops.conv_first_supported(3, ci, 8, w)
    g = gen(c)
    x = torch.randn(n, ci, d, h, w, generator=g)                 # float32, never rounded: the kernels read it as it is
    wt = torch.randn(co, ci, 3, 3, 3, generator=g) * 0.3
    if c.op == "first_fwd":
        nb = ops.conv_first_num_blocks((n, d, h, w))

        def run(dtype):
            out = first_buffer(c, dtype, n, d, h, w)
            stats = torch.full((nb, 2, 8), float("nan"), device="cuda")          # every row must be written
            ops.conv_first_fwd(x.cuda(), wt.cuda(), None, out, stats)
            torch.cuda.synchronize()
            return out, stats
        out, stats = run(dt)
        ref = F.conv3d(x.double(), wt.double(), None, 1, 1)
        got = check_first_fwd(c, out, stats, ref, co, ULP[dt] if lp else 1e-5)
        if lp:      # the same template does the same float32 arithmetic: the stored output is the fp32 kernel's, rounded
            o32 = from_cl(run("fp32")[0], co)
            assert torch.equal(got, rnd(o32, dt)), where(c, got, rnd(o32, dt))
        return
    ga = rnd(torch.randn(n, co, d, h, w, generator=gen(c, 3)), dt)
    if c.op == "first_dgrad":
        dx = ops.conv_first_bwd_data(first_grad(c, ga, dt), wt.cuda(), ci)
        torch.cuda.synchronize()
        assert dx.shape == x.shape and dx.dtype == torch.float32
        # the matrix-pipe route holds the weights as 16-bit fragments; the direct kernels read them as float32
        pair = c.route.startswith("lp_conv_fwd_pair_kernel")
        ref = torch.nn.grad.conv3d_input(x.shape, (rnd(wt, dt) if pair else wt).double(), ga.double(), 1, 1)
        check(c, dx.cpu(), ref, 1e-5)
        if lp and not pair:                                      # the fp32 instantiation on the same (rounded) gradient
            dx32 = ops.conv_first_bwd_data(first_grad(c, ga, "fp32"), wt.cuda(), ci)
            torch.cuda.synchronize()
            assert torch.equal(dx.cpu(), dx32.cpu()), where(c, dx.cpu(), dx32.cpu())
        return
    ws = torch.empty(ops.conv_first_wgrad_ws((n, d, h, w), ci), device="cuda")
    if c.op in ("first_wgrad", "first_wgrad_mfma"):
        xr = x
        if c.op == "first_wgrad_mfma":                           # the input enters the matrix pipe rounded to the storage type
            from ctunet_amd import _lib
            assert lp and _lib.load().ctu_lp_conv3d_wgrad_kernel_name(d, h, w, 3, 8, 8) == b"lp_wgrad8_kernel"
            monkeypatch.setattr(ops, "FIRST_WGRAD_MFMA_MIN_VOX", 0)
            xr = rnd(x, dt)
        elif lp:                                                 # below the threshold: the direct kernel
            assert n * d * h * w < ops.FIRST_WGRAD_MFMA_MIN_VOX
        dw = ops.conv_first_wgrad(x.cuda(), first_grad(c, ga, dt), co, ws)
        torch.cuda.synchronize()
        assert dw.shape == wt.shape
        check_w(c, "dW", dw, torch.nn.grad.conv3d_weight(xr.double(), wt.shape, ga.double(), 1, 1), 1e-4)
        return
    y = torch.randn(n, co, d, h, w, generator=gen(c, 5)) * 0.9 - 0.1
    gamma, beta, vec = bn_setup(c, y, co, 8)
    yc, gac = to_cl(y, 8, "fp32", c.cs, c.c0, SENT), to_cl(ga, 8, "fp32", c.cs, c.c0, SENT)
    part = torch.empty(ops.bn_bwd_partials_floats(n * d * h * w, 8), device="cuda")
    _, _, coef = ops.bn_relu_bwd(yc, gac, vec, gamma.cuda(), co, part, lazy=True)
    gy = ops.CL(torch.full_like(gac.buf, SENT), c.c0, 8)
    dw = ops.conv_first_wgrad_bn(x.cuda(), gac, yc, vec, coef, gy, co, ws)
    torch.cuda.synchronize()
    gy64 = bn_relu_grad64(y, gamma, beta, ga)
    check(c, from_cl(gy, co), gy64, 2e-4)
    assert torch.all(from_cl(gy, 8)[:, co:] == 0), f"{_id(c)}: padded channels of the raw-output gradient"
    if c.cs > 8:
        other = torch.ones(c.cs, dtype=torch.bool)
        other[c.c0:c.c0 + 8] = False
        assert torch.all(gy.buf[..., other.cuda()] == SENT), f"{_id(c)}: channels outside the slice were written"
    check_w(c, "dW", dw, torch.nn.grad.conv3d_weight(x.double(), wt.shape, gy64, 1, 1), 1e-4)


# ------------------------------------------------------------------ first layer: arguments the shipped classes do not use
def test_first_layer_pair_data_gradient_with_three_input_channels():
    """ctu_lp_conv3d_first_bwd_data_pair accepts C_in <= 4: with C_in = 3 and N = 2 every float32 plane of [2, 3, D, H, W]
    is written at its own (n * C_in + c) index.  Reference and gate as for the pair route of test_first_layer."""
    ops = _ops()
    c = Case("lp_conv_fwd_pair_kernel<OUT32>", "first_dgrad", "bf16", 2, 3, 7, 6, 12, 40, 3, False, 16, 8)
    g = gen(c)
    wt = torch.randn(c.Co, c.Ci, 3, 3, 3, generator=g) * 0.3
    ga = rnd(torch.randn(c.N, c.Co, c.D, c.H, c.W, generator=g), c.dtype)
    dx = ops.conv_first_bwd_data(first_grad(c, ga, c.dtype), wt.cuda(), c.Ci)
    torch.cuda.synchronize()
    shape = (c.N, c.Ci, c.D, c.H, c.W)
    assert tuple(dx.shape) == shape and dx.dtype == torch.float32
    check(c, dx.cpu(), torch.nn.grad.conv3d_input(shape, rnd(wt, c.dtype).double(), ga.double(), 1, 1), 1e-5)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_first_layer_forward_with_a_bias(dt):
    """The bias / nbias arguments of the first-layer forward, with C_out = 4: a whole quad of the 8 outputs is padding and
    stays exactly zero, in the output and in the statistics, bias or not."""
    ops = _ops()
    c = Case("first_fwd_kernel", "first_fwd", dt, 1, 2, 4, 6, 10, 40, 3, False, 16, 8)
    n, ci, co, d, h, w = c.N, c.Ci, c.Co, c.D, c.H, c.W
    g = gen(c)
    x = torch.randn(n, ci, d, h, w, generator=g)
    wt = torch.randn(co, ci, 3, 3, 3, generator=g) * 0.3
    bias = torch.randn(co, generator=g)
    out = first_buffer(c, dt, n, d, h, w)
    stats = torch.full((ops.conv_first_num_blocks((n, d, h, w)), 2, 8), float("nan"), device="cuda")
    ops.conv_first_fwd(x.cuda(), wt.cuda(), bias.cuda(), out, stats)
    torch.cuda.synchronize()
    ref = F.conv3d(x.double(), wt.double(), bias.double(), 1, 1)
    check_first_fwd(c, out, stats, ref, co, 1e-5 if dt == "fp32" else ULP[dt])
