"""MaxPool3d(2,2) forward / backward (csrc/elementwise.hip) and the first layer's data gradient (csrc/conv3d_first.hip)
against float64 torch on the CPU (max_pool3d + autograd, conv3d autograd), at the shapes where their lane mappings change:

pooling -- cp / 4 = 2, 4 and 32 take the kernels with lanes along the fine row (the two w of a window are two lanes of one
wave), cp = 24 (six quads) the (pooled voxel, quad) kernels; fine rows of 10 and 132 voxels do not fill a wave evenly and
the position counts are no multiple of the 256-thread block; input and gradient target are channel halves of 2 cp wide
buffers whose other half must stay untouched; accumulate on and off, the BatchNorm reduction rows on and off, three storage
types.  The tie input is small integers through ReLU, so most windows hold several equal maxima: every value is exact in
every type and the gradient must sit on the FIRST maximum in (d, h, w) scan order, bit for bit.

first layer -- volumes below one 4 x 4 x 32 tile in d and h, W no multiple of 32, several tiles per block, C_in 1 and 2,
fewer than 8 real output channels, the gradient read from a slice of a wider buffer, plain and written by the lazy
BatchNorm-backward weight-gradient kernel.

Gates: stored pooling values are exact for the tie input; for random input one rounding of the stored type (fp32: 1e-6);
summed reduction rows 1e-4 (test_stream_kernels_gpu.py's gate for dgamma / dbeta, which are these sums); dx 1e-5
(test_ops_gpu.py's gate for this op)."""
import pytest
import torch
import torch.nn.functional as F

import stream_ref as R
from util import gen, rel_err

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"fp32": 1e-6, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
SENTINEL = -77.0                                      # exact in every storage type
EPS = 1e-5


def _ops():
    from ctunet_amd import ops
    return ops


def _half(x, dt, upper, fill=SENTINEL):
    """[N, C, D, H, W] -> (buffer [N, D, H, W, 2 C] of dt on the GPU, its CL over one channel half)."""
    n, c, d, h, w = x.shape
    buf = torch.full((n, d, h, w, 2 * c), fill)
    c0 = c if upper else 0
    buf[..., c0:c0 + c] = x.permute(0, 2, 3, 4, 1)
    buf = buf.to(dt).cuda()
    return buf, _ops().CL(buf, c0, c)


def _read(buf, c0, c):
    return buf[..., c0:c0 + c].float().permute(0, 4, 1, 2, 3).cpu()


def _pool_ref(a64, gout64):
    a = a64.clone().requires_grad_(True)
    out = F.max_pool3d(a, 2, 2)
    out.backward(gout64)
    return out.detach(), a.grad


def _pool_problem(kind, cp, dims, dt):
    """raw y, the [4, cp] vectors of its lazy transform (scale, shift, mean, invstd), gout and the gradient target's start."""
    n, d, h, w = dims
    shape, pooled = (n, cp, d, h, w), (n, cp, d // 2, h // 2, w // 2)
    if kind == "ties":
        y = torch.randint(-2, 4, shape, generator=gen(1)).float()
        vec = torch.stack((torch.ones(cp), torch.zeros(cp), torch.full((cp,), 0.5), torch.full((cp,), 2.0)))
        gout = torch.randint(1, 5, pooled, generator=gen(2)).float()
        base = torch.randint(-3, 4, shape, generator=gen(3)).float()
        return y, vec, gout, base
    y = (torch.randn(shape, generator=gen(1)) * 1.3 + 0.2).to(dt).float()
    gamma, beta = torch.rand(cp, generator=gen(4)) + 0.25, torch.randn(cp, generator=gen(5)) * 0.2
    bn = lambda: F.batch_norm(y.double(), None, None, gamma.double(), beta.double(), True, 0.0, EPS)
    for _ in range(4):          # off ReLU's kink, so the float64 reference and the fp32 fma agree on every mask bit
        m = bn().abs() < 1e-5
        if not m.any():
            break
        y[m] = (y[m] + 0.25).to(dt).float()
    assert not (bn().abs() < 1e-5).any()
    vec = R.bn_vectors(y, gamma, beta, EPS, cp)
    gout = torch.randn(pooled, generator=gen(2)).to(dt).float()
    base = torch.randn(shape, generator=gen(3)).to(dt).float()
    return y, vec, gout, base


def _close(got, want, name, exact):
    if exact:
        assert torch.equal(got.double(), want)
    else:
        assert (got.double() - want).abs().max().item() <= ULP[name] * want.abs().max().item()


@pytest.mark.parametrize("name", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("dims", [(1, 4, 6, 10), (2, 2, 4, 132)])
@pytest.mark.parametrize("cp", [8, 16, 24, 128])
@pytest.mark.parametrize("kind", ["ties", "random"])
def test_pool_channel_halves(kind, cp, dims, name):
    ops, dt = _ops(), DT[name]
    n, d, h, w = dims
    exact = kind == "ties"
    y, vec, gout, base = _pool_problem(kind, cp, dims, dt)
    v_ = lambda r: vec[r].double().view(1, -1, 1, 1, 1)
    act64 = F.relu(y.double() * v_(0) + v_(1))
    vec_g = vec.cuda()
    for xf in (False, True):
        a64 = act64 if xf else y.double()
        out_ref, grad_ref = _pool_ref(a64, gout.double())
        ybuf, yc = _half(y, dt, True)
        if xf:
            yc = yc.with_xf(vec_g[0], vec_g[1], True)
        y_before = ybuf.clone()
        obuf, oc = _half(torch.zeros_like(gout), dt, False)
        ops.maxpool_fwd(yc, oc)
        got = _read(obuf, 0, cp)
        if exact or not xf:                      # a maximum of stored values is a stored value
            assert torch.equal(got.double(), out_ref)
        else:                                    # one fused multiply-add in fp32, then the type's rounding
            assert (got.double() - out_ref).abs().max().item() <= ULP[name] * out_ref.abs().max().item()
        assert torch.all(obuf[..., cp:] == SENTINEL)
        _, goc = _half(gout, dt, False)
        red_rows = ops.maxpool_bwd_bn_blocks(dims, cp)
        assert (red_rows > 0) == (cp != 24)                          # six quads do not divide the block
        for accumulate in (False, True):
            for red in ((False, True) if xf and red_rows else (False,)):
                gbuf, gc = _half(base, dt, True)
                want = grad_ref + (base.double() if accumulate else 0.0)
                if red:
                    part = torch.full((red_rows * 2 * cp,), float("nan"), device="cuda")
                    rows = ops.maxpool_bwd(yc, goc, gc, accumulate, (vec_g, part))
                    assert rows == red_rows
                else:
                    ops.maxpool_bwd(yc, goc, gc, accumulate)
                got = _read(gbuf, cp, cp)
                _close(got, want, name, exact)
                assert torch.all(gbuf[..., :cp] == SENTINEL)
                if red:
                    # rows of {sum gz, sum gz xhat}, gz = the stored gradient under ReLU's mask
                    gz = got.double() * (act64 > 0)
                    xhat = (y.double() - v_(2)) * v_(3)
                    s = part.view(red_rows, 2, cp).double().sum(0).cpu()
                    e1 = rel_err(s[0], gz.sum((0, 2, 3, 4)))
                    e2 = rel_err(s[1], (gz * xhat).sum((0, 2, 3, 4)))
                    print(f"{kind} cp {cp} {dims} {name} acc {accumulate}: rows {red_rows} sum gz {e1:.2e} sum gz xhat {e2:.2e}")
                    assert e1 < 1e-4 and e2 < 1e-4
        assert torch.equal(ybuf, y_before)


def test_pool_gradient_sits_on_the_first_maximum():
    """One window per scan position: the maximum is repeated from that position to the window's end, so the gradient belongs
    to that position; plus the all-equal window (position 0)."""
    ops = _ops()
    cp, dims = 8, (1, 2, 2, 16)
    x = torch.zeros(1, cp, 2, 2, 16)
    for wo in range(8):
        for t in range(wo, 8):
            x[0, :, t >> 2, (t >> 1) & 1, 2 * wo + (t & 1)] = 5.0
    gout = torch.arange(1, 9).float().view(1, 1, 1, 1, 8).expand(1, cp, 1, 1, 8).contiguous()
    want = torch.zeros_like(x)
    for wo in range(8):
        want[0, :, wo >> 2, (wo >> 1) & 1, 2 * wo + (wo & 1)] = wo + 1.0
    _, ref = _pool_ref(x.double(), gout.double())
    assert torch.equal(ref, want.double())                           # ATen agrees on the rule
    _, xc = _half(x, torch.float32, True)
    _, goc = _half(gout, torch.float32, False)
    gbuf, gc = _half(torch.zeros_like(x), torch.float32, True)
    ops.maxpool_bwd(xc, goc, gc, False)
    assert torch.equal(_read(gbuf, cp, cp), want)


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("case", [(1, 1, 3, 3, 5, 40), (2, 2, 7, 9, 6, 72), (1, 2, 5, 2, 2, 16),
                                  (2, 1, 3, 50, 42, 72)])       # 858 tiles: two per block
def test_first_layer_data_gradient(case, lazy):
    ops = _ops()
    n, ci, co, d, h, w = case
    assert ops.conv_first_supported(3, ci, 8, w)
    assert w % 32 != 0 and (d < 4 or h < 4 or d % 4 or h % 4)
    shape = (n, co, d, h, w)
    x = torch.randn(n, ci, d, h, w, generator=gen(11))
    wt = torch.randn(co, ci, 3, 3, 3, generator=gen(12)) * 0.3
    ga = torch.randn(shape, generator=gen(13))

    def cl(t):                                                       # 8 padded channels at offset 8 of a 24-wide buffer
        buf = torch.full((n, d, h, w, 24), SENTINEL)
        buf[..., 8:16] = 0.0
        buf[..., 8:8 + co] = t.permute(0, 2, 3, 4, 1)
        return ops.CL(buf.cuda(), 8, 8)

    if lazy:
        y = torch.randn(shape, generator=gen(14)) * 0.9 - 0.1
        gamma, beta = torch.rand(co, generator=gen(15)) + 0.3, torch.randn(co, generator=gen(16)) * 0.2
        bn = lambda: F.batch_norm(y.double(), None, None, gamma.double(), beta.double(), True, 0.0, EPS)
        for _ in range(4):
            m = bn().abs() < 1e-5
            if not m.any():
                break
            y[m] += 0.25
        assert not (bn().abs() < 1e-5).any()
        _, dy, _, _ = R.bn_relu_ref(y, gamma, beta, EPS, ga)
        vec = R.bn_vectors(y, gamma, beta, EPS, 8).cuda()
        yc, gac = cl(y), cl(ga)
        part = torch.empty(ops.bn_bwd_partials_floats(n * d * h * w, 8), device="cuda")
        ws = torch.empty(ops.conv_first_wgrad_ws((n, d, h, w), ci), device="cuda")
        _, _, coef = ops.bn_relu_bwd(yc, gac, vec, gamma.cuda(), co, part, lazy=True)
        src = ops.CL(torch.full_like(gac.buf, float("nan")), 8, 8)
        ops.conv_first_wgrad_bn(x.cuda(), gac, yc, vec, coef, src, co, ws)
    else:
        dy, src = ga.double(), cl(ga)
    x64 = x.double().requires_grad_(True)
    F.conv3d(x64, wt.double(), None, 1, 1).backward(dy.double())
    dx = ops.conv_first_bwd_data(src, wt.cuda(), ci)
    e = rel_err(dx, x64.grad)
    print(f"{case} lazy {lazy}: dx {e:.2e}")
    assert e < 1e-5
