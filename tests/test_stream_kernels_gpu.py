"""The streaming kernels at the two ends of the training step and the reductions between layers (csrc/head_loss.hip,
csrc/elementwise.hip) against the plain float64 references of tests/stream_ref.py, at the shapes where their code changes
path: the second trip of every grid-stride loop, the loss's scalar path, every head width, channel slices of wider buffers,
lane rows that idle when cp / 4 does not divide the block, more partial rows than a finalize block has threads, and BatchNorm
statistics of channels that are constant or far from zero mean.

Gates are the ones the small-shape tests of test_ops_gpu.py / test_lowp_gpu.py already use: loss terms 1e-5 * max(1, |ref|)
each, loss gradient 1e-4; head outputs 1e-5, gin / dw / db 1e-4; BatchNorm dgamma / dbeta and channel sums 1e-4, dy 2e-4; a
stored 16-bit value one ulp of the type (two for the BatchNorm apply, as in test_lp_glue_kernels...).  The kernels accumulate
a handful of voxels per thread in fp32 and everything above a block in double, so the gates do not grow with the volume.

The launch constants the shapes are sized by are restated below and every case asserts its own arithmetic."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stream_ref as R
from util import gen, rel_err

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}        # one unit in the last place, relative (test_lowp_gpu.py)
HB, HEAD_MAX_BLOCKS = 256, 2048                       # head_loss.hip: block size, head_blocks() cap
LOSS_BX = 1024                                        # head_loss.hip: loss blocks per batch item
EW_BLOCK, FIN_BLOCK = 256, 256                        # elementwise.hip
SENTINEL = -77.0                                      # exact in every storage type
EPS = 1e-5


def _ops():
    from ctunet_amd import ops
    return ops


def _lib():
    from ctunet_amd import _lib
    return _lib.load()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _rnd(x, dt):
    return x.to(dt).float()


# ============================================================================================================== loss
LAM = (0.5, 2.0)


def _loss_ref(p, t, sm, g_ce=1.0, g_dice=1.0, lam=LAM):
    p64 = p.double().requires_grad_(True)
    ce, dice = R.loss_ref(p64, t, lam[0], lam[1], sm)
    (g_ce * ce + g_dice * dice).backward()
    return ce.item(), dice.item(), p64.grad


def _check_terms(terms, ce, dice):
    got = terms.cpu().tolist()
    print(f"loss terms: kernel {got}, reference {[ce, dice]}")
    for v, ref in zip(got, (ce, dice)):
        assert math.isfinite(v) and abs(v - ref) <= 1e-5 * max(1.0, abs(ref)), (got, ce, dice)


def _check_grad(gp, ref):
    assert torch.isfinite(gp).all()
    err = rel_err(gp, ref)
    print(f"loss gradient rel err {err:.3e}")
    assert err < 1e-4


def _pred_target(shape, seed, soft=False):
    p = torch.randn(shape, generator=gen(seed)) * 2.0
    if soft:
        return p, torch.rand(shape, generator=gen(seed + 1))
    m = (torch.rand((shape[0],) + tuple(shape[2:]), generator=gen(seed + 1)) < 0.3).long()
    return p, F.one_hot(m, 2).movedim(4, 1).float().contiguous()


def _takes_vector_path(*tensors):
    v = tensors[0][0, 0].numel()
    return v % 4 == 0 and all(t.data_ptr() % 16 == 0 for t in tensors)


@pytest.mark.parametrize("sm", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
def test_loss_scalar_path_volume_not_a_multiple_of_four(sm, accumulate):
    ops = _ops()
    shape = (2, 2, 3, 5, 7)
    assert (3 * 5 * 7) % 4 != 0
    p, t = _pred_target(shape, 11)
    ce, dice, gref = _loss_ref(p, t, sm)
    pg, tg = p.cuda(), t.cuda()
    terms, ws = ops.loss_fwd(pg, tg, *LAM, sm)
    _check_terms(terms, ce, dice)
    base = torch.randn(shape, generator=gen(13))
    out = base.cuda() if accumulate else None
    gp = ops.loss_bwd(pg, tg, *LAM, sm, ws, None, None, out, accumulate)
    _check_grad(gp.cpu(), gref + base.double() if accumulate else gref)


@pytest.mark.parametrize("sm", [False, True])
def test_loss_scalar_path_misaligned_planes(sm):
    """V = 480 is a multiple of 4, but every plane starts one float into its allocation."""
    ops = _ops()
    shape = (2, 2, 6, 8, 10)
    numel = 2 * 2 * 480
    p, t = _pred_target(shape, 21)
    ce, dice, gref = _loss_ref(p, t, sm)

    def off_by_one(x, fill=0.0):
        big = torch.full((numel + 8,), fill, device="cuda")
        big[1:1 + numel] = x.flatten().cuda()
        view = big[1:1 + numel].view(shape)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return big, view
    _, pg = off_by_one(p)
    _, tg = off_by_one(t)
    assert not _takes_vector_path(pg, tg)
    terms, ws = ops.loss_fwd(pg, tg, *LAM, sm)
    _check_terms(terms, ce, dice)
    base = torch.randn(shape, generator=gen(23))
    for accumulate in (False, True):
        big, out = off_by_one(base, SENTINEL)
        big[0] = SENTINEL
        got = ops.loss_bwd(pg, tg, *LAM, sm, ws, None, None, out, accumulate)
        assert got.data_ptr() == out.data_ptr() and got.data_ptr() % 16 == 4
        _check_grad(out.cpu(), gref + base.double() if accumulate else gref)
        assert big[0].item() == SENTINEL and torch.all(big[1 + numel:] == SENTINEL)       # the floats around the span
    # one misaligned operand is enough to leave the vector path
    out = torch.empty(shape, device="cuda")
    assert not _takes_vector_path(p.cuda(), tg, out)
    _check_grad(ops.loss_bwd(p.cuda(), tg, *LAM, sm, ws, None, None, out).cpu(), gref)


@pytest.mark.parametrize("sm", [False, True])
@pytest.mark.parametrize("shape,vector", [((1, 2, 66, 128, 128), True), ((2, 2, 65, 65, 63), False)])
def test_loss_second_trip_of_the_grid_stride_loops(shape, vector, sm):
    ops = _ops()
    v = shape[2] * shape[3] * shape[4]
    lanes = v // 4 if vector else v
    assert (v % 4 == 0) == vector and LOSS_BX * HB < lanes < 2 * LOSS_BX * HB     # some lanes take two trips, some one
    p, t = _pred_target(shape, 31)
    ce, dice, gref = _loss_ref(p, t, sm)
    pg, tg = p.cuda(), t.cuda()
    assert _takes_vector_path(pg, tg) == vector
    terms, ws = ops.loss_fwd(pg, tg, *LAM, sm)
    _check_terms(terms, ce, dice)
    gp = ops.loss_bwd(pg, tg, *LAM, sm, ws, None, None)
    _check_grad(gp.cpu(), gref)


@pytest.mark.parametrize("sm", [False, True])
@pytest.mark.parametrize("shape", [(2, 2, 6, 8, 10), (2, 2, 3, 5, 7)])
def test_loss_distinct_upstream_gradients(shape, sm):
    """g_ce = 2, g_dice = 0.5: the gradient is 2 d(ce term) + 0.5 d(dice term); a swap of the two scales cannot pass."""
    ops = _ops()
    p, t = _pred_target(shape, 41)
    _, _, gref = _loss_ref(p, t, sm, 2.0, 0.5)
    _, _, gplain = _loss_ref(p, t, sm, 0.5, 2.0)
    assert rel_err(gplain, gref) > 0.1                              # the swapped gradient is far outside the gate
    pg, tg = p.cuda(), t.cuda()
    _, ws = ops.loss_fwd(pg, tg, *LAM, sm)
    g_ce, g_dice = torch.tensor(2.0).cuda(), torch.tensor(0.5).cuda()
    _check_grad(ops.loss_bwd(pg, tg, *LAM, sm, ws, g_ce, g_dice).cpu(), gref)
    base = torch.randn(shape, generator=gen(43))
    gp = ops.loss_bwd(pg, tg, *LAM, sm, ws, g_ce, g_dice, base.cuda(), True)
    _check_grad(gp.cpu(), gref + base.double())
    # one scale given, the other defaulting to 1
    _, _, g1 = _loss_ref(p, t, sm, 1.0, 0.5)
    _check_grad(ops.loss_bwd(pg, tg, *LAM, sm, ws, None, g_dice).cpu(), g1)


@pytest.mark.parametrize("sm", [False, True])
@pytest.mark.parametrize("shape", [(2, 2, 6, 8, 10), (2, 2, 3, 5, 7)])
def test_loss_wide_logits(shape, sm):
    """pred = 30 randn: |a - b| reaches ~100 and exp overflows fp32 without the max subtraction."""
    ops = _ops()
    _, t = _pred_target(shape, 51)
    p = torch.randn(shape, generator=gen(53)) * 30.0
    assert (p[:, 0] - p[:, 1]).abs().max().item() > 89.0            # exp(89) > FLT_MAX
    ce, dice, gref = _loss_ref(p, t, sm)
    pg, tg = p.cuda(), t.cuda()
    terms, ws = ops.loss_fwd(pg, tg, *LAM, sm)
    _check_terms(terms, ce, dice)
    _check_grad(ops.loss_bwd(pg, tg, *LAM, sm, ws, None, None).cpu(), gref)


@pytest.mark.parametrize("sm", [False, True])
@pytest.mark.parametrize("shape", [(2, 2, 6, 8, 10), (2, 2, 3, 5, 7)])
def test_loss_soft_and_tied_targets(shape, sm):
    """Targets that are not one-hot, one row with t0 == t1 exactly: the class of a tie is 0 (the first maximum)."""
    ops = _ops()
    p, t = _pred_target(shape, 61, soft=True)
    t[:, 1, 1, 2, :] = t[:, 0, 1, 2, :]
    tied = t[:, 1] == t[:, 0]
    assert tied.sum().item() == shape[0] * shape[4]
    ce, dice, gref = _loss_ref(p, t, sm)
    pg, tg = p.cuda(), t.cuda()
    terms, ws = ops.loss_fwd(pg, tg, *LAM, sm)
    _check_terms(terms, ce, dice)
    _check_grad(ops.loss_bwd(pg, tg, *LAM, sm, ws, None, None).cpu(), gref)
    # the cross-entropy gradient alone is lambda / (N V) * (softmax - onehot(class)): negative at the class, positive elsewhere
    lam = (LAM[0], 0.0)
    ce1, dice1, gce = _loss_ref(p, t, sm, lam=lam)
    terms, ws = ops.loss_fwd(pg, tg, *lam, sm)
    _check_terms(terms, ce1, 0.0)
    g_ = ops.loss_bwd(pg, tg, *lam, sm, ws, None, None).cpu()
    _check_grad(g_, gce)
    cls1 = t[:, 1] > t[:, 0]
    assert not cls1[tied].any()
    assert torch.all(g_[:, 0][~cls1] < 0) and torch.all(g_[:, 1][~cls1] > 0)
    assert torch.all(g_[:, 0][cls1] > 0) and torch.all(g_[:, 1][cls1] < 0)


@pytest.mark.parametrize("sm", [False, True])
def test_loss_three_items_one_empty(sm):
    """The middle item is all background with an all-zero prediction: sum p t = 0, so its Dice ratio is eps / (V + eps) and
    the backward's kd_t, kd_p come from the tail row (1e-7, V + 1e-7)."""
    ops = _ops()
    shape = (3, 2, 6, 8, 10)
    p, t = _pred_target(shape, 71)
    t[1, 0], t[1, 1] = 1.0, 0.0
    p[1] = 0.0
    ce, dice, gref = _loss_ref(p, t, sm)
    pg, tg = p.cuda(), t.cuda()
    terms, ws = ops.loss_fwd(pg, tg, *LAM, sm)
    _check_terms(terms, ce, dice)
    assert torch.isfinite(ws[-6:]).all()                             # (num + eps, den + eps) of the three items
    if not sm:
        assert abs(ws[-4].item() - 1e-7) < 1e-12 and ws[-3].item() == 480.0
    _check_grad(ops.loss_bwd(pg, tg, *LAM, sm, ws, None, None).cpu(), gref)


# ============================================================================================================== head
CI_OF = {8: 7, 16: 14, 32: 28}
HEAD_COMBOS = [(2, 2, 0), (2, 1, 0), (3, 2, 1), (3, 2, 2), (3, 3, 0), (1, 0, 0), (4, 1, 0), (4, 3, 0)]
FORMS = ["imap", "trailing", "plain"]


def _positions(cin_p, form):
    """Padded position of every logical input channel."""
    ci = CI_OF[cin_p]
    if form != "imap":
        return list(range(ci))                                   # trailing padding
    if cin_p == 8:
        return [0, 1, 2, 4, 5, 6, 7]                             # one hole
    half = ci // 2
    return list(range(half)) + list(range(cin_p // 2, cin_p // 2 + half))       # two halves of a concat buffer


class HeadCase:
    """A head problem on the GPU next to its float64 reference: outputs and the gradients of a, w, b under random output
    gradients.  The input sits at channel offset c0 of a cs-wide buffer; padding positions inside the slice hold zeros."""

    def __init__(self, cin_p, form, co, act, mode, dims, dt=torch.float32, c0=0, cs=None, seed=1):
        ops = _ops()
        n, d, h, w = dims
        self.dims, self.cin_p, self.dt, self.c0, self.args = dims, cin_p, dt, c0, (act, mode)
        self.pos = pos = _positions(cin_p, form)
        ci = len(pos)
        cs = self.cs = cs or cin_p
        x = _rnd(torch.randn(n, d, h, w, ci, generator=gen(seed)) * 1.2 + 0.2, dt)
        buf = torch.full((n, d, h, w, cs), SENTINEL if cs > cin_p else 0.0)
        buf[..., c0:c0 + cin_p] = 0.0
        buf[..., [c0 + q for q in pos]] = x
        a = x.double()
        sc = sh = None
        if form != "plain":
            sc, sh = torch.rand(cin_p, generator=gen(seed + 2)) + 0.2, torch.randn(cin_p, generator=gen(seed + 3)) * 0.3
            a = F.relu(a * sc[pos].double() + sh[pos].double())
            sc, sh = sc.cuda(), sh.cuda()
        self.x = ops.CL(buf.to(dt).cuda(), c0, cin_p, sc, sh, sc is not None)
        self.imap = torch.tensor(pos, dtype=torch.int32).cuda() if form == "imap" else None
        wt, b = torch.randn(co, ci, generator=gen(seed + 4)) * 0.4, torch.randn(co, generator=gen(seed + 5))
        self.w, self.b = wt.cuda(), b.cuda()
        self.a, self.w64, self.b64 = (t.double().requires_grad_(True) for t in (a.permute(0, 4, 1, 2, 3), wt, b))
        self.refs = R.head_ref(self.a, self.w64, self.b64, act, mode)
        self.gs = [torch.randn(r.shape, generator=gen(seed + 6 + i)) for i, r in enumerate(self.refs)]
        torch.autograd.backward(self.refs, [g_.double() for g_ in self.gs])
        self.g0 = self.gs[0].cuda()
        self.g1 = self.gs[1].cuda() if mode else None

    def check_forward(self):
        o0, o1 = _ops().head_fwd(self.x, self.w, self.b, self.imap, *self.args)
        assert rel_err(o0, self.refs[0]) < 1e-5
        assert (o1 is None) == (len(self.refs) == 1)
        if o1 is not None:
            assert rel_err(o1, self.refs[1]) < 1e-5

    def backward(self, **kw):
        """(gin buffer on the CPU as float32, dw, db) of ops.head_bwd into a sentinel-filled buffer laid out like the input."""
        n, d, h, w = self.dims
        gbuf = torch.full((n, d, h, w, self.cs), SENTINEL, dtype=self.dt, device="cuda")
        gin = _ops().CL(gbuf, self.c0, self.cin_p)
        dw, db = _ops().head_bwd(self.x, self.w, self.b, self.imap, *self.args, self.g0, self.g1, gin, **kw)
        return gbuf.cpu(), dw.cpu(), db.cpu()

    def check_backward(self, gin_tol=None, **kw):
        gbuf, dw, db = self.backward(**kw)
        sl = gbuf[..., self.c0:self.c0 + self.cin_p].float()
        got, want = sl[..., self.pos].permute(0, 4, 1, 2, 3), self.a.grad
        if gin_tol is None:
            assert rel_err(got, want) < 1e-4
        else:
            assert (got.double() - want).abs().max().item() <= gin_tol * want.abs().max().item()
        pad = [q for q in range(self.cin_p) if q not in self.pos]
        assert torch.all(sl[..., pad] == 0)                          # padding positions inside the slice: exact zeros
        outside = [q for q in range(self.cs) if not self.c0 <= q < self.c0 + self.cin_p]
        if outside:                                                  # the rest of the buffer: the sentinel, bit for bit
            assert torch.equal(_bits(gbuf[..., outside]), _bits(torch.full_like(gbuf[..., outside], SENTINEL)))
        assert rel_err(dw, self.w64.grad) < 1e-4
        assert rel_err(db, self.b64.grad) < 1e-4
        return gbuf, dw, db


@pytest.mark.parametrize("co,act,mode", HEAD_COMBOS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cin_p", [8, 16, 32])
def test_head_every_width_against_reference(cin_p, form, co, act, mode):
    case = HeadCase(cin_p, form, co, act, mode, (2, 4, 6, 10))
    case.check_forward()
    case.check_backward()


@pytest.mark.parametrize("co,act,mode", [(3, 2, 1), (4, 1, 0)])
@pytest.mark.parametrize("cin_p", [8, 16, 32])
def test_head_channel_slices_of_wider_buffers(cin_p, co, act, mode):
    """Input and gin at channel offset 8 of buffers 16 wider than cin_p (in_cs, gin_cs > cin_p)."""
    case = HeadCase(cin_p, "imap", co, act, mode, (2, 4, 6, 10), c0=8, cs=cin_p + 16)
    case.check_forward()
    case.check_backward()


@pytest.mark.parametrize("cin_p,dims", [(8, (2, 65, 64, 66)), (16, (2, 33, 34, 62)), (32, (2, 33, 34, 62))])
def test_head_second_trip_and_batch_boundary_inside_a_block(cin_p, dims):
    """Both kernels launch min(2048, ceil(total / 256)) blocks; a backward block covers 256 / Q voxels per trip (Q = cin_p / 4
    lanes per voxel), so it takes Q trips below the cap and more above it.  The cin_p = 8 volume is above the cap for both."""
    n, d, h, w = dims
    v, q = d * h * w, cin_p // 4
    vpb = HB // q
    nb = min(HEAD_MAX_BLOCKS, -(-n * v // HB))
    assert -(-n * v // (nb * vpb)) >= 2 and n * v > HEAD_MAX_BLOCKS * vpb        # the backward takes further trips
    if cin_p == 8:
        assert nb == HEAD_MAX_BLOCKS and -(-n * v // (nb * vpb)) > q and n * v > nb * HB       # capped grid: so does the forward
        assert v % HB != 0                                          # a forward block straddles the two items
    else:
        assert v % vpb != 0                                         # a backward block straddles the two items
    case = HeadCase(cin_p, "trailing", 3, 2, 1, dims)
    case.check_forward()
    case.check_backward()


@pytest.mark.parametrize("cp,bn_cp,co,act,mode", [(16, 8, 2, 1, 0), (8, 8, 2, 0, 0), (32, 16, 3, 2, 1)])
def test_head_bwd_fused_batchnorm_rows_against_reference(cp, bn_cp, co, act, mode):
    """head_bwd(bn=...) then bn_relu_bwd(pre_reduced=rows) against float64 autograd of head(relu(batch_norm(y))) over the
    first bn_cp channels of the head's input; the remaining channels carry another layer's transform."""
    ops = _ops()
    n, d, h, w = 2, 4, 6, 10
    c = bn_cp - 1                                                    # real channels of the BatchNorm; one padded
    y = torch.randn(n, cp, d, h, w, generator=gen(1)) * 1.2 + 0.1
    y[:, c:bn_cp] = 0.0
    gamma, beta = torch.rand(c, generator=gen(2)) + 0.3, torch.randn(c, generator=gen(3)) * 0.3
    vec = torch.zeros(4, cp)
    vec[:, :bn_cp] = R.bn_vectors(y[:, :c], gamma, beta, EPS, bn_cp)
    vec[0, bn_cp:] = torch.rand(cp - bn_cp, generator=gen(4)) + 0.3
    vec[1, bn_cp:] = torch.randn(cp - bn_cp, generator=gen(5)) * 0.3
    wt, b = torch.randn(co, cp, generator=gen(6)) * 0.4, torch.randn(co, generator=gen(7))
    # reference
    y64, g64, b64 = y.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    a_bn = F.relu(F.batch_norm(y64[:, :c], None, None, g64, b64, True, 0.0, EPS))
    v_ = lambda r: r[bn_cp:].double().view(1, -1, 1, 1, 1)
    a = torch.cat((a_bn, torch.zeros(n, bn_cp - c, d, h, w, dtype=torch.float64), F.relu(y64[:, bn_cp:] * v_(vec[0]) + v_(vec[1]))), 1)
    w64, hb64 = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    refs = R.head_ref(a, w64, hb64, act, mode)
    gs = [torch.randn(r.shape, generator=gen(8 + i)) for i, r in enumerate(refs)]
    torch.autograd.backward(refs, [g_.double() for g_ in gs])
    # kernels
    vec = vec.cuda()
    buf = y.permute(0, 2, 3, 4, 1).contiguous().cuda()
    xc = ops.CL(buf, 0, cp, vec[0], vec[1], True)
    bnvec = vec[:, :bn_cp]
    gin = ops.CL(torch.empty(n, d, h, w, cp, device="cuda"), 0, cp)
    part = torch.empty(max(ops.bn_bwd_partials_floats(n * d * h * w, bn_cp), ops.head_bwd_blocks((n, d, h, w)) * 2 * bn_cp), device="cuda")
    dw, db, rows = ops.head_bwd(xc, wt.cuda(), b.cuda(), None, act, mode, gs[0].cuda(), gs[1].cuda() if mode else None, gin,
                                (bnvec, part))
    dgam, dbet = ops.bn_relu_bwd(ops.CL(buf, 0, bn_cp), ops.CL(gin.buf, 0, bn_cp), bnvec, gamma.cuda(), c, part, None, rows)
    torch.cuda.synchronize()
    assert rel_err(dw, w64.grad) < 1e-4 and rel_err(db, hb64.grad) < 1e-4
    assert rel_err(dgam, g64.grad) < 1e-4
    assert rel_err(dbet, b64.grad) < 1e-4
    got = gin.buf.cpu().permute(0, 4, 1, 2, 3)
    assert rel_err(got[:, :c], y64.grad[:, :c]) < 2e-4
    assert torch.all(got[:, c:bn_cp] == 0)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("cin_p", [8, 32])
@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_head_16bit_widths_and_gradient_scale(name, cin_p, form):
    """Inputs rounded to the type first, so the reference sees what the kernel reads: gin is a stored 16-bit value (one ulp),
    dw / db are fp32 sums.  gscale multiplies the incoming gradients by a power of two: exact in fp32, and in bf16 storage
    (fp32's exponent range); fp16 storage may round a subnormal differently."""
    u = ULP[name]
    for co, act, mode in HEAD_COMBOS:
        case = HeadCase(cin_p, form, co, act, mode, (2, 4, 6, 10), DT[name])
        case.check_forward()
        g1, dw1, db1 = case.check_backward(gin_tol=u)
        g8, dw8, db8 = case.backward(gscale=8.0)
        assert torch.equal(dw8, 8 * dw1) and torch.equal(db8, 8 * db1)
        if name == "bf16":
            assert torch.equal(g8, 8 * g1)
        else:
            assert (g8.float() - 8 * g1.float()).abs().max().item() <= u * (8 * g1.float()).abs().max().item()
        gd, dwd, dbd = case.backward(gscale_dev=torch.tensor(8.0).cuda())
        assert torch.equal(_bits(gd), _bits(g8)) and torch.equal(dwd, dw8) and torch.equal(dbd, db8)


# ============================================================================ BatchNorm reduce / apply and channel sum
BN_CASES = [(1, 22, 12, 60, 62), (2, 56, 10, 30, 32), (2, 8, 33, 34, 62)]


def _cl_slice(x, cp, dt, pad_value=0.0):
    """[N, C, D, H, W] -> (whole buffer, CL) with the cp-wide slice at channel offset 8 of a (cp + 16)-wide sentinel buffer."""
    n, c, d, h, w = x.shape
    buf = torch.full((n, d, h, w, cp + 16), SENTINEL)
    buf[..., 8:8 + cp] = pad_value
    buf[..., 8:8 + c] = x.permute(0, 2, 3, 4, 1)
    buf = buf.to(dt).cuda()
    return buf, _ops().CL(buf, 8, cp)


def _bn_problem(shape, dt):
    """y, ga rounded to dt; gamma, beta.  Entries whose pre-activation gamma xhat + beta is within 1e-5 of ReLU's kink
    (a hundred fp32 roundings of the kernel's fma) are moved off it, so that the float64 reference and the kernel cannot
    disagree about a mask bit."""
    c = shape[1]
    y = _rnd(torch.randn(shape, generator=gen(1)) * 1.7 + 0.4, dt)
    ga = _rnd(torch.randn(shape, generator=gen(6)), dt)
    gamma = torch.rand(c, generator=gen(2)) * 1.5 - 0.25
    beta = torch.randn(c, generator=gen(3)) * 0.2
    near = lambda: F.batch_norm(y.double(), None, None, gamma.double(), beta.double(), True, 0.0, EPS).abs() < 1e-5
    for _ in range(4):
        m = near()
        if not m.any():
            break
        y[m] = _rnd(y[m] + 0.25, dt)
    assert not near().any()
    return y, ga, gamma, beta


@pytest.mark.parametrize("name", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", BN_CASES)
def test_bn_relu_bwd_idle_lanes_and_second_trip(shape, name):
    ops, dt = _ops(), DT[name]
    n, c, d, h, w = shape
    cp, nvox = ops.pad8(c), n * d * h * w
    tpv = EW_BLOCK // (cp // 4)
    assert nvox > _lib().ctu_bn_bwd_num_blocks(nvox) * tpv          # the reduce loops
    if c != 8:
        assert EW_BLOCK % (cp // 4) != 0                            # ... with idle lane rows
    y, ga, gamma, beta = _bn_problem(shape, dt)
    _, dy, dgamma, dbeta = R.bn_relu_ref(y, gamma, beta, EPS, ga)
    vec = R.bn_vectors(y, gamma, beta, EPS, cp).cuda()
    ybuf, yc = _cl_slice(y, cp, dt)
    gbuf, gc = _cl_slice(ga, cp, dt)
    y_before, g_before = ybuf.clone(), gbuf.clone()
    part = torch.empty(ops.bn_bwd_partials_floats(nvox, cp), device="cuda")
    dgam, dbet = ops.bn_relu_bwd(yc, gc, vec, gamma.cuda(), c, part)
    torch.cuda.synchronize()
    e = (rel_err(dgam, dgamma), rel_err(dbet, dbeta))
    got = gbuf[..., 8:8 + c].float().permute(0, 4, 1, 2, 3).cpu()
    e_dy = rel_err(got, dy)
    print(f"dgamma {e[0]:.3e} dbeta {e[1]:.3e} dy {e_dy:.3e}")
    assert e[0] < 1e-4 and e[1] < 1e-4
    assert e_dy < (2e-4 if name == "fp32" else 2 * ULP[name])
    assert torch.all(gbuf[..., 8 + c:8 + cp] == 0)                   # padded channels of the slice
    assert torch.equal(_bits(ybuf), _bits(y_before))
    for nb_ in (slice(0, 8), slice(8 + cp, None)):                   # the slice's neighbours
        assert torch.equal(_bits(gbuf[..., nb_]), _bits(g_before[..., nb_]))


@pytest.mark.parametrize("name", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", BN_CASES)
def test_channel_sum_against_float64(shape, name):
    ops, dt = _ops(), DT[name]
    n, c, d, h, w = shape
    cp, nvox = ops.pad8(c), n * d * h * w
    assert nvox > _lib().ctu_channel_sum_num_blocks(nvox) * (EW_BLOCK // (cp // 4))
    x = _rnd(torch.randn(shape, generator=gen(9)) + 0.25, dt)
    ref = x.double().sum((0, 2, 3, 4))
    buf, xc = _cl_slice(x, cp, dt)
    before = buf.clone()
    got = ops.channel_sum(xc, c)
    assert got.shape == (c,) and rel_err(got, ref) < 1e-4
    assert torch.equal(_bits(buf), _bits(before))
    if cp > c:                                                       # padded channels are not folded into real ones
        _, xp = _cl_slice(x, cp, dt, pad_value=5.0)
        assert torch.all(xp.buf[..., 8 + c:8 + cp] == 5.0)
        assert torch.equal(ops.channel_sum(xp, c), got)


def test_bn_finalize_more_rows_than_threads():
    ops = _ops()
    rows, c, cp = 600, 5, 8
    assert rows > 2 * FIN_BLOCK                                      # some threads sum three rows, some two
    count = 100.0 * rows
    stats = torch.full((rows, 2, cp), float("nan"))                  # columns past C are never read
    stats[:, 0, :c] = torch.rand(rows, c, generator=gen(1)) * 10
    stats[:, 1, :c] = torch.rand(rows, c, generator=gen(2)) * 50 + 40
    gamma, beta = torch.rand(c, generator=gen(3)) + 0.5, torch.rand(c, generator=gen(4)) + 1.0
    rm, rv = torch.rand(c, generator=gen(5)) * 0.1 + 0.05, torch.rand(c, generator=gen(6)) + 0.5
    s = stats[:, :, :c].double().sum(0)
    mean = s[0] / count
    var = s[1] / count - mean ** 2
    invstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma.double() * invstd
    want = torch.stack((scale, beta.double() - mean * scale, mean, invstd))
    rm_g, rv_g = rm.cuda(), rv.cuda()
    vec = ops.bn_finalize(stats.cuda(), rows, c, cp, count, gamma.cuda(), beta.cuda(), rm_g, rv_g, 0.1, EPS, 1).cpu()
    assert torch.allclose(vec[:, :c].double(), want, rtol=1e-5, atol=0)
    assert torch.all(vec[:, c:] == 0)
    assert torch.allclose(rm_g.cpu().double(), 0.9 * rm.double() + 0.1 * mean, rtol=1e-5, atol=0)
    assert torch.allclose(rv_g.cpu().double(), 0.9 * rv.double() + 0.1 * var * count / (count - 1), rtol=1e-5, atol=0)


def test_bn_bwd_finalize_more_rows_than_threads():
    """ctu_bn_bwd_finalize over 600 partial rows (ops.bn_relu_bwd with pre_reduced rows, lazy: neither reduce nor apply runs)."""
    ops = _ops()
    rows, c, cp = 600, 5, 8
    assert rows > 2 * EW_BLOCK
    part = torch.full((rows, 2, cp), float("nan"))
    part[:, 0, :c] = torch.rand(rows, c, generator=gen(1)) + 0.5     # one-signed sums: no cancellation in coef row 4
    part[:, 1, :c] = torch.rand(rows, c, generator=gen(2)) * 0.2
    gamma = torch.rand(c, generator=gen(3)) + 0.5
    vec = torch.zeros(4, cp)
    vec[2, :c] = torch.randn(c, generator=gen(4)) * 0.1
    vec[3, :c] = torch.rand(c, generator=gen(5)) + 0.5
    y = ops.CL(torch.zeros(1, 10, 10, 60, cp, device="cuda"), 0, cp)
    count = float(y.nvox)
    dgam, dbet, coef = ops.bn_relu_bwd(y, y, vec.cuda(), gamma.cuda(), c, part.cuda(), None, rows, lazy=True)
    s = part[:, :, :c].double().sum(0)
    mu, istd = vec[2, :c].double(), vec[3, :c].double()
    k0, k1, k2 = gamma.double() * istd, s[0] / count, s[1] / count
    want = torch.stack((k0, k1, k2, -k0 * k2 * istd, -k0 * (k1 - k2 * mu * istd)))
    assert torch.allclose(dbet.cpu().double(), s[0], rtol=1e-5, atol=0)
    assert torch.allclose(dgam.cpu().double(), s[1], rtol=1e-5, atol=0)
    assert torch.allclose(coef[:, :c].cpu().double(), want, rtol=1e-5, atol=0)
    assert torch.all(coef[:, c:] == 0)


# ============================================================================== BatchNorm statistics away from zero mean
def _stats_through_identity_conv(y, gamma, beta):
    """(raw output CL, vec [4, cp]) the way a layer gets them: partial rows from a conv's epilogue (an identity k = 3 conv, as
    in test_batchnorm_train_fwd_bwd), then bn_finalize."""
    ops = _ops()
    n, c, d, h, w = y.shape
    cp = ops.pad8(c)
    buf = torch.zeros(n, d, h, w, cp)
    buf[..., :c] = y.permute(0, 2, 3, 4, 1)
    wt = torch.zeros(c, c, 3, 3, 3); wt[range(c), range(c), 1, 1, 1] = 1.0
    wp = ops.pack_conv_w(wt.cuda(), None, cp, cp, 0)
    out = ops.CL(torch.empty(n, d, h, w, cp, device="cuda"), 0, cp)
    nb = ops.conv_num_blocks((n, d, h, w), cp, 0, 3)
    stats = torch.zeros(nb, 2, cp, device="cuda")
    ops.conv3d_fwd(ops.CL(buf.cuda(), 0, cp), wp, None, out, 3, stats)
    vec = ops.bn_finalize(stats, nb, c, cp, n * d * h * w, gamma.cuda(), beta.cuda(), None, None, 0.1, EPS, 0)
    torch.cuda.synchronize()
    assert torch.equal(out.buf[..., :c].cpu(), buf[..., :c])         # the identity conv reproduces y exactly
    return out, vec


def _activated(y, vec):
    c = y.shape[1]
    v = vec.cpu()
    return F.relu(y * v[0, :c].view(1, -1, 1, 1, 1) + v[1, :c].view(1, -1, 1, 1, 1))


def test_bn_statistics_dead_channels():
    """A channel of zeros and a channel of the constant 3.0 among random ones: the variance is exactly zero, invstd is
    1 / sqrt(eps) evaluated in float32 (F.batch_norm's own saved invstd keeps eps in double and is one float32 ulp below),
    and nothing downstream leaves the finite range."""
    ops = _ops()
    shape = (2, 8, 8, 8, 8)
    c = shape[1]
    y = torch.randn(shape, generator=gen(1)) * 1.7 + 0.4
    y[:, 2], y[:, 5] = 0.0, 3.0
    gamma, beta = torch.rand(c, generator=gen(2)) + 0.5, torch.randn(c, generator=gen(3)) * 0.5
    beta[5] = 0.3
    out, vec = _stats_through_identity_conv(y, gamma, beta)
    assert torch.isfinite(vec).all()
    dead = (1.0 / torch.sqrt(torch.tensor(0.0) + EPS)).item()
    assert vec[3, 2].item() == dead and vec[3, 5].item() == dead
    assert vec[2, 2].item() == 0.0 and vec[2, 5].item() == 3.0
    act = _activated(y, vec)
    ref = R.bn_relu_ref(y, gamma, beta, EPS)
    assert torch.isfinite(act).all()
    for ch in (2, 5):
        assert (act[:, ch] - F.relu(beta[ch])).abs().max().item() <= 1e-3
    live = [q for q in range(c) if q not in (2, 5)]
    assert rel_err(act[:, live], ref[:, live]) < 1e-4
    ga = torch.randn(shape, generator=gen(6))
    gac = ops.CL(ga.permute(0, 2, 3, 4, 1).contiguous().cuda(), 0, c)
    part = torch.empty(ops.bn_bwd_partials_floats(out.nvox, c), device="cuda")
    dgam, dbet = ops.bn_relu_bwd(out, gac, vec, gamma.cuda(), c, part)
    torch.cuda.synchronize()
    assert torch.isfinite(dgam).all() and torch.isfinite(dbet).all() and torch.isfinite(gac.buf).all()


@pytest.mark.parametrize("r", [0.0, 8.0, 32.0])
def test_bn_statistics_offset_envelope(r):
    """y = randn + r: var = E[x^2] - mean^2 loses log2(1 + r^2) bits.  The yardstick is the same one-pass formula done plainly
    in float32 (numpy sums, pairwise); the kernel's error in invstd (relative) and in the activated output (absolute) against
    float64 two-pass statistics must be at most 8x the yardstick's (floor 1e-6): the factor covers the summation order."""
    shape = (2, 8, 16, 16, 16)
    c = shape[1]
    y = torch.randn(shape, generator=gen(1)) + r
    gamma, beta = torch.rand(c, generator=gen(2)) + 0.5, torch.randn(c, generator=gen(3)) * 0.2
    ref_vec = R.bn_vectors(y, gamma, beta, EPS, c).double()
    ref_invstd = 1.0 / torch.sqrt(y.double().var(dim=(0, 2, 3, 4), unbiased=False) + EPS)
    ref_act = R.bn_relu_ref(y, gamma, beta, EPS)
    # yardstick: float32 one-pass
    yn = y.permute(1, 0, 2, 3, 4).reshape(c, -1).numpy()
    cnt = np.float32(yn.shape[1])
    mean = yn.sum(1, dtype=np.float32) / cnt
    var = np.maximum((yn * yn).sum(1, dtype=np.float32) / cnt - mean * mean, np.float32(0))
    invstd = (np.float32(1) / np.sqrt(var + np.float32(EPS))).astype(np.float32)
    sc = gamma.numpy() * invstd
    yard_vec = torch.from_numpy(np.stack((sc, beta.numpy() - mean * sc, mean, invstd)))
    _, vec = _stats_through_identity_conv(y, gamma, beta)

    def errors(v):
        e_is = ((v[3, :c].double().cpu() - ref_invstd).abs() / ref_invstd).max().item()
        e_act = (_activated(y, v).double() - ref_act).abs().max().item()
        return e_is, e_act
    (k_is, k_act), (y_is, y_act) = errors(vec), errors(yard_vec)
    print(f"offset {r}: invstd rel err kernel {k_is:.3e} yardstick {y_is:.3e}; activated abs err kernel {k_act:.3e} "
          f"yardstick {y_act:.3e}")
    assert torch.isfinite(vec).all() and ref_vec.shape == (4, c)
    assert k_is <= 8 * max(y_is, 1e-6)
    assert k_act <= 8 * max(y_act, 1e-6)
