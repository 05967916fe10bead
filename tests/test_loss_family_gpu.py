"""The segmentation loss family kernels (csrc/loss_family.hip: class-weighted / focal cross-entropy, Dice, Tversky, boundary)
against the float64 reference of tests/loss_family_ref.py, at the shapes where the code changes path -- the scalar path
(V not a multiple of 4, or a plane that is not 16-byte aligned), the vector path, the second trip of the grid-stride loops --
and through the host layers: ``seg_loss`` under autograd, ``boundary_map``, and a whole train step run eagerly and through
``GraphedTrainStep(loss=...)``.

Gates are those of the plain loss in test_stream_kernels_gpu.py: every term 1e-5 * max(1, |ref|), the gradient's largest
error under 1e-4 of the reference's largest entry.  The graphed-versus-eager gate is test_models_gpu.py's
test_graphed_step_equals_eager_step: losses 1e-5 absolute, state rtol 1e-4 / atol 1e-6.

Inputs: the prediction is 2 randn in the softmax view.  In the raw view the probability view is the prediction itself, and
the Tversky ratio's denominator alpha sum q + beta sum g + (1 - alpha - beta) TP passes through 0 for a zero-mean q; a single
head hands the loss sigmoid / softmax outputs, so the raw-view cases with a Tversky term use softmax(2 randn) + 0.05 randn.
The cases without one keep 2 randn (and 30 randn for the saturated logits) in both views."""
import math

import pytest
import torch
import torch.nn.functional as F

import loss_family_ref as LR
from util import gen, rel_err

pytestmark = pytest.mark.gpu

HB, LOSS_BX, ROW, TAIL = 256, 1024, 8, 4             # loss_family.hip: block size, blocks per item, partial row, tail per item
SENTINEL = -77.0
SMALL = [(2, 2, 3, 5, 7), (2, 2, 6, 8, 10)]          # scalar path (V = 105), vector path (V = 480)
VIEWS = [False, True]


def _ops():
    from ctunet_amd import ops
    return ops


def case(lam, w=(1.0, 1.0), gamma=0.0, ab=(0.5, 0.5)):
    return dict(lam=tuple(float(x) for x in lam), w=w, gamma=gamma, ab=ab)


FULL = case((0.5, 2.0, 1.5, 0.8), (0.2, 0.8), 2.0, (0.3, 0.7))
ALONE = {"ce": case((0.5, 0, 0, 0), (0.2, 0.8), 2.0), "dice": case((0, 2.0, 0, 0)), "tversky": case((0, 0, 1.5, 0), ab=(0.3, 0.7)),
         "boundary": case((0, 0, 0, 0.8)), "weighted_ce": case((0.5, 0, 0, 0), (0.2, 0.8)), "all": FULL}


def _kw(c):
    return dict(class_weight=c["w"], focal_gamma=c["gamma"], tversky_ab=c["ab"])


def _inputs(shape, seed, sm, c, soft=False, scale=2.0):
    """(pred, target, phi) on the CPU, float32 (module docstring)."""
    p = torch.randn(shape, generator=gen(seed)) * scale
    if not sm and c["lam"][2] != 0:
        p = F.softmax(p, 1) + 0.05 * torch.randn(shape, generator=gen(seed + 2))
    if soft:
        t = torch.rand(shape, generator=gen(seed + 1))
    else:
        m = (torch.rand((shape[0],) + tuple(shape[2:]), generator=gen(seed + 1)) < 0.3).long()
        t = F.one_hot(m, 2).movedim(4, 1).float().contiguous()
    phi = torch.randn((shape[0],) + tuple(shape[2:]), generator=gen(seed + 3)) * 3.0
    return p.contiguous(), t, phi


def _ref(p, t, phi, sm, c, up=(1.0, 1.0, 1.0, 1.0)):
    """float64 terms and the gradient of sum up_i term_i."""
    p64 = p.double().requires_grad_(True)
    lam = c["lam"]
    terms = LR.seg_loss_ref(p64, t, sm, ce_lambda=lam[0], dice_lambda=lam[1], class_weight=c["w"], focal_gamma=c["gamma"],
                            tversky_lambda=lam[2], tversky_alpha=c["ab"][0], tversky_beta=c["ab"][1], boundary_lambda=lam[3],
                            phi=phi)
    total = sum(u * x for u, x in zip(up, terms))
    if total.requires_grad:
        total.backward()
    return [x.item() for x in terms], (p64.grad if p64.grad is not None else torch.zeros_like(p64))


def _check_terms(terms, ref, lam):
    got = terms.cpu().tolist()
    print(f"loss terms: kernel {got}, reference {ref}")
    assert len(got) == 4
    for v, r, l in zip(got, ref, lam):
        assert math.isfinite(v) and abs(v - r) <= 1e-5 * max(1.0, abs(r)), (got, ref)
        if l == 0:
            assert v == 0.0


def _check_grad(gp, ref):
    assert torch.isfinite(gp).all()
    err = rel_err(gp, ref)
    print(f"loss gradient rel err {err:.3e} (largest reference entry {ref.abs().max().item():.3e})")
    assert err < 1e-4


def _run(pg, tg, fg, sm, c, up=(None,) * 4, out=None, accumulate=False):
    ops = _ops()
    phi = fg if c["lam"][3] != 0 else None
    terms, ws = ops.seg_loss_fwd(pg, tg, c["lam"], sm, boundary=phi, **_kw(c))
    gp = ops.seg_loss_bwd(pg, tg, c["lam"], sm, ws, up, boundary=phi, out=out, accumulate=accumulate, **_kw(c))
    return terms, ws, gp


def _takes_vector_path(*tensors):
    v = tensors[0][0].numel() // (2 if tensors[0].dim() == 5 else 1)
    return v % 4 == 0 and all(x.data_ptr() % 16 == 0 for x in tensors)


# ===================================================================================== each term, and all of them
@pytest.mark.parametrize("sm", VIEWS)
@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("name", list(ALONE))
def test_each_term_alone_and_all_together(name, shape, sm):
    c = ALONE[name]
    assert ((shape[2] * shape[3] * shape[4]) % 4 == 0) == (shape == SMALL[1])
    p, t, phi = _inputs(shape, 11, sm, c)
    ref, gref = _ref(p, t, phi, sm, c)
    assert [r != 0 for r in ref] == [l != 0 for l in c["lam"]]
    terms, _, gp = _run(p.cuda(), t.cuda(), phi.cuda(), sm, c)
    _check_terms(terms, ref, c["lam"])
    _check_grad(gp.cpu(), gref)
    if name in ("tversky", "boundary") and not sm:
        assert torch.all(gp[:, 0] == 0)               # raw view: only channel 1 receives these gradients


@pytest.mark.parametrize("sm", VIEWS)
def test_boundary_map_may_carry_a_channel_axis_and_is_not_read_without_its_term(sm):
    ops = _ops()
    shape = SMALL[1]
    p, t, phi = _inputs(shape, 15, sm, FULL)
    pg, tg, fg = p.cuda(), t.cuda(), phi.cuda()
    a, ws_a = ops.seg_loss_fwd(pg, tg, FULL["lam"], sm, boundary=fg, **_kw(FULL))
    b, ws_b = ops.seg_loss_fwd(pg, tg, FULL["lam"], sm, boundary=fg.unsqueeze(1), **_kw(FULL))
    assert torch.equal(a, b) and torch.equal(ws_a, ws_b)
    c = case((0.5, 2.0, 1.5, 0.0), (0.2, 0.8), 2.0, (0.3, 0.7))
    poison = torch.full_like(fg, float("nan"))
    x, ws_x = ops.seg_loss_fwd(pg, tg, c["lam"], sm, boundary=poison, **_kw(c))
    y, ws_y = ops.seg_loss_fwd(pg, tg, c["lam"], sm, boundary=None, **_kw(c))
    assert torch.equal(x, y) and torch.equal(x[:3], a[:3]) and x[3].item() == 0.0
    assert torch.equal(ops.seg_loss_bwd(pg, tg, c["lam"], sm, ws_x, boundary=poison, **_kw(c)),
                       ops.seg_loss_bwd(pg, tg, c["lam"], sm, ws_y, **_kw(c)))
    with pytest.raises(ValueError, match="boundary"):
        ops.seg_loss_fwd(pg, tg, FULL["lam"], sm, **_kw(FULL))
    with pytest.raises(ValueError, match="boundary map must be float32"):
        ops.seg_loss_fwd(pg, tg, FULL["lam"], sm, boundary=fg[:, :3], **_kw(FULL))


# ===================================================================================== paths
@pytest.mark.parametrize("sm", VIEWS)
def test_scalar_path_misaligned_planes(sm):
    """V = 480 is a multiple of 4, but every plane -- the distance map and the output included -- starts one float into its
    allocation; the floats around the written span keep their sentinel."""
    ops = _ops()
    shape = SMALL[1]
    p, t, phi = _inputs(shape, 21, sm, FULL)
    ref, gref = _ref(p, t, phi, sm, FULL)

    def off_by_one(x, fill=0.0):
        big = torch.full((x.numel() + 8,), fill, device="cuda")
        big[1:1 + x.numel()] = x.flatten().cuda()
        view = big[1:1 + x.numel()].view(x.shape)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return big, view
    _, pg = off_by_one(p)
    _, tg = off_by_one(t)
    _, fg = off_by_one(phi)
    assert not _takes_vector_path(pg, tg, fg)
    terms, ws = ops.seg_loss_fwd(pg, tg, FULL["lam"], sm, boundary=fg, **_kw(FULL))
    _check_terms(terms, ref, FULL["lam"])
    base = torch.randn(shape, generator=gen(23))
    for accumulate in (False, True):
        big, out = off_by_one(base, SENTINEL)
        big[0] = SENTINEL
        got = ops.seg_loss_bwd(pg, tg, FULL["lam"], sm, ws, boundary=fg, out=out, accumulate=accumulate, **_kw(FULL))
        assert got.data_ptr() == out.data_ptr() and got.data_ptr() % 16 == 4
        _check_grad(out.cpu(), gref + base.double() if accumulate else gref)
        assert big[0].item() == SENTINEL and torch.all(big[1 + p.numel():] == SENTINEL)
    # one misaligned operand is enough to leave the vector path: the distance map alone, then the output alone
    pa, ta = p.cuda(), t.cuda()
    assert _takes_vector_path(pa, ta) and not _takes_vector_path(pa, ta, fg)
    terms, ws = ops.seg_loss_fwd(pa, ta, FULL["lam"], sm, boundary=fg, **_kw(FULL))
    _check_terms(terms, ref, FULL["lam"])
    _check_grad(ops.seg_loss_bwd(pa, ta, FULL["lam"], sm, ws, boundary=fg, **_kw(FULL)).cpu(), gref)
    big, out = off_by_one(base, SENTINEL)
    _check_grad(ops.seg_loss_bwd(pa, ta, FULL["lam"], sm, ws, boundary=phi.cuda(), out=out, **_kw(FULL)).cpu(), gref)
    assert big[0].item() == SENTINEL and torch.all(big[1 + p.numel():] == SENTINEL)


@pytest.mark.parametrize("sm", VIEWS)
@pytest.mark.parametrize("shape,vector", [((1, 2, 66, 128, 128), True), ((2, 2, 65, 65, 63), False)])
def test_second_trip_of_the_grid_stride_loops_and_bit_equal_calls(shape, vector, sm):
    v = shape[2] * shape[3] * shape[4]
    lanes = v // 4 if vector else v
    assert (v % 4 == 0) == vector and LOSS_BX * HB < lanes < 2 * LOSS_BX * HB     # some lanes take two trips, some one
    p, t, phi = _inputs(shape, 31, sm, FULL)
    ref, gref = _ref(p, t, phi, sm, FULL)
    pg, tg, fg = p.cuda(), t.cuda(), phi.cuda()
    assert _takes_vector_path(pg, tg, fg) == vector
    terms, ws, gp = _run(pg, tg, fg, sm, FULL)
    _check_terms(terms, ref, FULL["lam"])
    _check_grad(gp.cpu(), gref)
    terms2, ws2, gp2 = _run(pg, tg, fg, sm, FULL)
    assert torch.equal(terms, terms2) and torch.equal(ws, ws2) and torch.equal(gp, gp2)


@pytest.mark.parametrize("sm", VIEWS)
@pytest.mark.parametrize("shape", SMALL)
def test_two_calls_are_bit_equal(shape, sm):
    p, t, phi = _inputs(shape, 35, sm, FULL)
    pg, tg, fg = p.cuda(), t.cuda(), phi.cuda()
    a = _run(pg, tg, fg, sm, FULL)
    b = _run(pg, tg, fg, sm, FULL)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ===================================================================================== parameters that a swap would hide
def _compare(shape, sm, c, other, seed):
    """The kernel follows ``c``; the reference of ``other`` is far outside the gate, so the two cannot be confused."""
    p, t, phi = _inputs(shape, seed, sm, c)
    ref, gref = _ref(p, t, phi, sm, c)
    _, gother = _ref(p, t, phi, sm, other)
    diff = rel_err(gother, gref)
    print(f"references differ by {diff:.3f} relative")
    assert diff > 0.1
    terms, _, gp = _run(p.cuda(), t.cuda(), phi.cuda(), sm, c)
    _check_terms(terms, ref, c["lam"])
    _check_grad(gp.cpu(), gref)


@pytest.mark.parametrize("sm", VIEWS)
@pytest.mark.parametrize("shape", SMALL)
def test_class_weights_against_the_swapped_pair(shape, sm):
    _compare(shape, sm, case((1.0, 0, 0, 0), (0.2, 0.8)), case((1.0, 0, 0, 0), (0.8, 0.2)), 41)


@pytest.mark.parametrize("sm", VIEWS)
@pytest.mark.parametrize("shape", SMALL)
def test_tversky_alpha_beta_against_the_swapped_pair(shape, sm):
    _compare(shape, sm, case((0, 0, 1.0, 0), ab=(0.3, 0.7)), case((0, 0, 1.0, 0), ab=(0.7, 0.3)), 43)


@pytest.mark.parametrize("sm", VIEWS)
@pytest.mark.parametrize("shape", SMALL)
def test_focal_gamma_two_against_zero(shape, sm):
    _compare(shape, sm, case((1.0, 0, 0, 0), gamma=2.0), case((1.0, 0, 0, 0)), 45)
    _compare(shape, sm, case((1.0, 0, 0, 0)), case((1.0, 0, 0, 0), gamma=2.0), 45)


@pytest.mark.parametrize("sm", VIEWS)
@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0, 5.0])
def test_focal_saturated_logits(gamma, sm):
    """pred = 30 randn: |a - b| passes 89, the other class's probability underflows; (1 - p)^(gamma - 1) log p would be
    inf * 0 for gamma < 1."""
    for shape in SMALL:
        c = case((0.5, 2.0, 0, 0), (0.2, 0.8), gamma)
        p, t, phi = _inputs(shape, 51, sm, c, scale=30.0)
        assert (p[:, 0] - p[:, 1]).abs().max().item() > 89.0        # exp(89) > FLT_MAX
        ref, gref = _ref(p, t, phi, sm, c)
        terms, _, gp = _run(p.cuda(), t.cuda(), phi.cuda(), sm, c)
        _check_terms(terms, ref, c["lam"])
        _check_grad(gp.cpu(), gref)


@pytest.mark.parametrize("sm", VIEWS)
@pytest.mark.parametrize("shape", SMALL)
def test_soft_and_tied_targets(shape, sm):
    """Targets that are not one-hot, one row with t0 == t1 exactly: the class of a tie is 0, and it takes w0."""
    p, t, phi = _inputs(shape, 61, sm, FULL, soft=True)
    t[:, 1, 1, 2, :] = t[:, 0, 1, 2, :]
    assert (t[:, 1] == t[:, 0]).sum().item() == shape[0] * shape[4]
    ref, gref = _ref(p, t, phi, sm, FULL)
    terms, _, gp = _run(p.cuda(), t.cuda(), phi.cuda(), sm, FULL)
    _check_terms(terms, ref, FULL["lam"])
    _check_grad(gp.cpu(), gref)
    _compare(shape, sm, case((1.0, 0, 0, 0), (0.2, 0.8)), case((1.0, 0, 0, 0), (0.8, 0.2)), 63)


@pytest.mark.parametrize("sm", VIEWS)
def test_three_items_the_middle_one_empty_with_infinite_phi(sm):
    """The middle item is all background with an all-zero prediction and phi = +inf (what signed_distance returns for it):
    its Dice and Tversky ratios come from eps alone, the tail and the gradient stay finite, and the boundary term skips it."""
    shape = (3, 2, 6, 8, 10)
    p, t, phi = _inputs(shape, 71, sm, FULL)
    t[1, 0], t[1, 1] = 1.0, 0.0
    p[1] = 0.0
    phi[1] = float("inf")
    phi[0, 0, 0, :3] = torch.tensor([float("-inf"), float("nan"), float("inf")])
    ref, gref = _ref(p, t, phi, sm, FULL)
    terms, ws, gp = _run(p.cuda(), t.cuda(), phi.cuda(), sm, FULL)
    _check_terms(terms, ref, FULL["lam"])
    tail = ws[3 * LOSS_BX * ROW:3 * LOSS_BX * ROW + 3 * TAIL + 1].cpu()
    print("tail", tail.tolist())
    assert torch.isfinite(tail).all()
    w = torch.where(t[:, 1] > t[:, 0], 0.8, 0.2).double().sum().item()
    assert abs(tail[-1].item() - w) <= 1e-5 * w                      # the global weight sum
    if not sm:
        assert abs(tail[TAIL + 0].item() - 1e-7) < 1e-12 and tail[TAIL + 1].item() == 480.0
    _check_grad(gp.cpu(), gref)
    # in the raw view the empty item's Tversky gradient is alpha / (N eps) per voxel and dwarfs the rest: the others apart
    _check_grad(gp.cpu()[[0, 2]], gref[[0, 2]])
    c = case((0, 0, 0, 0.8))
    _, _, gb = _run(p.cuda(), t.cuda(), phi.cuda(), sm, c)
    assert torch.all(gb[1] == 0) and torch.all(gb[0, :, 0, 0, :3] == 0) and gb[0].abs().sum().item() > 0


@pytest.mark.parametrize("sm", VIEWS)
@pytest.mark.parametrize("shape", SMALL)
def test_distinct_upstream_gradients(shape, sm):
    """Upstream 2, 0.5, 3, 0.25: the gradient is the sum of the four terms' gradients, each times its own; any other
    assignment of the four is far outside the gate."""
    up = (2.0, 0.5, 3.0, 0.25)
    p, t, phi = _inputs(shape, 81, sm, FULL)
    _, gref = _ref(p, t, phi, sm, FULL, up)
    for other in ((0.5, 2.0, 3.0, 0.25), (2.0, 0.5, 0.25, 3.0), (3.0, 0.5, 2.0, 0.25), (1.0, 1.0, 1.0, 1.0)):
        diff = rel_err(_ref(p, t, phi, sm, FULL, other)[1], gref)
        print(f"upstream {other}: references differ by {diff:.3f} relative")
        assert diff > 0.1
    pg, tg, fg = p.cuda(), t.cuda(), phi.cuda()
    ups = tuple(torch.tensor(u).cuda() for u in up)
    _, _, gp = _run(pg, tg, fg, sm, FULL, ups)
    _check_grad(gp.cpu(), gref)
    base = torch.randn(shape, generator=gen(83))
    _, _, gp = _run(pg, tg, fg, sm, FULL, ups, base.cuda(), True)
    _check_grad(gp.cpu(), gref + base.double())
    # some given, the others defaulting to 1
    _, g1 = _ref(p, t, phi, sm, FULL, (1.0, 0.5, 1.0, 0.25))
    _, _, gp = _run(pg, tg, fg, sm, FULL, (None, ups[1], None, ups[3]))
    _check_grad(gp.cpu(), g1)


@pytest.mark.parametrize("sm", VIEWS)
@pytest.mark.parametrize("shape", SMALL)
def test_accumulate_and_out(shape, sm):
    p, t, phi = _inputs(shape, 91, sm, FULL)
    _, gref = _ref(p, t, phi, sm, FULL)
    base = torch.randn(shape, generator=gen(93))
    out = base.cuda()
    _, _, gp = _run(p.cuda(), t.cuda(), phi.cuda(), sm, FULL, out=out, accumulate=True)
    assert gp.data_ptr() == out.data_ptr()
    _check_grad(gp.cpu(), gref + base.double())
    _, _, gp = _run(p.cuda(), t.cuda(), phi.cuda(), sm, FULL, out=out, accumulate=False)        # overwrites
    assert gp.data_ptr() == out.data_ptr()
    _check_grad(gp.cpu(), gref)


# ===================================================================================== host layer
@pytest.mark.parametrize("sm", VIEWS)
@pytest.mark.parametrize("shape", SMALL + [(1, 2, 66, 128, 128)])
def test_default_spec_is_bit_equal_to_the_plain_kernels(shape, sm):
    from ctunet_amd import LossSpec, seg_loss
    ops = _ops()
    p, t, _ = _inputs(shape, 101, sm, case((0.5, 2.0, 0, 0)))
    pg, tg = p.cuda(), t.cuda()
    terms, ws = ops.loss_fwd(pg, tg, 0.5, 2.0, sm)
    g0 = ops.loss_bwd(pg, tg, 0.5, 2.0, sm, ws, None, None)
    pl = pg.clone().requires_grad_(True)
    out = seg_loss(pl, tg, LossSpec(0.5, 2.0), sm)
    assert len(out) == 4 and all(x.dim() == 0 for x in out)
    assert torch.equal(out[0], terms[0]) and torch.equal(out[1], terms[1]) and out[2].item() == 0.0 and out[3].item() == 0.0
    (out[0] + out[1] + out[2] + out[3]).backward()
    assert torch.equal(pl.grad, g0)


@pytest.mark.parametrize("sm", VIEWS)
@pytest.mark.parametrize("shape", SMALL)
def test_new_kernels_without_extensions_give_the_plain_terms(shape, sm):
    """w = (1, 1), gamma = 0, no Tversky, no map on the NEW kernels: the plain CE + Dice values and gradient, at the gates
    (not bit for bit: one exponential per voxel instead of two)."""
    ops = _ops()
    c = case((0.5, 2.0, 0, 0))
    p, t, phi = _inputs(shape, 105, sm, c)
    pg, tg = p.cuda(), t.cuda()
    terms0, ws0 = ops.loss_fwd(pg, tg, 0.5, 2.0, sm)
    g0 = ops.loss_bwd(pg, tg, 0.5, 2.0, sm, ws0, None, None)
    terms, _, gp = _run(pg, tg, None, sm, c)
    _check_terms(terms, terms0.double().tolist() + [0.0, 0.0], c["lam"])
    _check_grad(gp.cpu(), g0.cpu().double())
    ref, gref = _ref(p, t, phi, sm, c)
    _check_terms(terms, ref, c["lam"])
    _check_grad(gp.cpu(), gref)


@pytest.mark.parametrize("sm", VIEWS)
def test_seg_loss_under_autograd(sm):
    """One autograd.Function, four 0-d outputs: distinct upstream factors, and a term left out of the total gets none."""
    from ctunet_amd import LossSpec, seg_loss
    shape = SMALL[1]
    spec = LossSpec(0.5, 2.0, class_weight=(0.2, 0.8), focal_gamma=2.0, tversky_lambda=1.5, tversky_alpha=0.3, tversky_beta=0.7,
                    boundary_lambda=0.8)
    p, t, phi = _inputs(shape, 111, sm, FULL)
    ref, gref = _ref(p, t, phi, sm, FULL, (2.0, 0.5, 3.0, 0.25))
    pl = p.cuda().requires_grad_(True)
    out = seg_loss(pl, t.cuda(), spec, sm, phi.cuda())
    assert all(x.dim() == 0 and x.dtype == torch.float32 for x in out)
    _check_terms(torch.stack([x.detach() for x in out]), ref, FULL["lam"])
    (2.0 * out[0] + 0.5 * out[1] + 3.0 * out[2] + 0.25 * out[3]).backward()
    _check_grad(pl.grad.cpu(), gref)
    _, g2 = _ref(p, t, phi, sm, FULL, (1.0, 0.0, 1.0, 0.0))
    pl = p.cuda().requires_grad_(True)
    out = seg_loss(pl, t.cuda(), spec, sm, phi.cuda())
    (out[0] + out[2]).backward()
    _check_grad(pl.grad.cpu(), g2)


def _blobs(n, side, seed):
    """One-hot targets [n,2,side^3] with a few boxes of foreground."""
    g = gen(seed)
    m = torch.zeros(n, side, side, side, dtype=torch.long)
    for i in range(n):
        for _ in range(3):
            lo = torch.randint(0, side - 4, (3,), generator=g).tolist()
            sz = torch.randint(2, 5, (3,), generator=g).tolist()
            m[i, lo[0]:lo[0] + sz[0], lo[1]:lo[1] + sz[1], lo[2]:lo[2] + sz[2]] = 1
    return F.one_hot(m, 2).movedim(4, 1).float().contiguous()


@pytest.mark.parametrize("sm", VIEWS)
def test_boundary_map_is_the_signed_distance_and_feeds_the_loss(sm):
    from ctunet_amd import LossSpec, boundary_map, postprocess, seg_loss
    t = _blobs(3, 12, 121)
    t[1, 0], t[1, 1] = 1.0, 0.0                                      # an item without foreground: +inf everywhere
    tg = t.cuda()
    sampling = (1.5, 0.5, 0.75)
    for sp in (None, sampling):
        phi = boundary_map(tg, sp)
        want = postprocess.signed_distance(tg[:, 1] > 0.5, sampling=sp)
        assert phi.dtype == torch.float32 and phi.shape == (3, 12, 12, 12) and phi.is_cuda and torch.equal(phi, want)
    assert torch.all(phi[1] == float("inf")) and torch.isfinite(phi[[0, 2]]).all()
    fg = t[:, 1] > 0.5
    assert torch.all(phi.cpu()[fg] < 0) and torch.all(phi.cpu()[~fg] > 0)        # negative inside, positive outside
    spec = LossSpec(0.0, 0.0, boundary_lambda=0.8)
    c = case((0, 0, 0, 0.8))
    p = torch.rand(3, 2, 12, 12, 12, generator=gen(123))
    ref, gref = _ref(p, t, phi.cpu(), sm, c)
    pl = p.cuda().requires_grad_(True)
    out = seg_loss(pl, tg, spec, sm, phi)
    _check_terms(torch.stack([x.detach() for x in out]), ref, c["lam"])
    out[3].backward()
    _check_grad(pl.grad.cpu(), gref)
    assert torch.all(pl.grad[1] == 0)
    # a prediction that leaks outside the object costs more than one that stays inside it
    inside = torch.stack([1 - t[:, 1], t[:, 1]], 1).cuda()
    leak = torch.ones_like(inside) * 0.5
    f = lambda x: seg_loss(x, tg, spec, False, phi)[3].item()
    assert f(inside) < 0 and f(inside) < f(leak)


# ===================================================================================== whole path
class _Holder:
    verbose = False
    pt_loss = None

    def __init__(self, **params):
        self.params = dict(save_dice_plots=False, save_hd_plots=False, **params)
        self.losses_and_metrics = {}


def _net(two):
    from ctunet_amd import models as M
    if not two:
        return M.UNet(input_channels=1, out_channels=2, n_blocks=2, i_size=2, use_checkpoint=False)

    class TinySP(M.UNetSP):
        def __init__(self):
            M.UNet.__init__(self, input_channels=2, out_channels=3, n_blocks=2, i_size=2, use_checkpoint=False)
            self._set_head()
    return TinySP()


@pytest.mark.parametrize("two", [False, True])
def test_graphed_step_with_a_loss_spec_equals_the_eager_step(two):
    """UNet(n_blocks=2, i_size=2) at 16^3 and its two-head form: eager ``seg_loss`` + backward + fused Adam against
    ``GraphedTrainStep(loss=spec, example_boundary=...)`` at the gate of test_graphed_step_equals_eager_step; then the
    replay follows a new map copied into ``step.boundary[0]``."""
    from ctunet_amd import LossSpec, boundary_map, optim, seg_loss
    from ctunet_amd.graph import GraphedTrainStep
    from ctunet_amd.losses import select_loss_terms
    spec = LossSpec(1.0, 1.0, class_weight=(0.3, 0.7), focal_gamma=2.0, tversky_lambda=1.0, tversky_alpha=0.3, tversky_beta=0.7,
                    boundary_lambda=0.1)
    n = 1 if two else 2
    x = torch.randn(n, 2 if two else 1, 16, 16, 16, generator=gen(3)).cuda()
    tg = [_blobs(n, 16, 131 + i).cuda() for i in range(2 if two else 1)]
    maps = [boundary_map(t) for t in tg]
    assert all(torch.isfinite(m).all() for m in maps)

    def make():
        torch.manual_seed(0)
        net = _net(two).cuda().train()
        return net, optim.Adam(net.parameters(), lr=1e-3, amsgrad=True)

    def eager_step(net, opt, phis):
        out = net(x.clone().requires_grad_(True))
        outs = list(out) if two else [out]
        heads = [seg_loss(o, t, spec, two, f) for o, t, f in zip(outs, tg, phis)]
        keys, terms = select_loss_terms(heads, spec)
        total = sum(terms[1:], terms[0])
        total.backward()
        opt.step()
        for p in net.parameters():
            p.grad = None
        return keys, total.item(), outs

    net_e, opt_e = make()
    losses_e = []
    for _ in range(3 + 2):                      # GraphedTrainStep runs 3 warm-up steps, the capture executes nothing
        keys_e, l, _ = eager_step(net_e, opt_e, maps)
        losses_e.append(l)
    net_g, opt_g = make()
    gs = GraphedTrainStep(net_g, opt_g, x, tg, 0.0, 0.0, warmup=3, loss=spec, example_boundary=maps)
    sfx = ("_sk", "_fl") if two else ("",)
    want = [k + s for k in ("ce", "dice_loss", "tversky_loss", "boundary_loss") for s in sfx] + ["epoch_loss"]
    assert gs.keys == want == keys_e + ["epoch_loss"]
    assert len(gs.boundary) == len(tg) and all(b.data_ptr() != m.data_ptr() for b, m in zip(gs.boundary, maps))
    l3 = gs(x, tg).tolist()[-1]
    l4 = gs(x, tg).tolist()[-1]
    print(f"graphed {l3} {l4}, eager {losses_e[3]} {losses_e[4]}")
    assert abs(l3 - losses_e[3]) < 1e-5 and abs(l4 - losses_e[4]) < 1e-5
    for (n_, a), (_, b) in zip(net_e.state_dict().items(), net_g.state_dict().items()):
        assert torch.allclose(a.float(), b.float(), rtol=1e-4, atol=1e-6), n_
    # a new map in the static buffer: the replay follows it
    new = [-2.0 * maps[0]] + maps[1:]
    _, l5_e, outs = eager_step(net_e, opt_e, new)
    with torch.no_grad():
        old_heads = [seg_loss(o.detach(), t, spec, two, f) for o, t, f in zip(outs, tg, maps)]
        l5_old = sum(x_.item() for x_ in select_loss_terms(old_heads, spec)[1])
    gs.boundary[0].copy_(new[0])
    l5 = gs().tolist()[-1]
    print(f"new map: graphed {l5}, eager {l5_e}; with the old map {l5_old}")
    assert abs(l5_old - l5_e) > 1e-3 and abs(l5 - l5_e) < 1e-5


@pytest.mark.parametrize("two", [False, True])
def test_handlers_read_the_optional_keys(two):
    """The problem handlers with the new keys: the boundary map comes from the target they were given, the new terms are
    logged behind the reference's, and pt_loss is the sum of ``seg_loss``'s terms."""
    from ctunet_amd import LossSpec, ProblemHandler, boundary_map, seg_loss
    n = 2
    shape = (n, 2, 12, 12, 12)
    tg = [_blobs(n, 12, 141 + i).cuda() for i in range(2 if two else 1)]
    pr = [torch.rand(shape, generator=gen(151 + i)).cuda().requires_grad_(True) for i in range(len(tg))]
    sampling = (1.0, 0.5, 0.5)
    h = _Holder(ce_lambda=1.0, dice_lambda=0.5, ce_weight_0=0.3, ce_weight_1=0.7, focal_gamma=2.0, tversky_lambda=1.0,
                tversky_alpha=0.3, tversky_beta=0.7, boundary_lambda=0.1, boundary_sampling=sampling)
    spec = LossSpec(1.0, 0.5, class_weight=(0.3, 0.7), focal_gamma=2.0, tversky_lambda=1.0, tversky_alpha=0.3, tversky_beta=0.7,
                    boundary_lambda=0.1)
    if two:
        ProblemHandler.FlapRecWithShapePriorDoubleOut.comp_losses_metrics(h, pr, tg, 0, 1)
    else:
        ProblemHandler.ProblemHandler.comp_losses_metrics(h, pr[0], tg[0], 0, 1)
    sfx = ("_sk", "_fl") if two else ("",)
    assert list(h.losses_and_metrics) == [k + s for k in ("ce", "dice_loss", "tversky_loss", "boundary_loss") for s in sfx] + ["epoch_loss"]
    want, logged = [], []
    for i, s in enumerate(sfx):
        terms = seg_loss(pr[i].detach(), tg[i], spec, two, boundary_map(tg[i], sampling))
        want.append(sum(x.item() for x in terms))
        for k, x in zip(("ce", "dice_loss", "tversky_loss", "boundary_loss"), terms):
            assert h.losses_and_metrics[k + s] == [x.item()]
    assert abs(h.pt_loss.item() - sum(want)) <= 1e-6 * max(1.0, abs(sum(want)))
    h.pt_loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum().item() > 0 for p in pr)
