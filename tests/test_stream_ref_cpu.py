"""The float64 references of tests/stream_ref.py against the graphs the per-op tests already trust: the oracle's loss
terms, the inline head graph of test_ops_gpu.test_head_fwd_bwd and torch's own float32 batch norm.  Keeps the references of
test_stream_kernels_gpu.py from being the thing that is wrong.  The float32 side carries the rounding: gates are 1e-5 of
each tensor's scale (values) and 1e-4 (gradients through sums over a few hundred voxels)."""
import pytest
import torch
import torch.nn.functional as F

import stream_ref as R
from oracle import unet_oracle as O
from util import gen, rel_err


@pytest.mark.parametrize("ce,dice,sm", [(1.0, 1.0, False), (1.0, 1.0, True), (0.0, 1.0, True), (1.0, 0.0, False), (0.5, 2.0, True)])
def test_loss_ref_matches_the_oracle_terms(ce, dice, sm):
    p = torch.rand(2, 2, 6, 8, 10, generator=gen(1)).requires_grad_(True)
    m = (torch.rand(2, 6, 8, 10, generator=gen(2)) < 0.3).long()
    t = F.one_hot(m, 2).movedim(4, 1).float().contiguous()
    o_ce, o_dice = ce * O.cross_entropy(p, t), dice * O.dice_loss(F.softmax(p, 1) if sm else p, t)
    (o_ce + o_dice).backward()
    p64 = p.detach().double().requires_grad_(True)
    r_ce, r_dice = R.loss_ref(p64, t, ce, dice, sm)
    assert r_ce.dtype == torch.float64 and r_dice.dtype == torch.float64
    (r_ce + r_dice).backward()
    assert abs(r_ce.item() - o_ce.item()) < 1e-5 * max(1.0, abs(o_ce.item()))
    assert abs(r_dice.item() - o_dice.item()) < 1e-5 * max(1.0, abs(o_dice.item()))
    assert rel_err(p.grad, p64.grad) < 1e-4


def test_loss_ref_class_of_a_tie_is_the_first():
    """Soft targets: the class is argmax(target, 1) and an exact tie goes to class 0."""
    p = torch.tensor([[[1.0, -2.0, 0.5]], [[3.0, 0.25, 0.5]]]).permute(1, 0, 2).contiguous()      # [1, 2, 3]
    t = torch.tensor([[[0.4, 0.2, 0.7]], [[0.4, 0.9, 0.1]]]).permute(1, 0, 2).contiguous()        # tie, class 1, class 0
    ce, _ = R.loss_ref(p, t, 1.0, 0.0, False)
    lse = torch.logsumexp(p.double(), 1)[0]
    want = ((lse[0] - 1.0) + (lse[1] - 0.25) + (lse[2] - 0.5)) / 3
    assert abs(ce.item() - want.item()) < 1e-12


@pytest.mark.parametrize("co,act,mode", [(2, 2, 0), (2, 1, 0), (3, 2, 1), (3, 2, 2), (3, 3, 0), (1, 0, 0)])
def test_head_ref_matches_the_inline_graph(co, act, mode):
    n, d, h, w = 2, 4, 6, 10
    a = F.relu(torch.randn(n, 14, d, h, w, generator=gen(1)) * 1.2 + 0.3)
    wt = torch.randn(co, 14, generator=gen(5)) * 0.4
    b = torch.randn(co, generator=gen(6))
    # the graph test_head_fwd_bwd builds, in float32
    a32, w32, b32 = (t.clone().requires_grad_(True) for t in (a, wt, b))
    lc = F.conv3d(a32, w32.view(co, 14, 1, 1, 1), b32)
    y = F.softmax(lc, 1) if act & 1 else lc
    y = torch.sigmoid(y) if act & 2 else y
    if mode == 0:
        outs = (y,)
    else:
        sk = torch.cat((y[:, 0:1], y[:, 1:2] + y[:, 2:3]), 1); fl = torch.cat((1 - y[:, 1:2], y[:, 1:2]), 1)
        outs = (F.softmax(sk, 1), F.softmax(fl, 1)) if mode == 2 else (sk, fl)
    gs = [torch.randn(r.shape, generator=gen(7 + i)) for i, r in enumerate(outs)]
    torch.autograd.backward(outs, gs)
    a64, w64, b64 = (t.double().requires_grad_(True) for t in (a, wt, b))
    refs = R.head_ref(a64, w64, b64, act, mode)
    assert len(refs) == len(outs) and all(r.dtype == torch.float64 for r in refs)
    torch.autograd.backward(refs, [g_.double() for g_ in gs])
    for o, r in zip(outs, refs):
        assert o.shape == r.shape and rel_err(o, r) < 1e-5
    assert rel_err(a32.grad, a64.grad) < 1e-4
    assert rel_err(w32.grad, w64.grad) < 1e-4
    assert rel_err(b32.grad, b64.grad) < 1e-4


@pytest.mark.parametrize("shape", [(2, 8, 8, 8, 8), (1, 7, 4, 6, 10), (1, 22, 2, 3, 5)])
def test_bn_relu_ref_matches_float32_batch_norm(shape):
    c = shape[1]
    y = torch.randn(shape, generator=gen(1)) * 1.7 + 0.4
    gamma = torch.rand(c, generator=gen(2)) * 1.5 - 0.25
    beta = torch.randn(c, generator=gen(3)) * 0.2
    ga = torch.randn(shape, generator=gen(6))
    yr, gr, br = (t.clone().requires_grad_(True) for t in (y, gamma, beta))
    a32 = F.relu(F.batch_norm(yr, None, None, gr, br, True, 0.1, 1e-5))
    a32.backward(ga)
    a, dy, dgamma, dbeta = R.bn_relu_ref(y, gamma, beta, 1e-5, ga)
    assert torch.equal(R.bn_relu_ref(y, gamma, beta, 1e-5), a)
    assert rel_err(a32, a) < 1e-5
    assert rel_err(yr.grad, dy) < 1e-4 and rel_err(gr.grad, dgamma) < 1e-4 and rel_err(br.grad, dbeta) < 1e-4
    # the lazy transform's vectors reproduce the activation
    vec = R.bn_vectors(y, gamma, beta, 1e-5, 24)
    v = lambda r: r[:c].view(1, -1, 1, 1, 1)
    assert rel_err(F.relu(y * v(vec[0]) + v(vec[1])), a) < 1e-5
    assert torch.all(vec[:, c:] == 0)
    assert rel_err((y - v(vec[2])) * v(vec[3]) * v(gamma) + v(beta), F.batch_norm(y, None, None, gamma, beta, True, 0.1, 1e-5)) < 1e-5
