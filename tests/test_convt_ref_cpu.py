"""The GEMM + scatter reference of tests/convt_ref.py against F.conv_transpose3d with autograd, both in float64 (no GPU).
Shapes: batch 2, odd D, H, W, unequal channel counts, with and without the input transform."""
import pytest
import torch
import torch.nn.functional as F

import convt_ref
from util import gen

CASES = [(1, 3, 5, 2, 3, 4, False), (2, 7, 6, 3, 5, 7, True), (2, 16, 9, 1, 3, 5, True)]     # n, ci, co, d, h, w, transform


@pytest.mark.parametrize("n,ci,co,d,h,w,xf", CASES)
def test_reference_matches_conv_transpose3d_autograd(n, ci, co, d, h, w, xf):
    g = gen(ci * 100 + co)
    x = torch.randn(n, ci, d, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(ci, co, 2, 2, 2, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(co, generator=g, dtype=torch.float64).requires_grad_(True)
    sc = sh = None
    if xf:
        sc = torch.rand(ci + 3, generator=g, dtype=torch.float64) * 1.5 - 0.25        # (vectors may be padded: only [:ci] is read)
        sh = torch.randn(ci + 3, generator=g, dtype=torch.float64) * 0.3
    a = convt_ref.activate(x, sc, sh, True)
    if xf:
        assert torch.equal(a, F.relu(x * sc[:ci].view(1, -1, 1, 1, 1) + sh[:ci].view(1, -1, 1, 1, 1)))
    else:
        assert torch.equal(a, x)
    a = a.clone().requires_grad_(True)
    ref = F.conv_transpose3d(a, wt, b, stride=2)
    go = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    ref.backward(go)
    tol = dict(rtol=1e-12, atol=1e-12)
    assert torch.allclose(convt_ref.forward(a.detach(), wt.detach(), b.detach()), ref.detach(), **tol)
    assert torch.allclose(convt_ref.forward(a.detach(), wt.detach()), F.conv_transpose3d(a.detach(), wt.detach(), None, stride=2), **tol)
    assert torch.allclose(convt_ref.data_gradient(go, wt.detach()), a.grad, **tol)
    dw, db = convt_ref.weight_gradient(a.detach(), go)
    assert torch.allclose(dw, wt.grad, **tol) and torch.allclose(db, b.grad, **tol)


def test_each_tap_lands_on_its_own_fine_voxel():
    """One unit weight at tap (i, j, l): the output is the input placed at (2d + i, 2h + j, 2w + l) and zero elsewhere."""
    x = torch.arange(1, 2 * 3 * 4 + 1, dtype=torch.float64).view(1, 1, 2, 3, 4)
    for i in range(2):
        for j in range(2):
            for l in range(2):
                wt = torch.zeros(1, 1, 2, 2, 2, dtype=torch.float64)
                wt[0, 0, i, j, l] = 1.0
                y = convt_ref.forward(x, wt)
                assert torch.equal(y[0, 0, i::2, j::2, l::2], x[0, 0])
                assert y.abs().sum() == x.abs().sum()


def test_store_rounds_the_transformed_value_once():
    x = torch.tensor([1.0, 3.0]).view(1, 2, 1, 1, 1)
    sc, sh = torch.tensor([1.0 + 2.0 ** -9, 1.0]), torch.tensor([0.0, -4.0])
    a = convt_ref.activate(x, sc, sh, True, store=torch.bfloat16)
    assert a.flatten().tolist() == [1.0, 0.0]            # 1 + 2^-9 rounds to 1 in bf16; relu(-1) = 0
