"""Plain float64 torch restatements of the streaming ops at the two ends of the training step: the 1x1x1 output head, the
fused Dice + cross-entropy loss and train-mode BatchNorm + ReLU.  No project code; gradients come from autograd on the
graphs built here (pass float64 leaves with requires_grad and call backward on what these return)."""
import torch
import torch.nn.functional as F


def head_ref(a, w, b, act, mode):
    """Tuple of head outputs for the ACTIVATED input a [N, Ci, D, H, W], weights w [Co, Ci] and bias b [Co].
    act bit 0: softmax over the channels, bit 1: sigmoid (after the softmax when both are set).
    mode 0: (y,); mode 1: the SP re-encoding (skull, flap) = ([y0, y1 + y2], [1 - y1, y1]); mode 2: softmax of each pair."""
    a, w, b = a.double(), w.double(), b.double()
    co, ci = w.shape
    y = F.conv3d(a, w.view(co, ci, 1, 1, 1), b)
    if act & 1:
        y = F.softmax(y, 1)
    if act & 2:
        y = torch.sigmoid(y)
    if mode == 0:
        return (y,)
    sk = torch.cat((y[:, 0:1], y[:, 1:2] + y[:, 2:3]), 1)
    fl = torch.cat((1 - y[:, 1:2], y[:, 1:2]), 1)
    if mode == 2:
        return F.softmax(sk, 1), F.softmax(fl, 1)
    return sk, fl


def loss_ref(pred, target, ce_lambda, dice_lambda, dice_softmax):
    """(ce_term, dice_term) of maps [N, C, ...], each already multiplied by its lambda.
    CE: the map as logits, class = argmax(target, 1) (the first maximum wins), mean over the N * V voxels.
    Dice: per item (sum p t + 1e-7) / (sum p^2 + sum t^2 + 1e-7) over all C * V entries, p = softmax(pred) when
    dice_softmax else pred; the term is lambda * (1 - 2 * mean over the items)."""
    pred, target = pred.double(), target.double()
    n = pred.shape[0]
    cls = torch.argmax(target, 1, keepdim=True)
    ce = (torch.logsumexp(pred, 1, keepdim=True) - torch.gather(pred, 1, cls)).mean()
    p = F.softmax(pred, 1) if dice_softmax else pred
    p, t = p.reshape(n, -1), target.reshape(n, -1)
    eps = 0.0000001
    ratio = ((p * t).sum(1) + eps) / ((p * p).sum(1) + (t * t).sum(1) + eps)
    return ce_lambda * ce, dice_lambda * (1 - 2 * ratio.mean())


def bn_relu_ref(y, gamma, beta, eps, ga=None):
    """relu(batch_norm(y)) with batch statistics in float64.  With the activated output's gradient ga also
    (a, dy, dgamma, dbeta) from autograd."""
    y, gamma, beta = (t.detach().double().requires_grad_(ga is not None) for t in (y, gamma, beta))
    a = F.relu(F.batch_norm(y, None, None, gamma, beta, True, 0.0, eps))
    if ga is None:
        return a
    a.backward(ga.double())
    return a.detach(), y.grad, gamma.grad, beta.grad


def bn_vectors(y, gamma, beta, eps, cp):
    """float32 [4, cp] rows (scale, shift, mean, invstd) of the lazy BatchNorm transform of y [N, C, ...], from float64
    two-pass batch statistics; rows are zero past the C real channels."""
    c = y.shape[1]
    dims = [0] + list(range(2, y.dim()))
    mean = y.double().mean(dim=dims)
    var = y.double().var(dim=dims, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    vec = torch.zeros(4, cp, dtype=torch.float64)
    vec[0, :c] = gamma.double() * invstd
    vec[1, :c] = beta.double() - mean * gamma.double() * invstd
    vec[2, :c] = mean
    vec[3, :c] = invstd
    return vec.float()
