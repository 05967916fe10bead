"""Plain float64 torch restatement of the segmentation loss family (ctunet_amd/losses.py's module docstring).  No project
code; gradients come from autograd on the graph built here (pass a float64 leaf with requires_grad and call backward on what
this returns).

pred, target [N, 2, ...]; c = 1 where t1 > t0 else 0; p = softmax(pred); pr = p when dice_softmax else pred; q = pr[:, 1],
g = target[:, 1]; eps = 1e-7.
  ce        ce_lambda * sum w_c (1 - p_c)^gamma (-log p_c) / sum w_c   (1 - p_c: the other class's probability)
  dice      dice_lambda * (1 - 2 mean_n (sum pr t + eps) / (sum pr^2 + sum t^2 + eps))
  tversky   tversky_lambda * (1 - mean_n (TP + eps) / (TP + alpha FP + beta FN + eps)), TP = sum q g, FP = sum q - TP,
            FN = sum g - TP
  boundary  boundary_lambda * sum q phi / (N V), a non-finite phi counting as 0
A term whose lambda is 0 is a constant 0."""
import torch
import torch.nn.functional as F

EPS = 0.0000001


def seg_loss_ref(pred, target, dice_softmax, ce_lambda=0.0, dice_lambda=0.0, class_weight=(1.0, 1.0), focal_gamma=0.0,
                 tversky_lambda=0.0, tversky_alpha=0.5, tversky_beta=0.5, boundary_lambda=0.0, phi=None):
    """(ce, dice, tversky, boundary) float64 0-d tensors, each already multiplied by its lambda."""
    pred, target = pred.double(), target.double()
    n = pred.shape[0]
    zero = torch.zeros((), dtype=torch.float64)
    cls1 = target[:, 1] > target[:, 0]
    logp = F.log_softmax(pred, 1)
    p = F.softmax(pred, 1)
    nll = -torch.where(cls1, logp[:, 1], logp[:, 0])
    other = torch.where(cls1, p[:, 0], p[:, 1])
    w = torch.where(cls1, torch.full_like(nll, class_weight[1]), torch.full_like(nll, class_weight[0]))
    # gamma = 0: the factor is exactly 1 also where the other probability is 0 (and pow's gradient is not asked for)
    focal = other.pow(focal_gamma) if focal_gamma != 0 else torch.ones_like(other)
    ce = ce_lambda * (w * focal * nll).sum() / w.sum() if ce_lambda != 0 else zero
    pr = p if dice_softmax else pred
    pf, tf = pr.reshape(n, -1), target.reshape(n, -1)
    ratio = ((pf * tf).sum(1) + EPS) / ((pf * pf).sum(1) + (tf * tf).sum(1) + EPS)
    dice = dice_lambda * (1 - 2 * ratio.mean()) if dice_lambda != 0 else zero
    q, g = pr[:, 1].reshape(n, -1), target[:, 1].reshape(n, -1)
    tp = (q * g).sum(1)
    fp, fn = q.sum(1) - tp, g.sum(1) - tp
    tv = (tp + EPS) / (tp + tversky_alpha * fp + tversky_beta * fn + EPS)
    tversky = tversky_lambda * (1 - tv.mean()) if tversky_lambda != 0 else zero
    boundary = zero
    if boundary_lambda != 0:
        f = phi.double().reshape(n, -1)
        f = torch.where(torch.isfinite(f), f, torch.zeros_like(f))
        boundary = boundary_lambda * (q * f).sum() / q.numel()
    return ce, dice, tversky, boundary
