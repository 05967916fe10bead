"""Dice / cross-entropy loss of the ctunet path on the fused gfx950 loss kernels.

API mirrors of
  ``ctunet.utilities.dice_loss``                                   utilities.py:35-50
  ``ProblemHandler.comp_losses_metrics``                            ProblemHandler.py:44-102
  ``FlapRecWithShapePriorDoubleOut.comp_losses_metrics``            ProblemHandler.py:213-309
(the reference's "binary cross entropy" is nn.CrossEntropyLoss on the 2-channel map taken as
logits with target argmax(one_hot, 1), ProblemHandler.py:67-69,247-256).

One kernel pass computes CE and Dice of a 2-channel map, one more its gradient; the reference
makes ~10 elementwise/reduction passes and 5 host syncs per batch for the same numbers.

Loss family (``LossSpec`` / ``seg_loss``, kernels in csrc/loss_family.hip).  ``pred`` and ``target`` are [N,2,D,H,W]
float32, V = D*H*W.  c(v) is the target class of voxel v: 1 where ``t1 > t0``, else 0 (ties go to class 0, as above).
p = softmax(pred) over the two channels.  The probability view ``pr`` is the one the Dice term uses: ``pred`` itself for
one head, softmax(pred) for the double-output handler (``dice_softmax``).  q = ``pr[:,1]``, g = ``target[:,1]``,
eps = 1e-7 (the reference's).  Four terms, in this order:

  ce        ``ce_lambda * sum_v w_c (1 - p_c)^gamma (-log p_c) / sum_v w_c`` over all items and voxels, with
            ``class_weight = (w0, w1)``, w > 0, and ``focal_gamma = gamma >= 0``.  w = (1, 1), gamma = 0 is the CE above;
            gamma = 0 with weights is ``nn.CrossEntropyLoss(weight=w)``.  1 - p_c is the other class's probability (taken
            from there, not by subtraction); gamma = 0 gives a factor of exactly 1 also where that probability is 0.
  dice      unchanged: ``dice_lambda * (1 - 2 mean_n (sum pr t + eps) / (sum pr^2 + sum t^2 + eps))``.
  tversky   ``tversky_lambda * (1 - mean_n (TP + eps) / (TP + alpha FP + beta FN + eps))`` with, per item,
            TP = sum q g, FP = sum q - TP, FN = sum g - TP: the foreground channel only.  alpha = beta = 0.5 is
            ``2 TP / (sum q + sum g)``; beta > alpha prices false negatives above false positives.
  boundary  ``boundary_lambda * sum_{n,v} q phi / (N V)``; phi is a float32 [N,D,H,W] (or [N,1,D,H,W]) signed distance
            map of the target, positive outside the object and negative inside (``postprocess.signed_distance``'s
            convention, ``boundary_map`` below).  A non-finite phi counts as 0 in the sum and in the gradient, so an item
            with empty or full foreground (+-inf everywhere) contributes nothing.

A term whose lambda is 0 is 0.0 and contributes no gradient.
"""
from __future__ import annotations

import math
from numbers import Real
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import ops


class _FusedLoss(torch.autograd.Function):
    """(ce_lambda * CE, dice_lambda * Dice) of one [N,2,D,H,W] map as two 0-d tensors."""

    @staticmethod
    def forward(ctx, pred, target, ce_lambda, dice_lambda, dice_softmax):
        pred_c, target_c = pred.contiguous(), target.contiguous()
        terms, ws = ops.loss_fwd(pred_c, target_c, float(ce_lambda), float(dice_lambda), bool(dice_softmax))
        ctx.save_for_backward(pred_c, target_c, ws)
        ctx.cfg = (float(ce_lambda), float(dice_lambda), bool(dice_softmax))
        return terms[0], terms[1]

    @staticmethod
    def backward(ctx, g_ce, g_dice):
        pred, target, ws = ctx.saved_tensors
        ce, dc, sm = ctx.cfg
        # a term nobody differentiated contributes nothing (lambda 0); the other upstream scalars are read in place
        gp = ops.loss_bwd(pred, target, ce if g_ce is not None else 0.0, dc if g_dice is not None else 0.0, sm, ws,
                          None if g_ce is None else g_ce.float(), None if g_dice is None else g_dice.float())
        return gp, None, None, None, None


def _check_map(pred: torch.Tensor, target: torch.Tensor) -> None:
    if pred.dim() != 5 or pred.shape[1] != 2 or pred.shape != target.shape:
        raise RuntimeError("ctunet_amd: the fused loss handles [N,2,D,H,W] prediction / one-hot target pairs "
                           f"(got {tuple(pred.shape)} / {tuple(target.shape)})")


def fused_ce_dice(pred, target, ce_lambda, dice_lambda, dice_softmax) -> Tuple[torch.Tensor, torch.Tensor]:
    _check_map(pred, target)
    return _FusedLoss.apply(pred, target, ce_lambda, dice_lambda, dice_softmax)


def _real(value, what: str, lo: Optional[float] = None, strict: bool = False) -> float:
    if isinstance(value, bool) or not isinstance(value, Real) or not math.isfinite(value):
        raise ValueError(f"LossSpec: {what} must be a finite real number, got {value!r}")
    if lo is not None and (value <= lo if strict else value < lo):
        raise ValueError(f"LossSpec: {what} must be {'>' if strict else '>='} {lo:g}, got {value!r}")
    return float(value)


class LossSpec:
    """What ``seg_loss`` and ``GraphedTrainStep(loss=)`` compute: the lambdas of the four terms and the parameters of the
    module docstring's definition.  ``class_weight=None`` is (1, 1).  Arguments are checked here, on the host."""

    def __init__(self, ce_lambda, dice_lambda, class_weight=None, focal_gamma=0.0, tversky_lambda=0.0, tversky_alpha=0.5,
                 tversky_beta=0.5, boundary_lambda=0.0):
        self.ce_lambda = _real(ce_lambda, "ce_lambda")
        self.dice_lambda = _real(dice_lambda, "dice_lambda")
        if class_weight is None:
            class_weight = (1.0, 1.0)
        if isinstance(class_weight, (str, bytes)) or not isinstance(class_weight, Sequence) or len(class_weight) != 2:
            raise ValueError(f"LossSpec: class_weight must be a pair (w0, w1), got {class_weight!r}")
        self.class_weight = tuple(_real(w, f"class_weight[{i}]", 0.0, strict=True) for i, w in enumerate(class_weight))
        self.focal_gamma = _real(focal_gamma, "focal_gamma", 0.0)
        self.tversky_lambda = _real(tversky_lambda, "tversky_lambda")
        self.tversky_alpha = _real(tversky_alpha, "tversky_alpha", 0.0)
        self.tversky_beta = _real(tversky_beta, "tversky_beta", 0.0)
        self.boundary_lambda = _real(boundary_lambda, "boundary_lambda")

    @property
    def lambdas(self) -> Tuple[float, float, float, float]:
        return self.ce_lambda, self.dice_lambda, self.tversky_lambda, self.boundary_lambda

    @property
    def extended(self) -> bool:
        """False: the plain CE + Dice pair, which runs on the ``ctu_loss_fwd`` / ``ctu_loss_bwd`` kernels as before."""
        return (self.class_weight != (1.0, 1.0) or self.focal_gamma != 0.0 or self.tversky_lambda != 0.0
                or self.boundary_lambda != 0.0)

    @property
    def kernel_args(self) -> Dict[str, object]:
        """Keyword arguments of ``ops.seg_loss_fwd`` / ``ops.seg_loss_bwd`` behind the lambdas."""
        return dict(class_weight=self.class_weight, focal_gamma=self.focal_gamma,
                    tversky_ab=(self.tversky_alpha, self.tversky_beta))

    def __repr__(self) -> str:
        return ("LossSpec(ce_lambda={}, dice_lambda={}, class_weight={}, focal_gamma={}, tversky_lambda={}, tversky_alpha={}, "
                "tversky_beta={}, boundary_lambda={})").format(self.ce_lambda, self.dice_lambda, self.class_weight,
                                                               self.focal_gamma, self.tversky_lambda, self.tversky_alpha,
                                                               self.tversky_beta, self.boundary_lambda)


class _SegLoss(torch.autograd.Function):
    """The four terms of an extended ``LossSpec`` on one [N,2,D,H,W] map as 0-d tensors."""

    @staticmethod
    def forward(ctx, pred, target, boundary, spec, dice_softmax):
        pred_c, target_c = pred.contiguous(), target.contiguous()
        terms, ws = ops.seg_loss_fwd(pred_c, target_c, spec.lambdas, bool(dice_softmax), boundary=boundary, **spec.kernel_args)
        ctx.save_for_backward(pred_c, target_c, ws)
        ctx.boundary = boundary                 # (no gradient flows into the map)
        ctx.cfg = (spec, bool(dice_softmax))
        return terms[0], terms[1], terms[2], terms[3]

    @staticmethod
    def backward(ctx, *gs):
        pred, target, ws = ctx.saved_tensors
        spec, sm = ctx.cfg
        # a term nobody differentiated contributes nothing (lambda 0); the other upstream scalars are read in place
        lam = tuple(l if g_ is not None else 0.0 for l, g_ in zip(spec.lambdas, gs))
        gp = ops.seg_loss_bwd(pred, target, lam, sm, ws, tuple(None if g_ is None else g_.float() for g_ in gs),
                              boundary=ctx.boundary, **spec.kernel_args)
        return gp, None, None, None, None


_ZEROS: Dict[torch.device, torch.Tensor] = {}


def seg_loss(pred, target, spec: LossSpec, dice_softmax, boundary: Optional[torch.Tensor] = None):
    """(ce, dice, tversky, boundary) terms of ``spec`` on one [N,2,D,H,W] map, each times its lambda (module docstring).
    A spec without extensions runs ``fused_ce_dice``: the CE + Dice kernels with the arguments they always had."""
    _check_map(pred, target)
    if not spec.extended:
        zero = _ZEROS.get(pred.device)          # (one constant per device: no fill launch per call)
        if zero is None:
            zero = _ZEROS[pred.device] = torch.zeros((), dtype=torch.float32, device=pred.device)
        return fused_ce_dice(pred, target, spec.ce_lambda, spec.dice_lambda, dice_softmax) + (zero, zero)
    if spec.boundary_lambda != 0.0 and boundary is None:
        raise ValueError("seg_loss: boundary_lambda != 0 needs the boundary map (losses.boundary_map(target))")
    return _SegLoss.apply(pred, target, boundary if spec.boundary_lambda != 0.0 else None, spec, dice_softmax)


def boundary_map(target_onehot: torch.Tensor, sampling=None) -> torch.Tensor:
    """float32 [N,D,H,W] signed distance map of the class-1 voxels of a one-hot target [N,2,D,H,W], on the device
    (``postprocess.signed_distance``: positive outside the object, negative inside, in the units of ``sampling``)."""
    from . import postprocess
    if target_onehot.dim() != 5 or target_onehot.shape[1] != 2:
        raise ValueError(f"boundary_map: the target must be one-hot [N,2,D,H,W], got {tuple(target_onehot.shape)}")
    return postprocess.signed_distance(target_onehot[:, 1] > target_onehot[:, 0], sampling=sampling)


class dice_loss(nn.Module):
    """Soft Dice loss, same call signature as ``ctunet.utilities.dice_loss`` (2-channel maps)."""

    def forward(self, output, masks):
        return fused_ce_dice(output, masks, 0.0, 1.0, False)[1]


def _total(terms: Sequence[torch.Tensor], like: torch.Tensor = None) -> torch.Tensor:
    """terms[0] + terms[1] + ... (the builtin sum() starts from int 0: one more elementwise launch per step).
    No term at all (both lambdas 0): the reference's ``sum([])`` is the int 0 (ProblemHandler.py:91) -- a zero scalar
    here, so that ``float(model.pt_loss)`` and the epoch_loss log behave the same."""
    if not terms:
        return torch.zeros((), dtype=torch.float32, device=None if like is None else like.device)
    total = terms[0]
    for t in terms[1:]:
        total = total + t
    return total


def select_terms(heads: Sequence[Tuple[torch.Tensor, torch.Tensor]], ce_on: bool,
                 dice_on: bool) -> Tuple[List[str], List[torch.Tensor]]:
    """Log keys and loss terms of one head [(ce, dice)] or two [(skull), (flap)] in the reference's list order: the CE
    terms, then the Dice terms, suffixed _sk / _fl for two heads (ProblemHandler.py:88-91, 252-273)."""
    sfx = ("_sk", "_fl") if len(heads) == 2 else ("",)
    keys, terms = [], []
    for on, name, i in ((ce_on, "ce", 0), (dice_on, "dice_loss", 1)):
        if on:
            keys += [name + s for s in sfx]
            terms += [h[i] for h in heads]
    return keys, terms


def select_loss_terms(heads: Sequence[Sequence[torch.Tensor]], spec: LossSpec, ce_on: Optional[bool] = None,
                      dice_on: Optional[bool] = None) -> Tuple[List[str], List[torch.Tensor]]:
    """Log keys and loss terms of one or two heads of ``seg_loss`` 4-tuples: ``select_terms``'s keys in its order, then
    ``tversky_loss`` and ``boundary_loss`` (suffixed _sk / _fl for two heads) where their lambda is not 0.
    ``ce_on`` / ``dice_on``: the handlers' own ``params[...] != 0`` (None: the spec's lambda is not 0)."""
    keys, terms = select_terms([(h[0], h[1]) for h in heads], spec.ce_lambda != 0 if ce_on is None else ce_on,
                               spec.dice_lambda != 0 if dice_on is None else dice_on)
    sfx = ("_sk", "_fl") if len(heads) == 2 else ("",)
    for on, name, i in ((spec.tversky_lambda != 0, "tversky_loss", 2), (spec.boundary_lambda != 0, "boundary_loss", 3)):
        if on:
            keys += [name + s for s in sfx]
            terms += [h[i] for h in heads]
    return keys, terms


def spec_from_params(params) -> LossSpec:
    """The handlers' ``LossSpec``: ``ce_lambda`` / ``dice_lambda`` as always (None is 0), plus the optional keys
    ``ce_weight_0``, ``ce_weight_1``, ``focal_gamma``, ``tversky_lambda``, ``tversky_alpha``, ``tversky_beta`` and
    ``boundary_lambda``; an absent (or None) key is its default, which leaves the plain CE + Dice pair."""
    def opt(key, default):
        v = params.get(key)
        return default if v is None else v
    return LossSpec(params["ce_lambda"] or 0.0, params["dice_lambda"] or 0.0,
                    (opt("ce_weight_0", 1.0), opt("ce_weight_1", 1.0)), opt("focal_gamma", 0.0), opt("tversky_lambda", 0.0),
                    opt("tversky_alpha", 0.5), opt("tversky_beta", 0.5), opt("boundary_lambda", 0.0))


def _head_losses(params, spec: LossSpec, pairs, dice_softmax: bool):
    """``seg_loss`` of every (prediction, target) pair; the boundary maps come from the targets (``boundary_sampling``)."""
    heads = []
    sampling = params.get("boundary_sampling")
    if spec.boundary_lambda != 0 and isinstance(sampling, str):      # an ini string: "0.8, 0.45, 0.45" (or one number)
        try:
            values = [float(v) for v in sampling.replace("(", " ").replace(")", " ").replace(",", " ").split()]
        except ValueError:
            values = []
        if len(values) not in (1, 3):
            raise ValueError(f"ctunet_amd: boundary_sampling must be one number or three (z, y, x), got {sampling!r}")
        sampling = values[0] if len(values) == 1 else tuple(values)
    for p, t in pairs:
        phi = boundary_map(t, sampling) if spec.boundary_lambda != 0 else None
        heads.append(seg_loss(p, t, spec, dice_softmax, phi))
    return heads


def _append(lm: Dict[str, List], key: str, value) -> None:
    lm.setdefault(key, []).append(value)


def _publish(model, keys: Sequence[str], tensors: Sequence[torch.Tensor], idx, n_imgs, verbose=True) -> None:
    """One device->host copy for all logged scalars (the reference syncs once per float())."""
    total = model.pt_loss
    vals = torch.stack([t.detach() for t in tensors] + [total.detach()]).tolist()
    lm = model.losses_and_metrics
    for k_, v in zip(keys, vals[:-1]):
        _append(lm, k_, v)
    _append(lm, "epoch_loss", vals[-1])
    if verbose:
        print("    Batch {}/{} ({:.0f}%)\tLoss: {:.6f}".format(idx + 1, n_imgs, 100.0 * (idx + 1) / n_imgs, vals[-1]))


def comp_losses_metrics_single(model, prediction, target, idx, n_imgs):
    """``ProblemHandler.comp_losses_metrics`` (ProblemHandler.py:44-102): CE + Dice on the raw map."""
    ce_l, dc_l = model.params["ce_lambda"], model.params["dice_lambda"]
    if target.dim() != 5:
        # integer class labels [N,D,H,W] are used as they are by the cross entropy (ProblemHandler.py:67-68); the Dice
        # term of the reference cannot take them (dice_loss multiplies [N,2V] by [N,V], utilities.py:45-47: RuntimeError)
        if dc_l != 0:
            raise RuntimeError("ctunet_amd: dice_loss needs a one-hot target of the prediction's shape "
                               f"(got {tuple(target.shape)} for {tuple(prediction.shape)}), as in the reference")
        if target.dim() != 4 or target.shape != prediction.shape[:1] + prediction.shape[2:]:
            raise RuntimeError(f"ctunet_amd: class-index target {tuple(target.shape)} does not match {tuple(prediction.shape)}")
        from . import ops
        target = ops.one_hot(target.float().contiguous(), prediction.shape[1])
    spec = spec_from_params(model.params)
    heads = _head_losses(model.params, spec, [(prediction, target)], False)
    keys, terms = select_loss_terms(heads, spec, ce_l != 0, dc_l != 0)
    model.pt_loss = _total(terms, prediction)
    _metrics(model, [("dice_coef", prediction, target)])
    _publish(model, keys, terms, idx, n_imgs, getattr(model, "verbose", True))


def comp_losses_metrics_double(model, prediction, target, idx, n_imgs):
    """``FlapRecWithShapePriorDoubleOut.comp_losses_metrics`` (ProblemHandler.py:213-309): CE on the
    raw maps, Dice on their softmax, list order ce_sk, ce_fl, dice_loss_sk, dice_loss_fl."""
    sk_p, fl_p = prediction
    sk_t, fl_t = target
    ce_l, dc_l = model.params["ce_lambda"], model.params["dice_lambda"]
    spec = spec_from_params(model.params)
    heads = _head_losses(model.params, spec, ((sk_p, sk_t), (fl_p, fl_t)), True)
    keys, terms = select_loss_terms(heads, spec, ce_l != 0, dc_l != 0)
    model.pt_loss = _total(terms, sk_p)
    _metrics(model, [("dice_coef_sk", sk_p, sk_t), ("dice_coef_fl", fl_p, fl_t)], hd=True)
    _publish(model, keys, terms, idx, n_imgs, getattr(model, "verbose", True))


def _metrics(model, items, hd: bool = False) -> None:
    if model.params.get("save_dice_plots") is True:
        from .utilities import dice_coeff
        for key, p, t in items:
            _append(model.losses_and_metrics, key, dice_coeff(p, t))
    # Hausdorff: only the double-output handler logs it (ProblemHandler.py:287-295: keys hd_coef_sk / hd_coef_fl)
    if hd and model.params.get("save_hd_plots") is True:
        from .utilities import hausdorff
        for key, p, t in items:
            hk = key.replace("dice_coef", "hd_coef")
            _append(model.losses_and_metrics, hk, hausdorff(p, t))
