"""The segmentation loss family without a GPU: the float64 reference of loss_family_ref.py pinned on torch's own
cross-entropy, on the plain CE + Dice reference of stream_ref.py and on the closed forms of its special cases; LossSpec's
validation; the handlers' log keys; the routing of a spec without extensions onto the old kernels; the C-ABI entry points
in the header, the ctypes table and the built library, and the arguments they refuse before anything is launched."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import loss_family_ref as LR
import stream_ref as R
from util import gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 2, 3, 5, 7)


def _pred_target(seed=1, shape=SHAPE):
    p = torch.randn(shape, generator=gen(seed), dtype=torch.float64) * 2.0
    m = (torch.rand((shape[0],) + tuple(shape[2:]), generator=gen(seed + 1)) < 0.3).long()
    return p, F.one_hot(m, 2).movedim(4, 1).double().contiguous()


# ------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("w", [(1.0, 1.0), (0.2, 0.8), (3.0, 0.5)])
def test_reference_is_torch_weighted_cross_entropy_at_gamma_zero(w):
    p, t = _pred_target()
    ce = LR.seg_loss_ref(p, t, False, ce_lambda=0.7, class_weight=w)[0]
    want = 0.7 * F.cross_entropy(p, t.argmax(1), weight=torch.tensor(w, dtype=torch.float64))
    assert abs(ce.item() - want.item()) < 1e-12


@pytest.mark.parametrize("sm", [False, True])
def test_reference_is_the_plain_loss_for_the_default_spec(sm):
    p, t = _pred_target(3)
    t[:, 1, 1, 2, :] = t[:, 0, 1, 2, :] = 0.5                       # ties: class 0 in both
    ce, dice, tv, bd = LR.seg_loss_ref(p, t, sm, ce_lambda=0.5, dice_lambda=2.0)
    ce0, dice0 = R.loss_ref(p, t, 0.5, 2.0, sm)
    assert abs(ce.item() - ce0.item()) < 1e-12 and abs(dice.item() - dice0.item()) < 1e-12
    assert tv.item() == 0.0 and bd.item() == 0.0


@pytest.mark.parametrize("sm", [False, True])
def test_reference_tversky_at_one_half_is_the_plain_overlap_ratio(sm):
    p, t = _pred_target(5)
    tv = LR.seg_loss_ref(p, t, sm, tversky_lambda=1.0)[2]
    q = (F.softmax(p, 1) if sm else p)[:, 1].reshape(2, -1)
    g = t[:, 1].reshape(2, -1)
    tp = (q * g).sum(1)
    want = 1 - ((2 * tp + 2e-7) / (q.sum(1) + g.sum(1) + 2e-7)).mean()      # (TP + eps) / ((sum q + sum g) / 2 + eps)
    assert abs(tv.item() - want.item()) < 1e-12
    # beta > alpha prices a missed foreground voxel above a false alarm
    fg, bg = t[:, 1] > 0.5, t[:, 1] < 0.5
    both = torch.zeros_like(p)
    both[:, 1], both[:, 0] = torch.where(fg, 9.0, -9.0).double(), torch.where(fg, -9.0, 9.0).double()
    miss, alarm = both.clone(), both.clone()
    i = fg.nonzero()[0]
    j = bg.nonzero()[0]
    miss[i[0], :, i[1], i[2], i[3]] = torch.tensor([9.0, -9.0], dtype=torch.float64)
    alarm[j[0], :, j[1], j[2], j[3]] = torch.tensor([-9.0, 9.0], dtype=torch.float64)
    f = lambda x: LR.seg_loss_ref(x, t, True, tversky_lambda=1.0, tversky_alpha=0.3, tversky_beta=0.7)[2].item()
    assert f(miss) > f(alarm) > f(both)


def test_reference_focal_factor():
    p, t = _pred_target(7)
    ce0 = LR.seg_loss_ref(p, t, False, ce_lambda=1.0)[0]
    ce2 = LR.seg_loss_ref(p, t, False, ce_lambda=1.0, focal_gamma=2.0)[0]
    assert 0 < ce2.item() < ce0.item()
    # by hand: (1 - p_c)^2 (-log p_c), mean
    logp = F.log_softmax(p, 1).gather(1, t.argmax(1, keepdim=True))
    assert abs(ce2.item() - ((1 - logp.exp()) ** 2 * -logp).mean().item()) < 1e-12
    # gamma = 0 gives a factor of exactly 1 where the other probability underflows to 0; 0 < gamma < 1 stays finite there
    big = torch.zeros(1, 2, 1, 1, 2, dtype=torch.float64)
    big[0, 0] = 2000.0
    tt = torch.zeros_like(big)
    tt[0, 0, 0, 0, 0] = 1.0
    tt[0, 1, 0, 0, 1] = 1.0                                            # one voxel right, one wrong by 2000
    assert LR.seg_loss_ref(big, tt, False, ce_lambda=1.0)[0].item() == 1000.0
    assert LR.seg_loss_ref(big, tt, False, ce_lambda=1.0, focal_gamma=0.5)[0].item() == 1000.0


def test_reference_ignores_non_finite_phi():
    p, t = _pred_target(9)
    phi = torch.randn(2, 3, 5, 7, generator=gen(10), dtype=torch.float64)
    bad = phi.clone()
    bad[1] = float("inf")
    bad[0, 0, 0, 0], bad[0, 1, 2, 3] = float("-inf"), float("nan")
    clean = torch.where(torch.isfinite(bad), bad, torch.zeros_like(bad))
    for sm in (False, True):
        pl = p.clone().requires_grad_(True)
        a = LR.seg_loss_ref(pl, t, sm, boundary_lambda=1.5, phi=bad)[3]
        a.backward()
        pc = p.clone().requires_grad_(True)
        b = LR.seg_loss_ref(pc, t, sm, boundary_lambda=1.5, phi=clean)[3]
        b.backward()
        assert torch.isfinite(a) and a.item() == b.item() and torch.equal(pl.grad, pc.grad)
        assert torch.all(pl.grad[1] == 0)                              # the all-inf item contributes nothing
        q = (F.softmax(p, 1) if sm else p)[:, 1]
        assert abs(a.item() - 1.5 * (q * clean).sum().item() / q.numel()) < 1e-12


def test_reference_zero_lambda_terms_are_zero_without_gradient():
    p, t = _pred_target(11)
    pl = p.clone().requires_grad_(True)
    terms = LR.seg_loss_ref(pl, t, True, dice_lambda=1.0)
    assert [x.item() == 0.0 for x in terms] == [True, False, True, True]
    assert not terms[0].requires_grad and not terms[2].requires_grad and not terms[3].requires_grad


# ------------------------------------------------------------------------------------------------- LossSpec
def test_loss_spec_defaults_and_extended():
    from ctunet_amd import LossSpec
    s = LossSpec(1.0, 0.5)
    assert s.lambdas == (1.0, 0.5, 0.0, 0.0) and s.class_weight == (1.0, 1.0) and not s.extended
    assert not LossSpec(1, 1, class_weight=(1, 1), tversky_alpha=0.3).extended     # parameters of absent terms do not count
    for kw in (dict(class_weight=(0.2, 0.8)), dict(focal_gamma=2.0), dict(tversky_lambda=1.0), dict(boundary_lambda=0.1)):
        assert LossSpec(1.0, 1.0, **kw).extended, kw
    assert LossSpec(1.0, 1.0, focal_gamma=2).kernel_args == dict(class_weight=(1.0, 1.0), focal_gamma=2.0, tversky_ab=(0.5, 0.5))


@pytest.mark.parametrize("kw,match", [
    (dict(class_weight=(0.0, 1.0)), r"class_weight\[0\] must be > 0"),
    (dict(class_weight=(1.0, -2.0)), r"class_weight\[1\] must be > 0"),
    (dict(class_weight=(1.0,)), "pair"),
    (dict(class_weight=0.5), "pair"),
    (dict(class_weight=(1.0, float("inf"))), "finite"),
    (dict(focal_gamma=-0.1), "focal_gamma must be >= 0"),
    (dict(focal_gamma=float("nan")), "finite"),
    (dict(tversky_alpha=-1.0), "tversky_alpha must be >= 0"),
    (dict(tversky_beta=-1e-3), "tversky_beta must be >= 0"),
    (dict(tversky_lambda="1"), "tversky_lambda must be a finite real"),
    (dict(boundary_lambda=None), "boundary_lambda must be a finite real"),
    (dict(ce_lambda=float("inf")), "ce_lambda must be a finite real"),
    (dict(dice_lambda=True), "dice_lambda must be a finite real"),
])
def test_loss_spec_validation(kw, match):
    from ctunet_amd import LossSpec
    args = dict(ce_lambda=1.0, dice_lambda=1.0)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        LossSpec(**args)


def test_seg_loss_refuses_a_boundary_term_without_a_map_and_bad_maps():
    from ctunet_amd import LossSpec, boundary_map, seg_loss
    p = torch.zeros(1, 2, 4, 4, 4)
    with pytest.raises(ValueError, match="needs the boundary map"):
        seg_loss(p, p, LossSpec(1.0, 0.0, boundary_lambda=0.5), False)
    with pytest.raises(RuntimeError, match=r"\[N,2,D,H,W\]"):
        seg_loss(torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 3, 4, 4, 4), LossSpec(1.0, 0.0, focal_gamma=1.0), False)
    with pytest.raises(ValueError, match="one-hot"):
        boundary_map(torch.zeros(1, 4, 4, 4))


def test_graphed_step_refuses_a_spec_without_loss_and_a_missing_map():
    import ctunet_amd
    from ctunet_amd import LossSpec, optim
    from ctunet_amd.graph import GraphedTrainStep
    net = ctunet_amd.UNet(n_blocks=2, i_size=2)
    args = (net, optim.Adam(net.parameters()), torch.zeros(1, 1, 8, 8, 8), [torch.zeros(1, 2, 8, 8, 8)])
    with pytest.raises(ValueError, match="every lambda of the LossSpec is 0"):
        GraphedTrainStep(*args, 1.0, 1.0, loss=LossSpec(0.0, 0.0, focal_gamma=2.0))
    with pytest.raises(ValueError, match="both 0"):                     # the lambda form keeps its own message
        GraphedTrainStep(*args, 0.0, 0.0)
    with pytest.raises(ValueError, match="example_boundary"):
        GraphedTrainStep(*args, 0.0, 0.0, loss=LossSpec(1.0, 0.0, boundary_lambda=1.0))


# ------------------------------------------------------------------------------------------------- log keys
def test_log_keys_keep_the_reference_order_and_append_the_new_terms():
    from ctunet_amd import LossSpec
    from ctunet_amd.losses import select_loss_terms, select_terms
    one = [("c", "d", "t", "b")]
    two = [("c0", "d0", "t0", "b0"), ("c1", "d1", "t1", "b1")]
    full = LossSpec(1.0, 1.0, tversky_lambda=1.0, boundary_lambda=1.0)
    assert select_loss_terms(one, full) == (["ce", "dice_loss", "tversky_loss", "boundary_loss"], ["c", "d", "t", "b"])
    assert select_loss_terms(two, full) == (
        ["ce_sk", "ce_fl", "dice_loss_sk", "dice_loss_fl", "tversky_loss_sk", "tversky_loss_fl", "boundary_loss_sk",
         "boundary_loss_fl"], ["c0", "c1", "d0", "d1", "t0", "t1", "b0", "b1"])
    assert select_loss_terms(two, LossSpec(0.0, 1.0, boundary_lambda=0.1)) == (
        ["dice_loss_sk", "dice_loss_fl", "boundary_loss_sk", "boundary_loss_fl"], ["d0", "d1", "b0", "b1"])
    assert select_loss_terms(one, LossSpec(1.0, 0.0, tversky_lambda=2.0))[0] == ["ce", "tversky_loss"]
    # without extensions: exactly select_terms
    for ce, dc in ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0)):
        assert select_loss_terms(two, LossSpec(ce, dc)) == select_terms([h[:2] for h in two], ce != 0, dc != 0)
    assert select_terms([("c", "d")], True, True) == (["ce", "dice_loss"], ["c", "d"])       # signature and behaviour kept


def test_spec_from_params_reads_the_optional_keys():
    from ctunet_amd.losses import spec_from_params
    s = spec_from_params(dict(ce_lambda=1.0, dice_lambda=None))
    assert s.lambdas == (1.0, 0.0, 0.0, 0.0) and not s.extended
    s = spec_from_params(dict(ce_lambda=1.0, dice_lambda=0.5, ce_weight_1=4.0, focal_gamma=2.0, tversky_lambda=0.3,
                              tversky_alpha=0.3, tversky_beta=0.7, boundary_lambda=0.01, boundary_sampling=(1, 1, 1)))
    assert s.class_weight == (1.0, 4.0) and s.focal_gamma == 2.0 and s.lambdas == (1.0, 0.5, 0.3, 0.01)
    assert (s.tversky_alpha, s.tversky_beta) == (0.3, 0.7) and s.extended
    with pytest.raises(ValueError, match="focal_gamma"):
        spec_from_params(dict(ce_lambda=1.0, dice_lambda=1.0, focal_gamma=-1.0))


# ------------------------------------------------------------------------------------------------- routing
class _Holder:
    verbose = False
    pt_loss = None

    def __init__(self, **params):
        self.params = dict(save_dice_plots=False, save_hd_plots=False, **params)
        self.losses_and_metrics = {}


def test_a_spec_without_extensions_reaches_the_old_kernels_with_the_old_arguments(monkeypatch):
    from ctunet_amd import LossSpec, losses, ops, seg_loss
    calls = []

    def loss_fwd(pred, target, ce, dice, sm):
        calls.append(("loss_fwd", ce, dice, sm))
        return torch.tensor([ce * 1.0, dice * 2.0]), torch.zeros(4)

    def seg_loss_fwd(*a, **k):
        calls.append(("seg_loss_fwd",) + tuple(a[2:4]) + (k,))
        return torch.tensor([1.0, 2.0, 3.0, 4.0]), torch.zeros(4)
    monkeypatch.setattr(ops, "loss_fwd", loss_fwd)
    monkeypatch.setattr(ops, "seg_loss_fwd", seg_loss_fwd)
    p, t = torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 2, 4, 4, 4)
    out = seg_loss(p, t, LossSpec(0.5, 2.0), True)
    assert calls == [("loss_fwd", 0.5, 2.0, True)]
    assert len(out) == 4 and [x.dim() for x in out] == [0] * 4 and [x.item() for x in out] == [0.5, 4.0, 0.0, 0.0]
    # the handlers without the new keys: the same calls as before, the reference's keys
    del calls[:]
    h = _Holder(ce_lambda=1.0, dice_lambda=1.0)
    losses.comp_losses_metrics_single(h, p, t, 0, 1)
    assert calls == [("loss_fwd", 1.0, 1.0, False)]
    assert list(h.losses_and_metrics) == ["ce", "dice_loss", "epoch_loss"]
    del calls[:]
    h = _Holder(ce_lambda=1.0, dice_lambda=0.0)
    losses.comp_losses_metrics_double(h, (p, p), (t, t), 0, 1)
    assert calls == [("loss_fwd", 1.0, 0.0, True)] * 2
    assert list(h.losses_and_metrics) == ["ce_sk", "ce_fl", "epoch_loss"]
    # an extended spec reaches the new kernels, with the spec's arguments, and the new keys are appended
    del calls[:]
    out = seg_loss(p, t, LossSpec(0.5, 2.0, class_weight=(0.2, 0.8), tversky_lambda=1.0), False)
    assert calls == [("seg_loss_fwd", (0.5, 2.0, 1.0, 0.0), False,
                      dict(boundary=None, class_weight=(0.2, 0.8), focal_gamma=0.0, tversky_ab=(0.5, 0.5)))]
    assert [x.item() for x in out] == [1.0, 2.0, 3.0, 4.0]
    del calls[:]
    h = _Holder(ce_lambda=1.0, dice_lambda=1.0, focal_gamma=2.0, tversky_lambda=0.5)
    losses.comp_losses_metrics_double(h, (p, p), (t, t), 0, 1)
    assert [c[0] for c in calls] == ["seg_loss_fwd"] * 2 and calls[0][2] is True
    assert list(h.losses_and_metrics) == ["ce_sk", "ce_fl", "dice_loss_sk", "dice_loss_fl", "tversky_loss_sk", "tversky_loss_fl",
                                          "epoch_loss"]
    assert h.losses_and_metrics["epoch_loss"] == [2 * (1.0 + 2.0 + 3.0)]


def test_handlers_hand_the_sampling_key_to_boundary_map(monkeypatch):
    """The map comes from the target the handler was given; an ini string of three numbers is parsed."""
    from ctunet_amd import losses, ops
    seen = []

    def boundary_map(target, sampling=None):
        seen.append((target, sampling))
        return torch.zeros(target.shape[:1] + target.shape[2:])
    monkeypatch.setattr(losses, "boundary_map", boundary_map)
    monkeypatch.setattr(ops, "seg_loss_fwd", lambda *a, **k: (torch.tensor([1.0, 2.0, 3.0, 4.0]), torch.zeros(4)))
    p, t0, t1 = torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 2, 4, 4, 4), torch.ones(1, 2, 4, 4, 4)
    for given, want in (("0.8, 0.45, 0.45", (0.8, 0.45, 0.45)), ("(1, 2, 3)", (1.0, 2.0, 3.0)), ("2.0", 2.0), (1.5, 1.5),
                        ((0.8, 0.45, 0.45), (0.8, 0.45, 0.45)), (None, None)):
        del seen[:]
        h = _Holder(ce_lambda=1.0, dice_lambda=1.0, boundary_lambda=0.5, boundary_sampling=given)
        losses.comp_losses_metrics_double(h, (p, p), (t0, t1), 0, 1)
        assert [s for _, s in seen] == [want, want] and seen[0][0] is t0 and seen[1][0] is t1
        assert list(h.losses_and_metrics) == ["ce_sk", "ce_fl", "dice_loss_sk", "dice_loss_fl", "boundary_loss_sk",
                                              "boundary_loss_fl", "epoch_loss"]
    for bad in ("0.8, 0.45", "a, b, c", ""):
        with pytest.raises(ValueError, match="boundary_sampling"):
            losses.comp_losses_metrics_single(_Holder(ce_lambda=1.0, dice_lambda=1.0, boundary_lambda=0.5, boundary_sampling=bad),
                                              p, t0, 0, 1)
    del seen[:]                                                        # no boundary term: no map is computed
    losses.comp_losses_metrics_single(_Holder(ce_lambda=1.0, dice_lambda=1.0, focal_gamma=1.0), p, t0, 0, 1)
    assert seen == []


# ------------------------------------------------------------------------------------------------- C ABI
ENTRIES = (("ctu_seg_loss_ws_floats", 2), ("ctu_seg_loss_fwd", 9), ("ctu_seg_loss_bwd", 14))


def test_entry_points_declared_bound_exported_and_exports():
    import ctunet_amd
    from ctunet_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctunet_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name)
    assert "ctu_seg_loss_cfg" in src
    fields = re.search(r"typedef struct ctu_seg_loss_cfg \{(.*?)\}", src, flags=re.S).group(1)
    declared = [n.strip() for part in fields.split(";") for n in re.sub(r"^\s*(float|int)\s", "", part.strip()).split(",")
                if n.strip()]
    assert declared == [f[0] for f in _lib.SegLossCfg._fields_]
    L = _lib.load()
    assert L.ctu_abi_version() == _lib.ABI_VERSION == 8              # additions: the version stays
    for n in (1, 3):
        # 1024 rows of 8 partial sums per item, then 4 tail floats per item and the weight sum
        assert L.ctu_seg_loss_ws_floats(n, 480) == L.ctu_seg_loss_ws_floats(n, 1 << 24) == n * 1024 * 8 + n * 4 + 1
    for fn in ("LossSpec", "seg_loss", "boundary_map"):
        assert fn in ctunet_amd.__all__ and callable(getattr(ctunet_amd, fn))
    assert callable(ops.seg_loss_fwd) and callable(ops.seg_loss_bwd)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from ctunet_amd import _lib
    L = _lib.load()
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)                   # never dereferenced: every call below is refused on its arguments

    def cfg(**kw):
        base = dict(ce_lambda=1.0, dice_lambda=1.0, tversky_lambda=0.0, boundary_lambda=0.0, w0=1.0, w1=1.0, focal_gamma=0.0,
                    tversky_alpha=0.5, tversky_beta=0.5, dice_softmax=0)
        base.update(kw)
        return _lib.SegLossCfg(**base)

    def fwd(pred=ptr, target=ptr, phi=None, n=1, v=8, c=None, terms=ptr, ws=ptr):
        return L.ctu_seg_loss_fwd(pred, target, phi, n, v, None if c is None else ctypes.byref(c), terms, ws, None)

    def bwd(pred=ptr, target=ptr, phi=None, n=1, v=8, c=None, ws=ptr, gpred=ptr):
        return L.ctu_seg_loss_bwd(pred, target, phi, n, v, None if c is None else ctypes.byref(c), ws, None, None, None, None,
                                  gpred, 0, None)
    ok = cfg()
    bad = [dict(n=0, c=ok), dict(n=-1, c=ok), dict(v=0, c=ok), dict(v=-5, c=ok), dict(pred=None, c=ok), dict(target=None, c=ok),
           dict(c=None), dict(c=cfg(w0=0.0)), dict(c=cfg(w1=-1.0)), dict(c=cfg(focal_gamma=-0.5)), dict(c=cfg(tversky_alpha=-0.1)),
           dict(c=cfg(tversky_beta=-0.1)), dict(c=cfg(w0=float("nan"))), dict(c=cfg(boundary_lambda=1.0), phi=None)]
    for kw in bad:
        assert fwd(**kw) != 0, kw
        assert L.ctu_last_error(), kw
        assert bwd(**kw) != 0, kw
    assert fwd(terms=None, c=ok) != 0 and fwd(ws=None, c=ok) != 0
    assert bwd(ws=None, c=ok) != 0 and bwd(gpred=None, c=ok) != 0
    assert b"class weights" in (fwd(c=cfg(w0=0.0)), L.ctu_last_error())[1]
