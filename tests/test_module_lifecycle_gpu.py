"""One network instance through the life a torch module leads in user code: weights written in every way torch offers,
several live graphs, gradient accumulation, frozen parameters, shapes / batch sizes / modes alternating, precision and device
moves, copies and pickles -- always on an instance whose engine caches (packed weight copies, fused up-convolution
composites) are already warm, which is where a stale or cross-talking cache would sit.

The reference of every assertion is oracle/unet_oracle.py on the model's state dict as it stands at that moment
(lifecycle_ref.OracleCache).  fp32: outputs 1e-4 of max |ref|, loss 1e-5, hard Dice 0.999, gradients and dx under the
small-patch fp64 rule of test_models_gpu.oracle_train_check (util.fp64_rule_misses).  bf16: the rule of
test_lowp_gpu.test_lowp_nets_against_the_fp32_oracle -- no further from the fp32 oracle than the oracle's own run under
torch.autocast.  Those gates would let a stale weight through only if the write were small, so every mutation is first shown
to move the oracle's outputs by >= 1e-2 of max |ref| (fp32: 100 x the gate; bf16: at least 4 x the gate in force, so an
output computed from the old weights cannot sit inside it)."""
import copy
import gc
from contextlib import contextmanager

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lifecycle_ref as R
from oracle import unet_oracle as O
from util import fp64_rule_misses, rel_err

pytestmark = pytest.mark.gpu

DT = {"fp32": None, "bf16": torch.bfloat16}
_ORA = {}


def _ora(kind):
    if kind not in _ORA:
        o = _ORA[kind] = R.OracleCache(kind)
        o.xg = {s: v.cuda() for s, v in o.x.items()}
        o.tg = {s: [t.cuda() for t in v] for s, v in o.t.items()}
    return _ORA[kind]


@contextmanager
def _fusion(on):
    """on=False: the decoder's ConvTranspose3d -> Conv3d pairs through the two separate kernels (and the pack cache instead
    of the composite cache), in fp32 and in 16-bit -- the switch of test_lowp_gpu.py's fuse=False cases."""
    from ctunet_amd import engine as E
    old = E.FUSE_UP, E.LP_FUSE_UP
    E.FUSE_UP = E.LP_FUSE_UP = on
    try:
        yield
    finally:
        E.FUSE_UP, E.LP_FUSE_UP = old


def _step(net, kind, shape, which="all", x_req=True):
    """Train-mode forward + backward at `shape`; returns (outputs, loss, dx | None).  Gradients accumulate into p.grad."""
    ora = _ora(kind)
    net.train()
    xi = ora.xg[shape].clone().requires_grad_(x_req)
    out = net(xi)
    loss = R.loss_of(kind, out, ora.tg[shape], which)
    loss.backward()
    outs = out if isinstance(out, tuple) else (out,)
    return [o.detach() for o in outs], loss.item(), xi.grad


def _warm(kind="plain", prec="fp32", chk=False, shapes=("A", "B")):
    """A model whose caches hold every layout the shapes reach: a train step and an eval forward at each."""
    net = R.make_net(kind, chk).cuda().set_precision(prec)
    for s in shapes:
        _step(net, kind, s)
        net.eval()
        with torch.no_grad():
            net(_ora(kind).xg[s])
    net.zero_grad(set_to_none=True)
    return net


def _dice(o, r):
    return float(O.hard_dice(o.float().cpu(), F.one_hot(O.argmax1(r), r.shape[1]).movedim(-1, 1).float()))


def _judge_outputs(outs, refs, prec, yard=None, what=""):
    for i, (o, r) in enumerate(zip(outs, refs)):
        assert o.dtype == torch.float32 and o.is_contiguous()
        if prec == "fp32":
            assert rel_err(o, r) < 1e-4, (what, i, rel_err(o, r))
            assert _dice(o, r) >= 0.999, (what, i)
        else:
            assert rel_err(o, r) <= 1.5 * rel_err(yard[i], r), (what, i, rel_err(o, r), rel_err(yard[i], r))
            assert _dice(o, r) >= _dice(yard[i], r) - 0.004, (what, i)


def check_eval(net, kind, shape, prec="fp32", what=""):
    ora = _ora(kind)
    sd = R.snapshot(net)
    net.eval()
    with torch.no_grad():
        out = net(ora.xg[shape])
    outs = out if isinstance(out, tuple) else (out,)
    yard = ora.eval_out(sd, shape, DT[prec]) if prec != "fp32" else None
    _judge_outputs(outs, ora.eval_out(sd, shape), prec, yard, f"{what} eval {shape}")
    assert all(torch.equal(a, b) for a, b in zip(R.snapshot(net).values(), sd.values()))      # eval moves no buffer


def _sum(dicts):
    out = {}
    for n_ in dicts[0]:
        vs = [d[n_] for d in dicts]
        out[n_] = None if vs[0] is None else sum(vs[1:], vs[0].clone())
    return out


def judge_grads(net, refs, frozen=(), what=""):
    """p.grad of every parameter against the SUM of the oracle steps `refs`, under the fp64 rule."""
    g32, g64 = _sum([r["g32"] for r in refs]), _sum([r["g64"] for r in refs])
    checks = []
    for n_, p in net.named_parameters():
        if n_.startswith(tuple(frozen)):
            assert p.grad is None, (what, n_)
            continue
        assert (p.grad is None) == (g64[n_] is None), (what, n_)       # (the dead centre block: None on both sides)
        if p.grad is not None:
            checks.append((n_, p.grad, g32[n_], g64[n_]))
    misses = fp64_rule_misses(checks, g64, False)
    assert not misses, (what, misses)


def judge_dx(dx, r, what=""):
    misses = fp64_rule_misses([("dx", dx, r["dx32"], r["dx64"])], {}, False)
    assert not misses, (what, misses)


def judge_buffers(net, post, prec="fp32", what=""):
    for n_, b in net.named_buffers():
        if n_.endswith("num_batches_tracked"):
            assert int(b) == int(post[n_]), (what, n_)
        elif prec == "fp32":
            assert np.allclose(b.cpu().numpy(), post[n_].numpy(), rtol=1e-4, atol=1e-5), (what, n_)


def check_train(net, kind, shape, prec="fp32", which="all", what="", chk=False):
    """One train step on the instance as it stands, everything against the oracle on its state dict before the step."""
    ora = _ora(kind)
    sd = R.snapshot(net)
    net.zero_grad(set_to_none=True)
    outs, loss, dx = _step(net, kind, shape, which)
    r = ora.train(sd, shape, which, autocast=DT[prec])
    what = f"{what} train {shape}"
    if prec == "fp32":
        _judge_outputs(outs, r["outs"], prec, None, what)
        assert abs(loss - r["loss"]) < 1e-5 and abs(loss - r["loss64"]) < 1e-5, (what, loss, r["loss"])
        judge_grads(net, [r], what=what)
        judge_dx(dx, r, what)
    else:
        from test_lowp_gpu import _metrics
        ac_outs, ac_loss, ac_g, ac_dx = r["ac"]
        _judge_outputs(outs, r["outs"], prec, ac_outs, what)
        y = _metrics(ac_outs, r["outs"], ac_loss, r["loss"], ac_g, r["g32"], ac_dx, r["dx32"])
        g = _metrics(outs, r["outs"], loss, r["loss"], {n_: p.grad for n_, p in net.named_parameters()}, r["g32"], dx, r["dx32"])
        assert g["loss_err"] <= max(3 * y["loss_err"], 2e-4), (what, g, y)
        assert g["grad_cos_min"] >= y["grad_cos_min"] - 0.05 and g["dx_cos"] >= y["dx_cos"] - 0.05, (what, g, y)
        assert g["grad_l2_max"] <= 1.3 * y["grad_l2_max"] + 0.05, (what, g, y)
    judge_buffers(net, r["post2"] if chk else r["post"], prec, what)
    net.zero_grad(set_to_none=True)
    return r


def assert_separated(kind, old, new, prec="fp32", train=True, shapes=("A", "B")):
    """The write must be large against the gate in force, or a stale cache would pass."""
    ora = _ora(kind)
    for s in shapes:
        e, t = ora.separation(old, new, s)
        need = R.SEPARATION
        if prec != "fp32":
            refs = ora.eval_out(new, s)
            need = max(need, 4 * 1.5 * max(rel_err(y, r) for y, r in zip(ora.eval_out(new, s, DT[prec]), refs)))
        assert e >= need and (t >= need or not train), (s, e, t, need)


def _keys(net):
    return {n_: (p._version, p.data_ptr()) for n_, p in net.named_parameters() if n_ in R.TARGETS}


def _mutate(net, name, k):
    """Apply pathway `name`; call invalidate_packed_weights() exactly when neither key of the caches moved."""
    fn, _, _, invisible = R.PATHWAYS[name]
    before = _keys(net)
    try:
        fn(net, k)
    except RuntimeError as e:
        if not name.endswith("_fused"):
            raise
        pytest.skip(f"torch.optim {name} is not available on this device: {e}")
    after = _keys(net)
    unseen = all(after[n_] == before[n_] for n_ in before)
    assert unseen == invisible, (name, before, after)
    if unseen:
        net.invalidate_packed_weights()           # in-place writes through .data need it


# ================================================================================================ 1. weight mutations
@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(R.PATHWAYS) + ["batchnorm_data"])
def test_weight_mutation_pathway(name, prec, fuse):
    """Warm instance, weights written through one pathway, then an eval forward and a train step at the fused shape and an
    eval forward at the unfused one: all on the NEW weights.  The .data in-place pathways make the documented call."""
    from ctunet_amd import ops
    with _fusion(fuse):
        net = _warm("plain", prec)
        eng = net.__dict__["_eng"]
        n, d, h, w = R.SHAPES["A"]
        sup = ops.upconv_fused_supported if prec == "fp32" else ops.lp_upconv_fused_supported
        assert sup((n, d // 2, h // 2, w // 2), 3, 32, 8)
        assert bool(eng._up_cache) == fuse                       # the composite cache is the one in use (or is not)
        assert any(k_[1] == "convt" for k_ in eng._pack_cache)    # the unfused ConvTranspose3d copies (bottom level; shape B)
        old = R.snapshot(net)
        if name == "batchnorm_data":
            R.m_batchnorm_data(net, 3)
        else:
            _mutate(net, name, 3)
        new = R.snapshot(net)
        assert_separated("plain", old, new, prec, train=name != "batchnorm_data")
        check_eval(net, "plain", "A", prec, name)
        check_train(net, "plain", "A", prec, what=name)
        check_eval(net, "plain", "B", prec, name)
        assert net.__dict__["_eng"] is eng                       # same engine, same buffers throughout


def test_invalidate_keeps_buffer_addresses():
    """invalidate_packed_weights() re-packs into the buffers a captured graph would keep reading."""
    net = _warm()
    eng = net.__dict__["_eng"]
    ptrs = sorted(e[1].data_ptr() for e in eng._pack_cache.values()) + [t.data_ptr() for h in eng._up_cache.values() for t in (h[1], h[2], h[5])]
    R.m_data_copy(net, 5)
    net.invalidate_packed_weights()
    check_eval(net, "plain", "A")
    check_train(net, "plain", "A")
    now = sorted(e[1].data_ptr() for e in eng._pack_cache.values()) + [t.data_ptr() for h in eng._up_cache.values() for t in (h[1], h[2], h[5])]
    assert ptrs == now


# ================================================================================================ 2. backward vs changed weights
@pytest.mark.parametrize("name", ["no_grad_mul", "data_assign"])
def test_backward_refuses_weights_changed_since_the_forward(name):
    net = _warm()
    ora = _ora("plain")
    net.train()
    out = net(ora.xg["A"])
    loss = R.loss_of("plain", out, ora.tg["A"])
    R.PATHWAYS[name][0](net, 1)
    with pytest.raises(RuntimeError, match="has been modified since the forward pass"):
        loss.backward()
    assert all(p.grad is None for p in net.parameters())
    check_train(net, "plain", "A", what="after the refusal")     # the instance stays usable


# ================================================================================================ 3. two live graphs
@pytest.mark.parametrize("kind,between", [("plain", None), ("sp", None), ("plain", "eval_forward"), ("plain", "eval_mode")])
def test_two_live_graphs(kind, between):
    """o1 = net(x1); o2 = net(x2) at another shape and batch size; one backward through both.  between="eval_forward": an
    eval-mode no_grad forward at a third shape sits between the forwards and the backward; "eval_mode": net.eval() is called
    before the backward."""
    net = _warm(kind, shapes=("A", "B", "C"))
    ora = _ora(kind)
    sd0 = R.snapshot(net)
    net.train()
    x1, x2 = ora.xg["A"].clone().requires_grad_(True), ora.xg["B"].clone().requires_grad_(True)
    o1 = net(x1)
    sd1 = R.snapshot(net)
    o2 = net(x2)
    r1, r2 = ora.train(sd0, "A"), ora.train(sd1, "B")
    if between == "eval_forward":
        check_eval(net, kind, "C", what="between")
        net.train()
    elif between == "eval_mode":
        net.eval()
    (R.loss_of(kind, o1, ora.tg["A"]) + R.loss_of(kind, o2, ora.tg["B"])).backward()
    for o, r, w_ in ((o1, r1, "first"), (o2, r2, "second")):
        _judge_outputs([t.detach() for t in (o if isinstance(o, tuple) else (o,))], r["outs"], "fp32", None, w_)
    judge_grads(net, [r1, r2], what="sum of both graphs")
    judge_dx(x1.grad, r1, "dx of the first graph")
    judge_dx(x2.grad, r2, "dx of the second graph")
    judge_buffers(net, r2["post"], what="after both forwards")
    assert all(torch.allclose(r1["post"][k_], sd1[k_], rtol=1e-4, atol=1e-5) for k_ in sd1 if "running" in k_)


# ================================================================================================ 4. accumulation, partial graphs
def test_gradient_accumulation_without_zero_grad():
    net = _warm()
    ora = _ora("plain")
    sd0 = R.snapshot(net)
    _step(net, "plain", "A")
    sd1 = R.snapshot(net)
    _step(net, "plain", "B")
    judge_grads(net, [ora.train(sd0, "A"), ora.train(sd1, "B")], what="accumulated")


def test_input_without_requires_grad_gets_no_dx():
    net = _warm()
    sd0 = R.snapshot(net)
    outs, loss, dx = _step(net, "plain", "A", x_req=False)
    r = _ora("plain").train(sd0, "A")
    assert dx is None
    _judge_outputs(outs, r["outs"], "fp32")
    judge_grads(net, [r], what="x without grad")


def test_frozen_encoder():
    net = _warm()
    sd0 = R.snapshot(net)
    for n_, p in net.named_parameters():
        if n_.startswith("d_blocks."):
            p.requires_grad_(False)
    outs, loss, dx = _step(net, "plain", "A")
    r = _ora("plain").train(sd0, "A")
    _judge_outputs(outs, r["outs"], "fp32")
    assert abs(loss - r["loss"]) < 1e-5
    judge_grads(net, [r], frozen=("d_blocks.",), what="frozen encoder")
    judge_dx(dx, r, "frozen encoder")
    judge_buffers(net, r["post"])


def test_only_the_first_output_in_the_loss():
    """The other output of the two-output head gets the zero-gradient path of _UNetFn.backward."""
    net = _warm("sp")
    check_train(net, "sp", "A", which="first", what="first output only")
    check_train(net, "sp", "B", which="all", what="both outputs again")


def test_second_backward_through_one_forward_is_refused():
    net = _warm()
    ora = _ora("plain")
    net.train()
    loss = R.loss_of("plain", net(ora.xg["A"]), ora.tg["A"])
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="backward through the same forward twice is not supported"):
        loss.backward()


# ================================================================================================ 5. alternation on one instance
@pytest.mark.parametrize("kind,chk", [("plain", False), ("sp", False), ("plain", True)])
def test_shape_batch_and_mode_alternation(kind, chk):
    """A-train, B-eval, A-train, B-train, A-eval on one instance, every step against the oracle -- outputs, gradients, running
    statistics and num_batches_tracked.  chk: use_checkpoint=True moves the statistics of every live BatchNorm twice per train
    step (the dead centre block once); a later step with chk off on the same engine must move them once again."""
    net = _warm(kind, chk=chk)
    for shape, mode in (("A", "train"), ("B", "eval"), ("A", "train"), ("B", "train"), ("A", "eval")):
        if mode == "eval":
            check_eval(net, kind, shape, what=f"{shape}-{mode}")
        else:
            check_train(net, kind, shape, what=f"{shape}-{mode}", chk=chk)
    if chk:
        net.chk = False
        check_train(net, kind, "B", what="chk off again", chk=False)
        net.chk = True
        check_train(net, kind, "A", what="chk on again", chk=True)


# ================================================================================================ 6. precision and device moves
def test_precision_moves_on_a_warm_instance():
    net = _warm()
    net.set_precision("bf16")
    check_eval(net, "plain", "A", "bf16", "fp32 -> bf16")
    old = R.snapshot(net)
    _mutate(net, "no_grad_mul", 1)
    assert_separated("plain", old, R.snapshot(net), "bf16")
    check_train(net, "plain", "A", "bf16", what="mutated in bf16")
    net.set_precision("fp32")
    check_eval(net, "plain", "A", what="bf16 -> fp32")
    check_train(net, "plain", "B", what="bf16 -> fp32")
    old = R.snapshot(net)
    _mutate(net, "load_state_dict", 2)
    assert_separated("plain", old, R.snapshot(net), "bf16")
    net.set_precision("bf16")
    check_eval(net, "plain", "A", "bf16", "mutated in fp32, back to bf16")
    check_eval(net, "plain", "B", "bf16", "mutated in fp32, back to bf16")


def test_device_moves_on_a_warm_instance():
    net = _warm()
    eng = net.__dict__["_eng"]
    old = R.snapshot(net)
    net.cpu()
    _mutate(net, "no_grad_mul", 1)                  # written while the parameters live on the host
    net.cuda()
    assert_separated("plain", old, R.snapshot(net))
    check_eval(net, "plain", "A", what="cpu -> cuda")
    check_train(net, "plain", "A", what="cpu -> cuda")
    check_eval(net, "plain", "B", what="cpu -> cuda")
    assert net.float() is net and net.__dict__["_eng"] is eng
    check_eval(net, "plain", "A", what="float()")
    check_train(net, "plain", "B", what="float()")


# ================================================================================================ 7. copies
@pytest.mark.parametrize("drop_original", [False, True])
def test_deepcopy_follows_its_own_weights(drop_original):
    net = _warm()
    old = R.snapshot(net)
    twin = copy.deepcopy(net)
    assert "_eng" not in twin.__dict__ and "_eng" in net.__dict__
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(twin.parameters(), net.parameters()))
    _mutate(twin, "no_grad_mul", 1)
    if drop_original:
        del net
        gc.collect()
        torch.cuda.empty_cache()
    else:
        _mutate(net, "detach_mul", 2)
        assert_separated("plain", R.snapshot(twin), R.snapshot(net))
        check_eval(net, "plain", "A", what="original")
        check_train(net, "plain", "A", what="original")
    assert_separated("plain", old, R.snapshot(twin))
    check_eval(twin, "plain", "A", what="copy")
    check_train(twin, "plain", "A", what="copy")
    check_eval(twin, "plain", "B", what="copy")


@pytest.mark.parametrize("kind,prec", [("plain", "fp32"), ("sp", "fp32"), ("plain", "bf16")])
def test_pickled_module_round_trip(kind, prec, tmp_path):
    """torch.save(net) of a warm instance: the file carries no engine (no device buffers of the original), the loaded model
    keeps its precision and is oracle-correct in eval and train, also after the original moved on."""
    net = _warm(kind, prec)
    path = tmp_path / "net.pt"
    torch.save(net, path)
    loaded = torch.load(path, weights_only=False)
    assert "_eng" not in loaded.__dict__ and "_eng" in net.__dict__
    assert loaded.__dict__.get("_act_dtype", torch.float32) == net.__dict__.get("_act_dtype", torch.float32)
    _mutate(net, "no_grad_mul", 1)
    assert loaded._engine().dtype == (DT[prec] or torch.float32) and not loaded._engine()._pack_cache
    check_eval(loaded, kind, "A", prec, "loaded")
    check_train(loaded, kind, "A", prec, what="loaded")
    check_eval(net, kind, "A", prec, "original")


def test_pickle_keeps_the_dynamic_loss_scaler_state(tmp_path):
    from ctunet_amd.loss_scale import DynamicLossScale
    net = R.make_net().cuda().set_precision("fp16", loss_scale=DynamicLossScale(init_scale=1024.0, growth_interval=7))
    _step(net, "plain", "A")
    torch.save(net, tmp_path / "net.pt")
    loaded = torch.load(tmp_path / "net.pt", weights_only=False)
    assert "_eng" not in loaded.__dict__
    sc = loaded.loss_scaler
    assert sc is not None and sc is not net.loss_scaler and sc.get_scale() == net.loss_scaler.get_scale() == 1024.0
    assert sc.growth_interval == 7 and sc.scale.data_ptr() != net.loss_scaler.scale.data_ptr()
    assert loaded._engine().dtype == torch.float16 and loaded._engine().scaler is sc
    outs, loss, dx = _step(loaded, "plain", "A")
    assert np.isfinite(loss) and not loaded.overflowed()
