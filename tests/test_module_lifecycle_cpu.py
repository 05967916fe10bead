"""What test_module_lifecycle_gpu.py relies on, checked without a device: how each way of writing a weight moves torch's
version counter and the tensor's address (the keys of the packed-weight caches -- a torch upgrade that changes one of these
facts shows up here), that every mutation the GPU cases use separates the oracle's outputs by at least 100 x the output gate
in eval AND train mode, that the chosen shapes reach the fused and the unfused up-convolution and two conv layouts, and
that copies and pickles of a model leave the engine behind."""
import copy
import io

import pytest
import torch

import lifecycle_ref as R


def _lib():
    from ctunet_amd import _lib as L
    return L.load()


CPU_PATHWAYS = [n for n in R.PATHWAYS if n != "project_adam"]


def _apply(name, net, k):
    try:
        R.PATHWAYS[name][0](net, k)
    except RuntimeError as e:
        if name.endswith("_fused"):
            pytest.skip(f"torch.optim {name} is not available for these parameters: {e}")
        raise


@pytest.mark.parametrize("name", CPU_PATHWAYS)
def test_version_counter_and_address_per_pathway(name):
    """The caches key on (p._version, p.data_ptr()).  In-place writes through .data move neither (the hole that
    invalidate_packed_weights() closes); re-seating .data moves the address only; everything else moves the version."""
    _, bumps, moves, via_data = R.PATHWAYS[name]
    net = R.make_net()
    before = {n_: (p, p._version, p.data_ptr(), p.detach().clone()) for n_, p in net.named_parameters() if n_ in R.TARGETS}
    _apply(name, net, 0)
    after = dict(net.named_parameters())
    for n_, (p, ver, ptr, val) in before.items():
        q = after[n_]
        assert not torch.equal(q.detach(), val), n_                # (the write happened)
        if bumps is None:                                          # load_state_dict(assign=True): a new Parameter object
            assert q is not p and q.data_ptr() != ptr, n_
            continue
        assert q is p, n_
        assert (q._version > ver) == bumps, (n_, ver, q._version)
        assert (q.data_ptr() != ptr) == moves, n_
        assert via_data == (not bumps and not moves), n_           # exactly the writes no key can see need the explicit call


@pytest.mark.parametrize("kind", ["plain", "sp"])
def test_every_mutation_separates_the_oracle_outputs(kind):
    """A stale packed weight passes a 1e-4 gate only if the write was small: a chain of all pathways (k = 0, 1, ...), each
    state at least 1e-2 of max |ref| away from the one before, eval and train, at the fused and the unfused shape."""
    ora = R.OracleCache(kind)
    net = R.make_net(kind)
    old = R.snapshot(net)
    worst = {}
    for k, name in enumerate(CPU_PATHWAYS + ["batchnorm_data"]):
        if name == "batchnorm_data":
            R.m_batchnorm_data(net, k)
        elif name.endswith("_fused"):
            try:
                R.PATHWAYS[name][0](net, k)
            except RuntimeError:
                continue
        else:
            R.PATHWAYS[name][0](net, k)
        new = R.snapshot(net)
        for shape in ("A", "B"):
            e, t = ora.separation(old, new, shape)
            worst[(name, shape)] = (e, t)
            assert e >= R.SEPARATION, (name, shape, e)
            if name != "batchnorm_data":           # (running statistics do not enter a train-mode forward)
                assert t >= R.SEPARATION, (name, shape, t)
        old = new
    print(worst)


def test_a_plain_factor_is_invisible_in_train_mode():
    """Why the mutations are not `weight * 0.5`: the BatchNorm behind every conv divides a factor out again."""
    ora = R.OracleCache("plain")
    net = R.make_net()
    old = R.snapshot(net)
    with torch.no_grad():
        for _, p in R._targets(net):
            p.mul_(0.5)
    e, t = ora.separation(old, R.snapshot(net), "A")
    assert e >= R.SEPARATION and t < R.SEPARATION, (e, t)


def test_shapes_reach_fused_and_unfused_upconv_and_two_layouts():
    lib = _lib()
    pad8 = lambda c: -(-c // 8) * 8
    for kind, spec in R.SPECS.items():
        w0, w1 = spec.i_size, 2 * spec.i_size
        top_in, top_out = 2 * pad8(w1), pad8(w0)                # the top decoder level reads level 1's concat buffer
        for shape, fused in (("A", True), ("B", False), ("C", True)):
            n, d, h, w = R.SHAPES[shape]
            assert bool(lib.ctu_upconv_fused_supported(3, d // 2, h // 2, w // 2, top_in, top_out)) == fused, (kind, shape)
            assert bool(lib.ctu_lp_upconv_fused_supported(3, d // 2, h // 2, w // 2, top_in, top_out)) == fused, (kind, shape)
            # the bottom level (coarse W <= 12) is unfused at every shape
            assert not lib.ctu_upconv_fused_supported(3, d // 4, h // 4, w // 4, pad8(w1), pad8(w1)), (kind, shape)
            assert lib.ctu_conv3d_first_supported(3, spec.in_ch, pad8(w0), w), (kind, shape)
        # the full-resolution 8 -> 8 conv: pair layout at W >= 32, layout 0 below -- two packed copies of one weight
        for code in ("fp32", "lp"):
            lay = {s: (lib.ctu_conv3d_layout(3, 8, R.SHAPES[s][3]) if code == "fp32" else
                       lib.ctu_lp_conv3d_layout(3, 8, 8, R.SHAPES[s][3])) for s in R.SHAPES}
            assert lay["A"] != lay["B"] and lay["A"] == lay["C"], (code, lay)


def _engine_with_fake_cache(net):
    eng = net._engine()
    eng._pack_cache[("x", "conv", 0, 8, 8, 0, eng.dtype)] = ((3, 1234), torch.zeros(4), None)
    eng._up_cache["u_blocks.1.block"] = (((1, 2),) * 3, torch.zeros(1), torch.zeros(1), (32, 8, eng.dtype), torch.zeros(1), torch.zeros(1))
    return eng


def test_invalidate_keeps_the_buffers_and_drops_the_keys():
    net = R.make_net()
    assert net.invalidate_packed_weights() is net                # no engine yet: nothing to do
    eng = _engine_with_fake_cache(net)
    bufs = [e[1] for e in eng._pack_cache.values()] + [t for h in eng._up_cache.values() for t in (h[1], h[2], h[4], h[5])]
    net.invalidate_packed_weights()
    assert all(e[0] is None for e in eng._pack_cache.values()) and all(h[0] is None for h in eng._up_cache.values())
    now = [e[1] for e in eng._pack_cache.values()] + [t for h in eng._up_cache.values() for t in (h[1], h[2], h[4], h[5])]
    assert all(a is b for a, b in zip(bufs, now))                # stable pointers: captured graphs keep reading them
    assert all(h[3] == (32, 8, eng.dtype) for h in eng._up_cache.values())


@pytest.mark.parametrize("kind", ["plain", "sp"])
def test_copies_and_pickles_leave_the_engine_behind(kind):
    net = R.make_net(kind).set_precision("fp16", loss_scale=512.0)
    _engine_with_fake_cache(net)
    assert "_eng" in net.__dict__
    buf = io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    for other in (copy.deepcopy(net), torch.load(buf, weights_only=False)):
        assert "_eng" not in other.__dict__
        assert other.__dict__["_act_dtype"] == torch.float16 and other.__dict__["_loss_scale"] == 512.0
        eng = other._engine()
        assert eng is not net.__dict__["_eng"] and eng.dtype == torch.float16 and eng.loss_scale == 512.0
        assert not eng._pack_cache and not eng._up_cache
        assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), net.state_dict().values()))
    assert "_eng" in net.__dict__                                # the original keeps its own
