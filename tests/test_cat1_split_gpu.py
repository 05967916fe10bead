"""The two-segment forms of the fused up-convolution entries (ctu_upconv_fused_fwd_seg2, ctu_upconv_fused_wgrad_seg2,
ctu_upconv_fused_wgrad_bn_seg2, ctu_upconv_fused_bwd_data_seg2; csrc/upconv_fused.hip, csrc/conv3d.hip) against the one-buffer
entries on the same values, and the engine with the level-1 concat buffer split in two dense halves (engine.SPLIT_CAT1)
against the interleaved buffer.

A staged 8-channel chunk (forward) and a 16-channel tile (weight and data gradient) lie in one segment, so the two forms
issue the same loads and stores per lane and the same arithmetic in the same order: the bound is 0 differing words.  Every
output is compared as raw 32-bit words.  Every buffer a kernel writes is NaN-prefilled and compared whole, guard channels
included, so a store outside a segment shows as a changed guard word and a word that was not written as a NaN the one-buffer
form does not have.

Coarse shapes: 4 x 4 x 16 is one forward box (two weight-gradient boxes), 8 x 4 x 32 several boxes per block loop,
5 x 6 x 18 ragged in every axis (the per-item border paths; the lazy-BatchNorm weight gradient takes full boxes only and is
left out there by its own *_supported query).  32 -> 8 runs the w-parity kernels, 32 -> 16 the channel-tile ones, 64 -> 16
has two 16-channel tiles per segment."""
import pytest
import torch

from util import gen

pytestmark = pytest.mark.gpu

NAN = float("nan")
SHAPES = [(4, 4, 16), (8, 4, 32), (5, 6, 18)]
CHANNELS = [(32, 8), (32, 16), (64, 16)]                   # (cin_p, nout_p)


def _lib():
    from ctunet_amd import _lib
    return _lib.load()


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if not a.dtype.is_floating_point:                      # (a BatchNorm's step counter)
        assert torch.equal(a, b), what
        return
    bits = torch.int16 if a.element_size() == 2 else torch.int32
    ndiff = int((a.contiguous().view(bits) != b.contiguous().view(bits)).sum().item())
    assert ndiff == 0, f"{what}: {ndiff} of {a.numel()} words differ"


def _p(t, off=0):
    return None if t is None else t.data_ptr() + off * t.element_size()


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


class Problem:
    """One fused up-convolution: coarse [n, d, h, w, cin_p] in, fine [n, 2d, 2h, 2w, nout_p] out, weights packed once."""

    def __init__(self, dims, n, cin_p, nout_p):
        from ctunet_amd import ops
        self.n, (self.d, self.h, self.w), self.cin_p, self.nout_p, self.seg = n, dims, cin_p, nout_p, cin_p // 2
        self.nv = n * self.d * self.h * self.w
        self.c, self.co = cin_p, nout_p - 2                # logical channels: every input position, two padded outputs
        self.x = (torch.randn(self.nv, cin_p, generator=gen(1)) * 1.3 + 0.2).cuda()
        self.xf = torch.stack([torch.rand(cin_p, generator=gen(2)) + 0.3, torch.randn(cin_p, generator=gen(3)) * 0.3]).cuda()
        self.wt = (torch.randn(self.c, self.c, 2, 2, 2, generator=gen(4)) * 0.2).cuda()
        self.bt = (torch.randn(self.c, generator=gen(5)) * 0.2).cuda()
        self.w3 = (torch.randn(self.co, self.c, 3, 3, 3, generator=gen(6)) * 0.1).cuda()
        self.wp, self.beff, self.pws, self.wpd = ops.upconv_fused_pack_all(self.wt, self.bt, self.w3, None, cin_p, nout_p)
        # fine-grid tensors of the backward entries: stride = nout_p (the w-parity weight gradient needs 8 = g_cs)
        self.g = torch.randn(8 * self.nv, nout_p, generator=gen(7)).cuda()
        self.y = torch.randn(8 * self.nv, nout_p, generator=gen(8)).cuda()
        self.bn = torch.stack([torch.rand(nout_p, generator=gen(9)) + 0.3, torch.randn(nout_p, generator=gen(10)) * 0.3]).cuda()
        self.coef = torch.randn(5, nout_p, generator=gen(11)).cuda()
        lib = _lib()
        geo = (n, self.d, self.h, self.w)
        self.rows = lib.ctu_upconv_fused_num_blocks(*geo, nout_p)
        self.ws_n = lib.ctu_upconv_fused_wgrad_ws_floats(*geo, cin_p, nout_p)
        self.lazy_ok = bool(lib.ctu_upconv_fused_wgrad_bn_supported(*geo, cin_p, nout_p))
        assert lib.ctu_upconv_fused_seg2_supported(3, self.d, self.h, self.w, cin_p, nout_p, self.seg)

    # ---- the coarse tensor: NaN everywhere but the channels that hold values
    def one_buffer(self, vals=True):
        """(tensor, ptr, cs): channels [8, 8 + cin_p) of a (cin_p + 12)-wide buffer."""
        buf = _nan(self.nv, self.cin_p + 12)
        if vals:
            buf[:, 8:8 + self.cin_p] = self.x
        return buf, _p(buf, 8), self.cin_p + 12

    def segments(self, sliced, vals=True):
        """(a, b, ptr_a, ptr_b, cs, c0_a, c0_b): two dense tensors, or slices (channels 8.. / 4..) of two wider ones."""
        s = self.seg
        cs, c0a, c0b = (s + 12, 8, 4) if sliced else (s, 0, 0)
        a, b = _nan(self.nv, cs), _nan(self.nv, cs)
        if vals:
            a[:, c0a:c0a + s] = self.x[:, :s]
            b[:, c0b:c0b + s] = self.x[:, s:]
        return a, b, _p(a, c0a), _p(b, c0b), cs, c0a, c0b

    def _xf(self, xform):
        return (_p(self.xf[0]), _p(self.xf[1]), 1) if xform else (None, None, 0)

    def _geo(self):
        return self.n, self.d, self.h, self.w

    def forward(self, src, xform):
        """src: (ptr, cs) or (ptr_a, ptr_b, cs).  Returns (out with 4 guard channels, BatchNorm partial rows + guard)."""
        lib = _lib()
        out = _nan(8 * self.nv, self.nout_p + 4)
        stats = _nan(self.rows * 2 * self.nout_p + 8)
        tail = (_p(self.wp), _p(self.beff), _p(out), self.nout_p + 4, self.nout_p, _p(stats), *self._geo(), None, None)
        if len(src) == 2:
            rc = lib.ctu_upconv_fused_fwd(src[0], src[1], self.cin_p, *self._xf(xform), *tail)
        else:
            rc = lib.ctu_upconv_fused_fwd_seg2(src[0], src[1], self.seg, src[2], self.cin_p, *self._xf(xform), *tail)
        assert rc == 0
        torch.cuda.synchronize()
        return {"out": out, "stats": stats}

    def wgrad(self, src, xform, lazy):
        """dW_eff, the slab workspace and (lazy) the raw-output gradient the kernel wrote."""
        lib = _lib()
        dweff = _nan(8 * 8 * self.cin_p * self.nout_p + 8)
        ws = _nan(self.ws_n + 8)
        gy = _nan(8 * self.nv, self.nout_p)
        act = (src[0], src[1], self.cin_p) if len(src) == 2 else (src[0], src[1], self.seg, src[2], self.cin_p)
        sfx = "" if len(src) == 2 else "_seg2"
        if lazy:
            rc = getattr(lib, "ctu_upconv_fused_wgrad_bn" + sfx)(*act, *self._xf(xform), _p(self.g), self.nout_p, self.nout_p,
                                                                 _p(self.y), _p(self.bn[0]), _p(self.bn[1]), _p(self.coef),
                                                                 _p(gy), _p(dweff), _p(ws), *self._geo(), None)
        else:
            rc = getattr(lib, "ctu_upconv_fused_wgrad" + sfx)(*act, *self._xf(xform), _p(self.g), self.nout_p, self.nout_p,
                                                              _p(dweff), _p(ws), *self._geo(), None)
        assert rc == 0
        torch.cuda.synchronize()
        return {"dweff": dweff, "slabs": ws, "gy": gy}

    def params(self, x, lazy):
        """(dwt, dbt, dw3) through ops.upconv_fused_wgrad: x a CL or a CL2."""
        from ctunet_amd import ops
        fine = (self.n, 2 * self.d, 2 * self.h, 2 * self.w, self.nout_p)
        g = ops.CL(self.g.view(fine), 0, self.nout_p)
        lz = None
        if lazy:
            lz = (ops.CL(self.y.view(fine), 0, self.nout_p), self.bn, self.coef, ops.CL(_nan(*fine), 0, self.nout_p))
        dwt, dbt, dw3 = ops.upconv_fused_wgrad(x, g, self.c, self.co, self.bt, self.pws, None, lz)
        torch.cuda.synchronize()
        return {"dwt": dwt, "dbt": dbt, "dw3": dw3}


CASES = [(s, n, c) for s in SHAPES for n in (1, 2) for c in CHANNELS]


@pytest.mark.parametrize("dims,n,ch", CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-n{n}-{c[0]}to{c[1]}" for s, n, c in CASES])
def test_two_segment_entries_write_the_one_buffer_entries_words(dims, n, ch):
    from ctunet_amd import ops
    lib = _lib()
    pr = Problem(dims, n, *ch)
    s = pr.seg
    buf, ptr, cs1 = pr.one_buffer()
    layouts = {sliced: pr.segments(sliced) for sliced in (False, True)}
    for xform in (True, False):
        ref_f = pr.forward((ptr, cs1), xform)
        ref_w = {lz: pr.wgrad((ptr, cs1), xform, lz) for lz in (False, True) if pr.lazy_ok or not lz}
        for sliced, (a, b, pa, pb, cs, c0a, c0b) in layouts.items():
            tag = f"xform={xform} sliced={sliced}"
            got = pr.forward((pa, pb, cs), xform)
            for k in ref_f:
                _same(got[k], ref_f[k], f"forward {k} ({tag})")
            for lz, ref in ref_w.items():
                got = pr.wgrad((pa, pb, cs), xform, lz)
                for k in ref:
                    _same(got[k], ref[k], f"weight gradient lazy={lz} {k} ({tag})")
    # the parameter gradients through the host layer (CL against CL2), with the transform
    sc, sh = pr.xf[0], pr.xf[1]
    x1 = ops.CL(buf.view(n, *dims, cs1), 8, pr.cin_p, sc, sh, True)
    a, b, _, _, cs, c0a, c0b = layouts[True]
    x2 = ops.CL2(ops.CL(a.view(n, *dims, cs), c0a, s), ops.CL(b.view(n, *dims, cs), c0b, s), sc, sh, True)
    for lz in ((False, True) if pr.lazy_ok else (False,)):
        ref, got = pr.params(x1, lz), pr.params(x2, lz)
        for k in ref:
            _same(got[k], ref[k], f"parameter gradient lazy={lz} {k}")
    # data gradient: both segments, guard channels included
    gin, gptr, _ = pr.one_buffer(vals=False)
    assert lib.ctu_upconv_fused_bwd_data(_p(pr.g), pr.nout_p, pr.nout_p, _p(pr.wpd), gptr, cs1, pr.cin_p, n, *dims, None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(gin[:, :8]).all()) and bool(torch.isnan(gin[:, 8 + pr.cin_p:]).all())
    assert not bool(torch.isnan(gin[:, 8:8 + pr.cin_p]).any())
    for sliced in (False, True):
        ga, gb, pa, pb, cs, c0a, c0b = pr.segments(sliced, vals=False)
        assert lib.ctu_upconv_fused_bwd_data_seg2(_p(pr.g), pr.nout_p, pr.nout_p, _p(pr.wpd), pa, pb, s, cs, pr.cin_p, n, *dims,
                                                  None) == 0
        torch.cuda.synchronize()
        exp_a, exp_b = _nan(pr.nv, cs), _nan(pr.nv, cs)
        exp_a[:, c0a:c0a + s] = gin[:, 8:8 + s]
        exp_b[:, c0b:c0b + s] = gin[:, 8 + s:8 + 2 * s]
        _same(ga, exp_a, f"data gradient, first segment (sliced={sliced})")
        _same(gb, exp_b, f"data gradient, second segment (sliced={sliced})")


def test_malformed_segments_are_refused_before_any_launch():
    lib = _lib()
    n, dims = 1, (4, 4, 16)
    pr = Problem(dims, n, 32, 8)
    s = pr.seg
    a, b, pa, pb, cs, _, _ = pr.segments(True)
    out = _nan(8 * pr.nv, 8)
    stats = _nan(pr.rows * 16)
    dweff, ws, gy = _nan(8 * 8 * 32 * 8), _nan(pr.ws_n), _nan(8 * pr.nv, 8)
    ga, gb, pga, pgb, _, _, _ = pr.segments(True, vals=False)
    good = dict(a=pa, b=pb, seg=s, cs=cs, cin=32)

    def fwd(**kw):
        k = dict(good, **kw)
        return lib.ctu_upconv_fused_fwd_seg2(k["a"], k["b"], k["seg"], k["cs"], k["cin"], *pr._xf(True), _p(pr.wp), _p(pr.beff),
                                             _p(out), 8, 8, _p(stats), n, *dims, None, None)

    def wg(**kw):
        k = dict(good, **kw)
        return lib.ctu_upconv_fused_wgrad_seg2(k["a"], k["b"], k["seg"], k["cs"], k["cin"], *pr._xf(True), _p(pr.g), 8, 8,
                                               _p(dweff), _p(ws), n, *dims, None)

    def wgbn(**kw):
        k = dict(good, **kw)
        return lib.ctu_upconv_fused_wgrad_bn_seg2(k["a"], k["b"], k["seg"], k["cs"], k["cin"], *pr._xf(True), _p(pr.g), 8, 8,
                                                  _p(pr.y), _p(pr.bn[0]), _p(pr.bn[1]), _p(pr.coef), _p(gy), _p(dweff), _p(ws),
                                                  n, *dims, None)

    def bwd(**kw):
        k = dict(dict(good, a=pga, b=pgb), **kw)
        return lib.ctu_upconv_fused_bwd_data_seg2(_p(pr.g), 8, 8, _p(pr.wpd), k["a"], k["b"], k["seg"], k["cs"], k["cin"], n,
                                                  *dims, None)

    # a null segment; pointers off by 4 and 8 bytes; the common stride below seg_c or no multiple of 4 (one stride serves both
    # segments: unequal strides cannot be expressed, and the host layer refuses them -- below); 2 seg_c != cin_p
    bad = [dict(a=None), dict(b=None), dict(cs=s - 4), dict(cs=s + 2), dict(seg=8), dict(seg=24), dict(seg=0), dict(cin=48)]
    for kw in bad + [dict(a=_p(a, 9)), dict(b=_p(b, 6))]:
        for f in (fwd, wg, wgbn):
            assert f(**kw) < 0, (f.__name__, kw)
    for kw in bad + [dict(a=_p(ga, 9)), dict(b=_p(gb, 6))]:
        assert bwd(**kw) < 0, kw
    # seg_c no multiple of 8 (forward) / of 16 (the gradients), with cin_p = 2 seg_c
    assert fwd(seg=12, cin=24) < 0 and fwd(seg=4, cin=8) < 0
    for f in (wg, wgbn, bwd):
        assert f(seg=8, cin=16) < 0 and f(seg=24, cin=48) < 0, f.__name__
    assert not lib.ctu_upconv_fused_seg2_supported(3, *dims, 16, 8, 8)
    assert not lib.ctu_upconv_fused_seg2_supported(3, *dims, 32, 8, 8)
    assert not lib.ctu_upconv_fused_seg2_supported(3, 4, 4, 8, 32, 8, 16)          # what the one-buffer kernels refuse
    torch.cuda.synchronize()
    for t in (out, stats, dweff, ws, gy, ga, gb):
        assert bool(torch.isnan(t).all())
    from ctunet_amd import ops
    wide = _nan(n, *dims, s + 8)
    with pytest.raises(AssertionError):                    # segments of unequal voxel strides
        ops.CL2(ops.CL(a.view(n, *dims, cs), 8, s), ops.CL(wide, 0, s)).up_args()
    assert fwd() == 0 and wg() == 0 and wgbn() == 0 and bwd() == 0                 # and the well-formed calls go through
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(dweff).any()) and not bool(torch.isnan(gy).any())


# ====================================================================================================== engine
def _engine_step(make, split, monkeypatch, dtype=torch.float32, expect_split=None, fuse_up=True):
    """One forward, fused loss and backward of the engine at 32^3; everything it produced."""
    from ctunet_amd import engine as E, ops
    monkeypatch.setattr(E, "SPLIT_CAT1", split)
    if not fuse_up:
        monkeypatch.setattr(E, "FUSE_UP", False)
    torch.manual_seed(0)
    net = make().cuda().train()
    if dtype != torch.float32:
        net.set_precision(dtype)
    x = torch.randn(1, 1, 32, 32, 32, generator=gen(3)).cuda()
    t = (torch.rand(1, 1, 32, 32, 32, generator=gen(4)) < 0.3).float()
    t = torch.cat((1 - t, t), 1).cuda()
    eng = net._engine()
    P = E._tensor_dict(net)
    with torch.no_grad():
        out0, out1, ctx = eng.forward(P, x, True, True, bool(getattr(net, "chk", False)))
        assert out1 is None
        want = split if expect_split is None else expect_split
        assert ctx["cat_split"][1] == want and not any(ctx["cat_split"][2:])
        cp1 = 16
        assert tuple(ctx["cat"][1].shape) == ((2, 16, 16, 16, cp1) if want else (1, 16, 16, 16, 2 * cp1))
        terms, ws = ops.loss_fwd(out0, t, 1.0, 1.0, False)
        g0 = ops.loss_bwd(out0, t, 1.0, 1.0, False, ws, None, None)
        grads, dx = eng.backward(P, ctx, g0, None, True, None)
    torch.cuda.synchronize()
    res = {"grad:" + k: v.detach().clone() for k, v in grads.items() if v is not None}
    res.update({"buf:" + k: v.detach().clone() for k, v in net.named_buffers()})
    res.update(out0=out0.clone(), terms=terms.clone(), dx=dx.detach().clone())
    return res


def _unet():
    import ctunet_amd
    return ctunet_amd.UNet()


def test_engine_is_bitwise_the_same_with_the_split_level_1_buffer(monkeypatch):
    on = _engine_step(_unet, True, monkeypatch)
    off = _engine_step(_unet, False, monkeypatch)
    assert set(on) == set(off) and len(on) > 40
    for k in on:
        _same(on[k], off[k], k)
        assert bool(torch.isfinite(on[k].double()).all()), k


@pytest.mark.parametrize("what", ["unfused", "add", "bf16"])
def test_level_1_stays_interleaved_where_its_consumer_reads_one_buffer(what, monkeypatch):
    """The unfused ConvTranspose3d kernels, the additive skip and the 16-bit fused kernels read one buffer: with the switch on
    the level is allocated interleaved, and the step runs and gives what it gives with the switch off."""
    import ctunet_amd
    make = (lambda: ctunet_amd.UNet(cat=False)) if what == "add" else _unet
    kw = dict(dtype=torch.bfloat16 if what == "bf16" else torch.float32, expect_split=False, fuse_up=what != "unfused")
    on = _engine_step(make, True, monkeypatch, **kw)
    off = _engine_step(make, False, monkeypatch, **kw)
    assert set(on) == set(off)
    for k in on:
        _same(on[k], off[k], f"{what}: {k}")


def _graphed(split, monkeypatch):
    from ctunet_amd import engine as E, optim
    from ctunet_amd.graph import GraphedTrainStep
    monkeypatch.setattr(E, "SPLIT_CAT1", split)
    torch.manual_seed(0)
    net = _unet().cuda().train()
    opt = optim.Adam(net.parameters(), lr=1e-3)
    x = torch.randn(1, 1, 32, 32, 32, generator=gen(3)).cuda()
    t = (torch.rand(1, 1, 32, 32, 32, generator=gen(4)) < 0.3).float()
    t = torch.cat((1 - t, t), 1).cuda()
    gs = GraphedTrainStep(net, opt, x, [t], 1.0, 1.0, warmup=1)
    vals = []
    for _ in range(3):
        gs(x, [t])
        vals.append(gs.values.clone())
    torch.cuda.synchronize()
    res = {k: v.detach().clone() for k, v in net.state_dict().items()}
    res.update({f"values{i}": v for i, v in enumerate(vals)})
    return res


def test_graphed_train_step_is_bitwise_the_same_over_three_replays(monkeypatch):
    on = _graphed(True, monkeypatch)
    off = _graphed(False, monkeypatch)
    assert set(on) == set(off)
    for k in on:
        _same(on[k], off[k], k)
