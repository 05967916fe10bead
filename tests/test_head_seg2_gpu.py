"""The two-segment head entries (ctu_head_fwd_seg2, ctu_head_bwd_bn_seg2 and the ctu_lp_* counterparts, csrc/head_loss.hip)
against the one-buffer entries on the same values, and the engine with the top-level concat buffer split in two dense halves
(engine.SPLIT_CAT0) against the interleaved buffer.

The two forms issue the same loads per lane and the same arithmetic in the same order, so the bound is 0 differing words:
every output is compared as raw 32-bit (16-bit) words.  Every buffer a kernel writes is NaN-prefilled and compared whole,
guard words around the segments included, so a store outside a segment's channels shows as a changed guard word and a word
the kernel should have written but did not shows as a NaN that the one-buffer form does not have.

Shapes: 5 x 6 x 18 = 540 voxels per item is no multiple of the forward's 256 voxels per block nor of the backward's
256 / (2 cp / 4) = 128, 64 or 32, and takes more than one block; N = 2 puts the batch boundary inside a block."""
import pytest
import torch

from util import gen

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CODE = {"fp32": 0, "bf16": 1, "fp16": 2}
DIMS = (5, 6, 18)
COMBOS = [(2, 1, 0), (3, 2, 1), (3, 1, 2), (1, 2, 0)]          # (Co, act: 1 softmax / 2 sigmoid, head_mode)
NAN = float("nan")


def _lib():
    from ctunet_amd import _lib
    return _lib.load()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if not a.dtype.is_floating_point:                      # (a BatchNorm's step counter)
        assert torch.equal(a, b), what
        return
    ndiff = int((_bits(a) != _bits(b)).sum().item())
    assert ndiff == 0, f"{what}: {ndiff} of {a.numel()} words differ"


def _p(t, off=0):
    return None if t is None else t.data_ptr() + off * t.element_size()


class Problem:
    """One head problem: 2 cp padded channels, cp - 1 logical channels per half (imap) unless ``full``."""

    def __init__(self, name, cp, n, co, act, mode, full=False, xform=True):
        self.name, self.dt, self.cp, self.n, self.co, self.act, self.mode = name, DT[name], cp, n, co, act, mode
        d, h, w = DIMS
        self.v = d * h * w
        self.nv = n * self.v
        c = cp if full else cp - 1
        self.ci = 2 * c
        self.imap = None if full else torch.tensor(list(range(c)) + list(range(cp, cp + c)), dtype=torch.int32).cuda()
        x = torch.randn(self.nv, 2 * cp, generator=gen(1)) * 1.3 + 0.2
        if not full:
            x[:, c:cp] = 0.0
            x[:, cp + c:] = 0.0
        self.x = x.to(self.dt).cuda()
        self.xform = xform
        # scale / shift / mean / invstd of all 2 cp channels (the BatchNorm rows use the first cp)
        self.vec = torch.stack([torch.rand(2 * cp, generator=gen(2)) + 0.3, torch.randn(2 * cp, generator=gen(3)) * 0.3,
                                torch.randn(2 * cp, generator=gen(4)) * 0.2, torch.rand(2 * cp, generator=gen(5)) + 0.5]).cuda()
        self.w = (torch.randn(co, self.ci, generator=gen(6)) * 0.4).cuda()
        self.b = torch.randn(co, generator=gen(7)).cuda()
        oc = co if mode == 0 else 2
        self.out_shape = (n, oc, d, h, w)
        self.g0 = torch.randn(self.out_shape, generator=gen(8)).cuda()
        self.g1 = torch.randn(self.out_shape, generator=gen(9)).cuda() if mode else None
        lib = _lib()
        self.rows = lib.ctu_head_bwd_num_blocks(n, self.v)
        self.ws_n = lib.ctu_head_bwd_ws_floats(n, self.v, 2 * cp, co)

    # ---- buffers: NaN everywhere, the values in channels [c0, c0 + width) of a cs-wide buffer
    def _hold(self, vals, cs, c0):
        buf = torch.full((self.nv, cs), NAN, dtype=self.dt, device="cuda")
        if vals is not None:
            buf[:, c0:c0 + vals.shape[1]] = vals
        return buf

    def _common(self):
        sc, sh = (self.vec[0], self.vec[1]) if self.xform else (None, None)
        return (_p(sc), _p(sh), 1 if self.xform else 0, self.w.data_ptr(), self.b.data_ptr(), _p(self.imap), self.ci, self.co,
                self.act, self.mode)

    def _call(self, entry, lp_entry, *args):
        lib = _lib()
        code = CODE[self.name]
        return getattr(lib, lp_entry)(code, *args) if code else getattr(lib, entry)(*args)

    def forward(self, layout):
        """layout None: one buffer (cs = 2 cp + 8, slice at channel 8); (cs_a, c0_a, cs_b, c0_b): two segments."""
        cp = self.cp
        out0 = torch.full(self.out_shape, NAN, device="cuda")
        out1 = torch.full(self.out_shape, NAN, device="cuda") if self.mode else None
        if layout is None:
            buf = self._hold(self.x, 2 * cp + 8, 8)
            rc = self._call("ctu_head_fwd", "ctu_lp_head_fwd", _p(buf, 8), 2 * cp + 8, 2 * cp, *self._common(), _p(out0),
                            _p(out1), self.n, self.v, None)
        else:
            cs_a, c0_a, cs_b, c0_b = layout
            a, b = self._hold(self.x[:, :cp], cs_a, c0_a), self._hold(self.x[:, cp:], cs_b, c0_b)
            rc = self._call("ctu_head_fwd_seg2", "ctu_lp_head_fwd_seg2", _p(a, c0_a), cs_a, _p(b, c0_b), cs_b, cp,
                            *self._common(), _p(out0), _p(out1), self.n, self.v, None)
        assert rc == 0
        torch.cuda.synchronize()
        return out0, out1

    def backward(self, layout, bn=True, scale=None):
        """scale: None, a float (16-bit entries' gscale) or a device float32[1] (the _dscale entries).
        Returns {name: tensor} of everything the launch pair wrote; gin as (channels [0, cp), [cp, 2 cp), guard words)."""
        cp = self.cp
        dw = torch.full_like(self.w, NAN)
        db = torch.full_like(self.b, NAN)
        ws = torch.full((self.ws_n + 8,), NAN, device="cuda")
        part = torch.full((self.rows * 2 * cp + 8,), NAN, device="cuda")
        bn_args = (_p(self.vec[2]), _p(self.vec[3]), cp, _p(part)) if bn else (None, None, 0, None)
        lp = CODE[self.name] != 0
        dscale = isinstance(scale, torch.Tensor)
        tail = (None,) + ((_p(scale),) if dscale else ((float(scale or 1.0),) if lp else ()))
        suffix = "_dscale" if dscale else ""
        if layout is None:
            buf = self._hold(self.x, 2 * cp + 8, 8)
            gin = self._hold(None, 2 * cp + 8, 8)
            rc = self._call("ctu_head_bwd_bn", "ctu_lp_head_bwd_bn" + suffix, _p(buf, 8), 2 * cp + 8, 2 * cp, *self._common(),
                            _p(self.g0), _p(self.g1), _p(gin, 8), 2 * cp + 8, _p(dw), _p(db), _p(ws), self.n, self.v, *bn_args,
                            *tail, None)
            guards = [gin[:, :8]]
            ga, gb = gin[:, 8:8 + cp], gin[:, 8 + cp:]
        else:
            cs_a, c0_a, cs_b, c0_b = layout
            a, b = self._hold(self.x[:, :cp], cs_a, c0_a), self._hold(self.x[:, cp:], cs_b, c0_b)
            # the gradient segments take the other segment's layout, so that input and gradient strides differ
            gin_a, gin_b = self._hold(None, cs_b, c0_b), self._hold(None, cs_a, c0_a)
            rc = self._call("ctu_head_bwd_bn_seg2", "ctu_lp_head_bwd_bn" + suffix + "_seg2", _p(a, c0_a), cs_a, _p(b, c0_b),
                            cs_b, cp, *self._common(), _p(self.g0), _p(self.g1), _p(gin_a, c0_b), cs_b, _p(gin_b, c0_a), cs_a,
                            _p(dw), _p(db), _p(ws), self.n, self.v, *bn_args, *tail, None)
            guards = [gin_a[:, :c0_b], gin_a[:, c0_b + cp:], gin_b[:, :c0_a], gin_b[:, c0_a + cp:]]
            ga, gb = gin_a[:, c0_b:c0_b + cp], gin_b[:, c0_a:c0_a + cp]
        assert rc == 0
        torch.cuda.synchronize()
        for g in guards:                                   # nothing was stored outside the segments' channels
            assert bool(torch.isnan(g.float()).all())
        res = dict(gin_a=ga, gin_b=gb, dw=dw, db=db, ws=ws)
        if bn:
            res["bn_rows"] = part
        return res


def _layouts(cp, name):
    """Dense segments, and segments that are themselves slices of wider buffers with different strides.  (16-bit slices
    start on 16-byte boundaries: channel offsets that are multiples of 8.)"""
    return [(cp, 0, cp, 0), (cp + 8, 8, cp + 16, 0) if name != "fp32" else (cp + 8, 4, cp + 20, 12)]


def lay_8(name):
    return _layouts(8, name)[1]


def _compare(one, two, what):
    assert set(one) == set(two)
    for k in one:
        _same(one[k], two[k], f"{what}: {k}")


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("cp", [4, 8, 16])
@pytest.mark.parametrize("name", ["fp32", "bf16", "fp16"])
def test_two_segment_head_is_bitwise_the_one_buffer_head(name, cp, n):
    """out0 / out1, gin, dW, db, the block partials and the BatchNorm reduction rows: 0 words differ, for both head modes
    and both activations, a channel map with one padded channel per half, dense and sliced segments."""
    for co, act, mode in COMBOS:
        pr = Problem(name, cp, n, co, act, mode)
        f1 = pr.forward(None)
        scale = 8.0 if name == "fp16" else None
        b1 = pr.backward(None, scale=scale)
        assert not bool(torch.isnan(b1["gin_a"].float()).any()) and not bool(torch.isnan(b1["bn_rows"][:-8]).any())
        assert not bool(torch.isnan(f1[0]).any())
        for lay in _layouts(cp, name):
            what = f"{name} cp={cp} n={n} head={co, act, mode} layout={lay}"
            f2 = pr.forward(lay)
            _same(f1[0], f2[0], what + ": out0")
            if mode:
                _same(f1[1], f2[1], what + ": out1")
            _compare(b1, pr.backward(lay, scale=scale), what)


@pytest.mark.parametrize("name", ["fp32", "bf16", "fp16"])
def test_two_segment_head_variants(name):
    """cp = 4 with all 8 channels logical (no channel map); the plain backward (no BatchNorm rows) on an input without a
    transform; fp16 with the loss scale read from device memory."""
    lay = _layouts(4, name)[1]
    pr = Problem(name, 4, 2, 2, 1, 0, full=True)
    _same(pr.forward(None)[0], pr.forward(lay)[0], "full map: out0")
    _compare(pr.backward(None), pr.backward(lay), "full map")
    pr = Problem(name, 8, 1, 3, 2, 1, xform=False)
    for k in (0, 1):
        _same(pr.forward(None)[k], pr.forward(lay_8(name))[k], f"no transform: out{k}")
    _compare(pr.backward(None, bn=False), pr.backward(lay_8(name), bn=False), "plain backward")
    if name != "fp32":
        pr = Problem(name, 8, 2, 2, 1, 0)
        s = torch.tensor([8.0], device="cuda")
        one = pr.backward(None, scale=s)
        _compare(one, pr.backward(lay_8(name), scale=s), "device loss scale")
        _compare(one, pr.backward(lay_8(name), scale=8.0), "device loss scale against the host one")


def test_two_segment_head_refuses_malformed_arguments():
    """Every refusal returns a negative code before any launch: the NaN-prefilled outputs stay untouched."""
    lib = _lib()
    cp, n = 8, 1
    pr = Problem("fp32", cp, n, 2, 1, 0)
    a = torch.zeros(pr.nv, cp + 8, device="cuda")
    b = torch.zeros(pr.nv, cp + 8, device="cuda")
    ga, gb = torch.full_like(a, NAN), torch.full_like(b, NAN)
    out0 = torch.full(pr.out_shape, NAN, device="cuda")
    dw, db = torch.full_like(pr.w, NAN), torch.full_like(pr.b, NAN)
    ws = torch.full((pr.ws_n,), NAN, device="cuda")
    part = torch.full((pr.rows * 2 * cp,), NAN, device="cuda")
    good = dict(in_a=_p(a), cs_a=cp + 8, in_b=_p(b), cs_b=cp + 8, cp=cp, gin_a=_p(ga), gcs_a=cp + 8, gin_b=_p(gb), gcs_b=cp + 8)

    def fwd(**kw):
        k = dict(good, **kw)
        return lib.ctu_head_fwd_seg2(k["in_a"], k["cs_a"], k["in_b"], k["cs_b"], k["cp"], *pr._common(), _p(out0), None, n, pr.v,
                                     None)

    def bwd(**kw):
        k = dict(good, **kw)
        return lib.ctu_head_bwd_bn_seg2(k["in_a"], k["cs_a"], k["in_b"], k["cs_b"], k["cp"], *pr._common(), _p(pr.g0), None,
                                        k["gin_a"], k["gcs_a"], k["gin_b"], k["gcs_b"], _p(dw), _p(db), _p(ws), n, pr.v,
                                        _p(pr.vec[2]), _p(pr.vec[3]), cp, _p(part), None, None)

    bad_in = [dict(in_a=None), dict(in_b=None), dict(in_a=_p(a, 1)), dict(in_b=_p(b, 2)),      # null, 4- and 8-byte offsets
              dict(cs_a=cp - 4), dict(cs_b=cp - 4), dict(cs_a=cp + 2), dict(cs_b=cp + 1),       # below cp, no multiple of 4
              dict(cp=6), dict(cp=12), dict(cp=32), dict(cp=0)]                                 # cp outside {4, 8, 16}
    bad_gin = [dict(gin_a=None), dict(gin_b=None), dict(gin_a=_p(ga, 1)), dict(gin_b=_p(gb, 2)),
               dict(gcs_a=cp - 4), dict(gcs_b=cp - 4), dict(gcs_a=cp + 2), dict(gcs_b=cp + 3)]
    for kw in bad_in:
        assert fwd(**kw) < 0, kw
        assert bwd(**kw) < 0, kw
    for kw in bad_gin:
        assert bwd(**kw) < 0, kw
    for code in (1, 2):                                    # the 16-bit entries share the checks
        args16 = (code, _p(a), cp + 8, _p(b, 2), cp + 8, cp, *pr._common(), _p(out0), None, n, pr.v, None)
        assert lib.ctu_lp_head_fwd_seg2(*args16) < 0
    assert lib.ctu_lp_head_fwd_seg2(3, _p(a), cp + 8, _p(b), cp + 8, cp, *pr._common(), _p(out0), None, n, pr.v, None) < 0
    torch.cuda.synchronize()
    for t in (out0, ga, gb, dw, db, ws, part):
        assert bool(torch.isnan(t).all())
    assert fwd() == 0 and bwd() == 0                       # and the well-formed call goes through
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out0).any()) and not bool(torch.isnan(dw).any())


# ====================================================================================================== engine
def _makers():
    import ctunet_amd
    return {"cat": lambda: ctunet_amd.UNet(), "add": lambda: ctunet_amd.UNet(cat=False),
            "none": lambda: ctunet_amd.UNet(use_skip_connections=False)}


def _engine_step(make, split, monkeypatch, dtype=torch.float32):
    """One forward, fused loss and backward of the engine at 32^3; everything it produced."""
    from ctunet_amd import engine as E, ops
    monkeypatch.setattr(E, "SPLIT_CAT0", split)
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
        assert (ctx["cat"][0].dim() == 6) == split and all(c.dim() == 5 for c in ctx["cat"][1:])
        terms, ws = ops.loss_fwd(out0, t, 1.0, 1.0, False)
        g0 = ops.loss_bwd(out0, t, 1.0, 1.0, False, ws, None, None)
        grads, dx = eng.backward(P, ctx, g0, None, True, None)
    torch.cuda.synchronize()
    res = {"grad:" + k: v.detach().clone() for k, v in grads.items() if v is not None}
    res.update({"buf:" + k: v.detach().clone() for k, v in net.named_buffers()})
    res.update(out0=out0.clone(), terms=terms.clone(), dx=dx.detach().clone())
    return res


@pytest.mark.parametrize("skip", ["cat", "add", "none"])
def test_engine_is_bitwise_the_same_with_the_split_top_level_buffer(skip, monkeypatch):
    on = _engine_step(_makers()[skip], True, monkeypatch)
    off = _engine_step(_makers()[skip], False, monkeypatch)
    assert set(on) == set(off) and len(on) > 40
    for k in on:
        _same(on[k], off[k], f"{skip}: {k}")
        assert bool(torch.isfinite(on[k].double()).all()), k


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_engine_16bit_is_bitwise_the_same_with_the_split_top_level_buffer(name, monkeypatch):
    on = _engine_step(_makers()["cat"], True, monkeypatch, DT[name])
    off = _engine_step(_makers()["cat"], False, monkeypatch, DT[name])
    assert set(on) == set(off)
    for k in on:
        _same(on[k], off[k], f"{name}: {k}")


def _graphed(split, dtype, monkeypatch):
    import ctunet_amd
    from ctunet_amd import engine as E, optim
    from ctunet_amd.graph import GraphedTrainStep
    monkeypatch.setattr(E, "SPLIT_CAT0", split)
    torch.manual_seed(0)
    net = ctunet_amd.UNet().cuda().train()
    if dtype != torch.float32:
        net.set_precision(dtype)
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


@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_graphed_train_step_is_bitwise_the_same_over_three_replays(name, monkeypatch):
    on = _graphed(True, DT[name], monkeypatch)
    off = _graphed(False, DT[name], monkeypatch)
    assert set(on) == set(off)
    for k in on:
        _same(on[k], off[k], f"{name}: {k}")
    assert not torch.equal(on["values0"], on["values2"])          # the replays trained
