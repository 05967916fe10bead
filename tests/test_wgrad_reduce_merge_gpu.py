"""Deferred weight-gradient slab reductions (csrc/wgrad_reduce.h, ctu_*_slabs, ctu_bn_bwd_finalize_jobs,
ctu_wgrad_reduce_jobs; engine.DEFER_WGRAD_REDUCE).

The reduction bodies and the BatchNorm-backward finalize body are the stand-alone kernels' own code, hosted by another
launch, so every comparison here is bit for bit (raw 32-bit words, tolerance 0): the immediate entry against the
slabs-only entry whose job rides on a finalize launch, and against the same job through the stand-alone flush.  Every
output buffer is pre-filled with NaN, so an element a launch does not write shows.  Shapes are the smallest that reach
each index path (one box, gx > 1, two channel groups, a channel map, a ragged volume)."""
import ctypes
import functools

import pytest
import torch

from util import gen, onehot_target

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _lib():
    from ctunet_amd import _lib
    return _lib


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f"{what}: {int((_bits(a) != _bits(b)).sum())} words differ"


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


def _rand(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=gen(seed)) * scale).cuda()


def _check(rc, what):
    _lib().check(rc, what)


def _st():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------ a small finalize for the jobs to ride on
@functools.lru_cache(maxsize=None)
def _fin_inputs(c, cp, nb, seed=7):
    """(partials [nb][2][cp], gamma, invstd, mean) of a BatchNorm-backward finalize; left unchanged."""
    return (_rand((nb, 2, cp), seed), _rand((c,), seed + 1), _rand((cp,), seed + 2).abs() + 0.5, _rand((cp,), seed + 3))


def _finalize(c, cp, nb, replay, jobs=None, njobs=0, merged=True):
    """One finalize through ctu_bn_bwd_finalize (merged=False) or ctu_bn_bwd_finalize_jobs -> every tensor it writes."""
    lib = _lib().load()
    partials, gamma, invstd, mean = _fin_inputs(c, cp, nb)
    dgamma, dbeta, coef = _nan(c), _nan(c), _nan(5, cp)
    rm = rv = nbt = None
    if replay:
        rm, rv = _rand((c,), 21), _rand((c,), 22).abs() + 0.1
        nbt = torch.tensor([5], dtype=torch.int64, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    args = (partials.data_ptr(), nb, c, cp, 4096.0, gamma.data_ptr(), invstd.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
            coef.data_ptr(), mean.data_ptr(), p(rm), p(rv), 0.1, 1e-5, p(nbt))
    if merged:
        rc = lib.ctu_bn_bwd_finalize_jobs(*args, jobs, njobs, _st())
    else:
        rc = lib.ctu_bn_bwd_finalize(*args, _st())
    out = dict(dgamma=dgamma, dbeta=dbeta, coef=coef)
    if replay:
        out.update(running_mean=rm, running_var=rv, num_batches_tracked=nbt)
    return rc, out


def _job_array(jobs):
    L = _lib()
    return (L.WgradJob * max(len(jobs), 1))(*jobs), len(jobs)


def _run_jobs(jobs, how):
    """Launch the pending jobs: riding on a finalize ("merged") or through the stand-alone flush ("flush")."""
    arr, n = _job_array(jobs)
    if how == "merged":
        rc, _ = _finalize(5, 8, 7, False, arr, n)
        _check(rc, "bn_bwd_finalize_jobs")
    else:
        _check(_lib().load().ctu_wgrad_reduce_jobs(arr, n, _st()), "wgrad_reduce_jobs")


def _three_ways(family, expect_job=True):
    """family(mode) -> (outputs, job): mode "now" calls the immediate entry (job None), "slabs" the slabs-only entry.
    The deferred outputs must equal the immediate ones bit for bit, through the merged launch and through the flush."""
    ref, _ = family("now")
    torch.cuda.synchronize()
    for how in ("merged", "flush"):
        outs, job = family("slabs")
        assert bool(job.kind) == expect_job
        _run_jobs([job], how)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(ref, outs)):
            _same(a, b, f"{how} output {i}")
    return ref


# ------------------------------------------------------------------ families
def _cinv_of(segs, cin_p):
    pos = [start + q for cnt, start in segs for q in range(cnt)]
    cinv = torch.full((cin_p,), -1, dtype=torch.int32)
    cinv[pos] = torch.arange(len(pos), dtype=torch.int32)
    return cinv.cuda()


def _conv_family(dims, ci, co, cin_p, cout_p, segs=None, lazy=False, k=3, bias=False, seed=100):
    lib = _lib().load()
    n, d, h, w = dims
    x = _rand((n, d, h, w, cin_p), seed)
    g = _rand((n, d, h, w, cout_p), seed + 1)
    cinv = None if segs is None else _cinv_of(segs, cin_p)
    ws_n = lib.ctu_conv3d_wgrad_ws_floats(n, d, h, w, k, cin_p, cout_p)
    if lazy:
        assert lib.ctu_conv3d_wgrad_bn_supported(n, d, h, w, k, cin_p, cout_p)
        y, sc, sh, coef = _rand((n, d, h, w, cout_p), seed + 2), _rand((cout_p,), seed + 3), _rand((cout_p,), seed + 4), _rand((5, cout_p), seed + 5)

    def family(mode):
        dw, ws = _nan(co, ci, k, k, k), _nan(ws_n)
        db = _nan(co) if bias else None
        job = _lib().WgradJob()
        tail = () if mode == "now" else (ctypes.byref(job),)
        cp = None if cinv is None else cinv.data_ptr()
        if lazy:
            gy = _nan(n, d, h, w, cout_p)
            fn = lib.ctu_conv3d_wgrad_bn if mode == "now" else lib.ctu_conv3d_wgrad_bn_slabs
            _check(fn(x.data_ptr(), cin_p, cin_p, None, None, 0, g.data_ptr(), cout_p, cout_p, y.data_ptr(), sc.data_ptr(),
                      sh.data_ptr(), coef.data_ptr(), gy.data_ptr(), dw.data_ptr(), co, ci, cp, ws.data_ptr(), n, d, h, w, k,
                      *tail, _st()), "conv3d_wgrad_bn")
            family.keep = (ws, gy)
            return (dw, gy), job
        fn = lib.ctu_conv3d_wgrad if mode == "now" else lib.ctu_conv3d_wgrad_slabs
        _check(fn(x.data_ptr(), cin_p, cin_p, None, None, 0, g.data_ptr(), cout_p, cout_p, dw.data_ptr(),
                  None if db is None else db.data_ptr(), co, ci, cp, ws.data_ptr(), n, d, h, w, k, *tail, _st()), "conv3d_wgrad")
        family.keep = (ws,)
        return ((dw, db) if bias else (dw,)), job
    return family


def _first_family(dims, cin, co, lazy=False, seed=200):
    lib = _lib().load()
    n, d, h, w = dims
    x = _rand((n, cin, d, h, w), seed)
    g = _rand((n, d, h, w, 8), seed + 1)
    ws_n = lib.ctu_conv3d_first_wgrad_ws_floats(n, d, h, w, cin)
    y, sc, sh, coef = _rand((n, d, h, w, 8), seed + 2), _rand((8,), seed + 3), _rand((8,), seed + 4), _rand((5, 8), seed + 5)

    def family(mode):
        dw, ws = _nan(co, cin, 3, 3, 3), _nan(ws_n)
        job = _lib().WgradJob()
        tail = () if mode == "now" else (ctypes.byref(job),)
        family.keep = (ws,)
        if lazy:
            gy = _nan(n, d, h, w, 8)
            fn = lib.ctu_conv3d_first_wgrad_bn if mode == "now" else lib.ctu_conv3d_first_wgrad_bn_slabs
            _check(fn(x.data_ptr(), cin, g.data_ptr(), 8, y.data_ptr(), sc.data_ptr(), sh.data_ptr(), coef.data_ptr(),
                      gy.data_ptr(), dw.data_ptr(), co, ws.data_ptr(), n, d, h, w, *tail, _st()), "conv3d_first_wgrad_bn")
            return (dw, gy), job
        fn = lib.ctu_conv3d_first_wgrad if mode == "now" else lib.ctu_conv3d_first_wgrad_slabs
        _check(fn(x.data_ptr(), cin, g.data_ptr(), 8, dw.data_ptr(), co, ws.data_ptr(), n, d, h, w, *tail, _st()),
               "conv3d_first_wgrad")
        return (dw,), job
    return family


def _convt_family(dims, ci, co, cin_p, cout_p, seed=300):
    lib = _lib().load()
    n, d, h, w = dims
    x = _rand((n, d, h, w, cin_p), seed)
    g = _rand((n, 2 * d, 2 * h, 2 * w, cout_p), seed + 1)
    ws_n = lib.ctu_convt2_wgrad_ws_floats(n, d, h, w, cin_p, cout_p)

    def family(mode):
        dw, db, ws = _nan(ci, co, 2, 2, 2), _nan(co), _nan(ws_n)
        job = _lib().WgradJob()
        tail = () if mode == "now" else (ctypes.byref(job),)
        fn = lib.ctu_convt2_wgrad if mode == "now" else lib.ctu_convt2_wgrad_slabs
        _check(fn(x.data_ptr(), cin_p, cin_p, None, None, 0, g.data_ptr(), cout_p, cout_p, dw.data_ptr(), db.data_ptr(), ci, co,
                  None, ws.data_ptr(), n, d, h, w, *tail, _st()), "convt2_wgrad")
        family.keep = (ws,)
        return (dw, db), job
    return family


# (dims, Ci, Co, cin_p, cout_p, segs): the k = 3 instantiations <SM, SN> by padded channel counts
K3S_CASES = {
    "22_one_box": ((1, 4, 4, 16), 8, 8, 8, 8, None),
    "22_gx": ((1, 8, 8, 32), 8, 8, 8, 8, None),
    "12_one_box": ((1, 4, 4, 16), 16, 8, 16, 8, None),
    "12_boxes": ((1, 8, 8, 16), 16, 8, 16, 8, None),
    "21_one_box": ((1, 4, 4, 16), 8, 16, 8, 16, None),
    "21_boxes": ((1, 8, 8, 16), 8, 16, 8, 16, None),
    "11_16_16": ((1, 8, 8, 16), 16, 16, 16, 16, None),
    "11_32_16": ((1, 8, 8, 16), 32, 16, 32, 16, None),                   # two ci groups: pairs > 1
    "11_map_12_of_16": ((1, 8, 8, 16), 12, 13, 16, 16, ((6, 0), (6, 8))),  # concat input: cinv, Ci < cin_p, Co < cout_p
}


@pytest.mark.parametrize("name", list(K3S_CASES))
def test_k3s_reduction_deferred_equals_immediate(name):
    dims, ci, co, cin_p, cout_p, segs = K3S_CASES[name]
    (dw,) = _three_ways(_conv_family(dims, ci, co, cin_p, cout_p, segs))
    assert torch.isfinite(dw).all()                      # every element of dW is written


@pytest.mark.parametrize("name", [n for n in K3S_CASES if "map" not in n])
def test_k3s_lazy_reduction_deferred_equals_immediate(name):
    dims, ci, co, cin_p, cout_p, segs = K3S_CASES[name]
    dw, gy = _three_ways(_conv_family(dims, ci, co, cin_p, cout_p, segs, lazy=True))
    assert torch.isfinite(dw).all() and torch.isfinite(gy).all()


def test_k3s_ragged_volume():
    (dw,) = _three_ways(_conv_family((1, 5, 6, 18), 16, 8, 16, 8))
    assert torch.isfinite(dw).all()


def test_many_slabs_per_thread():
    """The deferred bodies issue 16 loads before their adds (the stand-alone kernels one): 420 slabs walk every stage of that
    loop -- one round of 16 terms, two of 4, then single terms, the last of them only on the first four thread groups."""
    for fam in (_conv_family((1, 60, 56, 160), 8, 8, 8, 8), _conv_family((1, 60, 56, 80), 16, 16, 16, 16),
                _first_family((1, 60, 56, 64), 1, 8), _convt_family((1, 28, 30, 32), 16, 16, 16, 16)):
        outs, job = fam("slabs")
        assert job.gx == 420
        _run_jobs([job], "flush")
        torch.cuda.synchronize()
        ref, _ = fam("now")
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(ref, outs)):
            _same(a, b, f"kind {job.kind} output {i}")
            assert torch.isfinite(a).all()
        outs, job = fam("slabs")
        _run_jobs([job], "merged")
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(ref, outs)):
            _same(a, b, f"merged, kind {job.kind} output {i}")


def test_routes_without_a_deferred_form_reduce_immediately():
    """k = 5 and a conv bias gradient (its channel sum reuses ws): the slabs entry reduces at once and returns an empty job,
    which both launches skip."""
    _three_ways(_conv_family((1, 4, 4, 16), 8, 8, 8, 8, k=5), expect_job=False)
    dw, db = _three_ways(_conv_family((1, 4, 4, 16), 8, 8, 8, 8, bias=True), expect_job=False)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()


@pytest.mark.parametrize("cin,co,dims,lazy", [(1, 8, (1, 4, 4, 32), False), (2, 7, (1, 4, 4, 32), False),
                                              (1, 8, (1, 8, 8, 32), True), (2, 7, (1, 8, 8, 32), True),
                                              (1, 5, (1, 8, 8, 32), False), (2, 8, (1, 8, 8, 32), False)])
def test_first_layer_reduction_deferred_equals_immediate(cin, co, dims, lazy):
    outs = _three_ways(_first_family(dims, cin, co, lazy))
    assert all(torch.isfinite(t).all() for t in outs)


@pytest.mark.parametrize("side,c", [(4, 16), (8, 16), (4, 32)])      # (32 channels: the <2, 2> tile, 32 tiles per slab)
def test_convt_reduction_deferred_equals_immediate(side, c):
    dw, db = _three_ways(_convt_family((1, side, side, side), c, c, c, c))
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()


# ------------------------------------------------------------------ the finalize half
@pytest.mark.parametrize("c,cp", [(5, 8), (16, 16), (64, 64)])
@pytest.mark.parametrize("nb", [1, 7, 513])
@pytest.mark.parametrize("replay", [False, True])
def test_finalize_half_of_the_merged_launch(c, cp, nb, replay):
    """ctu_bn_bwd_finalize alone == ctu_bn_bwd_finalize_jobs with no job (the same kernel) == with a job riding (the merged
    kernel's first cp blocks): dgamma, dbeta, the five coefficient rows and the replayed running statistics."""
    rc, ref = _finalize(c, cp, nb, replay, merged=False)
    _check(rc, "bn_bwd_finalize")
    rc, none = _finalize(c, cp, nb, replay, None, 0)
    _check(rc, "bn_bwd_finalize_jobs")
    outs, job = _conv_family((1, 4, 4, 16), 8, 8, 8, 8)("slabs")
    arr, n = _job_array([job])
    rc, merged = _finalize(c, cp, nb, replay, arr, n)
    _check(rc, "bn_bwd_finalize_jobs")
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all() and torch.isfinite(ref["coef"]).all()
    for key, t in ref.items():
        assert torch.equal(t.view(-1).view(torch.int32 if t.dtype == torch.float32 else torch.int64),
                           none[key].view(-1).view(torch.int32 if t.dtype == torch.float32 else torch.int64)), ("njobs=0", key)
        assert torch.equal(t.view(-1).view(torch.int32 if t.dtype == torch.float32 else torch.int64),
                           merged[key].view(-1).view(torch.int32 if t.dtype == torch.float32 else torch.int64)), ("merged", key)
    if replay:
        assert int(ref["num_batches_tracked"]) == 6


# ------------------------------------------------------------------ several jobs, bad arguments
def _mixed_families():
    return [_conv_family((1, 8, 8, 32), 8, 8, 8, 8), _first_family((1, 8, 8, 32), 2, 7),
            _conv_family((1, 8, 8, 16), 32, 16, 32, 16, seed=120), _convt_family((1, 4, 4, 4), 16, 16, 16, 16)]


@pytest.mark.parametrize("njobs", [2, 4])
@pytest.mark.parametrize("how", ["merged", "flush"])
def test_several_jobs_of_different_kinds_in_one_launch(njobs, how):
    fams = _mixed_families()[:njobs]
    refs = [f("now")[0] for f in fams]
    pend, keep = [], []
    for f in fams:
        outs, job = f("slabs")
        assert job.kind
        pend.append((outs, job))
        keep.append(f.keep)
    _run_jobs([j for _, j in pend], how)
    torch.cuda.synchronize()
    for fi, (ref, (outs, _)) in enumerate(zip(refs, pend)):
        for i, (a, b) in enumerate(zip(ref, outs)):
            _same(a, b, f"job {fi} output {i}")


def test_bad_job_tables_are_refused_and_launch_nothing():
    L = _lib()
    lib = L.load()
    outs, job = _conv_family((1, 4, 4, 16), 8, 8, 8, 8)("slabs")
    too_many = (L.WgradJob * 5)(*([job] * 5))
    assert lib.ctu_wgrad_reduce_jobs(too_many, 5, _st()) != 0
    rc, fin = _finalize(5, 8, 7, False, too_many, 5)
    assert rc != 0 and b"njobs" in lib.ctu_last_error()
    bad = L.WgradJob.from_buffer_copy(job)
    bad.ws = None
    arr, n = _job_array([bad])
    assert lib.ctu_wgrad_reduce_jobs(arr, n, _st()) != 0
    rc2, fin2 = _finalize(5, 8, 7, False, arr, n)
    assert rc2 != 0
    assert lib.ctu_wgrad_reduce_jobs(None, -1, _st()) != 0 and lib.ctu_wgrad_reduce_jobs(None, 1, _st()) != 0
    torch.cuda.synchronize()
    # nothing ran: dW still holds the NaN fill, and so does what the refused finalize launches would have written
    assert torch.isnan(outs[0]).all()
    for f in (fin, fin2):
        assert all(torch.isnan(t).all() for t in f.values())
    _run_jobs([job], "flush")                       # the job itself is sound
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all()


# ------------------------------------------------------------------ engine level
class _RecordingSync:
    """Stands in for parallel.GradSync: keeps a copy of every gradient as it is pushed (block boundaries of backward)."""

    def __init__(self):
        self.seen = {}

    def push(self, named):
        for name, g in named:
            self.seen[name] = g.detach().clone()

    def finish(self):
        return {}


def _engine_backward(make, in_ch, defer, with_sync, monkeypatch):
    from ctunet_amd import engine as E
    monkeypatch.setattr(E, "DEFER_WGRAD_REDUCE", defer)
    torch.manual_seed(0)
    net = make().cuda().train()
    x = torch.randn(1, in_ch, 32, 32, 32, generator=gen(3)).cuda()
    g0 = torch.randn(1, 2, 32, 32, 32, generator=gen(4)).cuda()
    eng = net._engine()
    P = E._tensor_dict(net)
    sync = _RecordingSync() if with_sync else None
    with torch.no_grad():
        out0, out1, ctx = eng.forward(P, x, True, True, bool(getattr(net, "chk", False)))
        assert out1 is None
        grads, dx = eng.backward(P, ctx, g0, None, True, sync)
    torch.cuda.synchronize()
    res = {k: v.detach().clone() for k, v in grads.items() if v is not None}
    res["__dx__"] = dx.detach().clone()
    if sync is not None:
        res.update({"pushed:" + k: v for k, v in sync.seen.items()})
    return res


def _net_makers():
    import ctunet_amd
    return {"UNet": lambda: ctunet_amd.UNet(), "UNet_add": lambda: ctunet_amd.UNet(cat=False)}


@pytest.mark.parametrize("with_sync", [False, True], ids=["plain", "sync"])
@pytest.mark.parametrize("name", ["UNet", "UNet_add"])
def test_engine_backward_is_bitwise_the_same_with_and_without_deferral(name, with_sync, monkeypatch):
    make = _net_makers()[name]
    on = _engine_backward(make, 1, True, with_sync, monkeypatch)
    off = _engine_backward(make, 1, False, with_sync, monkeypatch)
    assert set(on) == set(off) and len(on) > 20
    for k in on:
        _same(on[k], off[k], k)
        assert torch.isfinite(on[k]).all(), k
    if with_sync:                                   # what a gradient exchange is handed at a block boundary is final
        for k in on:
            if k.startswith("pushed:"):
                _same(on[k], on[k[len("pushed:"):]], k)


def _graphed(defer, dtype, monkeypatch, replays=3):
    import ctunet_amd
    from ctunet_amd import engine as E, optim
    from ctunet_amd.graph import GraphedTrainStep
    monkeypatch.setattr(E, "DEFER_WGRAD_REDUCE", defer)
    torch.manual_seed(0)
    net = ctunet_amd.UNet().cuda().train()
    if dtype != torch.float32:
        net.set_precision(dtype)
    x = torch.randn(1, 1, 32, 32, 32, generator=gen(5)).cuda()
    t = onehot_target((1, 2, 32, 32, 32), 6, 0.3).cuda()
    opt = optim.Adam(net.parameters(), lr=1e-3, amsgrad=True)
    gs = GraphedTrainStep(net, opt, x, [t], 1.0, 1.0, warmup=1)
    losses = [gs(x, [t]).clone() for _ in range(replays)]
    torch.cuda.synchronize()
    return losses, {k: v.detach().clone() for k, v in net.state_dict().items()}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_graphed_step_is_bitwise_the_same_with_and_without_deferral(dtype, monkeypatch):
    """Three replays of the captured step: loss terms, parameters and BatchNorm buffers.  bf16: the 16-bit path never
    defers, so the switch changes nothing there either."""
    l_on, sd_on = _graphed(True, dtype, monkeypatch)
    l_off, sd_off = _graphed(False, dtype, monkeypatch)
    for a, b in zip(l_on, l_off):
        _same(a, b, "loss terms")
        assert torch.isfinite(a).all()
    for k in sd_on:
        assert torch.equal(sd_on[k], sd_off[k]), k
