"""Weight-space kernels around the fused up-convolution (csrc/upconv_fused.hip): the pack chain (transposes -> composite
weights + border-class bias -> gathers into the PW and data-gradient packings) and the projection chain (gradient sums ->
V -> dWT, dbT, dW3).

Every output buffer the test hands in is pre-filled with NaN: an element a launch does not write fails the comparison.
The gathers are checked exactly, by index arithmetic on the returned standard packing; the sums against fp64 references
built here from the torch-layout tensors (tolerances of tests/test_ops_gpu.py's fused up-convolution tests: 1e-4 of the
scale for the composite, 2e-4 for the projected gradients, 2e-3 for the 16-bit projection as in tests/test_lowp_gpu.py).
The volume only matters to the face sums, so the coarse volume is one 4 x 4 x 16 box (every voxel on a face)."""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")

# (C, C_out, cin_p, nout_p, segments (count, start) of the padded input layout | None, coarse dims)
CASES = {
    "pw_8_8": (8, 8, 8, 8, None, (1, 4, 4, 16)),                            # PW path; cin_p % 16 == 8: zero positions in wpd
    "top_32_8": (32, 8, 32, 8, None, (1, 4, 4, 16)),                        # flagship top block
    "lvl1_64_16": (64, 16, 64, 16, None, (1, 4, 4, 16)),                    # flagship level 1
    "mapped_24_16": (24, 16, 32, 16, ((12, 0), (12, 16)), (1, 4, 4, 16)),   # mapped positions
    "sp_56_14": (56, 14, 64, 16, ((28, 0), (28, 32)), (1, 4, 4, 16)),       # UNetSP channels; C_out not a multiple of 4
    "guard_16_6": (16, 6, 16, 8, None, (1, 4, 4, 16)),                      # co + q < Co guards
    "n32_16_32": (16, 32, 16, 32, None, (1, 4, 4, 16)),                     # nout_p 32
    "n64_16_64": (16, 64, 16, 64, None, (1, 4, 4, 16)),                     # nout_p 64
    "batch2_32_8": (32, 8, 32, 8, None, (2, 8, 4, 16)),                     # non-cubic, batch 2
}
IDS = list(CASES)


def _ops():
    from ctunet_amd import ops
    return ops


def _lib():
    from ctunet_amd import _lib
    return _lib


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _axis(p, t):
    """One axis of the composite: fine voxel 2i + p, conv tap t reads fine position 2i + p + t - 1 = 2i' + a of the transposed
    conv's output -> (transposed-conv tap a, tap bit j of the 2-wide coarse window that starts at i + p - 1)."""
    s = p + t - 1
    a, d = s % 2, s // 2
    return a, d - (p - 1)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs (CPU, fp32) and the fp64 references of one case, computed once and left unchanged."""
    c, co, cin_p, nout_p, segs, dims = CASES[name]
    n, d, h, w = dims
    seed = 1000 + 10 * IDS.index(name)
    wt = torch.randn(c, c, 2, 2, 2, generator=_gen(seed)) * 0.2
    bt = torch.randn(c, generator=_gen(seed + 1))
    w3 = torch.randn(co, c, 3, 3, 3, generator=_gen(seed + 2)) * 0.1
    x = torch.randn(n, c, d, h, w, generator=_gen(seed + 3))
    dy = torch.randn(n, co, 2 * d, 2 * h, 2 * w, generator=_gen(seed + 4))
    pos = list(range(c)) if segs is None else [start + q for cnt, start in segs for q in range(cnt)]
    # composite weights [parity 8][tap 8][padded position][nout_p] and the 27 border-class biases, fp64
    weff = torch.zeros(8, 8, cin_p, nout_p, dtype=torch.float64)
    wt64, bt64, w364 = wt.double(), bt.double(), w3.double()
    for pz in range(2):
        for py in range(2):
            for px in range(2):
                for tz in range(3):
                    for ty in range(3):
                        for tx in range(3):
                            (az, jz), (ay, jy), (ax, jx) = _axis(pz, tz), _axis(py, ty), _axis(px, tx)
                            weff[pz * 4 + py * 2 + px, jz * 4 + jy * 2 + jx][pos, :co] += wt64[:, :, az, ay, ax] @ w364[:, :, tz, ty, tx].T
    s = torch.einsum("m,omzyx->zyxo", bt64, w364)                      # S[t][co]
    beff = torch.zeros(27, nout_p, dtype=torch.float64)
    keep = ([0, 1, 2], [1, 2], [0, 1])                                 # per axis: interior / first fine voxel / last
    for cz in range(3):
        for cy in range(3):
            for cx in range(3):
                beff[(cz * 3 + cy) * 3 + cx, :co] = s[keep[cz]][:, keep[cy]][:, :, keep[cx]].sum((0, 1, 2))
    # parameter gradients: fp64 autograd of the two unfused ops
    g64 = [t.clone().requires_grad_(True) for t in (wt64, bt64, w364)]
    F.conv3d(F.conv_transpose3d(x.double(), g64[0], g64[1], stride=2), g64[2], padding=1).backward(dy.double())
    return SimpleNamespace(name=name, c=c, co=co, cin_p=cin_p, nout_p=nout_p, dims=dims, pos=pos, mapped=segs is not None,
                           wt=wt, bt=bt, w3=w3, x=x, dy=dy, weff=weff, beff=beff, grads=tuple(t.grad for t in g64))


def _maps(k):
    return _maps_of(k.name)


@functools.lru_cache(maxsize=None)
def _maps_of(name):
    """(cinv: padded position -> logical channel, imap: logical channel -> padded position) on the GPU, None = identity."""
    k = _case(name)
    if not k.mapped:
        return None, None
    cinv = torch.full((k.cin_p,), -1, dtype=torch.int32)
    cinv[k.pos] = torch.arange(k.c, dtype=torch.int32)
    return cinv.cuda(), torch.tensor(k.pos, dtype=torch.int32).cuda()


def _nan_bufs(k, with_wpd=True):
    lib = _lib().load()
    sizes = [lib.ctu_upconv_fused_packed_floats(k.cin_p, k.nout_p), (27, k.nout_p), lib.ctu_upconv_fused_pack_ws_floats(k.c, k.nout_p)]
    if with_wpd:
        sizes.append(lib.ctu_upconv_fused_bwd_packed_floats(k.cin_p, k.nout_p))
    return tuple(torch.full(s if isinstance(s, tuple) else (s,), NAN, device="cuda") for s in sizes)


def _pack(k, wts=None, into=None):
    """pack_all into NaN-filled (or the given) buffers -> (wp, beff, ws, wpd)"""
    wt, bt, w3 = wts if wts is not None else (k.wt.cuda(), k.bt.cuda(), k.w3.cuda())
    return _ops().upconv_fused_pack_all(wt, bt, w3, _maps(k)[0], k.cin_p, k.nout_p, into if into is not None else _nan_bufs(k))


def _std(k, wp):
    """the standard packing wp[chunk][parity][tap][ntp][kq][n][j] un-permuted to W_eff[parity][tap][position][ntp * 16]"""
    ntpt = (k.nout_p + 15) // 16
    std = wp[:(k.cin_p // 8) * 64 * ntpt * 128].view(k.cin_p // 8, 8, 8, ntpt, 4, 16, 2)
    return std.permute(1, 2, 0, 4, 6, 3, 5).reshape(8, 8, k.cin_p, ntpt * 16)


def _wpd_from(k, w):
    """wpd[parity][q][e][n16][kq][n][j] = W_eff[parity][tap = e ^ 7][position n16 * 16 + n][co = q * 8 + kq * 2 + j], 0 past cin_p"""
    n16 = (k.cin_p + 15) // 16
    wpad = torch.zeros(8, 8, n16 * 16, k.nout_p, device=w.device)
    wpad[:, :, :k.cin_p] = w[..., :k.nout_p]
    v = wpad.flip(1).view(8, 8, n16, 16, k.nout_p // 8, 4, 2)          # [parity][e][n16][n][q][kq][j]
    return v.permute(0, 4, 1, 2, 5, 3, 6).reshape(-1)


def _pw_from(k, w):
    """wpw[chunk][par4][tap12 = (dz * 2 + dy) * 3 + dxx][kq][n = px * 8 + co][j] = W_eff[par4 * 2 + px][(dz * 2 + dy) * 2 + dxx - px]
    [position chunk * 8 + kq * 2 + j][co] where dxx - px is 0 or 1, else 0"""
    nchunk = k.cin_p // 8
    out = torch.zeros(nchunk, 4, 4, 3, 4, 2, 8, 2, device=w.device)    # [chunk][par4][dzy][dxx][kq][px][co][j]
    wv = w[..., :8].reshape(4, 2, 4, 2, nchunk, 4, 2, 8)               # [par4][px][dzy][jx][chunk][kq][j][co]
    for px in range(2):
        for jx in range(2):
            out[:, :, :, jx + px, :, px] = wv[:, px, :, jx].permute(2, 0, 1, 3, 5, 4)
    return out.reshape(-1)


@pytest.mark.parametrize("name", IDS)
def test_pack_writes_every_buffer_gathers_exact_composite_close(name):
    """One pack_all call: no element of wp / beff / ws / wpd keeps its NaN; wpd and the PW packing are exact gathers of the
    standard packing (zeros included); unmapped and padded entries of the standard packing are exact zeros; W_eff and b_eff
    match the fp64 composite to 1e-4 of their scale; the two older entry points return the same bits."""
    ops = _ops()
    k = _case(name)
    wp, beff, ws, wpd = _pack(k)
    for nm, t in (("wp", wp), ("beff", beff), ("ws", ws), ("wpd", wpd)):
        assert not torch.isnan(t).any(), nm
    w = _std(k, wp)
    assert torch.equal(wpd, _wpd_from(k, w))
    if k.nout_p == 8:
        assert torch.equal(wp[(k.cin_p // 8) * 64 * 128:], _pw_from(k, w))
    dead = torch.ones(k.cin_p, dtype=torch.bool)
    dead[k.pos] = False
    assert (w[:, :, dead.cuda()] == 0).all() and (w[..., k.co:] == 0).all()
    err = (w[..., :k.nout_p].double().cpu() - k.weff).abs().max().item()
    assert err <= 1e-4 * k.weff.abs().max().item(), err
    assert (beff[:, k.co:] == 0).all()
    err = (beff.double().cpu() - k.beff).abs().max().item()
    assert err <= 1e-4 * k.beff.abs().max().item(), err
    wp2, beff2, ws2 = ops.upconv_fused_pack(k.wt.cuda(), k.bt.cuda(), k.w3.cuda(), _maps(k)[0], k.cin_p, k.nout_p, _nan_bufs(k, False))
    wpd2 = ops.upconv_fused_pack_bwd(wp2, k.cin_p, k.nout_p, torch.full_like(wpd, NAN))
    assert torch.equal(wp2, wp) and torch.equal(beff2, beff) and torch.equal(ws2, ws) and torch.equal(wpd2, wpd)


def _inputs(k, dtype=torch.float32):
    """(coarse input CL, fine-grid gradient CL) of the case on the GPU"""
    ops = _ops()
    n, d, h, w = k.dims
    buf = torch.zeros(n, d, h, w, k.cin_p)
    buf[..., k.pos] = k.x.permute(0, 2, 3, 4, 1)
    gbuf = torch.zeros(n, 2 * d, 2 * h, 2 * w, k.nout_p)
    gbuf[..., :k.co] = k.dy.permute(0, 2, 3, 4, 1)
    return ops.CL(buf.to(dtype).cuda(), 0, k.cin_p), ops.CL(gbuf.to(dtype).cuda(), 0, k.nout_p)


def _project(k, xc, gc, bt, pws):
    """composite-weight gradient, then ctu_upconv_fused_project into NaN-filled outputs and scratch -> (dwt, dbt, dw3)"""
    lib = _lib().load()
    check = _lib().check
    n, d, h, w = k.dims
    st = torch.cuda.current_stream().cuda_stream
    new = lambda *s: torch.full(s, NAN, device="cuda")
    dweff = new(8, 8, k.cin_p, k.nout_p)
    ws = new(lib.ctu_upconv_fused_wgrad_ws_floats(n, d, h, w, k.cin_p, k.nout_p))
    check(lib.ctu_upconv_fused_wgrad(xc.ptr, xc.cs, xc.cp, None, None, 0, gc.ptr, gc.cs, gc.cp, dweff.data_ptr(), ws.data_ptr(),
                                     n, d, h, w, st), "upconv_fused_wgrad")
    dwt, dbt, dw3 = new(k.c, k.c, 2, 2, 2), new(k.c), new(k.co, k.c, 3, 3, 3)
    ws2 = new(lib.ctu_upconv_fused_project_ws_floats(k.nout_p, gc.nvox))
    imap = _maps(k)[1]
    check(lib.ctu_upconv_fused_project(dweff.data_ptr(), gc.ptr, gc.cs, gc.cp, n, d, h, w, bt.data_ptr(), pws.data_ptr(),
                                       None if imap is None else imap.data_ptr(), k.c, k.co, k.cin_p, dwt.data_ptr(),
                                       dbt.data_ptr(), dw3.data_ptr(), ws2.data_ptr(), st), "upconv_fused_project")
    return dwt, dbt, dw3


@pytest.mark.parametrize("name", IDS)
def test_projection_matches_fp64_autograd(name):
    """dWT, dbT, dW3 (every element written) against fp64 autograd of ConvTranspose3d -> Conv3d, 2e-4 of each tensor's scale;
    ops.upconv_fused_wgrad returns the same bits."""
    ops = _ops()
    k = _case(name)
    pws = _pack(k)[2]
    xc, gc = _inputs(k)
    bt = k.bt.cuda()
    got = _project(k, xc, gc, bt, pws)
    for nm, t, want in zip(("dWT", "dbT", "dW3"), got, k.grads):
        err = (t.double().cpu() - want).abs().max().item()
        assert err <= 2e-4 * want.abs().max().item(), (nm, err, want.abs().max().item())       # (a NaN fails this too)
    again = ops.upconv_fused_wgrad(xc, gc, k.c, k.co, bt, pws, _maps(k)[1])
    assert all(torch.equal(a, b) for a, b in zip(again, got))


@pytest.mark.parametrize("lp", ["bf16", "fp16"])
def test_projection_from_16bit_gradient(lp):
    """The 16-bit instantiation of the gradient sums through ops.lp_upconv_fused_wgrad (32 -> 8 channels): fp64 autograd on the
    rounded activations and gradient, 2e-3 of each tensor's scale (tests/test_lowp_gpu.py's tolerance for this op)."""
    ops = _ops()
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[lp]
    k = _case("batch2_32_8")
    xr, dyr = k.x.to(dt).double(), k.dy.to(dt).double()
    g64 = [t.double().requires_grad_(True) for t in (k.wt, k.bt, k.w3)]
    F.conv3d(F.conv_transpose3d(xr, g64[0], g64[1], stride=2), g64[2], padding=1).backward(dyr)
    pws = _pack(k)[2]
    xc, gc = _inputs(k, dt)
    got = ops.lp_upconv_fused_wgrad(xc, gc, k.c, k.co, k.bt.cuda(), pws, None)
    for nm, t, want in zip(("dWT", "dbT", "dW3"), got, (t.grad for t in g64)):
        err = (t.double().cpu() - want).abs().max().item()
        assert err <= 2e-3 * want.abs().max().item(), (nm, err, want.abs().max().item())


@pytest.mark.parametrize("name", ["pw_8_8", "mapped_24_16"])
def test_repack_in_place(name):
    """A second pack with into= and other weights: same pointers, and the bits of a fresh pack of those weights (nothing relies
    on what the buffers held before)."""
    k = _case(name)
    bufs = _pack(k)
    ptrs = [t.data_ptr() for t in bufs]
    other = tuple((t * 1.5 + 0.01).cuda() for t in (k.wt, k.bt, k.w3))
    again = _pack(k, other, bufs)
    assert [t.data_ptr() for t in again] == ptrs
    fresh = _pack(k, other)
    assert all(torch.equal(a, b) for a, b in zip(again, fresh))


@pytest.mark.parametrize("name", ["top_32_8", "sp_56_14"])
def test_pack_and_projection_replay_from_a_graph(name):
    """Pack and projection captured once; after each in-place change of the weights a replay gives the eager bits."""
    ops = _ops()
    k = _case(name)
    wts = tuple(t.cuda() for t in (k.wt, k.bt, k.w3))
    xc, gc = _inputs(k)
    bufs = _nan_bufs(k)
    imap = _maps(k)[1]

    def run():
        _pack(k, wts, bufs)
        return ops.upconv_fused_wgrad(xc, gc, k.c, k.co, wts[1], bufs[2], imap)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                         # warm-up: library loaded, kernels resident
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.gc_paused(), torch.cuda.graph(graph):
        outs = run()
    for step in (1, 2):
        for t in wts:
            t.mul_(1.0 + 0.25 * step).add_(0.01 * step)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in bufs + tuple(outs)]
        eager_bufs = _pack(k, wts)
        eager = eager_bufs + tuple(ops.upconv_fused_wgrad(xc, gc, k.c, k.co, wts[1], eager_bufs[2], imap))
        assert all(torch.equal(a, b) for a, b in zip(replayed, eager)), step
