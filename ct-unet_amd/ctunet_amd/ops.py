"""Thin tensor-level wrappers over the C ABI (include/ctunet_hip.h).

PyTorch is plumbing here: it owns device memory and the stream; every computation is a call into
libctunet_hip.so.  All functions require CUDA (ROCm) tensors and raise otherwise -- there is no
CPU path.

``CL`` describes a channels-last activation: a slice ``[c0, c0+cp)`` of the channels of a
contiguous ``[N, D, H, W, cs]`` fp32 buffer plus its lazy-BN transform (``scale``/``shift`` over
the slice, ``relu``): consumers see ``relu(raw * scale + shift)``.
"""
from __future__ import annotations

import contextlib
import ctypes
import gc
import os

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import _lib


def pad8(c: int) -> int:
    return (c + 7) // 8 * 8


LP_CODE = {torch.bfloat16: 1, torch.float16: 2}          # CTU_BF16 / CTU_F16 of include/ctunet_hip.h
ACT_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _need_cuda(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"ctunet_amd: {name} must live on the GPU (MI355X); this path has no CPU fallback")
    if t.dtype != torch.float32 and t.dtype != torch.int32:
        raise RuntimeError(f"ctunet_amd: {name} must be float32, got {t.dtype}")


def _ptr(t: Optional[torch.Tensor], off_elems: int = 0):
    if t is None:
        return None
    return t.data_ptr() + t.element_size() * off_elems


def _dual(code: int, name: str, *args) -> None:
    """ctu_<name>(args) for fp32 tensors, ctu_lp_<name>(dtype code, args) for 16-bit ones (same argument lists)."""
    entries = _LP_ENTRIES if code else _ENTRIES
    fn = entries.get(name)
    if fn is None:
        fn = entries[name] = getattr(_lib.load(), ("ctu_lp_" if code else "ctu_") + name)
    status = fn(code, *args) if code else fn(*args)
    if status:
        _lib.check(status, ("lp_" if code else "") + name)


# entry points _dual has resolved, by name (every launch of a step passes through it: one dict look-up per call)
_ENTRIES: dict = {}
_LP_ENTRIES: dict = {}


def _query(code: int, name: str, *args):
    """Value of ctu_<name>(args) / ctu_lp_<name>(args): the geometry queries (*_ws_floats, *_supported) take no dtype code."""
    return getattr(_lib.load(), ("ctu_lp_" if code else "ctu_") + name)(*args)


def _tail_arg(tail):
    """ctypes argument of an optional ctu_bn_tail / ctu_bn_bwd_tail."""
    return None if tail is None else ctypes.byref(tail)


def _lp_name(code: int) -> str:
    return "bf16" if code == 1 else "f16"


def make_bn_tail(c: int, count, gamma, beta, rmean, rvar, momentum: float, eps: float, n_updates: int, vec4, nbt, counter):
    """ctu_bn_tail: the launch that writes the BatchNorm partial rows also finalizes them (no ctu_bn_finalize launch).
    vec4: [4, cp] rows receiving scale, shift, mean, invstd; counter: one zeroed int32 device word owned by the layer."""
    assert counter.dtype == torch.int32 and counter.is_cuda and counter.numel() == 1
    assert nbt is None or (nbt.dtype == torch.int64 and nbt.is_cuda and nbt.numel() == 1)
    t = _lib.BnTail()
    t.gamma, t.beta = gamma.data_ptr(), beta.data_ptr()
    t.running_mean, t.running_var = _ptr(rmean), _ptr(rvar)
    t.scale, t.shift, t.mean, t.invstd = (vec4[i].data_ptr() for i in range(4))
    t.num_batches_tracked = None if nbt is None else nbt.data_ptr()
    t.counter = counter.data_ptr()
    t.count, t.momentum, t.eps, t.C, t.n_updates = float(count), momentum, eps, c, n_updates
    return t


def _replay_args(replay):
    """(running_mean, running_var, momentum, eps, num_batches_tracked) of a replay= tuple as in bn_relu_bwd (None: no update)."""
    rm, rv, mom, eps, nbt = (tuple(replay) + (None,))[:5] if replay is not None else (None, None, 0.0, 0.0, None)
    assert nbt is None or (nbt.dtype == torch.int64 and nbt.is_cuda and nbt.numel() == 1)
    return rm, rv, mom, eps, nbt


def make_bn_bwd_tail(c: int, count, gamma, vec4, dgb, coef, replay, counter):
    """ctu_bn_bwd_tail (replaces the ctu_bn_bwd_finalize launch); replay as in bn_relu_bwd."""
    assert counter is None or (counter.dtype == torch.int32 and counter.is_cuda and counter.numel() == 1)
    rm, rv, mom, eps, nbt = _replay_args(replay)
    t = _lib.BnBwdTail()
    t.gamma, t.invstd, t.mean = gamma.data_ptr(), vec4[3].data_ptr(), vec4[2].data_ptr()
    t.dgamma, t.dbeta, t.coef = dgb[0].data_ptr(), dgb[1].data_ptr(), coef.data_ptr()
    t.running_mean, t.running_var = _ptr(rm), _ptr(rv)
    t.num_batches_tracked = None if nbt is None else nbt.data_ptr()
    t.counter = None if counter is None else counter.data_ptr()
    t.count, t.momentum, t.eps, t.C = float(count), mom, eps, c
    return t


def _bn_bwd_outputs(c: int, cp: int, count, gamma, vec4, replay, counter, device, tail: bool = True):
    """(ctu_bn_bwd_tail | None, (dgb [2, c], coef [5, cp])): what a BatchNorm backward finalize writes, freshly allocated,
    and (tail=True) the struct that makes the launch writing the reduction rows finalize them into it."""
    dgb = torch.empty((2, c), dtype=torch.float32, device=device)
    coef = torch.empty((5, cp), dtype=torch.float32, device=device)
    return (make_bn_bwd_tail(c, count, gamma, vec4, dgb, coef, replay, counter) if tail else None), (dgb, coef)


def lp(t_or_dtype) -> int:
    """dtype code of the ctu_lp_* entry points for a 16-bit activation tensor / dtype; 0 for float32."""
    dt = t_or_dtype if isinstance(t_or_dtype, torch.dtype) else t_or_dtype.dtype
    return LP_CODE.get(dt, 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def gc_paused():
    """Cyclic garbage collection off for the length of a graph capture.  A dead object cycle can hold an earlier capture
    (a model keeps its sliding-window graph, whose window keeps the model); freed by the collector while another capture
    is under way, that graph's teardown makes HIP calls a capture forbids and the process aborts.  So collect first,
    outside the capture, and keep the collector off until the capture has ended."""
    was = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


class KernelTimer:
    """Optional HIP-event bracketing of individual launches (bench.py's roofline leg).

    Events are recorded on the stream the kernels are launched on (torch's current stream), so they
    time exactly one launch each.  ``records`` holds (tag, algorithmic_flops, algorithmic_bytes, start, end).
    """

    def __init__(self):
        self.records = []
        self.details = []
        self._empty = []           # event pairs around NOTHING, interleaved with the timed launches: the bracket's own cost

    def _overhead_ms(self) -> float:
        """Median elapsed time of the empty event pairs (recorded every 16th launch): what an event pair measures when
        there is no kernel between the two records (2-5 us on this stack) -- subtracted from every bracketed launch, so the
        per-launch figures agree with the kernel-trace durations of rocprofv3."""
        ts = sorted(a.elapsed_time(b) for a, b in self._empty)
        return ts[len(ts) // 2] if ts else 0.0

    def begin(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def end(self, tag, flops, nbytes, start, detail=None):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.records.append((tag, flops, nbytes, start, ev))
        self.details.append(detail)
        if len(self.records) % 16 == 1:
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            b.record()
            self._empty.append((a, b))

    def by_layer(self):
        """{(tag, detail): dict(launches, total_ms, flops)} -- per-geometry split of ``summary`` (dev tool)."""
        out = {}
        ovh = self._overhead_ms()
        for (tag, fl, nb, a, b), det in zip(self.records, self.details):
            d = out.setdefault((tag, det), dict(launches=0, total_ms=0.0, flops=0.0))
            d["launches"] += 1
            d["total_ms"] += max(a.elapsed_time(b) - ovh, 1e-4)
            d["flops"] += fl
        return out

    def summary(self):
        """{tag: dict(launches, total_ms, avg_ms, flops, bytes)} -- call after a device synchronize.
        A launch site (tag, geometry) is represented by the MEDIAN of its timed launches: a one-off stall that lands between
        an event pair (an allocator hipMalloc, RCCL's lazy channel set-up in the first eager distributed step: 73 ms once,
        measured) would otherwise be booked on whatever kernel happened to be bracketed."""
        sites = {}
        ovh = self._overhead_ms()
        for (tag, fl, nb, a, b), det in zip(self.records, self.details):
            sites.setdefault((tag, det, fl, nb), []).append(max(a.elapsed_time(b) - ovh, 1e-4))
        out = {}
        for (tag, det, fl, nb), ts in sites.items():
            ts.sort()
            med = ts[len(ts) // 2] if len(ts) % 2 else 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])
            d = out.setdefault(tag, dict(launches=0, total_ms=0.0, flops=0.0, bytes=0.0))
            d["launches"] += len(ts)
            d["total_ms"] += med * len(ts)
            d["flops"] += fl * len(ts)
            d["bytes"] += nb * len(ts)
        for d in out.values():
            d["avg_ms"] = d["total_ms"] / d["launches"]
        return out


TIMER: Optional[KernelTimer] = None      # set by bench.py; None in normal operation
# 16-bit first-layer weight gradient: volumes with at least this many voxels go through the matrix pipe (conv_first_wgrad)
FIRST_WGRAD_MFMA_MIN_VOX = int(os.environ.get("CTUNET_FIRST_WGRAD_MFMA_MIN_VOX", "4000000"))


class _timed:
    """``with _timed(record):`` around a launch site -- one TIMER record when TIMER is set, nothing otherwise.
    record() -> (tag, algorithmic flops, algorithmic bytes, detail) of what the bracket encloses; it is called only when
    timing, after the launch (so a ctu_*_kernel_name look-up or an f-string costs the normal path nothing)."""
    __slots__ = ("record", "t0")

    def __init__(self, record):
        self.record = record

    def __enter__(self):
        self.t0 = TIMER.begin() if TIMER is not None else None

    def __exit__(self, exc_type, exc, tb):
        if self.t0 is not None and exc_type is None:
            tag, flops, nbytes, detail = self.record()
            TIMER.end(tag, flops, nbytes, self.t0, detail)


class WgradJobs:
    """The fp32 weight-gradient slab reductions a backward pass has not launched yet (ctu_wgrad_job): nothing reads dW
    before the optimizer, so a weight-gradient call given ``jobs=`` leaves its reduction here, and the next bn_relu_bwd that
    launches a BatchNorm-backward finalize runs the pending ones in spare blocks of that launch.  flush() reduces what is
    pending in one launch of its own.  Each entry keeps its workspace and outputs alive until it has been launched."""

    def __init__(self):
        self.items = []                          # (WgradJob, (ws, dw, db, ...))

    def __len__(self) -> int:
        return len(self.items)

    def uses(self, ws: torch.Tensor) -> bool:
        """Does a pending reduction still read this workspace?"""
        return any(keep[0] is ws for _, keep in self.items)

    def add(self, job, ws: torch.Tensor, *outs) -> None:
        if not job.kind:                         # the entry reduced immediately (a route without a deferred form)
            return
        if len(self.items) == _lib.WGRAD_JOBS_MAX:
            self.flush()
        self.items.append((job, (ws,) + outs))

    def take(self):
        """(ctypes job array, count) of the pending reductions, which the caller launches now."""
        n = len(self.items)
        arr = (_lib.WgradJob * max(n, 1))(*(j for j, _ in self.items))
        self.items = []
        return arr, n

    def flush(self) -> None:
        if self.items:
            arr, n = self.take()
            _lib.check(_lib.load().ctu_wgrad_reduce_jobs(arr, n, _stream()), "wgrad_reduce_jobs")


def _deferred(jobs: Optional[WgradJobs], code: int = 0) -> bool:
    """Does a weight-gradient call leave its slab reduction in ``jobs``?  fp32 only, and not while launches are bracketed
    (the "(+slab reduce)" brackets of the stage table time the reduction with its kernel)."""
    return jobs is not None and not code and TIMER is None


@dataclass
class CL:
    buf: torch.Tensor                       # [N, D, H, W, cs] contiguous fp32
    c0: int = 0
    cp: int = 0                             # padded channels of this slice (multiple of 8)
    scale: Optional[torch.Tensor] = None    # [cp] (already sliced) or None
    shift: Optional[torch.Tensor] = None
    relu: bool = False

    def __post_init__(self):
        if self.cp == 0:
            self.cp = self.buf.shape[-1] - self.c0
        assert self.buf.dim() == 5 and self.buf.is_contiguous() and self.buf.dtype in ACT_DTYPES
        assert self.cp % 8 == 0 and self.c0 % 4 == 0 and self.c0 + self.cp <= self.buf.shape[-1]
        # 16-bit tensors: slices start on 16-byte boundaries and the voxel stride keeps them there
        assert self.buf.dtype == torch.float32 or (self.c0 % 8 == 0 and self.buf.shape[-1] % 8 == 0)

    @property
    def dtype(self) -> torch.dtype:
        return self.buf.dtype

    @property
    def lp(self) -> int:
        return LP_CODE.get(self.buf.dtype, 0)

    @property
    def cs(self) -> int:
        return self.buf.shape[-1]

    @property
    def dims(self) -> Tuple[int, int, int, int]:
        n, d, h, w, _ = self.buf.shape
        return n, d, h, w

    @property
    def nvox(self) -> int:
        n, d, h, w = self.dims
        return n * d * h * w

    @property
    def ptr(self):
        return _ptr(self.buf, self.c0)

    def slice(self, c0: int, cp: int) -> "CL":
        sc = None if self.scale is None else self.scale[c0:c0 + cp]
        sh = None if self.shift is None else self.shift[c0:c0 + cp]
        return CL(self.buf, self.c0 + c0, cp, sc, sh, self.relu)

    def raw(self) -> "CL":
        return CL(self.buf, self.c0, self.cp)

    def with_xf(self, scale, shift, relu=True) -> "CL":
        return CL(self.buf, self.c0, self.cp, scale, shift, relu)


@dataclass
class CL2:
    """A channels-last tensor of 2 * a.cp padded channels kept in two slices of equal width: ``a`` holds channels
    [0, a.cp), ``b`` holds [a.cp, 2 * a.cp).  Only the head reads or writes a whole voxel of the top-level concat buffer and
    only the fused up-convolution one of the level below, so their halves can be two dense tensors (whole 128-byte lines
    for every kernel that streams one half).  scale / shift span all 2 * a.cp channels."""
    a: CL
    b: CL
    scale: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    relu: bool = False

    def __post_init__(self):
        assert self.a.cp == self.b.cp and self.a.dims == self.b.dims and self.a.dtype == self.b.dtype

    @property
    def cp(self) -> int:
        return 2 * self.a.cp

    @property
    def dtype(self) -> torch.dtype:
        return self.a.dtype

    @property
    def nvox(self) -> int:
        return self.a.nvox

    @property
    def lp(self) -> int:
        return self.a.lp

    @property
    def dims(self) -> Tuple[int, int, int, int]:
        return self.a.dims

    def seg_args(self):
        """(ptr_a, cs_a, ptr_b, cs_b) as the ctu_head_*_seg2 entries take them."""
        return self.a.ptr, self.a.cs, self.b.ptr, self.b.cs

    def up_args(self):
        """(ptr_a, ptr_b, seg_c, cs, cp) as the ctu_upconv_fused_*_seg2 entries take them (one stride for both segments)."""
        assert self.a.cs == self.b.cs, "the two-segment up-convolution kernels take segments of equal voxel stride"
        return self.a.ptr, self.b.ptr, self.a.cp, self.a.cs, self.cp


def new_cl(n, d, h, w, cs, device, zero=False, dtype=torch.float32) -> torch.Tensor:
    f = torch.zeros if zero else torch.empty
    return f((n, d, h, w, cs), dtype=dtype, device=device)


# ---------------------------------------------------------------------------- layout
def ncdhw_to_cl(x: torch.Tensor, cp: Optional[int] = None, dtype=torch.float32) -> CL:
    _need_cuda(x, "input")
    x = x.contiguous()
    n, c, d, h, w = x.shape
    cp = cp or pad8(c)
    out = new_cl(n, d, h, w, cp, x.device, dtype=dtype)
    _dual(lp(dtype), "ncdhw_to_ndhwc", x.data_ptr(), out.data_ptr(), n, c, d, h, w, cp, cp, _stream())
    return CL(out, 0, cp)


def cl_to_ncdhw(a: CL, c: int) -> torch.Tensor:
    n, d, h, w = a.dims
    out = torch.empty((n, c, d, h, w), dtype=torch.float32, device=a.buf.device)
    _dual(a.lp, "ndhwc_to_ncdhw", a.ptr, out.data_ptr(), n, c, d, h, w, a.cs, _stream())
    return out


# ---------------------------------------------------------------------------- conv3d
def conv_layout(k: int, nout_p: int, w: int, dtype=torch.float32, rin_p: int = 0) -> int:
    """Packed-weight layout the forward kernel wants for this output width / volume width (16-bit path: depends on the
    padded input channel count too)."""
    if lp(dtype):
        return _lib.load().ctu_lp_conv3d_layout(k, rin_p, nout_p, w)
    return _lib.load().ctu_conv3d_layout(k, nout_p, w)


def pack_conv_w(w: torch.Tensor, cinv: Optional[torch.Tensor], rin_p: int, nout_p: int, mode: int,
                layout: int = 0) -> torch.Tensor:
    """cinv: int32 map padded input-channel position -> logical channel (-1 = padding), None = identity."""
    _need_cuda(w, "conv weight")
    co, ci, k = w.shape[0], w.shape[1], w.shape[2]
    lib = _lib.load()
    n = lib.ctu_conv3d_packed_floats(k, rin_p, nout_p, layout)
    wp = torch.empty(n, dtype=torch.float32, device=w.device)
    _lib.check(lib.ctu_pack_conv3d_weight(w.contiguous().data_ptr(), wp.data_ptr(), co, ci, k, _ptr(cinv), rin_p,
                                          nout_p, mode, layout, _stream()), "pack_conv3d_weight")
    return wp


def packed_floats(kind: str, k: int, rin_p: int, nout_p: int, layout: int) -> int:
    lib = _lib.load()
    return lib.ctu_conv3d_packed_floats(k, rin_p, nout_p, layout) if kind == "conv" else \
        lib.ctu_convt_packed_floats(rin_p, nout_p)


def pack_batch(jobs, dtype: torch.dtype = torch.float32) -> None:
    """jobs: list of (kind 'conv'|'convt', w, wp, cinv, rin_p, nout_p, mode, layout): every job in ONE launch.
    dtype: element type of the packed copies wp (16-bit: the fragment-ordered copies of the fp32 masters)."""
    if not jobs:
        return
    code = 0 if dtype == torch.float32 else LP_CODE[dtype]
    arr = (_lib.PackJob * len(jobs))()
    for a, (kind, w, wp, cinv, rin_p, nout_p, mode, layout) in zip(arr, jobs):
        _need_cuda(w, "weight")
        assert w.is_contiguous() and (not code or wp.dtype == dtype)
        a.w, a.wp, a.cinv = w.data_ptr(), wp.data_ptr(), (None if cinv is None else cinv.data_ptr())
        if kind == "conv":
            a.kind, a.Co, a.Ci, a.k = 0, w.shape[0], w.shape[1], w.shape[2]
        else:
            a.kind, a.Ci, a.Co, a.k = 1, w.shape[0], w.shape[1], 2
            if code:
                layout = 0              # (the 16-bit transposed-conv copy has one layout)
        a.rin_p, a.nout_p, a.mode, a.layout = rin_p, nout_p, mode, layout
    _dual(code, "pack_batch", arr, len(jobs), _stream())


def conv_num_blocks(dims, nout_p: int, layout: int = 0, k: int = 3, dtype=torch.float32, rin_p: int = 32) -> int:
    """Rows of the BN partial-sum buffer a conv3d_fwd call with this geometry writes (16-bit path: depends on the padded
    input channel count too, pass rin_p)."""
    n, d, h, w = dims
    if lp(dtype):
        return _lib.load().ctu_lp_conv3d_num_blocks(n, d, h, w, k, rin_p, nout_p, layout)
    return _lib.load().ctu_conv3d_num_blocks(n, d, h, w, k, nout_p, layout)


def conv3d_fwd(x: CL, wp: torch.Tensor, bias: Optional[torch.Tensor], out: CL, k: int,
               stats: Optional[torch.Tensor] = None, algo_ch: Optional[Tuple[int, int]] = None, layout: int = 0,
               tail=None) -> None:
    """algo_ch = (logical Cin, logical Cout) -- only used to count algorithmic FLOPs when timing.
    tail: make_bn_tail(...) -- the launch finalizes the BatchNorm of its output itself."""
    n, d, h, w = x.dims
    assert out.dims == x.dims
    code = x.lp
    assert not code or (out.dtype == x.dtype and wp.dtype == x.dtype), (x.dtype, out.dtype, wp.dtype)

    def record():
        ci, co = algo_ch if algo_ch is not None else (x.cp, out.cp)
        vox = n * d * h * w
        if code:
            name = _lib.load().ctu_lp_conv3d_fwd_kernel_name(n, d, h, w, k, x.cp, out.cp, layout).decode()
            tag = f"{name}<{_lp_name(code)}, {k}>"
        else:
            tag = _lib.load().ctu_conv3d_fwd_kernel_name(n, d, h, w, k, out.cp, layout).decode()
        return tag, 2.0 * ci * co * k ** 3 * vox, (2.0 if code else 4.0) * vox * (ci + co), (w, x.cp, out.cp)
    with _timed(record):
        _dual(code, "conv3d_fwd", x.ptr, x.cs, x.cp, _ptr(x.scale), _ptr(x.shift), int(x.relu), wp.data_ptr(), _ptr(bias),
              0 if bias is None else bias.numel(), out.ptr, out.cs, out.cp, _ptr(stats), n, d, h, w, k, layout,
              _tail_arg(tail), _stream())


def _wgrad_setup(x: CL, g: CL, co: int, ci: int, k: int, ws: torch.Tensor):
    """What conv3d_wgrad and conv3d_wgrad_bn share around their launch: the workspace check, dw and the timing bracket."""
    n, d, h, w = x.dims
    code = x.lp
    assert not code or g.dtype == x.dtype
    need = _query(code, "conv3d_wgrad_ws_floats", n, d, h, w, k, x.cp, g.cp)
    assert ws.numel() >= need, (ws.numel(), need)
    dw = torch.empty((co, ci, k, k, k), dtype=torch.float32, device=x.buf.device)

    def record():
        vox = n * d * h * w
        if code:
            name = _lib.load().ctu_lp_conv3d_wgrad_kernel_name(d, h, w, k, x.cp, g.cp).decode()
            tag = f"{name}<{_lp_name(code)}, {k}> (+slab reduce)"
        else:
            tag = _lib.load().ctu_conv3d_wgrad_kernel_name(w, k, x.cp, g.cp).decode() + " (+slab reduce)"
        return tag, 2.0 * ci * co * k ** 3 * vox, (2.0 if code else 4.0) * vox * (ci + co), (w, x.cp, g.cp)
    return dw, _timed(record)


def conv3d_wgrad(x: CL, g: CL, co: int, ci: int, k: int, cinv: Optional[torch.Tensor], ws: torch.Tensor,
                 want_bias: bool, jobs: Optional[WgradJobs] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """jobs: leave the slab reduction pending there (WgradJobs) instead of launching it."""
    n, d, h, w = x.dims
    code = x.lp
    dw, timed = _wgrad_setup(x, g, co, ci, k, ws)
    # the fp32 kernel's reduction writes the bias gradient too; the 16-bit one leaves it to a channel_sum launch
    db = torch.empty(co, dtype=torch.float32, device=x.buf.device) if want_bias and not code else None
    if _deferred(jobs, code):
        job = _lib.WgradJob()
        _dual(0, "conv3d_wgrad_slabs", x.ptr, x.cs, x.cp, _ptr(x.scale), _ptr(x.shift), int(x.relu), g.ptr, g.cs, g.cp,
              dw.data_ptr(), _ptr(db), co, ci, _ptr(cinv), ws.data_ptr(), n, d, h, w, k, ctypes.byref(job), _stream())
        jobs.add(job, ws, dw, cinv)
        return dw, db
    with timed:
        _dual(code, "conv3d_wgrad", x.ptr, x.cs, x.cp, _ptr(x.scale), _ptr(x.shift), int(x.relu), g.ptr, g.cs, g.cp,
              dw.data_ptr(), *(() if code else (_ptr(db),)), co, ci, _ptr(cinv), ws.data_ptr(), n, d, h, w, k, _stream())
    if want_bias and code:
        db = channel_sum(g, co)
    return dw, db


def conv3d_wgrad_bn_supported(dims, k: int, cin_p: int, cout_p: int, dtype=torch.float32) -> bool:
    """Can conv3d_wgrad_bn take this layer (k = 3, full boxes [and channel tiles for fp32])?"""
    n, d, h, w = dims
    return bool(_query(lp(dtype), "conv3d_wgrad_bn_supported", n, d, h, w, k, cin_p, cout_p))


def conv3d_wgrad_bn(x: CL, ga: CL, y: CL, vec: torch.Tensor, coef: torch.Tensor, gy: CL, co: int, ci: int, k: int,
                    cinv: Optional[torch.Tensor], ws: torch.Tensor, jobs: Optional[WgradJobs] = None) -> torch.Tensor:
    """Weight gradient with the layer's BatchNorm + ReLU backward folded in: ga = gradient w.r.t. the ACTIVATED output, y =
    the raw conv output, vec = its [4, cp] BatchNorm vectors, coef = bn_relu_bwd(lazy=True)'s rows; gy (same buffer shape
    and channel offset as ga) receives the raw-output gradient for the data-gradient kernel.  jobs: as in conv3d_wgrad."""
    n, d, h, w = x.dims
    assert ga.dims == x.dims and y.dims == x.dims and gy.dims == x.dims and ga.dtype == x.dtype == y.dtype == gy.dtype
    assert y.cs == ga.cs == gy.cs and y.cp == ga.cp == gy.cp and gy.buf.data_ptr() != ga.buf.data_ptr()
    dw, timed = _wgrad_setup(x, ga, co, ci, k, ws)
    if _deferred(jobs, x.lp):
        job = _lib.WgradJob()
        _dual(0, "conv3d_wgrad_bn_slabs", x.ptr, x.cs, x.cp, _ptr(x.scale), _ptr(x.shift), int(x.relu), ga.ptr, ga.cs, ga.cp,
              y.ptr, vec[0].data_ptr(), vec[1].data_ptr(), coef.data_ptr(), gy.ptr, dw.data_ptr(), co, ci, _ptr(cinv),
              ws.data_ptr(), n, d, h, w, k, ctypes.byref(job), _stream())
        jobs.add(job, ws, dw, cinv)
        return dw
    with timed:
        _dual(x.lp, "conv3d_wgrad_bn", x.ptr, x.cs, x.cp, _ptr(x.scale), _ptr(x.shift), int(x.relu), ga.ptr, ga.cs, ga.cp,
              y.ptr, vec[0].data_ptr(), vec[1].data_ptr(), coef.data_ptr(), gy.ptr, dw.data_ptr(), co, ci, _ptr(cinv),
              ws.data_ptr(), n, d, h, w, k, _stream())
    return dw


def conv3d_wgrad_ws(dims, k, cin_p, cout_p, dtype=torch.float32) -> int:
    n, d, h, w = dims
    return _query(lp(dtype), "conv3d_wgrad_ws_floats", n, d, h, w, k, cin_p, cout_p)


def pack_conv_w_lp(w: torch.Tensor, cinv: Optional[torch.Tensor], rin_p: int, nout_p: int, mode: int, dtype: torch.dtype,
                   into: Optional[torch.Tensor] = None, layout: int = 0) -> torch.Tensor:
    """16-bit MFMA-fragment-ordered copy of an fp32 master Conv3d weight (mode 0 forward, 1 data gradient; layout as
    conv_layout(..., dtype, rin_p) says for the launch that will read it)."""
    _need_cuda(w, "conv weight")
    co, ci, k = w.shape[0], w.shape[1], w.shape[2]
    lib = _lib.load()
    n = lib.ctu_lp_conv3d_packed_elems(k, rin_p, nout_p)
    wp = into if into is not None else torch.empty(n, dtype=dtype, device=w.device)
    assert wp.numel() == n and wp.dtype == dtype
    _lib.check(lib.ctu_lp_pack_conv3d_weight(LP_CODE[dtype], w.contiguous().data_ptr(), wp.data_ptr(), co, ci, k, _ptr(cinv),
                                             rin_p, nout_p, mode, layout, _stream()), "lp_pack_conv3d_weight")
    return wp


# ---------------------------------------------------------------------------- first layer (C_in <= 2)
def conv_first_supported(k: int, cin: int, nout_p: int, w: int) -> bool:
    return bool(_lib.load().ctu_conv3d_first_supported(k, cin, nout_p, w))


def conv_first_num_blocks(dims) -> int:
    n, d, h, w = dims
    return _lib.load().ctu_conv3d_first_num_blocks(n, d, h, w)


def conv_first_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], out: CL,
                   stats: Optional[torch.Tensor], tail=None) -> None:
    """x: NCDHW float32 on the GPU (read in place); w: torch Conv3d weight [Co, cin, 3, 3, 3]."""
    _need_cuda(x, "input")
    n, cin, d, h, w_ = x.shape
    vox = n * d * h * w_
    with _timed(lambda: (f"first_fwd_kernel<{cin}>", 2.0 * cin * w.shape[0] * 27 * vox, 4.0 * vox * (cin + w.shape[0]), None)):
        _dual(out.lp, "conv3d_first_fwd", x.data_ptr(), cin, w.data_ptr(), _ptr(bias), 0 if bias is None else bias.numel(),
              out.ptr, out.cs, w.shape[0], _ptr(stats), n, d, h, w_, _tail_arg(tail), _stream())


def conv_first_bwd_data(g: CL, w: torch.Tensor, cin: int) -> torch.Tensor:
    """dx (float32 NCDHW) of the first encoder convolution.  16-bit gradients of volumes at least 32 wide go through the
    matrix pipe (the 8 -> 8 pair-layout kernel with a float32-plane epilogue; the weight's 9 KB fragment copy is made here,
    one tiny launch), everything else through the direct kernel."""
    n, d, h, w_ = g.dims
    dx = torch.empty((n, cin, d, h, w_), dtype=torch.float32, device=g.buf.device)
    lib = _lib.load()
    pair = bool(g.lp and g.cp == 8 and lib.ctu_lp_conv3d_first_bwd_data_pair_supported(cin, w_))

    def record():
        tag = f"lp_conv_fwd_pair_kernel<{_lp_name(g.lp)}, dx of the first layer>" if pair else f"first_bwd_data_kernel<{cin}>"
        vox = n * d * h * w_
        return tag, 2.0 * cin * w.shape[0] * 27 * vox, (2.0 * w.shape[0] if g.lp else 4.0 * w.shape[0]) * vox + 4.0 * vox * cin, None
    with _timed(record):
        if pair:                                     # (the bracket takes the small pack launch with the pair kernel)
            wp = pack_conv_w_lp(w, None, 8, 8, 1, g.dtype, None, 1)
            _lib.check(lib.ctu_lp_conv3d_first_bwd_data_pair(g.lp, g.ptr, g.cs, wp.data_ptr(), cin, dx.data_ptr(), n, d, h, w_,
                                                             _stream()), "lp_conv3d_first_bwd_data_pair")
        else:
            _dual(g.lp, "conv3d_first_bwd_data", g.ptr, g.cs, w.data_ptr(), cin, w.shape[0], dx.data_ptr(), n, d, h, w_, _stream())
    return dx


def conv_first_wgrad(x: torch.Tensor, g: CL, co: int, ws: torch.Tensor, jobs: Optional[WgradJobs] = None) -> torch.Tensor:
    n, cin, d, h, w_ = x.shape
    lib = _lib.load()
    if (g.lp and g.cp == 8 and n * d * h * w_ >= FIRST_WGRAD_MFMA_MIN_VOX
            and lib.ctu_lp_conv3d_wgrad_kernel_name(d, h, w_, 3, 8, 8) == b"lp_wgrad8_kernel"):
        # large 16-bit volumes: an 8-channel 16-bit copy of the input (one streaming pass) + the 8 -> 8 matrix-pipe weight
        # gradient instead of the direct VALU kernel (192^3 x 2 channels: 223 -> 75 + 45 us; 256^3: 520 -> 196 + 100; no gain at
        # 128^3 x 1, hence the threshold).  The input enters this product rounded to 16 bits, like every other layer's.
        x8 = ncdhw_to_cl(x, 8, g.dtype)
        need = lib.ctu_lp_conv3d_wgrad_ws_floats(n, d, h, w_, 3, 8, 8)
        return conv3d_wgrad(x8, g, co, cin, 3, None, ws if ws.numel() >= need else torch.empty(need, device=x.device), False)[0]
    assert ws.numel() >= lib.ctu_conv3d_first_wgrad_ws_floats(n, d, h, w_, cin)
    dw = torch.empty((co, cin, 3, 3, 3), dtype=torch.float32, device=x.device)
    if _deferred(jobs, g.lp):
        job = _lib.WgradJob()
        _dual(0, "conv3d_first_wgrad_slabs", x.data_ptr(), cin, g.ptr, g.cs, dw.data_ptr(), co, ws.data_ptr(), n, d, h, w_,
              ctypes.byref(job), _stream())
        jobs.add(job, ws, dw)
        return dw
    with _timed_first_wgrad(cin, co, n * d * h * w_):
        _dual(g.lp, "conv3d_first_wgrad", x.data_ptr(), cin, g.ptr, g.cs, dw.data_ptr(), co, ws.data_ptr(), n, d, h, w_, _stream())
    return dw


def _timed_first_wgrad(cin: int, co: int, vox: int) -> _timed:
    return _timed(lambda: (f"first_wgrad_kernel<{cin}> (+slab reduce)", 2.0 * cin * co * 27 * vox, 4.0 * vox * (cin + co), None))


def conv_first_wgrad_bn(x: torch.Tensor, ga: CL, y: CL, vec: torch.Tensor, coef: torch.Tensor, gy: CL, co: int,
                        ws: torch.Tensor, jobs: Optional[WgradJobs] = None) -> torch.Tensor:
    """conv_first_wgrad with the BatchNorm + ReLU backward folded in (see conv3d_wgrad_bn); fp32 only."""
    n, cin, d, h, w_ = x.shape
    lib = _lib.load()
    assert not ga.lp and y.cs == ga.cs == gy.cs and ga.cp == 8 and gy.buf.data_ptr() != ga.buf.data_ptr()
    assert ws.numel() >= lib.ctu_conv3d_first_wgrad_ws_floats(n, d, h, w_, cin)
    dw = torch.empty((co, cin, 3, 3, 3), dtype=torch.float32, device=x.device)
    if _deferred(jobs):
        job = _lib.WgradJob()
        _dual(0, "conv3d_first_wgrad_bn_slabs", x.data_ptr(), cin, ga.ptr, ga.cs, y.ptr, vec[0].data_ptr(), vec[1].data_ptr(),
              coef.data_ptr(), gy.ptr, dw.data_ptr(), co, ws.data_ptr(), n, d, h, w_, ctypes.byref(job), _stream())
        jobs.add(job, ws, dw)
        return dw
    with _timed_first_wgrad(cin, co, n * d * h * w_):
        _lib.check(lib.ctu_conv3d_first_wgrad_bn(x.data_ptr(), cin, ga.ptr, ga.cs, y.ptr, vec[0].data_ptr(), vec[1].data_ptr(),
                                                 coef.data_ptr(), gy.ptr, dw.data_ptr(), co, ws.data_ptr(), n, d, h, w_, _stream()),
                   "conv3d_first_wgrad_bn")
    return dw


def conv_first_wgrad_ws(dims, cin: int) -> int:
    n, d, h, w = dims
    return _lib.load().ctu_conv3d_first_wgrad_ws_floats(n, d, h, w, cin)


# ---------------------------------------------------------------------------- batch norm
def bn_finalize_into(stats, nblocks, c, cp, count, gamma, beta, rmean, rvar, momentum, eps, n_updates, vec4, nbt=None):
    """vec4: [4, cp] view (rows may be strided) receiving scale, shift, mean, invstd.
    nbt: the BatchNorm's num_batches_tracked (int64 device scalar), advanced by n_updates in the same launch."""
    lib = _lib.load()
    assert nbt is None or (nbt.dtype == torch.int64 and nbt.is_cuda and nbt.numel() == 1)
    _lib.check(lib.ctu_bn_finalize(stats.data_ptr(), nblocks, c, cp, float(count), gamma.data_ptr(), beta.data_ptr(),
                                   _ptr(rmean), _ptr(rvar), momentum, eps, n_updates, vec4[0].data_ptr(),
                                   vec4[1].data_ptr(), vec4[2].data_ptr(), vec4[3].data_ptr(),
                                   None if nbt is None else nbt.data_ptr(), _stream()), "bn_finalize")


def bn_finalize(stats, nblocks, c, cp, count, gamma, beta, rmean, rvar, momentum, eps, n_updates):
    vec = torch.empty((4, cp), dtype=torch.float32, device=stats.device)     # scale, shift, mean, invstd
    bn_finalize_into(stats, nblocks, c, cp, count, gamma, beta, rmean, rvar, momentum, eps, n_updates, vec)
    return vec


def bn_eval_affine_into(gamma, beta, rmean, rvar, eps, c, cp, vec):
    lib = _lib.load()
    _lib.check(lib.ctu_bn_eval_affine(gamma.data_ptr(), beta.data_ptr(), rmean.data_ptr(), rvar.data_ptr(), eps, c, cp,
                                      vec[0].data_ptr(), vec[1].data_ptr(), _stream()), "bn_eval_affine")


def bn_eval_affine(gamma, beta, rmean, rvar, eps, c, cp):
    vec = torch.empty((2, cp), dtype=torch.float32, device=gamma.device)
    bn_eval_affine_into(gamma, beta, rmean, rvar, eps, c, cp, vec)
    return vec


def bn_relu_bwd(y: CL, ga: CL, vec: torch.Tensor, gamma: torch.Tensor, c: int, partials: torch.Tensor,
                replay=None, pre_reduced: Optional[int] = None, counter: Optional[torch.Tensor] = None, finalized=None,
                lazy: bool = False, jobs: Optional[WgradJobs] = None):
    """In place: ga <- gradient w.r.t. the raw conv output y.  Returns (dgamma, dbeta).
    replay = (running_mean, running_var, momentum, eps[, num_batches_tracked]): also apply the running-stat update a
    second time (the one torch.utils.checkpoint's recompute performs in backward, models.py:232-255).
    counter: the reduction launch finalizes itself (ctu_bn_bwd_tail) instead of a ctu_bn_bwd_finalize launch.
    finalized = (dgb, coef): the kernel that produced ga already reduced AND finalized (maxpool_bwd / head_bwd with fin=).
    lazy: reduce and finalize only -- ga stays the gradient w.r.t. the ACTIVATED output and the weight-gradient kernel
    applies the backward while it stages ga (conv3d_wgrad_bn / upconv_fused_wgrad_bn); returns (dgamma, dbeta, coef).
    jobs: pending weight-gradient slab reductions (WgradJobs) -- they run in spare blocks of the finalize launch; where this
    call launches no finalize of its own (counter / finalized), in one launch of theirs.  Empty afterwards either way."""
    lib = _lib.load()
    nvox = y.nvox
    cp = y.cp
    sc, sh, mu, istd = (vec[i].data_ptr() for i in range(4))
    st = _stream()
    if jobs is not None and (finalized is not None or (counter is not None and pre_reduced is None)):
        jobs.flush()
    if finalized is not None:
        dgb, coef = finalized
        if lazy:
            return dgb[0], dgb[1], coef
        _dual(y.lp, "bn_relu_bwd_apply", y.ptr, y.cs, ga.ptr, ga.cs, cp, sc, sh, mu, istd, coef.data_ptr(), nvox, st)
        return dgb[0], dgb[1]
    nb = lib.ctu_bn_bwd_num_blocks(nvox) if pre_reduced is None else pre_reduced
    assert partials.numel() >= nb * 2 * cp
    tail, (dgb, coef) = _bn_bwd_outputs(c, cp, nvox, gamma, vec, replay, counter, y.buf.device,
                                        tail=counter is not None and pre_reduced is None)
    if pre_reduced is None:       # (else: the kernel that produced ga wrote the nb reduction rows, maxpool_bwd(bn=...))
        assert ga.dtype == y.dtype
        _dual(y.lp, "bn_relu_bwd_reduce", y.ptr, y.cs, ga.ptr, ga.cs, cp, sc, sh, mu, istd, nvox, partials.data_ptr(),
              _tail_arg(tail), st)
    if tail is None:
        rm, rv, mom, eps, nbt = _replay_args(replay)
        fin = (partials.data_ptr(), nb, c, cp, float(nvox), gamma.data_ptr(), istd, dgb[0].data_ptr(), dgb[1].data_ptr(),
               coef.data_ptr(), mu, _ptr(rm), _ptr(rv), mom, eps, None if nbt is None else nbt.data_ptr())
        if jobs:
            arr, n = jobs.take()
            _lib.check(lib.ctu_bn_bwd_finalize_jobs(*fin, arr, n, st), "bn_bwd_finalize_jobs")
        else:
            _lib.check(lib.ctu_bn_bwd_finalize(*fin, st), "bn_bwd_finalize")
    if lazy:
        return dgb[0], dgb[1], coef
    _dual(y.lp, "bn_relu_bwd_apply", y.ptr, y.cs, ga.ptr, ga.cs, cp, sc, sh, mu, istd, coef.data_ptr(), nvox, st)
    return dgb[0], dgb[1]


def bn_bwd_partials_floats(nvox: int, cp: int) -> int:
    return _lib.load().ctu_bn_bwd_num_blocks(nvox) * 2 * cp


# ---------------------------------------------------------------------------- pool
def maxpool_fwd(x: CL, out: CL) -> None:
    n, d, h, w = x.dims
    assert out.dtype == x.dtype
    _dual(x.lp, "maxpool2_fwd", x.ptr, x.cs, x.cp, _ptr(x.scale), _ptr(x.shift), int(x.relu), out.ptr, out.cs, n, d, h, w,
          _stream())


def maxpool_bwd_bn_blocks(dims, cp: int) -> int:
    n, d, h, w = dims
    return _lib.load().ctu_maxpool2_bwd_bn_num_blocks(n, d, h, w, cp)


def maxpool_bwd(x: CL, gout: CL, gin: CL, accumulate: bool, bn=None, fin=None):
    """bn = (vec [4, cp] scale/shift/mean/invstd of x's BatchNorm, partials): also emit that BatchNorm's backward
    reduction rows into partials; returns their number (pass it to bn_relu_bwd(pre_reduced=...)).
    fin = (gamma, c, replay, counter) with bn: the launch also finalizes that reduction (ctu_bn_bwd_tail); returns
    (rows, (dgb, coef)) -- pass the pair to bn_relu_bwd(finalized=...)."""
    n, d, h, w = x.dims
    if bn is not None:
        vec, partials = bn
        nb = maxpool_bwd_bn_blocks(x.dims, x.cp)
        assert x.scale is not None and x.relu and partials.numel() >= nb * 2 * x.cp
        assert vec[0].data_ptr() == x.scale.data_ptr() and vec[1].data_ptr() == x.shift.data_ptr()
        tail, done = None, None
        if fin is not None:
            gamma, c, replay, counter = fin
            tail, done = _bn_bwd_outputs(c, x.cp, x.nvox, gamma, vec, replay, counter, x.buf.device)
        _dual(x.lp, "maxpool2_bwd_bn", x.ptr, x.cs, x.cp, vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(),
              vec[3].data_ptr(), gout.ptr, gout.cs, gin.ptr, gin.cs, int(accumulate), n, d, h, w, partials.data_ptr(),
              _tail_arg(tail), _stream())
        return nb if fin is None else (nb, done)
    _dual(x.lp, "maxpool2_bwd", x.ptr, x.cs, x.cp, _ptr(x.scale), _ptr(x.shift), int(x.relu), gout.ptr, gout.cs, gin.ptr,
          gin.cs, int(accumulate), n, d, h, w, _stream())


# ---------------------------------------------------------------------------- conv transpose
def pack_convt_w(w: torch.Tensor, cinv, rin_p: int, nout_p: int, mode: int) -> torch.Tensor:
    _need_cuda(w, "convT weight")
    ci, co = w.shape[0], w.shape[1]
    lib = _lib.load()
    wp = torch.empty(lib.ctu_convt_packed_floats(rin_p, nout_p), dtype=torch.float32, device=w.device)
    _lib.check(lib.ctu_pack_convt_weight(w.contiguous().data_ptr(), wp.data_ptr(), ci, co, _ptr(cinv), rin_p, nout_p,
                                         mode, _stream()), "pack_convt_weight")
    return wp


def pack_convt_w_lp(w: torch.Tensor, cinv, rin_p: int, nout_p: int, mode: int, dtype: torch.dtype,
                    into: Optional[torch.Tensor] = None) -> torch.Tensor:
    """16-bit fragment-ordered copy of an fp32 master ConvTranspose3d weight [Ci,Co,2,2,2] (mode 0 forward, 1 data gradient)."""
    _need_cuda(w, "convT weight")
    ci, co = w.shape[0], w.shape[1]
    lib = _lib.load()
    n = lib.ctu_lp_convt_packed_elems(rin_p, nout_p, mode)
    wp = into if into is not None else torch.empty(n, dtype=dtype, device=w.device)
    assert wp.numel() == n and wp.dtype == dtype
    _lib.check(lib.ctu_lp_pack_convt_weight(LP_CODE[dtype], w.contiguous().data_ptr(), wp.data_ptr(), ci, co, _ptr(cinv), rin_p,
                                            nout_p, mode, _stream()), "lp_pack_convt_weight")
    return wp


def _convt_bracket(name: str, x: CL, x_cp: int, o_cp: int, dims) -> _timed:
    """Bracket of the ConvTranspose launches of the stage table: algorithmic 2*8*C*C FLOP and (C + 8C) elements per coarse voxel."""
    n, d, h, w = dims
    vox = n * d * h * w
    return _timed(lambda: (name + ("_lp" if x.lp else ""), 16.0 * x_cp * o_cp * vox,
                           float(x.buf.element_size()) * vox * (x_cp + 8 * o_cp), (w, x_cp, o_cp)))


def convt_fwd(x: CL, wp: torch.Tensor, bias: Optional[torch.Tensor], out: CL) -> None:
    n, d, h, w = x.dims
    with _convt_bracket("convt2_fwd", x, x.cp, out.cp, x.dims):
        assert not x.lp or (out.dtype == x.dtype and wp.dtype == x.dtype)
        _dual(x.lp, "convt2_fwd", x.ptr, x.cs, x.cp, _ptr(x.scale), _ptr(x.shift), int(x.relu), wp.data_ptr(), _ptr(bias),
              0 if bias is None else bias.numel(), out.ptr, out.cs, out.cp, n, d, h, w, _stream())


def convt_bwd_data(gout: CL, wp: torch.Tensor, gin: CL) -> None:
    n, d, h, w = gin.dims
    with _convt_bracket("convt2_bwd_data", gout, gin.cp, gout.cp, gin.dims):
        assert not gout.lp or (gin.dtype == gout.dtype and wp.dtype == gout.dtype)
        _dual(gout.lp, "convt2_bwd_data", gout.ptr, gout.cs, gout.cp, wp.data_ptr(), gin.ptr, gin.cs, gin.cp, n, d, h, w,
              _stream())


def convt_wgrad(x: CL, g: CL, ci: int, co: int, imap, ws: torch.Tensor, jobs: Optional[WgradJobs] = None):
    n, d, h, w = x.dims
    if _deferred(jobs, x.lp):
        assert ws.numel() >= convt_wgrad_ws(x.dims, x.cp, g.cp, x.dtype)
        dw = torch.empty((ci, co, 2, 2, 2), dtype=torch.float32, device=x.buf.device)
        db = torch.empty(co, dtype=torch.float32, device=x.buf.device)
        job = _lib.WgradJob()
        _dual(0, "convt2_wgrad_slabs", x.ptr, x.cs, x.cp, _ptr(x.scale), _ptr(x.shift), int(x.relu), g.ptr, g.cs, g.cp,
              dw.data_ptr(), db.data_ptr(), ci, co, _ptr(imap), ws.data_ptr(), n, d, h, w, ctypes.byref(job), _stream())
        jobs.add(job, ws, dw, db, imap)
        return dw, db
    with _convt_bracket("convt2_wgrad", x, x.cp, g.cp, x.dims):
        assert not x.lp or g.dtype == x.dtype
        assert ws.numel() >= convt_wgrad_ws(x.dims, x.cp, g.cp, x.dtype)
        dw = torch.empty((ci, co, 2, 2, 2), dtype=torch.float32, device=x.buf.device)
        # the fp32 kernel's reduction writes the bias gradient too; the 16-bit one leaves it to a channel_sum launch
        db = None if x.lp else torch.empty(co, dtype=torch.float32, device=x.buf.device)
        _dual(x.lp, "convt2_wgrad", x.ptr, x.cs, x.cp, _ptr(x.scale), _ptr(x.shift), int(x.relu), g.ptr, g.cs, g.cp,
              dw.data_ptr(), *(() if x.lp else (db.data_ptr(),)), ci, co, _ptr(imap), ws.data_ptr(), n, d, h, w, _stream())
        if x.lp:
            db = channel_sum(g, co)
    return dw, db


def convt_wgrad_ws(dims, cin_p, cout_p, dtype=torch.float32) -> int:
    n, d, h, w = dims
    return _query(lp(dtype), "convt2_wgrad_ws_floats", n, d, h, w, cin_p, cout_p)


# ---------------------------------------------------------------------------- head
def head_fwd(x, w: torch.Tensor, b: torch.Tensor, imap, act: int, head_mode: int):
    """x: CL, or CL2 (the input voxel in two segments: ctu_head_fwd_seg2, same values bit for bit)."""
    n, d, h, w_ = x.dims
    co, ci = w.shape[0], w.shape[1]
    v = d * h * w_
    dev = w.device
    if head_mode == 0:
        out0 = torch.empty((n, co, d, h, w_), dtype=torch.float32, device=dev)
        out1 = None
    else:
        out0 = torch.empty((n, 2, d, h, w_), dtype=torch.float32, device=dev)
        out1 = torch.empty((n, 2, d, h, w_), dtype=torch.float32, device=dev)
    seg2 = isinstance(x, CL2)
    assert not seg2 or x.a.cp in (8, 16), "the two-segment head kernels take at most 16 channels per segment"
    src = (*x.seg_args(), x.a.cp) if seg2 else (x.ptr, x.cs, x.cp)
    _dual(x.lp, "head_fwd_seg2" if seg2 else "head_fwd", *src, _ptr(x.scale), _ptr(x.shift), int(x.relu), w.data_ptr(),
          b.data_ptr(), _ptr(imap), ci, co, act, head_mode, out0.data_ptr(), _ptr(out1), n, v, _stream())
    return out0, out1


def head_bwd(x, w: torch.Tensor, b: torch.Tensor, imap, act: int, head_mode: int, g0: torch.Tensor,
             g1: Optional[torch.Tensor], gin, bn=None, fin=None, gscale: float = 1.0,
             gscale_dev: Optional[torch.Tensor] = None):
    """x / gin: both CL, or both CL2 (input and input gradient in two segments: the ctu_*_seg2 entries).
    bn = (vec [4, bn_cp] of the BatchNorm whose activated output is x's first bn_cp channels, partials): also emit
    that BatchNorm's backward reduction rows; returns (dw, db, rows) then (rows -> bn_relu_bwd(pre_reduced=...)).
    fin = (gamma, c, replay) with bn: the launch pair also finalizes that reduction; returns (dw, db, rows, (dgb, coef)).
    gscale (16-bit tensors): g0 / g1 are multiplied by it as they are read (float16 loss scale).
    gscale_dev: float32[1] device tensor that replaces gscale (the dynamic loss scale, read by the kernel)."""
    assert gscale == 1.0 or x.lp, "gscale is the 16-bit path's loss scale"
    assert gscale_dev is None or (x.lp and gscale_dev.is_cuda and gscale_dev.dtype == torch.float32), \
        "gscale_dev is the 16-bit path's device loss scale"
    n, d, h, w_ = x.dims
    co, ci = w.shape[0], w.shape[1]
    v = d * h * w_
    dev = w.device
    seg2 = isinstance(x, CL2)
    assert seg2 == isinstance(gin, CL2), "head_bwd: input and input gradient are both one buffer or both two segments"
    assert not seg2 or x.a.cp in (8, 16), "the two-segment head kernels take at most 16 channels per segment"
    lib = _lib.load()
    ws = torch.empty(lib.ctu_head_bwd_ws_floats(n, v, x.cp, co), dtype=torch.float32, device=dev)
    dw = torch.empty_like(w)
    db = torch.empty_like(b)
    bn_args, tail, done = (None, None, 0, None), None, None
    if bn is not None:
        vec, partials = bn
        bn_cp = vec.shape[1]
        rows = lib.ctu_head_bwd_num_blocks(n, v)
        assert x.scale is not None and x.relu and vec[0].data_ptr() == x.scale.data_ptr() and partials.numel() >= rows * 2 * bn_cp
        bn_args = (vec[2].data_ptr(), vec[3].data_ptr(), bn_cp, partials.data_ptr())
        if fin is not None:
            gamma, c, replay = fin[:3]
            tail, done = _bn_bwd_outputs(c, bn_cp, n * v, gamma, vec, replay, None, dev)
    # the 16-bit entries carry the loss scale in front of the stream: a float, or (_dscale) a pointer to the device scale
    entry, scale = "head_bwd_bn", ((float(gscale),) if x.lp else ())
    if gscale_dev is not None:
        entry, scale = "head_bwd_bn_dscale", (gscale_dev.data_ptr(),)
    if seg2:
        entry, src, dst = entry + "_seg2", (*x.seg_args(), x.a.cp), gin.seg_args()
    else:
        src, dst = (x.ptr, x.cs, x.cp), (gin.ptr, gin.cs)
    _dual(x.lp, entry, *src, _ptr(x.scale), _ptr(x.shift), int(x.relu), w.data_ptr(), b.data_ptr(), _ptr(imap),
          ci, co, act, head_mode, g0.data_ptr(), _ptr(g1), *dst, dw.data_ptr(), db.data_ptr(), ws.data_ptr(), n, v,
          *bn_args, _tail_arg(tail), *scale, _stream())
    if bn is None:
        return dw, db
    return (dw, db, rows) if fin is None else (dw, db, rows, done)


def head_bwd_blocks(dims) -> int:
    n, d, h, w_ = dims
    return _lib.load().ctu_head_bwd_num_blocks(n, d * h * w_)


# ---------------------------------------------------------------------------- loss
def loss_fwd(pred: torch.Tensor, target: torch.Tensor, ce_lambda: float, dice_lambda: float, dice_softmax: bool):
    _need_cuda(pred, "prediction")
    _need_cuda(target, "target")
    assert pred.shape == target.shape and pred.shape[1] == 2, "loss kernel handles 2-channel maps"
    pred, target = pred.contiguous(), target.contiguous()
    n = pred.shape[0]
    v = pred[0, 0].numel()
    lib = _lib.load()
    ws = torch.empty(lib.ctu_loss_ws_floats(n, v), dtype=torch.float32, device=pred.device)
    terms = torch.empty(2, dtype=torch.float32, device=pred.device)
    _lib.check(lib.ctu_loss_fwd(pred.data_ptr(), target.data_ptr(), n, v, ce_lambda, dice_lambda, int(dice_softmax),
                                terms.data_ptr(), ws.data_ptr(), _stream()), "loss_fwd")
    return terms, ws


def loss_bwd(pred, target, ce_lambda, dice_lambda, dice_softmax, ws, g_ce: Optional[torch.Tensor],
             g_dice: Optional[torch.Tensor], out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """g_ce / g_dice: the upstream gradients of the two terms (0-d float32 device tensors, read in place; None = 1)."""
    pred, target = pred.contiguous(), target.contiguous()
    for g_ in (g_ce, g_dice):
        assert g_ is None or (g_.is_cuda and g_.dtype == torch.float32 and g_.numel() == 1)
    n = pred.shape[0]
    v = pred[0, 0].numel()
    g = out if out is not None else torch.empty_like(pred)
    lib = _lib.load()
    _lib.check(lib.ctu_loss_bwd(pred.data_ptr(), target.data_ptr(), n, v, ce_lambda, dice_lambda, int(dice_softmax),
                                ws.data_ptr(), _ptr(g_ce), _ptr(g_dice), g.data_ptr(), int(accumulate), _stream()),
               "loss_bwd")
    return g


def _seg_loss_args(pred, target, lambdas, dice_softmax, class_weight, focal_gamma, tversky_ab, boundary):
    """(contiguous pred, target, boundary map or None, N, V, ctu_seg_loss_cfg) of one loss-family call."""
    _need_cuda(pred, "prediction")
    _need_cuda(target, "target")
    assert pred.shape == target.shape and pred.dim() == 5 and pred.shape[1] == 2, "loss kernel handles 2-channel maps"
    pred, target = pred.contiguous(), target.contiguous()
    n, v = pred.shape[0], pred[0, 0].numel()
    ce, dice, tv, bd = (float(x) for x in lambdas)
    if bd != 0.0:
        if boundary is None:
            raise ValueError("ctunet_amd: boundary_lambda != 0 needs a boundary (signed distance) map")
        _need_cuda(boundary, "boundary map")
        if boundary.dtype != torch.float32 or tuple(boundary.shape) not in ((n,) + tuple(pred.shape[2:]),
                                                                            (n, 1) + tuple(pred.shape[2:])):
            raise ValueError(f"ctunet_amd: the boundary map must be float32 [N,D,H,W] or [N,1,D,H,W] of the prediction's "
                             f"grid, got {boundary.dtype} {tuple(boundary.shape)} for {tuple(pred.shape)}")
        boundary = boundary.contiguous()
    else:
        boundary = None                  # not read
    cfg = _lib.SegLossCfg(ce, dice, tv, bd, float(class_weight[0]), float(class_weight[1]), float(focal_gamma),
                          float(tversky_ab[0]), float(tversky_ab[1]), int(bool(dice_softmax)))
    return pred, target, boundary, n, v, cfg


def seg_loss_fwd(pred: torch.Tensor, target: torch.Tensor, lambdas: Sequence[float], dice_softmax: bool,
                 class_weight: Sequence[float] = (1.0, 1.0), focal_gamma: float = 0.0,
                 tversky_ab: Sequence[float] = (0.5, 0.5), boundary: Optional[torch.Tensor] = None):
    """Loss family of csrc/loss_family.hip on one [N,2,D,H,W] map.  lambdas = (ce, dice, tversky, boundary); returns
    (terms [4] in that order, workspace for ``seg_loss_bwd``)."""
    pred, target, boundary, n, v, cfg = _seg_loss_args(pred, target, lambdas, dice_softmax, class_weight, focal_gamma,
                                                      tversky_ab, boundary)
    lib = _lib.load()
    ws = torch.empty(lib.ctu_seg_loss_ws_floats(n, v), dtype=torch.float32, device=pred.device)
    terms = torch.empty(4, dtype=torch.float32, device=pred.device)
    _lib.check(lib.ctu_seg_loss_fwd(pred.data_ptr(), target.data_ptr(), _ptr(boundary), n, v, ctypes.byref(cfg),
                                    terms.data_ptr(), ws.data_ptr(), _stream()), "seg_loss_fwd")
    return terms, ws


def seg_loss_bwd(pred, target, lambdas, dice_softmax, ws, upstream: Sequence[Optional[torch.Tensor]] = (None,) * 4,
                 class_weight: Sequence[float] = (1.0, 1.0), focal_gamma: float = 0.0,
                 tversky_ab: Sequence[float] = (0.5, 0.5), boundary: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """upstream: the gradients of the four terms (0-d float32 device tensors, read in place; None = 1)."""
    pred, target, boundary, n, v, cfg = _seg_loss_args(pred, target, lambdas, dice_softmax, class_weight, focal_gamma,
                                                      tversky_ab, boundary)
    assert len(upstream) == 4
    for g_ in upstream:
        assert g_ is None or (g_.is_cuda and g_.dtype == torch.float32 and g_.numel() == 1)
    g = out if out is not None else torch.empty_like(pred)
    lib = _lib.load()
    _lib.check(lib.ctu_seg_loss_bwd(pred.data_ptr(), target.data_ptr(), _ptr(boundary), n, v, ctypes.byref(cfg),
                                    ws.data_ptr(), *(_ptr(g_) for g_ in upstream), g.data_ptr(), int(accumulate),
                                    _stream()), "seg_loss_bwd")
    return g


# ---------------------------------------------------------------------------- misc

def skip_add(a: CL, b: Optional[CL], out: CL) -> None:
    """out = act(a) + act(b) (additive skip, UNet(cat=False)); b None: out = act(a) (channel-slice copy)."""
    assert out.dims == a.dims and out.cp == a.cp and (b is None or (b.dims == a.dims and b.cp == a.cp))
    assert out.dtype == a.dtype and (b is None or b.dtype == a.dtype)
    _dual(a.lp, "skip_add", a.ptr, a.cs, _ptr(a.scale), _ptr(a.shift), int(a.relu), 0 if b is None else b.ptr,
          0 if b is None else b.cs, _ptr(b.scale) if b is not None else 0, _ptr(b.shift) if b is not None else 0,
          int(b.relu) if b is not None else 0, out.ptr, out.cs, out.cp, a.nvox, _stream())


def channel_sum(x: CL, c: int) -> torch.Tensor:
    lib = _lib.load()
    nb = lib.ctu_channel_sum_num_blocks(x.nvox)
    part = torch.empty(nb * x.cp, dtype=torch.float32, device=x.buf.device)
    out = torch.empty(c, dtype=torch.float32, device=x.buf.device)
    _dual(x.lp, "channel_sum", x.ptr, x.cs, x.cp, x.nvox, part.data_ptr(), out.data_ptr(), c, _stream())
    return out


# ---------------------------------------------------------------------------- fused up-convolution (decoder)
def upconv_fused_supported(dims, k: int, cin_p: int, nout_p: int) -> bool:
    n, d, h, w = dims
    return bool(_lib.load().ctu_upconv_fused_supported(k, d, h, w, cin_p, nout_p))


def upconv_fused_seg2_supported(dims, k: int, cin_p: int, nout_p: int, seg_c: int) -> bool:
    """Do the two-segment forms of the fused forward / weight gradient / data gradient (a CL2 coarse tensor) take this geometry?"""
    n, d, h, w = dims
    return bool(_lib.load().ctu_upconv_fused_seg2_supported(k, d, h, w, cin_p, nout_p, seg_c))


def upconv_fused_pack(wt: torch.Tensor, bt: torch.Tensor, w3: torch.Tensor, cinv, cin_p: int, nout_p: int,
                      into=None):
    """Composite weights (fragment order) and the 27 border-class biases of ConvTranspose3d(C,C,2,2) -> Conv3d(C,Co,3).
    into = (wp, beff, ws): re-pack in place (stable pointers for graph replay)."""
    return _upconv_pack(wt, bt, w3, cinv, cin_p, nout_p, into, False)


def upconv_fused_pack_all(wt: torch.Tensor, bt: torch.Tensor, w3: torch.Tensor, cinv, cin_p: int, nout_p: int,
                          into=None):
    """upconv_fused_pack and upconv_fused_pack_bwd in one call (three launches): returns (wp, beff, ws, wpd).
    into = (wp, beff, ws, wpd): re-pack in place."""
    return _upconv_pack(wt, bt, w3, cinv, cin_p, nout_p, into, True)


def _upconv_pack(wt, bt, w3, cinv, cin_p, nout_p, into, with_wpd: bool):
    lib = _lib.load()
    c, co = wt.shape[0], w3.shape[0]
    assert wt.shape == (c, c, 2, 2, 2) and w3.shape == (co, c, 3, 3, 3) and bt.shape == (c,)
    if into is not None:
        bufs = tuple(into)
        assert len(bufs) == 3 + with_wpd
    else:
        new = lambda n: torch.empty(n, dtype=torch.float32, device=wt.device)
        bufs = (new(lib.ctu_upconv_fused_packed_floats(cin_p, nout_p)), new((27, nout_p)),
                new(lib.ctu_upconv_fused_pack_ws_floats(c, nout_p)))
        if with_wpd:
            bufs += (new(lib.ctu_upconv_fused_bwd_packed_floats(cin_p, nout_p)),)
    wp, beff, ws = bufs[:3]
    _lib.check(lib.ctu_upconv_fused_pack_all(wt.detach().contiguous().data_ptr(), bt.detach().contiguous().data_ptr(),
                                             w3.detach().contiguous().data_ptr(), c, co, _ptr(cinv), cin_p, nout_p, wp.data_ptr(),
                                             beff.data_ptr(), ws.data_ptr(), bufs[3].data_ptr() if with_wpd else None, _stream()),
               "upconv_fused_pack")
    return bufs


def upconv_fused_num_blocks(dims, nout_p: int) -> int:
    n, d, h, w = dims
    return _lib.load().ctu_upconv_fused_num_blocks(n, d, h, w, nout_p)


def upconv_fused_fwd(x, wp: torch.Tensor, beff: torch.Tensor, out: CL, stats: Optional[torch.Tensor],
                     algo_ch: Optional[Tuple[int, int]] = None, tail=None) -> None:
    """out (fine grid, raw) = conv3(convT(act(x))) in one kernel; x is the COARSE input: a CL, or a CL2 (its channels in two
    segments: ctu_upconv_fused_fwd_seg2, same values bit for bit)."""
    n, d, h, w = x.dims
    assert out.dims == (n, 2 * d, 2 * h, 2 * w)
    ci, co = algo_ch if algo_ch is not None else (x.cp, out.cp)
    vox = n * d * h * w
    # algorithmic work of the two layers it replaces: convT 2*ci*ci*8 per coarse voxel + conv 2*27*ci*co per fine voxel
    with _timed(lambda: (f"upconv_fused_fwd_kernel<{out.cp}>", vox * (16.0 * ci * ci + 8 * 54.0 * ci * co),
                         4.0 * vox * (ci + 8 * co), (w, x.cp, out.cp))):
        seg2 = isinstance(x, CL2)
        entry = getattr(_lib.load(), "ctu_upconv_fused_fwd_seg2" if seg2 else "ctu_upconv_fused_fwd")
        _lib.check(entry(*(x.up_args() if seg2 else (x.ptr, x.cs, x.cp)), _ptr(x.scale), _ptr(x.shift), int(x.relu),
                         wp.data_ptr(), beff.data_ptr(), out.ptr, out.cs, out.cp, _ptr(stats),
                         n, d, h, w, _tail_arg(tail), _stream()), "upconv_fused_fwd")


def upconv_fused_wgrad_bn_supported(dims, cin_p: int, nout_p: int, dtype=torch.float32) -> bool:
    n, d, h, w = dims
    return dtype == torch.float32 and bool(_lib.load().ctu_upconv_fused_wgrad_bn_supported(n, d, h, w, cin_p, nout_p))


def upconv_fused_wgrad(x, g: CL, c: int, co: int, bt: torch.Tensor, pack_ws: torch.Tensor, imap, lazy=None):
    """(dWT [C,C,2,2,2], dbT [C], dW3 [Co,C,3,3,3]) of the fused ConvTranspose3d -> Conv3d pair: x = COARSE input of the
    transposed conv (CL, or CL2: the ctu_upconv_fused_wgrad*_seg2 entries), g = fine-grid gradient w.r.t. the conv's raw output, pack_ws = scratch of this step's
    upconv_fused_pack (transposed weights).
    lazy = (y, vec, coef, gy): g is the gradient w.r.t. the ACTIVATED output; the BatchNorm + ReLU backward is applied while
    the weight-gradient kernel stages it and the raw-output gradient lands in gy (read by the projections here and by
    upconv_fused_bwd_data afterwards) -- see conv3d_wgrad_bn."""
    n, d, h, w = x.dims
    assert g.dims == (n, 2 * d, 2 * h, 2 * w) and not x.lp
    return _upconv_wgrad(x, g, c, co, bt, pack_ws, imap, lazy,
                         lambda: (f"upconv_fused_wgrad_kernel<{g.cp}> (+slab reduce)", 4.0 * (n * d * h * w) * (c + 8 * co)))


def _upconv_wgrad(x, g: CL, c: int, co: int, bt, pack_ws, imap, lazy, tag_bytes):
    """Body of upconv_fused_wgrad / lp_upconv_fused_wgrad: composite-weight gradient (with the lazy BatchNorm backward or
    without), then its projection onto the two layers' parameters.  The 16-bit weight-gradient entries carry no g.cp (it is 8).
    tag_bytes() -> (tag, algorithmic bytes) of the timer record."""
    n, d, h, w = x.dims
    dev = g.buf.device
    seg2 = isinstance(x, CL2)                            # (fp32 only: the 16-bit entries take one buffer)
    assert not (seg2 and x.lp)
    sfx = "_seg2" if seg2 else ""
    gcp = () if x.lp else (g.cp,)
    dweff = torch.empty((8, 8, x.cp, g.cp), dtype=torch.float32, device=dev)
    ws = torch.empty(_query(x.lp, "upconv_fused_wgrad_ws_floats", n, d, h, w, x.cp, *gcp), dtype=torch.float32, device=dev)
    act = (*(x.up_args() if seg2 else (x.ptr, x.cs, x.cp)), _ptr(x.scale), _ptr(x.shift), int(x.relu), g.ptr, g.cs, *gcp)
    detail = (w, x.cp, g.cp)

    def record():
        tag, nbytes = tag_bytes()
        return tag, (n * d * h * w) * (16.0 * c * c + 8 * 54.0 * c * co), nbytes, detail
    with _timed(record):
        if lazy is not None:
            y, vec, coef, gy = lazy
            assert y.dims == g.dims and gy.dims == g.dims and y.cs == g.cs == gy.cs and y.cp == g.cp == gy.cp
            assert gy.buf.data_ptr() != g.buf.data_ptr()
            _dual(x.lp, "upconv_fused_wgrad_bn" + sfx, *act, y.ptr, vec[0].data_ptr(), vec[1].data_ptr(), coef.data_ptr(), gy.ptr,
                  dweff.data_ptr(), ws.data_ptr(), n, d, h, w, _stream())
            g = gy
        else:
            _dual(x.lp, "upconv_fused_wgrad" + sfx, *act, dweff.data_ptr(), ws.data_ptr(), n, d, h, w, _stream())
    dwt = torch.empty((c, c, 2, 2, 2), dtype=torch.float32, device=dev)
    dbt = torch.empty(c, dtype=torch.float32, device=dev)
    dw3 = torch.empty((co, c, 3, 3, 3), dtype=torch.float32, device=dev)
    ws2 = torch.empty(_lib.load().ctu_upconv_fused_project_ws_floats(g.cp, g.nvox), dtype=torch.float32, device=dev)
    _dual(x.lp, "upconv_fused_project", dweff.data_ptr(), g.ptr, g.cs, g.cp, n, d, h, w, bt.detach().data_ptr(),
          pack_ws.data_ptr(), _ptr(imap), c, co, x.cp, dwt.data_ptr(), dbt.data_ptr(), dw3.data_ptr(), ws2.data_ptr(), _stream())
    return dwt, dbt, dw3


# ---- 16-bit twins (upconv_lp.hip): 8 padded output channels, input channels a multiple of 32
def lp_upconv_fused_supported(dims, k: int, cin_p: int, nout_p: int) -> bool:
    n, d, h, w = dims
    return bool(_lib.load().ctu_lp_upconv_fused_supported(k, d, h, w, cin_p, nout_p))


def lp_upconv_fused_pack(wp32: torch.Tensor, cin_p: int, dtype: torch.dtype, into: Optional[torch.Tensor] = None) -> torch.Tensor:
    """16-bit MFMA fragments (forward, then data gradient) of upconv_fused_pack's fp32 composite weights (nout_p = 8)."""
    lib = _lib.load()
    n = lib.ctu_lp_upconv_fused_packed_elems(cin_p)
    wp16 = into if into is not None else torch.empty(n, dtype=dtype, device=wp32.device)
    assert wp16.numel() == n and wp16.dtype == dtype
    _lib.check(lib.ctu_lp_upconv_fused_pack(LP_CODE[dtype], wp32.data_ptr(), cin_p, wp16.data_ptr(), _stream()), "lp_upconv_fused_pack")
    return wp16


def lp_upconv_fused_num_blocks(dims) -> int:
    n, d, h, w = dims
    return _lib.load().ctu_lp_upconv_fused_num_blocks(n, d, h, w)


def lp_upconv_fused_fwd(x: CL, wp16: torch.Tensor, beff: torch.Tensor, out: CL, stats: Optional[torch.Tensor],
                        algo_ch: Optional[Tuple[int, int]] = None) -> None:
    """out (fine grid, 16-bit, raw) = conv3(convT(act(x))) in one kernel; x = the COARSE 16-bit input."""
    n, d, h, w = x.dims
    assert out.dims == (n, 2 * d, 2 * h, 2 * w) and x.lp and out.dtype == x.dtype and wp16.dtype == x.dtype and out.cp == 8
    ci, co = algo_ch if algo_ch is not None else (x.cp, out.cp)
    vox = n * d * h * w
    with _timed(lambda: (f"lp_upconv_fwd_kernel<{_lp_name(x.lp)}>", vox * (16.0 * ci * ci + 8 * 54.0 * ci * co),
                         2.0 * vox * (x.cp + 8 * out.cp), (w, x.cp, out.cp))):
        _lib.check(_lib.load().ctu_lp_upconv_fused_fwd(x.lp, x.ptr, x.cs, x.cp, _ptr(x.scale), _ptr(x.shift), int(x.relu),
                                                       wp16.data_ptr(), beff.data_ptr(), out.ptr, out.cs, _ptr(stats),
                                                       n, d, h, w, _stream()), "lp_upconv_fused_fwd")


def lp_upconv_fused_wgrad_bn_supported(dims, cin_p: int) -> bool:
    n, d, h, w = dims
    return bool(_lib.load().ctu_lp_upconv_fused_wgrad_bn_supported(n, d, h, w, cin_p))


def lp_upconv_fused_wgrad(x: CL, g: CL, c: int, co: int, bt: torch.Tensor, pack_ws: torch.Tensor, imap, lazy=None):
    """(dWT, dbT, dW3) as upconv_fused_wgrad, from 16-bit tensors: x = COARSE input, g = fine-grid raw-output gradient.
    lazy = (y, vec, coef, gy) as in upconv_fused_wgrad."""
    n, d, h, w = x.dims
    assert g.dims == (n, 2 * d, 2 * h, 2 * w) and x.lp and g.dtype == x.dtype and g.cp == 8 and g.cs == 8
    return _upconv_wgrad(x, g, c, co, bt, pack_ws, imap, lazy,
                         lambda: (f"lp_upconv_wgrad_kernel<{_lp_name(x.lp)}> (+slab reduce)", 2.0 * (n * d * h * w) * (x.cp + 8 * g.cp)))


def lp_upconv_fused_bwd_data(g: CL, wp16: torch.Tensor, gin: CL, algo_ch: Optional[Tuple[int, int]] = None) -> None:
    """gin (coarse, 16-bit) <- gradient of the fused pair w.r.t. its activated input, from the fine-grid gradient g."""
    n, d, h, w = gin.dims
    assert g.dims == (n, 2 * d, 2 * h, 2 * w) and g.lp and gin.dtype == g.dtype and wp16.dtype == g.dtype and g.cp == 8
    ci, co = algo_ch if algo_ch is not None else (gin.cp, g.cp)
    vox = n * d * h * w
    with _timed(lambda: (f"lp_upconv_bwd_data_kernel<{_lp_name(g.lp)}>", vox * (16.0 * ci * ci + 8 * 54.0 * ci * co),
                         2.0 * vox * (gin.cp + 8 * g.cp), (w, gin.cp, g.cp))):
        _lib.check(_lib.load().ctu_lp_upconv_fused_bwd_data(g.lp, g.ptr, g.cs, wp16.data_ptr(), gin.ptr, gin.cs, gin.cp,
                                                            n, d, h, w, _stream()), "lp_upconv_fused_bwd_data")


def upconv_fused_pack_bwd(wp: torch.Tensor, cin_p: int, nout_p: int, into: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    wpd = into if into is not None else torch.empty(lib.ctu_upconv_fused_bwd_packed_floats(cin_p, nout_p),
                                                     dtype=torch.float32, device=wp.device)
    _lib.check(lib.ctu_upconv_fused_pack_bwd(wp.data_ptr(), cin_p, nout_p, wpd.data_ptr(), _stream()), "upconv_fused_pack_bwd")
    return wpd


def upconv_fused_bwd_data(g: CL, wpd: torch.Tensor, gin, algo_ch: Optional[Tuple[int, int]] = None) -> None:
    """gin (coarse; CL, or CL2: written as two segments, ctu_upconv_fused_bwd_data_seg2) <- gradient of the fused
    ConvTranspose3d -> Conv3d pair w.r.t. its (activated) input."""
    n, d, h, w = gin.dims
    assert g.dims == (n, 2 * d, 2 * h, 2 * w)
    ci, co = algo_ch if algo_ch is not None else (gin.cp, g.cp)
    vox = n * d * h * w
    with _timed(lambda: (f"upconv_fused_bwd_data_kernel<{g.cp}>", vox * (16.0 * ci * ci + 8 * 54.0 * ci * co),
                         4.0 * vox * (ci + 8 * co), (w, gin.cp, g.cp))):
        seg2 = isinstance(gin, CL2)
        entry = getattr(_lib.load(), "ctu_upconv_fused_bwd_data_seg2" if seg2 else "ctu_upconv_fused_bwd_data")
        _lib.check(entry(g.ptr, g.cs, g.cp, wpd.data_ptr(), *(gin.up_args() if seg2 else (gin.ptr, gin.cs, gin.cp)),
                         n, d, h, w, _stream()), "upconv_fused_bwd_data")


# ---------------------------------------------------------------------------- inference tail / sample schema
def _ncv(t: torch.Tensor):
    """(N, C, V) of a contiguous fp32 NCDHW (5-D) or CDHW (4-D) CUDA map."""
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.dim() not in (4, 5):
        raise RuntimeError("ctunet_amd: expected a contiguous float32 CUDA map [N,C,D,H,W] or [C,D,H,W]")
    n = t.shape[0] if t.dim() == 5 else 1
    c = t.shape[1] if t.dim() == 5 else t.shape[0]
    return n, c, t.numel() // (n * c)


def hard_segm(prob: torch.Tensor) -> torch.Tensor:
    """argmax over the class dimension as float32 ([N,D,H,W] or [D,H,W]); first maximum wins."""
    n, c, v = _ncv(prob)
    out = torch.empty(prob.shape[:1] + prob.shape[2:] if prob.dim() == 5 else prob.shape[1:], dtype=torch.float32,
                      device=prob.device)
    _lib.check(_lib.load().ctu_hard_segm(prob.data_ptr(), n, c, v, out.data_ptr(), _stream()), "hard_segm")
    return out


def one_hot(label: torch.Tensor, num_classes: int) -> torch.Tensor:
    """one_hot(label.long(), C).movedim(-1, 1).float() for a float32 CUDA label volume [N,D,H,W]."""
    if label.dtype != torch.float32 or not label.is_cuda or not label.is_contiguous() or label.dim() != 4:
        raise RuntimeError("ctunet_amd: expected a contiguous float32 CUDA label volume [N,D,H,W]")
    n = label.shape[0]
    out = torch.empty((n, num_classes) + tuple(label.shape[1:]), dtype=torch.float32, device=label.device)
    _lib.check(_lib.load().ctu_one_hot(label.data_ptr(), n, num_classes, label.numel() // n, out.data_ptr(), _stream()),
               "one_hot")
    return out


def hard_dice_counts(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """float64 [N, C, 3]: per item and class {|hard & target|, |hard|, |target|}, hard = one_hot(argmax(pred, 1))."""
    n, c, v = _ncv(pred)
    if target.shape != pred.shape or _ncv(target) != (n, c, v):
        raise RuntimeError("ctunet_amd: prediction and one-hot target must have the same shape")
    lib = _lib.load()
    ws = torch.empty(lib.ctu_hard_dice_ws_doubles(n), dtype=torch.float64, device=pred.device)
    counts = torch.empty((n, c, 3), dtype=torch.float64, device=pred.device)
    _lib.check(lib.ctu_hard_dice_counts(pred.data_ptr(), target.data_ptr(), n, c, v, counts.data_ptr(), ws.data_ptr(),
                                        _stream()), "hard_dice_counts")
    return counts


def hausdorff(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """float32 [N, C-1]: symmetric Euclidean Hausdorff distance between the surfaces of argmax(pred, 1) == c and
    target[:, c] for c = 1..C-1 (NaN where either surface is empty)."""
    n, c, v = _ncv(pred)
    if pred.dim() != 5 or target.shape != pred.shape or _ncv(target) != (n, c, v):
        raise RuntimeError("ctunet_amd: hausdorff expects a [N,C,D,H,W] prediction and a one-hot target of the same shape")
    d, h, w = pred.shape[2:]
    lib = _lib.load()
    ws = torch.empty(lib.ctu_hausdorff_ws_bytes(n, c, d, h, w), dtype=torch.uint8, device=pred.device)
    out = torch.empty((n, c - 1), dtype=torch.float32, device=pred.device)
    _lib.check(lib.ctu_hausdorff(pred.data_ptr(), target.data_ptr(), n, c, d, h, w, out.data_ptr(), ws.data_ptr(), _stream()),
               "hausdorff")
    return out


def extract_patches(vol: torch.Tensor, coords: torch.Tensor, patch: Tuple[int, int, int]) -> torch.Tensor:
    """vol [C,D,H,W] float32 CUDA, coords int32 CUDA [P,3] (z0,y0,x0) -> [P,C,pd,ph,pw] (zero outside the volume)."""
    _need_cuda(vol, "volume")
    _need_cuda(coords, "patch coordinates")
    if vol.dim() != 4 or coords.dim() != 2 or coords.shape[1] != 3 or coords.dtype != torch.int32:
        raise RuntimeError("ctunet_amd: extract_patches expects vol [C,D,H,W] and int32 coords [P,3]")
    vol, coords = vol.contiguous(), coords.contiguous()
    c, d, h, w = vol.shape
    p = coords.shape[0]
    out = torch.empty((p, c) + tuple(patch), dtype=torch.float32, device=vol.device)
    _lib.check(_lib.load().ctu_extract_patches(vol.data_ptr(), coords.data_ptr(), p, c, d, h, w, patch[0], patch[1], patch[2],
                                               out.data_ptr(), _stream()), "extract_patches")
    return out


def stitch_patches(patches: torch.Tensor, coords: torch.Tensor, shape: Tuple[int, int, int]) -> torch.Tensor:
    """patches [P,C,pd,ph,pw] + coords -> [C,D,H,W]: mean over the patches covering each voxel."""
    _need_cuda(patches, "patches")
    _need_cuda(coords, "patch coordinates")
    if patches.dim() != 5 or coords.shape != (patches.shape[0], 3) or coords.dtype != torch.int32:
        raise RuntimeError("ctunet_amd: stitch_patches expects patches [P,C,pd,ph,pw] and int32 coords [P,3]")
    patches, coords = patches.contiguous(), coords.contiguous()
    p, c, pd, ph, pw = patches.shape
    out = torch.empty((c,) + tuple(shape), dtype=torch.float32, device=patches.device)
    _lib.check(_lib.load().ctu_stitch_patches(patches.data_ptr(), coords.data_ptr(), p, c, shape[0], shape[1], shape[2], pd, ph,
                                              pw, out.data_ptr(), _stream()), "stitch_patches")
    return out


def window_accumulate(patches: torch.Tensor, coords: torch.Tensor, valid: torch.Tensor, box: torch.Tensor,
                      tables: Tuple[torch.Tensor, torch.Tensor, torch.Tensor], wmin: float, extent: Tuple[int, int, int],
                      num: torch.Tensor, wsum: Optional[torch.Tensor]) -> None:
    """Blend one batch of patch predictions [B,K,pd,ph,pw] into num [K,D,H,W] (and wsum [D,H,W] unless None), in place:
    w = max(wz[i]*wy[j]*wx[k], wmin) per patch-local voxel, num += w*y, wsum += w over the valid patches in order.
    coords int32 [B,3], valid int32 [B], box int32 [3] (bounding-box origin, x a multiple of 4) live on the device;
    extent = (bz, by, bx) the launch covers from that origin."""
    for t, nm in ((patches, "patches"), (coords, "coordinates"), (valid, "valid flags"), (box, "box origin"), (num, "num")):
        _need_cuda(t, nm)
        assert t.is_contiguous(), nm
    assert wsum is None or (wsum.is_cuda and wsum.dtype == torch.float32 and wsum.is_contiguous())
    b, k, pd, ph, pw = patches.shape
    _, d, h, w = num.shape
    wz, wy, wx = tables
    assert num.shape[0] == k and (wsum is None or wsum.shape == num.shape[1:]), "accumulator shapes"
    assert coords.shape == (b, 3) and valid.numel() == b and box.numel() == 3 and coords.dtype == torch.int32
    assert all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
               for t, n in zip(tables, (pd, ph, pw))), "weight tables"
    _lib.check(_lib.load().ctu_window_accumulate(patches.data_ptr(), coords.data_ptr(), valid.data_ptr(), box.data_ptr(), b,
                                                 k, d, h, w, pd, ph, pw, wz.data_ptr(), wy.data_ptr(), wx.data_ptr(),
                                                 float(wmin), extent[0], extent[1], extent[2], num.data_ptr(), _ptr(wsum),
                                                 _stream()), "window_accumulate")


def window_finalize(num: torch.Tensor, wsum: torch.Tensor, probs: torch.Tensor,
                    labels: Optional[torch.Tensor] = None) -> None:
    """probs [K,D,H,W] = num / wsum (0 where wsum == 0; probs may be num), labels uint8 [D,H,W] = first argmax over K."""
    _need_cuda(num, "num")
    _need_cuda(wsum, "wsum")
    _need_cuda(probs, "probs")
    k = num.shape[0]
    v = wsum.numel()
    assert num.is_contiguous() and wsum.is_contiguous() and probs.is_contiguous() and num.numel() == k * v == probs.numel()
    assert labels is None or (labels.is_cuda and labels.dtype == torch.uint8 and labels.numel() == v and labels.is_contiguous())
    _lib.check(_lib.load().ctu_window_finalize(num.data_ptr(), wsum.data_ptr(), k, v, probs.data_ptr(), _ptr(labels),
                                               _stream()), "window_finalize")


def _flip_word(flip: torch.Tensor) -> torch.Tensor:
    if not (flip.is_cuda and flip.dtype == torch.int32 and flip.numel() == 1):
        raise RuntimeError("ctunet_amd: the flip word must be one int32 on the GPU")
    return flip


def extract_patches_flip(vol: torch.Tensor, coords: torch.Tensor, patch: Tuple[int, int, int],
                         flip: torch.Tensor) -> torch.Tensor:
    """extract_patches with every patch mirrored on the axes of the flip word (device int32 [1]: bit 0 = x, 1 = y, 2 = z);
    the zero padding of an overhanging tile is mirrored with it.  At flip 0 the bits of extract_patches.  16-byte row
    accesses where the volume row allows; patch[2] a multiple of 4."""
    _need_cuda(vol, "volume")
    _need_cuda(coords, "patch coordinates")
    if vol.dim() != 4 or coords.dim() != 2 or coords.shape[1] != 3 or coords.dtype != torch.int32:
        raise RuntimeError("ctunet_amd: extract_patches_flip expects vol [C,D,H,W] and int32 coords [P,3]")
    vol, coords = vol.contiguous(), coords.contiguous()
    c, d, h, w = vol.shape
    p = coords.shape[0]
    out = torch.empty((p, c) + tuple(patch), dtype=torch.float32, device=vol.device)
    _lib.check(_lib.load().ctu_extract_patches_flip(vol.data_ptr(), coords.data_ptr(), _flip_word(flip).data_ptr(), p, c, d, h,
                                                    w, patch[0], patch[1], patch[2], out.data_ptr(), _stream()),
               "extract_patches_flip")
    return out


def window_accumulate_flip(patches: torch.Tensor, coords: torch.Tensor, valid: torch.Tensor, box: torch.Tensor,
                           flip: torch.Tensor, tables: Tuple[torch.Tensor, torch.Tensor, torch.Tensor], wmin: float,
                           extent: Tuple[int, int, int], num: torch.Tensor, wsum: Optional[torch.Tensor],
                           sq: Optional[torch.Tensor] = None, sh: Optional[torch.Tensor] = None) -> None:
    """window_accumulate for a mirrored pass: the patch predictions are read at the mirrored patch-local index (flip:
    device int32 [1]), the weights at the un-mirrored one.  sq [K,D,H,W]: also sq += w*y*y; sh [D,H,W]: also
    sh += w*h(y), the normalised entropy of the contribution (K >= 2)."""
    for t, nm in ((patches, "patches"), (coords, "coordinates"), (valid, "valid flags"), (box, "box origin"), (num, "num")):
        _need_cuda(t, nm)
        assert t.is_contiguous(), nm
    b, k, pd, ph, pw = patches.shape
    _, d, h, w = num.shape
    wz, wy, wx = tables
    for t, shp in ((wsum, num.shape[1:]), (sq, num.shape), (sh, num.shape[1:])):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == shp), "accumulators"
    assert num.shape[0] == k, "accumulator shapes"
    assert coords.shape == (b, 3) and valid.numel() == b and box.numel() == 3 and coords.dtype == torch.int32
    assert all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
               for t, n in zip(tables, (pd, ph, pw))), "weight tables"
    _lib.check(_lib.load().ctu_window_accumulate_flip(patches.data_ptr(), coords.data_ptr(), valid.data_ptr(), box.data_ptr(),
                                                      _flip_word(flip).data_ptr(), b, k, d, h, w, pd, ph, pw, wz.data_ptr(),
                                                      wy.data_ptr(), wx.data_ptr(), float(wmin), extent[0], extent[1],
                                                      extent[2], num.data_ptr(), _ptr(wsum), _ptr(sq), _ptr(sh), _stream()),
               "window_accumulate_flip")


def window_finalize_stats(num: torch.Tensor, wsum: torch.Tensor, probs: torch.Tensor, labels: Optional[torch.Tensor] = None,
                          sq: Optional[torch.Tensor] = None, sh: Optional[torch.Tensor] = None,
                          var: Optional[torch.Tensor] = None, ent: Optional[torch.Tensor] = None,
                          mi: Optional[torch.Tensor] = None) -> None:
    """window_finalize plus var [K,D,H,W] = max(sq/wsum - probs^2, 0) (may be sq), ent [D,H,W] = h(probs) and
    mi [D,H,W] = max(h(probs) - sh/wsum, 0), each only where given; everything 0 where wsum == 0."""
    _need_cuda(num, "num")
    _need_cuda(wsum, "wsum")
    _need_cuda(probs, "probs")
    k = num.shape[0]
    v = wsum.numel()
    assert num.is_contiguous() and wsum.is_contiguous() and probs.is_contiguous() and num.numel() == k * v == probs.numel()
    assert labels is None or (labels.is_cuda and labels.dtype == torch.uint8 and labels.numel() == v and labels.is_contiguous())
    for t, n in ((sq, k * v), (var, k * v), (sh, v), (ent, v), (mi, v)):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n), "statistics"
    _lib.check(_lib.load().ctu_window_finalize_stats(num.data_ptr(), wsum.data_ptr(), _ptr(sq), _ptr(sh), k, v, probs.data_ptr(),
                                                     _ptr(labels), _ptr(var), _ptr(ent), _ptr(mi), _stream()),
               "window_finalize_stats")


def _tensor_table(tensors):
    """(pointer array, element-count array, length) over the tensors of a list that are not None: the first three arguments
    of ctu_scale_tensors / ctu_unscale_tensors."""
    ts = [t for t in tensors if t is not None]
    for t in ts:
        _need_cuda(t, "tensor")
        assert t.is_contiguous() and t.dtype == torch.float32
    return ((ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), (ctypes.c_int64 * len(ts))(*[t.numel() for t in ts]),
            len(ts))


def scale_tensors(tensors, s: float, nonfinite: Optional[torch.Tensor] = None) -> None:
    """Every float32 CUDA tensor of the list scaled in place by s, one launch (un-scaling of loss-scaled gradients).
    nonfinite: float32[1] device flag set to 1 when any scaled value is inf / NaN (fp16 overflow detection)."""
    pa, sa, n = _tensor_table(tensors)
    if not n:
        return
    assert nonfinite is None or (nonfinite.is_cuda and nonfinite.dtype == torch.float32 and nonfinite.numel() == 1)
    _lib.check(_lib.load().ctu_scale_tensors(pa, sa, n, float(s), _ptr(nonfinite), _stream()), "scale_tensors")


def unscale_tensors(tensors, scale: torch.Tensor, found_inf: torch.Tensor) -> None:
    """Every float32 CUDA tensor of the list multiplied in place by 1 / scale[0] (scale: the float32[1] device loss scale
    of dynamic loss scaling), one launch; found_inf (float32[1] device flag) is set on inf / NaN and never cleared here."""
    pa, sa, n = _tensor_table(tensors)
    if not n:
        return
    for f in (scale, found_inf):
        assert f.is_cuda and f.dtype == torch.float32 and f.numel() == 1
    _lib.check(_lib.load().ctu_unscale_tensors(pa, sa, n, scale.data_ptr(), found_inf.data_ptr(), _stream()),
               "unscale_tensors")


FLAP_CHUNK = 8192          # CTU_FLAP_CHUNK of ctunet_hip.h
FLAP_RECORD = 16           # CTU_FLAP_RECORD
FLAP_HOLE, FLAP_NOISE = 1, 2


def _skull_kind(t: torch.Tensor, name: str) -> int:
    if not t.is_cuda:
        raise RuntimeError(f"ctunet_amd: {name} must live on the GPU (MI355X); this path has no CPU fallback")
    if t.dtype not in (torch.float32, torch.uint8):
        raise RuntimeError(f"ctunet_amd: {name} must be float32 or uint8, got {t.dtype}")
    assert t.is_contiguous(), name
    return int(t.dtype == torch.uint8)


def flap_count(skulls: torch.Tensor, counts: torch.Tensor) -> None:
    """counts int32 [N, ceil(V / FLAP_CHUNK)] = bone voxels per chunk of each sample of skulls [N,1,D,H,W]."""
    u8 = _skull_kind(skulls, "skulls")
    n, v = skulls.shape[0], skulls[0].numel()
    assert counts.is_cuda and counts.dtype == torch.int32 and counts.numel() == n * -(-v // FLAP_CHUNK)
    _lib.check(_lib.load().ctu_flap_count(skulls.data_ptr(), u8, n, v, counts.data_ptr(), _stream()), "flap_count")


def flap_draw(skulls: torch.Tensor, counts: Optional[torch.Tensor], mode: int, hole_seq: Optional[torch.Tensor],
              hole_seed: int, p_hole: float, size_range: Tuple[int, int], shapes: int, noise_seq: Optional[torch.Tensor],
              noise_nd: Optional[torch.Tensor], noise_seed: int, p_noise: float, salt_ratio: float, decay: bool,
              params: torch.Tensor) -> None:
    """params int32 [N, FLAP_RECORD] = the per-sample records (layout: ctunet_hip.h), drawn from the device counters."""
    u8 = _skull_kind(skulls, "skulls")
    n, _, d, h, w = skulls.shape
    assert params.is_cuda and params.dtype == torch.int32 and params.numel() == n * FLAP_RECORD
    _lib.check(_lib.load().ctu_flap_draw(skulls.data_ptr(), u8, n, d, h, w, _ptr(counts), mode, _ptr(hole_seq),
                                         hole_seed, float(p_hole), size_range[0], size_range[1], shapes, _ptr(noise_seq),
                                         _ptr(noise_nd), noise_seed, float(p_noise), float(salt_ratio), int(decay),
                                         params.data_ptr(), _stream()), "flap_draw")


def flap_apply(skulls: torch.Tensor, atlas: Optional[torch.Tensor], params: torch.Tensor, mode: int,
               hole_seq: Optional[torch.Tensor], noise_seq: Optional[torch.Tensor], noise_nd: Optional[torch.Tensor],
               noise_seed: int, decay: bool, x: torch.Tensor, full: Optional[torch.Tensor],
               flap: Optional[torch.Tensor]) -> None:
    """x [N,C,D,H,W] (image, + atlas channel), full / flap [N,2,D,H,W] one-hot targets, from the records; advances the
    device counters (and the density with decay)."""
    u8 = _skull_kind(skulls, "skulls")
    n, _, d, h, w = skulls.shape
    for t, nm, c in ((x, "x", x.shape[1]), (full, "full-skull target", 2), (flap, "flap target", 2)):
        if t is None:
            continue
        _need_cuda(t, nm)
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (n, c, d, h, w), nm
    if atlas is not None:
        _need_cuda(atlas, "atlas")
        assert atlas.is_contiguous() and atlas.numel() == d * h * w, "atlas [D,H,W]"
    _lib.check(_lib.load().ctu_flap_apply(skulls.data_ptr(), u8, _ptr(atlas), n, d, h, w, params.data_ptr(), mode,
                                          _ptr(hole_seq), _ptr(noise_seq), _ptr(noise_nd), noise_seed, int(decay),
                                          x.data_ptr(), x.shape[1], _ptr(full), _ptr(flap), _stream()), "flap_apply")


DEFECT_RECORD = 64                               # CTU_DEFECT_RECORD of ctunet_hip.h
DEFECT_MAX_BALLS, DEFECT_MAX_LATTICE = 12, 64    # CTU_DEFECT_MAX_BALLS / CTU_DEFECT_MAX_LATTICE
DILATE_MAX_ITERATIONS = 3                        # CTU_DILATE_MAX_ITERATIONS


def _defect_buffers(n: int, grid: Tuple[int, int, int], record: torch.Tensor, lattice: torch.Tensor) -> None:
    for t, nm, numel in ((record, "record", n * DEFECT_RECORD), (lattice, "lattice", n * grid[0] * grid[1] * grid[2])):
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == numel, f"defect {nm}"


def defect_draw(skulls: torch.Tensor, counts: torch.Tensor, spacing, seq: torch.Tensor, seed: int, p: float, ranges,
                balls: Tuple[int, int], grid: Tuple[int, int, int], record: torch.Tensor, lattice: torch.Tensor) -> None:
    """record float64 [N, DEFECT_RECORD] and lattice float64 [N, Gz, Gy, Gx] of the N skulls, drawn from the device counter
    seq behind flap_count's counts (layout and rule: ctunet_hip.h, transforms.py).  ranges: the 6 host doubles of
    ctu_defect_draw.  One launch."""
    u8 = _skull_kind(skulls, "skulls")
    n, _, d, h, w = skulls.shape
    _defect_buffers(n, grid, record, lattice)
    assert counts.is_cuda and counts.dtype == torch.int32 and counts.numel() == n * -(-d * h * w // FLAP_CHUNK)
    assert seq.is_cuda and seq.dtype == torch.int64 and seq.numel() == 1 and len(ranges) == 6
    _lib.check(_lib.load().ctu_defect_draw(skulls.data_ptr(), u8, n, d, h, w, _lib.double_array(spacing), counts.data_ptr(),
                                           seq.data_ptr(), seed, float(p), _lib.double_array(ranges), balls[0], balls[1],
                                           grid[0], grid[1], grid[2], record.data_ptr(), lattice.data_ptr(), _stream()),
               "defect_draw")


def defect_apply(skulls: torch.Tensor, atlas: Optional[torch.Tensor], spacing, record: torch.Tensor, lattice: torch.Tensor,
                 grid: Tuple[int, int, int], scale: float, amp: float, params: Optional[torch.Tensor], mode: int,
                 hole_seq: torch.Tensor, noise_seq: Optional[torch.Tensor], noise_nd: Optional[torch.Tensor],
                 noise_seed: int, decay: bool, x: torch.Tensor, full: Optional[torch.Tensor],
                 flap: Optional[torch.Tensor]) -> None:
    """flap_apply's pass with the records' defects as the holes (params: flap_draw's noise records, or None); advances the
    device counters (and the density with decay)."""
    u8 = _skull_kind(skulls, "skulls")
    n, _, d, h, w = skulls.shape
    _defect_buffers(n, grid, record, lattice)
    for t, nm, c in ((x, "x", x.shape[1]), (full, "full-skull target", 2), (flap, "flap target", 2)):
        if t is None:
            continue
        _need_cuda(t, nm)
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (n, c, d, h, w), nm
    if atlas is not None:
        _need_cuda(atlas, "atlas")
        assert atlas.is_contiguous() and atlas.numel() == d * h * w, "atlas [D,H,W]"
    if params is not None:
        assert params.is_cuda and params.dtype == torch.int32 and params.numel() == n * FLAP_RECORD
    _lib.check(_lib.load().ctu_defect_apply(skulls.data_ptr(), u8, _ptr(atlas), n, d, h, w, _lib.double_array(spacing),
                                            record.data_ptr(), lattice.data_ptr(), grid[0], grid[1], grid[2], float(scale),
                                            float(amp), _ptr(params), mode, hole_seq.data_ptr(), _ptr(noise_seq),
                                            _ptr(noise_nd), noise_seed, int(decay), x.data_ptr(), x.shape[1], _ptr(full),
                                            _ptr(flap), _stream()), "defect_apply")


def random_dilate(x: torch.Tensor, out: torch.Tensor, iterations: int, seq: torch.Tensor, seed: int, p: float) -> None:
    """out uint8 [N,1,D,H,W] = the bone of x (uint8 / float32) dilated by `iterations` steps of the 6-neighbour cross for
    the samples drawn with probability p from the device counter seq, which advances by N.  One gather launch."""
    _skull_kind(x, "x")
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.shape == x.shape, "random_dilate out"
    assert x.dim() == 5 and x.shape[1] == 1, "random_dilate x"
    assert seq.is_cuda and seq.dtype == torch.int64 and seq.numel() == 1
    n, _, d, h, w = x.shape
    _lib.check(_lib.load().ctu_random_dilate(x.data_ptr(), _lib.DTYPE_CODE[x.dtype], n, d, h, w, int(iterations),
                                             seq.data_ptr(), seed, float(p), out.data_ptr(), _stream()), "random_dilate")


RESAMPLE_NEAREST, RESAMPLE_LINEAR, RESAMPLE_LABEL_LINEAR = 0, 1, 2          # CTU_RESAMPLE_* of ctunet_hip.h
RESAMPLE_CODE = _lib.DTYPE_CODE              # the dtype codes of ctu_resample


def resample(x: torch.Tensor, out: torch.Tensor, mode: int, num_classes: int, n: int, in_shape: Tuple[int, int, int],
             out_shape: Tuple[int, int, int], tables: Tuple[torch.Tensor, torch.Tensor, torch.Tensor]) -> None:
    """out [n, d, h, w] = x [n, D, H, W] resampled through the device tables (i0 int32, wt float32, near int32, each the
    z, y and x table of the output grid one after the other; rule: ctunet_amd/resample.py).  One launch, nothing allocated."""
    for t, nm in ((x, "input"), (out, "output")):
        if not t.is_cuda:
            raise RuntimeError(f"ctunet_amd: resample {nm} must live on the GPU (MI355X); this path has no CPU fallback")
        assert t.is_contiguous(), nm
    (d0, h0, w0), (d1, h1, w1) = in_shape, out_shape
    assert x.numel() == n * d0 * h0 * w0 and out.numel() == n * d1 * h1 * w1, "resample shapes"
    i0, wt, near = tables
    assert all(t.is_cuda and t.is_contiguous() and t.numel() == d1 + h1 + w1 for t in tables), "resample tables"
    assert i0.dtype == torch.int32 and near.dtype == torch.int32 and wt.dtype == torch.float32, "resample tables"
    _lib.check(_lib.load().ctu_resample(x.data_ptr(), RESAMPLE_CODE[x.dtype], mode, num_classes, n, d0, h0, w0, d1, h1, w1,
                                        i0.data_ptr(), wt.data_ptr(), near.data_ptr(), out.data_ptr(), _stream()),
               "resample")


def affine_resample(x: torch.Tensor, out: torch.Tensor, mode: int, num_classes: int, n: int, in_shape: Tuple[int, int, int],
                    out_shape: Tuple[int, int, int], matrix: torch.Tensor, spacing, origin, out_spacing, out_origin,
                    fill: float) -> None:
    """out [n, d, h, w] = x [n, D, H, W] pulled through the DEVICE float64 matrix [3,4] / [4,4] (output world -> input world;
    rule: ctunet_amd/resample.py).  spacing .. out_origin: host (z, y, x) triples or None.  One launch, nothing allocated."""
    for t, nm in ((x, "input"), (out, "output"), (matrix, "matrix")):
        if not t.is_cuda:
            raise RuntimeError(f"ctunet_amd: affine_resample {nm} must live on the GPU (MI355X); this path has no CPU fallback")
        assert t.is_contiguous(), nm
    (d0, h0, w0), (d1, h1, w1) = in_shape, out_shape
    assert x.numel() == n * d0 * h0 * w0 and out.numel() == n * d1 * h1 * w1, "affine_resample shapes"
    assert matrix.dtype == torch.float64 and matrix.numel() in (12, 16), "affine_resample matrix"
    _lib.check(_lib.load().ctu_affine_resample(x.data_ptr(), RESAMPLE_CODE[x.dtype], mode, num_classes, n, d0, h0, w0, d1, h1,
                                               w1, matrix.data_ptr(), _lib.double_array(spacing), _lib.double_array(origin),
                                               _lib.double_array(out_spacing), _lib.double_array(out_origin), float(fill),
                                               out.data_ptr(), _stream()), "affine_resample")


SPATIAL_RECORD = 26                              # CTU_SPATIAL_RECORD of ctunet_hip.h
SPATIAL_MIN_POINTS, SPATIAL_MAX_POINTS = 4, 12   # CTU_SPATIAL_MIN_POINTS / CTU_SPATIAL_MAX_POINTS


def _spatial_buffers(n: int, grid: Tuple[int, int, int], record: torch.Tensor, control: torch.Tensor) -> None:
    for t, nm, numel in ((record, "record", n * SPATIAL_RECORD), (control, "control", n * 3 * grid[0] * grid[1] * grid[2])):
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == numel, f"spatial {nm}"


def spatial_draw(n: int, shape: Tuple[int, int, int], spacing, seq: torch.Tensor, seed: int, flip_mask: int, flip_p: float,
                 affine_p: float, elastic_p: float, ranges, grid: Tuple[int, int, int], locked: int, record: torch.Tensor,
                 control: torch.Tensor) -> None:
    """record float64 [N, SPATIAL_RECORD] and control float64 [N, 3, Gz, Gy, Gx] of N samples, drawn from the device counter
    seq (layout and rule: ctunet_hip.h, transforms.py).  ranges: the 11 host doubles of ctu_spatial_draw.  One launch."""
    _spatial_buffers(n, grid, record, control)
    assert seq.is_cuda and seq.dtype == torch.int64 and seq.numel() == 1 and len(ranges) == 11
    _lib.check(_lib.load().ctu_spatial_draw(n, shape[0], shape[1], shape[2], _lib.double_array(spacing), seq.data_ptr(), seed,
                                            flip_mask, float(flip_p), float(affine_p), float(elastic_p),
                                            _lib.double_array(ranges), grid[0], grid[1], grid[2], locked,
                                            record.data_ptr(), control.data_ptr(), _stream()), "spatial_draw")


def spatial_warp(x: torch.Tensor, out: torch.Tensor, spacing, grid: Tuple[int, int, int], record: torch.Tensor,
                 control: torch.Tensor, seq: torch.Tensor) -> None:
    """out [N,C,D,H,W] = x warped by the samples' records and control grids (uint8 or float32, nearest, fill 0); advances
    the device counter seq by N.  One launch, nothing allocated."""
    for t, nm in ((x, "input"), (out, "output")):
        if not t.is_cuda:
            raise RuntimeError(f"ctunet_amd: spatial_warp {nm} must live on the GPU (MI355X); this path has no CPU fallback")
        assert t.is_contiguous() and t.dim() == 5, nm
    assert x.dtype in (torch.uint8, torch.float32) and out.dtype == x.dtype and out.shape == x.shape, "spatial_warp tensors"
    n, c, d, h, w = x.shape
    _spatial_buffers(n, grid, record, control)
    assert seq.is_cuda and seq.dtype == torch.int64 and seq.numel() == 1
    _lib.check(_lib.load().ctu_spatial_warp(x.data_ptr(), RESAMPLE_CODE[x.dtype], n, c, d, h, w, _lib.double_array(spacing),
                                            grid[0], grid[1], grid[2], record.data_ptr(), control.data_ptr(), seq.data_ptr(),
                                            out.data_ptr(), _stream()), "spatial_warp")
