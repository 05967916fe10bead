"""Launch plans of the stand-alone ConvTranspose3d(k = 2, s = 2) kernels (no GPU: the library's host-only plan queries).

csrc/convt.hip (fp32) and csrc/convt_lp.hip (bf16 / fp16) pick their instantiation, grid, staging depth and chunks per block
from the geometry.  This file checks that
  * the plan queries (ctu_convt2_plan, ctu_convt2_wgrad_plan, ctu_lp_convt2_plan, ctu_lp_convt2_wgrad_plan: the functions
    the launchers themselves read) reproduce the launch arithmetic the launchers carried inline before, over a sweep,
  * every case of tests/test_convt_plans_gpu.py still lands on the plan it names,
  * every plan the shipped classes reach at their benchmark sizes, at the levels the engine does not fuse, has a GPU case,
  * cases that claim a partial last block / chunk / wave have a voxel count that leaves one,
  * the entry points refuse rin_p > 128, which the forward / data-gradient kernel's staging does not cover."""
import ctypes
from collections import namedtuple
from types import SimpleNamespace

import pytest

# dtype, logical Ci -> Co, coarse N, D, H, W, segs (((n logical, padded start), ...) of a concat input with holes, or None),
# the plan the case is there for (see plan_key)
Case = namedtuple("Case", "dtype Ci Co N D H W segs plan")
Plan = namedtuple("Plan", "fwd dgrad wgrad")
RPARTS = 16                # common.h: thread groups of the slab reductions


def cdiv(a, b):
    return -(-a // b)


def pad8(c):
    return cdiv(c, 8) * 8


def _lib():
    from ctunet_amd import _lib as L
    return L.load()


def cin_p(c):
    return pad8(c.Ci) if c.segs is None else pad8(c.segs[-1][1] + c.segs[-1][0])


def _query(fn, n, *args):
    buf = (ctypes.c_int * n)()
    name = fn(*args, buf)
    return None if name is None else (name.decode(),) + tuple(buf)


def plans(dtype, rin, nout, N, D, H, W):
    """The three launches of a transposed conv with rin padded input and nout padded output channels on a coarse N x D x H x W
    grid, as the library plans them.  fp32: fwd / dgrad = (name, grid.x, grid.y, tps, lds), wgrad = (name, gx, grid.y, ntiles);
    16-bit: fwd / dgrad = (name, grid.x, grid.y), wgrad = (name, gx, grid.y, chunks per block, lds)."""
    L = _lib()
    if dtype == "fp32":
        return Plan(_query(L.ctu_convt2_plan, 4, 0, rin, nout, N, D, H, W), _query(L.ctu_convt2_plan, 4, 1, nout, rin, N, D, H, W),
                    _query(L.ctu_convt2_wgrad_plan, 3, rin, nout, N, D, H, W))
    return Plan(_query(L.ctu_lp_convt2_plan, 2, 0, rin, nout, N, D, H, W), _query(L.ctu_lp_convt2_plan, 2, 1, nout, rin, N, D, H, W),
                _query(L.ctu_lp_convt2_wgrad_plan, 4, rin, nout, N, D, H, W))


def plan_keys(dtype, p):
    """What distinguishes one launch plan from another, per family: (family, instantiation, split / un-split grid, tps) for
    forward and data gradient, (family, instantiation, more than one tile trip or chunk per block) for the weight gradient."""
    if dtype == "fp32":
        return {("fp32:fwd", p.fwd[0], p.fwd[2] > 1, p.fwd[3]), ("fp32:dgrad", p.dgrad[0], p.dgrad[2] > 1, p.dgrad[3]),
                ("fp32:wgrad", p.wgrad[0], p.wgrad[3] > p.wgrad[1])}
    return {("lp:fwd", p.fwd[0], p.fwd[2] > 1, 0), ("lp:dgrad", p.dgrad[0], p.dgrad[2] > 1, 0), ("lp:wgrad", p.wgrad[0], p.wgrad[3] > 1)}


def case_plans(c):
    return plans(c.dtype, cin_p(c), pad8(c.Co), c.N, c.D, c.H, c.W)


# ------------------------------------------------------------------ the launch arithmetic as the launchers carried it inline
def old_convt(rin, nout, nvox):
    """launch_convt of convt.hip before the plan functions: (ntt, grid.x, grid.y, tps, lds)."""
    n16 = cdiv(nout, 16)
    ntt_total = 1 if n16 <= 1 else (2 if n16 <= 2 else (4 if n16 <= 4 else 8))
    grid = cdiv(nvox, 64)
    ntt = ntt_total
    while ntt > 1 and grid * (ntt_total // ntt) < 256:
        ntt >>= 1
    a_b = 64 * (rin + 4) * 4
    w_b = (rin // 8) * ntt * 128 * 4
    tps = 8
    while tps > 1 and a_b + tps * w_b > 72 * 1024:
        tps >>= 1
    return ntt, grid, ntt_total // ntt, tps, a_b + tps * w_b


def old_convt_wgrad(cip, cop, nvox):
    """ct_wgrad_geom / ct_wgrad_gx: (mi, nj, gx, grid.y, ntiles)."""
    mi, nj = (2 if cip > 16 else 1), (2 if cop > 16 else 1)
    pairs = cdiv(cip, 16 * mi) * cdiv(cop, 16 * nj)
    ntiles = cdiv(nvox, 64)
    return mi, nj, min(max(512 // pairs, 1), ntiles), pairs, ntiles


def old_lp_convt(mode, rin, nout, nvox):
    """ctu_lp_convt2_fwd / ctu_lp_convt2_bwd_data: (name, grid.x, grid.y)."""
    wide = nvox > 65536
    gx = cdiv(nvox, 256 if wide else 64)
    n16 = cdiv(nout, 16)
    if mode == 0:
        return f"lp_convt_fwd_kernel<T, {min(cdiv(rin, 32), 8)}, {4 if wide else 1}>", gx, (n16 if gx < 256 else 1)
    passes = (n16 + 1) >> 1
    return f"lp_convt_bwd_data_kernel<T, {4 if wide else 1}>", gx, (passes if gx < 256 and passes > 1 else 1)


def old_lp_convt_wgrad(cip, cop, nvox):
    """ctw_grid and the mt / ntl choice of ctu_lp_convt2_wgrad: (name, gx, grid.y, chunks per block, lds)."""
    nci, nco = cdiv(cip, 16), cdiv(cop, 16)
    nchunks = cdiv(nvox, 128)
    g = min(max(1024 // (nci * nco), 16), nchunks)
    cpb = cdiv(nchunks, g)
    mt4 = nci >= 4
    mt, ntl = (4 if mt4 else (2 if nci >= 2 else 1)), (1 if mt4 else (2 if nco >= 2 else 1))
    return (f"lp_convt_wgrad_kernel<T, {mt}, {ntl}>", cdiv(nchunks, cpb), cdiv(nci, mt) * cdiv(nco, ntl), cpb,
            512 + 128 * mt * 32 + 8 * 128 * ntl * 32)


SWEEP_DIMS = [(1, 1, 1, 1), (1, 2, 3, 5), (2, 6, 10, 11), (1, 8, 8, 8), (1, 16, 16, 16), (2, 16, 16, 16), (1, 6, 20, 20), (1, 10, 20, 33),
              (1, 12, 30, 33), (1, 16, 32, 32), (1, 17, 31, 31), (1, 16, 32, 33), (1, 24, 40, 41), (1, 32, 32, 64), (1, 32, 64, 32),
              (1, 33, 45, 45), (2, 33, 45, 45), (1, 64, 64, 64), (2, 64, 64, 64), (1, 96, 96, 96), (1, 128, 128, 128), (2, 128, 128, 128)]
SWEEP_CH = (8, 16, 24, 32, 40, 48, 56, 64, 72, 96, 128, 136, 160, 192, 256)


def test_queries_reproduce_the_inline_launch_arithmetic():
    """Over channel counts x volumes (both sides of every threshold: 256 blocks, 65536 voxels, 512 / 1024 slabs): the plan the
    launchers now read equals what they computed inline, and the workspace queries agree with the planned grids."""
    L = _lib()
    seen = 0
    for (N, D, H, W) in SWEEP_DIMS:
        nvox = N * D * H * W
        for rin in SWEEP_CH:
            for nout in SWEEP_CH:
                lp = plans("bf16", rin, nout, N, D, H, W)
                assert lp.fwd == old_lp_convt(0, rin, nout, nvox), (rin, nout, N, D, H, W)
                assert lp.dgrad == old_lp_convt(1, nout, rin, nvox), (rin, nout, N, D, H, W)
                assert lp.wgrad == old_lp_convt_wgrad(rin, nout, nvox), (rin, nout, N, D, H, W)
                assert L.ctu_lp_convt2_wgrad_ws_floats(N, D, H, W, rin, nout) == lp.wgrad[1] * cdiv(rin, 16) * cdiv(nout, 16) * 2048
                mi, nj, gx, gy, ntiles = old_convt_wgrad(rin, nout, nvox)
                wg = _query(L.ctu_convt2_wgrad_plan, 3, rin, nout, N, D, H, W)
                assert wg == (f"convt2_wgrad_kernel<{mi}, {nj}>", gx, gy, ntiles), (rin, nout, N, D, H, W)
                assert L.ctu_convt2_wgrad_ws_floats(N, D, H, W, rin, nout) == gy * gx * 8 * mi * nj * 256 + cdiv(nout, 16 * nj) * gx * 16 * nj
                if rin > 128 or nout > 128:
                    continue
                for mode in (0, 1):
                    ntt, gx, gy, tps, lds = old_convt(rin, nout, nvox)
                    got = _query(L.ctu_convt2_plan, 4, mode, rin, nout, N, D, H, W)
                    assert got == (f"convt2_kernel<{ntt}, {mode}>", gx, gy, tps, lds), (mode, rin, nout, N, D, H, W)
                seen += 1
    assert seen > 1000


def test_wide_reduction_sides_are_refused_before_any_launch():
    """The fp32 forward / data-gradient kernel stages 8 float4 items per thread: 64 voxels x rin_p channels only up to
    rin_p = 128.  Wider reduction sides (which no shipped class has while nout_p <= 128) used to pass the argument checks and
    would have left rows 32 .. 63 of the block unstaged; now the entry points and the plan query refuse them."""
    L = _lib()
    fake = ctypes.c_void_p(4096)          # never dereferenced: the argument checks come before anything else
    for rin in (136, 256):
        assert L.ctu_convt2_plan(0, rin, 64, 1, 4, 4, 4, None) is None and L.ctu_convt2_plan(1, rin, 64, 1, 4, 4, 4, None) is None
        assert L.ctu_convt2_fwd(fake, rin, rin, None, None, 0, fake, None, 0, fake, 64, 64, 1, 4, 4, 4, None) != 0
        assert f"convt2_fwd: rin_p={rin} nout_p=64 (multiples of 8, at most 128)" in L.ctu_last_error().decode()
        assert L.ctu_convt2_bwd_data(fake, rin, rin, fake, fake, 64, 64, 1, 4, 4, 4, None) != 0
        assert f"convt2_bwd_data: rout_p={rin} nin_p=64 (multiples of 8, at most 128)" in L.ctu_last_error().decode()
    assert L.ctu_convt2_plan(0, 128, 128, 1, 4, 4, 4, None) == b"convt2_kernel<1, 0>"
    assert L.ctu_convt2_plan(0, 64, 136, 1, 4, 4, 4, None) is None and L.ctu_convt2_plan(2, 64, 64, 1, 4, 4, 4, None) is None
    assert L.ctu_lp_convt2_plan(0, 264, 64, 1, 4, 4, 4, None) is None and L.ctu_lp_convt2_plan(0, 256, 64, 1, 4, 4, 4, None) is not None


# ------------------------------------------------------------------ the GPU table
def gpu_cases():
    import test_convt_plans_gpu as G
    return G.CASES


def test_every_case_lands_on_the_plan_it_names():
    wrong = []
    for c in gpu_cases():
        p = case_plans(c)
        assert None not in p, c
        got = plan_keys(c.dtype, p)
        wrong += [f"{c.dtype} {c.Ci}->{c.Co} {c.N}x{c.D}x{c.H}x{c.W}: names {k}, runs {sorted(got)}" for k in c.plan if k not in got]
    assert not wrong, "cases off their plan (a launcher retune moved them):\n  " + "\n  ".join(wrong)


def test_named_edges_of_the_fp32_cases():
    """The properties the fp32 table is built around, read from the queries: the raised-LDS launch, the slab count past the
    reduce kernel's RPARTS thread groups, half-empty and wholly empty last output tiles, partial channel groups."""
    by = {(c.Ci, c.Co, c.N * c.D * c.H * c.W): case_plans(c) for c in gpu_cases() if c.dtype == "fp32"}
    assert by[(128, 128, 11880)].fwd[4] > 64 * 1024 and by[(128, 128, 11880)].dgrad[4] > 64 * 1024
    assert by[(128, 128, 16337)].fwd[4] > 96 * 1024 and by[(128, 128, 16337)].fwd[2] == 1
    assert by[(128, 128, 6600)].wgrad[1] == 32 and by[(128, 128, 6600)].wgrad[3] == 104
    assert by[(8, 8, 39360)].wgrad[1] == 512 > RPARTS and by[(8, 8, 39360)].wgrad[3] == 615
    # 56 outputs: 4 tiles, the last half empty; 40 outputs: ntt_total 4 for 3 tiles' worth of channels, so one tile of the packed
    # weights lies wholly past nout_p; 24 / 40 inputs resp. outputs: a partial last channel group of the <2, 2> weight gradient
    assert by[(64, 56, 16337)].fwd[0] == "convt2_kernel<4, 0>" and 56 % 16 == 8
    assert by[(24, 40, 16337)].fwd[0] == "convt2_kernel<4, 0>" and cdiv(40, 16) == 3
    assert by[(24, 40, 16337)].dgrad[0] == "convt2_kernel<2, 1>" and 24 % 16 == 8
    assert by[(24, 40, 16337)].wgrad[0] == "convt2_wgrad_kernel<2, 2>" and 24 % 32 and 40 % 32


def test_tail_cases_leave_a_partial_block_chunk_or_wave():
    """fp32 blocks own 64 voxels, 16-bit waves 16 (narrow) or 64 (wide) and blocks 64 / 256, weight-gradient chunks 128: every
    family has a case whose voxel count leaves the last of them partial, and one with a batch boundary inside a block."""
    cases = gpu_cases()
    fp32 = [c for c in cases if c.dtype == "fp32"]
    lp = [c for c in cases if c.dtype != "fp32"]
    nv = lambda c: c.N * c.D * c.H * c.W
    for ntt in (1, 2, 4, 8):
        for mode in (0, 1):
            assert any(nv(c) % 64 and case_plans(c)[mode][0] == f"convt2_kernel<{ntt}, {mode}>" for c in fp32), (ntt, mode)
    for name in ("<1, 1>", "<1, 2>", "<2, 1>", "<2, 2>"):
        assert any(nv(c) % 64 and case_plans(c).wgrad[0] == "convt2_wgrad_kernel" + name for c in fp32), name
    for ctv, unit in ((1, 64), (4, 256)):
        assert any(nv(c) % unit and nv(c) % 16 and case_plans(c).fwd[0].endswith(f", {ctv}>") for c in lp), ctv
        assert any(nv(c) % unit and nv(c) % 16 and case_plans(c).dgrad[0].endswith(f"<T, {ctv}>") for c in lp), ctv
    for name in ("<T, 1, 1>", "<T, 1, 2>", "<T, 2, 1>", "<T, 2, 2>", "<T, 4, 1>"):
        assert any(nv(c) % 128 and case_plans(c).wgrad[0].endswith(name) for c in lp), name
    # chunks per block > 1 with a last block that has fewer chunks than the others and a partial last chunk
    for name in ("<T, 1, 1>", "<T, 2, 2>", "<T, 4, 1>"):
        assert any(nv(c) % 128 and case_plans(c).wgrad[0].endswith(name) and case_plans(c).wgrad[3] > 1
                   and cdiv(nv(c), 128) % case_plans(c).wgrad[3] for c in lp), name
    for group in (fp32, lp):
        assert any(c.N == 2 and (c.D * c.H * c.W) % 64 for c in group)


# ------------------------------------------------------------------ what the shipped classes reach
SIZES = (128, 192, 256)


def class_levels():
    """(class, dtype, batch, rin_p, nout_p, coarse D, H, W) of every decoder level whose up-convolution the engine does NOT fuse,
    for the shipped classes at the benchmark sizes: the decoder walk of UNetEngine.forward with the engine's own _fuse_up."""
    import torch
    from ctunet_amd import engine, models
    from util import CLASS_INPUT
    out = []
    for name in CLASS_INPUT:
        plan = getattr(models, name)()._plan
        nlev = len(plan.enc)
        for size in SIZES:
            for dt in ("fp32", "bf16", "fp16"):
                tdt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[dt]
                for n in (1, 2):
                    s = size >> nlev
                    cur_cp = pad8(plan.center.cout if plan.center_live else plan.enc[-1].cout)
                    for blk in plan.dec:
                        cp = pad8(blk.cout)
                        x = SimpleNamespace(dims=(n, s, s, s), cp=cur_cp)
                        if not engine.UNetEngine._fuse_up(SimpleNamespace(plan=plan, dtype=tdt), x, cp):
                            out.append((name, dt, n, cur_cp, pad8(blk.cin), s, s, s))
                        cur_cp = 2 * cp if plan.skip == "cat" else cp
                        s *= 2
    return out


def test_every_plan_the_shipped_classes_reach_has_a_gpu_case():
    covered = set()
    for c in gpu_cases():
        covered |= plan_keys(c.dtype, case_plans(c))
    reached = {}
    levels = class_levels()
    assert len(levels) > 100
    for (name, dt, n, rin, nout, d, h, w) in levels:
        p = plans(dt, rin, nout, n, d, h, w)
        assert None not in p, (name, dt, n, rin, nout, d, h, w)
        for k in plan_keys(dt, p):
            reached.setdefault(k, f"{name} {dt} batch {n}: {rin}->{nout} at {d}x{h}x{w}")
    missing = [f"{k}  e.g. {eg}" for k, eg in sorted(reached.items()) if k not in covered]
    assert not missing, "transposed-conv plans without a per-op GPU case:\n  " + "\n  ".join(missing)
