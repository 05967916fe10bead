"""The stand-alone ConvTranspose3d(k = 2, s = 2) kernels on every launch plan, against the float64 reference of convt_ref.py.

test_ops_gpu.py::test_convtranspose and test_lowp_gpu.py::test_lp_conv_transpose_forward_dgrad_wgrad stop at 480 resp. 1024
coarse voxels, where csrc/convt.hip and csrc/convt_lp.hip always pick the same launch plan.  The cases below are the
smallest volumes that reach the other plans -- 2 / 4 / 8 output tiles per block, 4 / 2 / 1 taps staged per barrier pair, the
launch with more than 64 KB of LDS, the un-split grids, second trips of the weight gradient's tile loop, more slabs than the
reduce kernel has thread groups, 64 voxels per wave, every K-step count the concat widths give, several chunks per block in
the 16-bit weight gradient's software pipeline with a short last block and a partial last chunk -- plus half-empty and
wholly empty last channel tiles and the concat input's channel maps.  tests/test_convt_plans_cpu.py checks without a GPU
that each case lands on the plan it names and that every plan the shipped classes reach has a case here.

Every operand is a channel slice at offset 8 of a buffer 16 channels wider that is filled with a sentinel; after the call
the neighbouring channels are compared bit for bit and the padded channels inside the slice must hold exact zeros.

Gates (those of the two per-op tests named above, references in float64):
  fp32 output, dx, dW, db ............. 1e-4 of max |ref|
  16-bit stored output and dx ......... one ulp of the type times max |ref|, inputs and weights rounded to the type first
  16-bit dW ........................... 1e-4 of max |ref|
  16-bit db (ops.channel_sum) ......... 1e-5 of max |ref|
A failure names the worst voxel, the block and wave that own it, and the tap."""
import functools
import zlib

import pytest
import torch

import convt_ref
from test_convt_plans_cpu import Case, case_plans, cin_p, pad8

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
SENT = 7.0                       # exact in fp32, bf16 and fp16
HOLES = ((7, 0), (7, 8))         # the segments UNetEngine._maps gets for a concat input of 2 x 7 channels in a 16-wide buffer

# The plan keys are (family, instantiation, grid.y > 1, taps per barrier pair) for forward / data gradient and
# (family, instantiation, second tile trip [fp32] or chunks per block > 1 [16-bit]) for the weight gradient.
F32 = [
    # <2, .>, tps 2; weight gradient <2, 2> with gx 32 < 104 tiles: 3 - 4 trips of the tile loop per block
    Case("fp32", 128, 128, 1, 10, 20, 33, None, (("fp32:fwd", "convt2_kernel<2, 0>", True, 2), ("fp32:dgrad", "convt2_kernel<2, 1>", True, 2),
                                                  ("fp32:wgrad", "convt2_wgrad_kernel<2, 2>", True))),
    # <4, .>, tps 1, 65 KB of LDS: the launch that raises the dynamic-LDS limit
    Case("fp32", 128, 128, 1, 12, 30, 33, None, (("fp32:fwd", "convt2_kernel<4, 0>", True, 1), ("fp32:dgrad", "convt2_kernel<4, 1>", True, 1))),
    # <8, .>, tps 1, 97 KB of LDS, un-split grid of 256 blocks, the last one with 17 of 64 voxels
    Case("fp32", 128, 128, 1, 17, 31, 31, None, (("fp32:fwd", "convt2_kernel<8, 0>", False, 1), ("fp32:dgrad", "convt2_kernel<8, 1>", False, 1))),
    # <1, .> with tps 4 on a split grid (the deepest level of the five-level classes)
    Case("fp32", 128, 128, 1, 3, 5, 7, None, (("fp32:fwd", "convt2_kernel<1, 0>", True, 4), ("fp32:dgrad", "convt2_kernel<1, 1>", True, 4),
                                               ("fp32:wgrad", "convt2_wgrad_kernel<2, 2>", False))),
    # <4, .> from ntt_total 4, half-empty last tile (56 = 3.5 tiles); tps 2 forward, 4 backward
    Case("fp32", 64, 56, 1, 17, 31, 31, None, (("fp32:fwd", "convt2_kernel<4, 0>", False, 2), ("fp32:dgrad", "convt2_kernel<4, 1>", False, 4))),
    Case("fp32", 64, 64, 1, 17, 31, 31, None, (("fp32:fwd", "convt2_kernel<4, 0>", False, 2), ("fp32:dgrad", "convt2_kernel<4, 1>", False, 2))),
    # 40 outputs: ntt_total 4 with a tile wholly past nout_p; 24 inputs: half-empty last tile of the data gradient;
    # weight gradient <2, 2> with a partial last channel group on both sides
    Case("fp32", 24, 40, 1, 17, 31, 31, None, (("fp32:fwd", "convt2_kernel<4, 0>", False, 8), ("fp32:dgrad", "convt2_kernel<2, 1>", False, 8),
                                                ("fp32:wgrad", "convt2_wgrad_kernel<2, 2>", False))),
    Case("fp32", 32, 32, 1, 17, 31, 31, None, (("fp32:fwd", "convt2_kernel<2, 0>", False, 8), ("fp32:dgrad", "convt2_kernel<2, 1>", False, 8))),
    # <2, .> on a split grid with tps 4 (64 channels) and tps 8 (56 channels): 130 blocks x 2
    Case("fp32", 64, 64, 1, 11, 27, 28, None, (("fp32:fwd", "convt2_kernel<2, 0>", True, 4), ("fp32:dgrad", "convt2_kernel<2, 1>", True, 4))),
    Case("fp32", 56, 56, 1, 11, 27, 28, None, (("fp32:fwd", "convt2_kernel<2, 0>", True, 8), ("fp32:dgrad", "convt2_kernel<2, 1>", True, 8))),
    # weight gradient <1, 2> and <2, 1>; batch boundary inside a 64-voxel block (660 voxels per sample)
    Case("fp32", 8, 24, 2, 6, 10, 11, None, (("fp32:fwd", "convt2_kernel<1, 0>", True, 8), ("fp32:wgrad", "convt2_wgrad_kernel<1, 2>", False))),
    Case("fp32", 24, 8, 2, 6, 10, 11, None, (("fp32:dgrad", "convt2_kernel<1, 1>", True, 8), ("fp32:wgrad", "convt2_wgrad_kernel<2, 1>", False))),
    # weight gradient <1, 1>: gx 512 < 615 tiles (second trip for 103 blocks), reduce over 512 > RPARTS slabs
    Case("fp32", 8, 8, 1, 24, 40, 41, None, (("fp32:fwd", "convt2_kernel<1, 0>", False, 8), ("fp32:dgrad", "convt2_kernel<1, 1>", False, 8),
                                              ("fp32:wgrad", "convt2_wgrad_kernel<1, 1>", True))),
    # concat input with holes: cinv in both packings, imap in the reduce
    Case("fp32", 14, 14, 2, 6, 10, 11, HOLES, (("fp32:wgrad", "convt2_wgrad_kernel<1, 1>", False),)),
]
LP = [
    # wide (64 voxels per wave), partial last wave and block; weight gradient <2, 2> with 3 chunks per block
    Case("lp", 32, 32, 1, 33, 45, 45, None, (("lp:fwd", "lp_convt_fwd_kernel<T, 1, 4>", False, 0), ("lp:dgrad", "lp_convt_bwd_data_kernel<T, 4>", False, 0),
                                              ("lp:wgrad", "lp_convt_wgrad_kernel<T, 2, 2>", True))),
    # wide; weight gradient <1, 1> with 2 chunks per block (1045 chunks > 1024 blocks), batch boundary inside a wave
    Case("lp", 8, 8, 2, 33, 45, 45, None, (("lp:fwd", "lp_convt_fwd_kernel<T, 1, 4>", False, 0), ("lp:wgrad", "lp_convt_wgrad_kernel<T, 1, 1>", True))),
    # wide with two K-steps; weight gradient <2, 2> with 3 x 3 tiles: the second tile of the last groups is skipped
    Case("lp", 40, 40, 1, 33, 45, 45, None, (("lp:fwd", "lp_convt_fwd_kernel<T, 2, 4>", False, 0), ("lp:wgrad", "lp_convt_wgrad_kernel<T, 2, 2>", True))),
    # split grid; weight gradient <4, 1> with 2 chunks per block: 19 chunks, the last block has one, the last chunk 96 voxels
    Case("lp", 128, 128, 1, 6, 20, 20, None, (("lp:fwd", "lp_convt_fwd_kernel<T, 4, 1>", True, 0), ("lp:dgrad", "lp_convt_bwd_data_kernel<T, 1>", True, 0),
                                               ("lp:wgrad", "lp_convt_wgrad_kernel<T, 4, 1>", True))),
    # un-split narrow grid at 4 K-steps: one block walks all 8 output tiles / 4 passes
    Case("lp", 128, 128, 1, 17, 31, 31, None, (("lp:fwd", "lp_convt_fwd_kernel<T, 4, 1>", False, 0), ("lp:dgrad", "lp_convt_bwd_data_kernel<T, 1>", False, 0))),
    # KSN 3; weight gradient <4, 1> with 5 input tiles: the block of the second group skips tiles 5 .. 7
    Case("lp", 72, 72, 1, 6, 20, 20, None, (("lp:fwd", "lp_convt_fwd_kernel<T, 3, 1>", True, 0), ("lp:wgrad", "lp_convt_wgrad_kernel<T, 4, 1>", False))),
    # KSN 5 .. 8: the concat-input widths (and 192, 224 for 6 and 7)
    Case("lp", 160, 40, 1, 4, 8, 16, None, (("lp:fwd", "lp_convt_fwd_kernel<T, 5, 1>", True, 0),)),
    Case("lp", 192, 24, 1, 4, 8, 16, None, (("lp:fwd", "lp_convt_fwd_kernel<T, 6, 1>", True, 0),)),
    Case("lp", 224, 24, 1, 4, 8, 16, None, (("lp:fwd", "lp_convt_fwd_kernel<T, 7, 1>", True, 0),)),
    Case("lp", 256, 64, 1, 4, 8, 16, None, (("lp:fwd", "lp_convt_fwd_kernel<T, 8, 1>", True, 0),)),
    # KSN 2 on a split and on an un-split grid
    Case("lp", 64, 64, 2, 6, 10, 11, None, (("lp:fwd", "lp_convt_fwd_kernel<T, 2, 1>", True, 0),)),
    Case("lp", 64, 64, 1, 17, 31, 31, None, (("lp:fwd", "lp_convt_fwd_kernel<T, 2, 1>", False, 0), ("lp:wgrad", "lp_convt_wgrad_kernel<T, 4, 1>", True))),
    # non-wide, un-split: one block walks both output tiles
    Case("lp", 32, 32, 1, 16, 32, 33, None, (("lp:fwd", "lp_convt_fwd_kernel<T, 1, 1>", False, 0), ("lp:dgrad", "lp_convt_bwd_data_kernel<T, 1>", False, 0),
                                              ("lp:wgrad", "lp_convt_wgrad_kernel<T, 2, 2>", False))),
    Case("lp", 24, 8, 2, 6, 10, 11, None, (("lp:wgrad", "lp_convt_wgrad_kernel<T, 2, 1>", False),)),
    Case("lp", 8, 24, 2, 6, 10, 11, None, (("lp:wgrad", "lp_convt_wgrad_kernel<T, 1, 2>", False),)),
    Case("lp", 14, 14, 2, 6, 10, 11, HOLES, (("lp:wgrad", "lp_convt_wgrad_kernel<T, 1, 1>", False),)),
]
CASES = F32 + [c._replace(dtype=dt) for c in LP for dt in ("bf16", "fp16")]


def _ops():
    from ctunet_amd import ops
    return ops


def _id(c):
    return f"{c.dtype}-{c.Ci}to{c.Co}{'-holes' if c.segs else ''}-{c.N}x{c.D}x{c.H}x{c.W}"


def rnd(x, dt):
    return x.to(DT[dt]).float() if dt != "fp32" else x


class Data:
    """Inputs of a case (CPU, already rounded to the case's type) and, on first use, the float64 references.  pos: the padded
    position of each logical input channel inside the slice (the engine's imap); scale / shift are per padded position."""

    def __init__(self, c):
        g = torch.Generator().manual_seed(zlib.crc32(repr(tuple(c[:8])).encode()) % (1 << 31))
        self.c, dt = c, c.dtype
        n, d, h, w = c.N, c.D, c.H, c.W
        self.cip, self.cop = cin_p(c), pad8(c.Co)
        self.pos = list(range(c.Ci)) if c.segs is None else [s + i for (k, s) in c.segs for i in range(k)]
        self.x = rnd(torch.randn(n, c.Ci, d, h, w, generator=g), dt)
        self.wt = rnd(torch.randn(c.Ci, c.Co, 2, 2, 2, generator=g) * (1.0 / c.Ci) ** 0.5, dt)
        self.b = torch.randn(c.Co, generator=g) * 0.5
        self.sc, self.sh = torch.zeros(self.cip), torch.zeros(self.cip)
        self.sc[self.pos] = torch.rand(c.Ci, generator=g) * 1.5 - 0.25
        self.sh[self.pos] = torch.randn(c.Ci, generator=g) * 0.3
        self.go = rnd(torch.randn(n, c.Co, 2 * d, 2 * h, 2 * w, generator=g), dt)
        # what the kernels multiply: relu(x * scale + shift), rounded to the storage type on the 16-bit path
        self.a = convt_ref.activate(self.x, self.sc[self.pos], self.sh[self.pos], True, None if dt == "fp32" else DT[dt])

    @functools.cached_property
    def out(self):
        return convt_ref.forward(self.a, self.wt, self.b)

    @functools.cached_property
    def dx(self):
        return convt_ref.data_gradient(self.go, self.wt)

    @functools.cached_property
    def dw_db(self):
        return convt_ref.weight_gradient(self.a, self.go)

    def maps(self):
        """(imap, cinv) device tensors as UNetEngine._maps builds them; (None, None) = identity."""
        if self.c.segs is None:
            return None, None
        inv = [-1] * self.cip
        for logical, p in enumerate(self.pos):
            inv[p] = logical
        return torch.tensor(self.pos, dtype=torch.int32, device="cuda"), torch.tensor(inv, dtype=torch.int32, device="cuda")


@functools.lru_cache(maxsize=1)
def data(c):
    """The three ops of a case run back to back (the op is the fastest-varying parameter) and share one Data."""
    return Data(c)


def to_slice(x, pos, cp, dt):
    """Logical NCDHW (CPU) -> a cp-channel slice at offset 8 of a GPU buffer 16 channels wider: logical channel i at padded
    position pos[i], the other positions of the slice zero, the neighbours the sentinel."""
    ops = _ops()
    n, c, d, h, w = x.shape
    buf = torch.full((n, d, h, w, cp + 16), SENT, dtype=DT[dt])
    v = torch.zeros(n, d, h, w, cp)
    v[..., pos] = x.permute(0, 2, 3, 4, 1).float()
    buf[..., 8:8 + cp] = v.to(DT[dt])
    return ops.CL(buf.cuda(), 8, cp)


def sentinel_slice(n, d, h, w, cp, dt):
    ops = _ops()
    return ops.CL(torch.full((n, d, h, w, cp + 16), SENT, dtype=DT[dt], device="cuda"), 8, cp)


def from_slice(a, pos):
    return a.buf[..., [a.c0 + p for p in pos]].float().permute(0, 4, 1, 2, 3).contiguous().cpu()


def check_neighbours_and_padding(c, a, pos, what):
    """The 8 channels on either side of the slice still hold the sentinel, bit for bit; positions of the slice that carry no
    logical channel hold exact zeros (the kernel owns them: a consumer reads them as zero activations)."""
    buf = a.buf.cpu()
    sent = torch.full((), SENT, dtype=buf.dtype)
    assert torch.equal(buf[..., :a.c0], sent.expand_as(buf[..., :a.c0])), f"{_id(c)} {what}: channels below the slice were written"
    hi = buf[..., a.c0 + a.cp:]
    assert torch.equal(hi, sent.expand_as(hi)), f"{_id(c)} {what}: channels above the slice were written"
    pad = [a.c0 + p for p in range(a.cp) if p not in set(pos)]
    if pad:
        z = buf[..., pad].float()
        assert torch.all(z == 0), f"{_id(c)} {what}: padded channels hold {z.abs().max().item()}"


def where(c, what, got, ref, fine, vox_per_block, tiles_per_group):
    """Worst element of a voxel tensor: the coarse voxel, the tap (fine tensors), the block and wave that own the voxel and the
    blockIdx.y group of its 16-channel tile."""
    err = (got.double() - ref).abs()
    i = int(err.flatten().argmax())
    n, ch, d, h, w = [int(v) for v in torch.unravel_index(torch.tensor(i), err.shape)]
    tap = ""
    if fine:
        tap = f", tap {(d & 1) * 4 + (h & 1) * 2 + (w & 1)} (i, j, l = {d & 1}, {h & 1}, {w & 1})"
        d, h, w = d // 2, h // 2, w // 2
    v = ((n * c.D + d) * c.H + h) * c.W + w
    return (f"{_id(c)} {what}: worst |err| {err.flatten()[i].item():.3e} (max |ref| {ref.abs().max().item():.3e}) at channel {ch}, coarse voxel "
            f"{v} (n={n} d={d} h={h} w={w}){tap}; block {v // vox_per_block} of {-(-c.N * c.D * c.H * c.W // vox_per_block)}, wave "
            f"{v % vox_per_block // (vox_per_block // 4)}, channel tile {ch // 16} = blockIdx.y group {ch // 16 // tiles_per_group}")


def gate(c, what, got, ref, tol, report=None):
    scale = ref.abs().max().item()
    err = (got.double() - ref).abs().max().item()
    print(f"{_id(c)} {what}: max |err| / max |ref| = {err / scale:.3e} (gate {tol:.3e})")
    assert err <= tol * scale, report() if report else f"{_id(c)} {what}: max |err| {err:.3e}, max |ref| {scale:.3e}"


def far_outside(c, what, wrong, ref, tol):
    """A reference built with a wrong-but-plausible channel map (the identity) must miss the gate by far: a kernel that ignored
    the map would produce it, so such a kernel cannot pass."""
    assert (wrong - ref).abs().max().item() > 100 * tol * ref.abs().max().item(), f"{_id(c)} {what}: the identity map is not told apart"


def _n16(name):
    """Output tiles per block from 'convt2_kernel<N, MODE>'; 16-bit forward blocks take one tile per blockIdx.y when split."""
    return int(name.split("<")[1].split(",")[0])


@pytest.mark.parametrize("c", [pytest.param(c, id=_id(c)) for c in CASES])
@pytest.mark.parametrize("op", ["fwd", "dgrad", "wgrad"])
def test_convt_plan(op, c):
    ops = _ops()
    dt = c.dtype
    lp = dt != "fp32"
    n, d, h, w = c.N, c.D, c.H, c.W
    D = data(c)
    cip, cop, pos = D.cip, D.cop, D.pos
    opos = list(range(c.Co))
    imap, cinv = D.maps()
    plan = case_plans(c)
    vpb = 64 if not lp else (256 if plan.fwd[0].endswith(", 4>") else 64)
    utol = ULP[dt] if lp else 1e-4

    if op == "fwd":
        xc = to_slice(D.x, pos, cip, dt).with_xf(D.sc.cuda(), D.sh.cuda(), True)
        if lp:
            wp = ops.pack_convt_w_lp(D.wt.cuda(), cinv, cip, cop, 0, DT[dt])
        else:
            wp = ops.pack_convt_w(D.wt.cuda(), cinv, cip, cop, 0)
        out = sentinel_slice(n, 2 * d, 2 * h, 2 * w, cop, dt)
        ops.convt_fwd(xc, wp, D.b.cuda(), out)
        torch.cuda.synchronize()
        got = from_slice(out, opos)
        tpg = (_n16(plan.fwd[0]) if not lp else 1) if plan.fwd[2] > 1 else 8
        gate(c, "output", got, D.out, utol, lambda: where(c, "output", got, D.out, True, vpb, tpg))
        check_neighbours_and_padding(c, out, opos, "output")
        if c.segs is not None:      # the identity map: buffer positions 0 .. Ci - 1 taken for the logical channels
            xb = torch.zeros(n, cip, d, h, w, dtype=torch.float64)
            xb[:, pos] = D.a
            far_outside(c, "output", convt_ref.forward(xb[:, :c.Ci], D.wt, D.b), D.out, utol)
        return

    gc = to_slice(D.go, opos, cop, dt)
    if op == "dgrad":
        if lp:
            wpd = ops.pack_convt_w_lp(D.wt.cuda(), cinv, cop, cip, 1, DT[dt])
        else:
            wpd = ops.pack_convt_w(D.wt.cuda(), cinv, cop, cip, 1)
        gin = sentinel_slice(n, d, h, w, cip, dt)
        ops.convt_bwd_data(gc, wpd, gin)
        torch.cuda.synchronize()
        got = from_slice(gin, pos)
        tpg = (_n16(plan.dgrad[0]) if not lp else 2) if plan.dgrad[2] > 1 else 8
        gate(c, "dx", got, D.dx, utol, lambda: where(c, "dx", got, D.dx, False, vpb, tpg))
        check_neighbours_and_padding(c, gin, pos, "dx")
        if c.segs is not None:      # the expected slice with dx scattered through the identity instead of the map
            right, wrong = torch.zeros(n, cip, d, h, w, dtype=torch.float64), torch.zeros(n, cip, d, h, w, dtype=torch.float64)
            right[:, pos] = D.dx
            wrong[:, :c.Ci] = D.dx
            far_outside(c, "dx", wrong, right, utol)
        return

    xc = to_slice(D.x, pos, cip, dt).with_xf(D.sc.cuda(), D.sh.cuda(), True)
    ws = torch.full((ops.convt_wgrad_ws((n, d, h, w), cip, cop, DT[dt]),), float("nan"), device="cuda")    # every slab must be written
    dw, db = ops.convt_wgrad(xc, gc, c.Ci, c.Co, imap, ws)
    torch.cuda.synchronize()
    rdw, rdb = D.dw_db

    def where_w():
        err = (dw.cpu().double() - rdw).abs()
        ci, co, i, j, l = [int(v) for v in torch.unravel_index(err.flatten().argmax(), err.shape)]
        return (f"{_id(c)} dW: worst |err| {err.max().item():.3e} (max |ref| {rdw.abs().max().item():.3e}) at ci={ci} (padded position {pos[ci]}) "
                f"co={co} tap {i * 4 + j * 2 + l}; plan {plan.wgrad}")
    gate(c, "dW", dw.cpu(), rdw, 1e-4, where_w)
    gate(c, "db", db.cpu(), rdb, 1e-5 if lp else 1e-4)
    if c.segs is not None:
        xb = torch.zeros(n, cip, d, h, w, dtype=torch.float64)
        xb[:, pos] = D.a
        far_outside(c, "dW", convt_ref.weight_gradient(xb[:, :c.Ci], D.go)[0], rdw, 1e-4)
