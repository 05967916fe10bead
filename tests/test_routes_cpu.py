"""Route manifest of the convolution launches (no GPU: the library's host-only routing queries).

Every convolution family picks its kernel at run time from the geometry.  This file sweeps the dispatchers over the layer
geometries of the shipped classes (32^3 .. 256^3, batch 1 - 2, k = 3 and 5, plus non-cubic volumes) and checks that the
per-op GPU tables reach every route the sweep reaches -- and, for the persistent kernels (a block loops over several
boxes), that some case runs at least two boxes per block and some case has a volume that is not a multiple of the box.

Families with a name query (ctu_conv3d_*_kernel_name, ctu_lp_conv3d_*_kernel_name) are routed by the library.  The fused
up-convolutions and the first-layer kernels have none: `route()` restates their selection rules below, and
`test_restated_grids_match_the_library` holds the restatement to the library's *_num_blocks queries at every swept shape.
Where no query gives a grid, a block count cap mirrors the line of C++ that bounds it; boxes > cap then guarantees at least
two boxes for a block.

The first encoder convolution is swept at both precisions.  Its 16-bit routes are the T = bf16 / half instantiations of the
three first-layer kernels (one name `<CIN, T>` for both types), the matrix-pipe data gradient `lp_conv_fwd_pair_kernel<OUT32>`
of volumes at least 32 wide and, for large volumes, the matrix-pipe weight gradient `lp_wgrad8_kernel<first>`; a GPU case
forces the last one with the op spelling `first_wgrad_mfma` (it sets ops.FIRST_WGRAD_MFMA_MIN_VOX to 0).  First layers the
first-layer kernels do not take (k = 5, W < 16) are swept as ordinary convolutions on 8 padded input channels."""
from collections import namedtuple

Case = namedtuple("Case", "route op dtype N Ci Co D H W k xf cs c0")
Route = namedtuple("Route", "name persistent box boxes tpb")      # box (d, h, w); tpb: boxes per block (a lower bound)


def cdiv(a, b):
    return -(-a // b)


def _lib():
    from ctunet_amd import _lib as L
    return L.load()


def pad8(c):
    return cdiv(c, 8) * 8


# ------------------------------------------------------------------ grid caps (each mirrors one line of the C++)
WG_BLOCKS = 512          # conv3d.hip: CTU_WG_BLOCKS, the cap `CTU_WG_BLOCKS / (pairs * planes)` in wgrad_plan / k3s_grid / upwg_plan
LP_WG8_CAP = 512         # conv3d_lp.hip: `persist_grid(r.ntiles, 512)` in lp_wg_plan (LP_WG_K8)
LP_WG16_CAP = 256        # conv3d_lp.hip: the cap `256 / r.pairs` in lp_wg_plan (LP_WG_K16; at least 8)
LP_WG_CAP = 768          # conv3d_lp.hip: `int g = 768 / groups;` in lp_wg_cap (at least 16)
LP_PAIR_CAP = 768        # conv3d_lp.hip: `persist_grid(r.ntiles, 768)` in lp_fwd_plan (LP_FWD_PAIR)
LP_P1_CAP = 512          # conv3d_lp.hip: `persist_grid(r.ntiles, 512)` in lp_fwd_plan (LP_FWD_PERSIST)
LP_UPWG4_CAP = 256       # conv3d_lp.hip: `persist_grid(r.ntiles, 256)` in lp_upwg_plan (lp_upwg4_kernel)
UP_CAP = 512             # upconv_fused.hip: `persist_grid(r.ntiles, 512 / r.ny)` in up_plan
UL_CAP = 256             # upconv_lp.hip: `persist_grid(r.ntiles, 256)` in ul_plan
FIRST_PER_CU = {"fwd": 4, "dgrad": 3, "wgrad": 5}    # conv3d_first.hip: FWD_PER_CU, DGRAD_PER_CU, WGRAD_PER_CU (x 256 blocks)
LP_SC = 32               # conv3d_lp.hip: input channels per stage


def persist_grid(ntiles, cap):
    """The shared tail of every persistent grid helper: g = min(cap, ntiles), tpb = ceil(ntiles / g), gx = ceil(ntiles / tpb)."""
    g = max(1, min(cap, ntiles))
    tpb = cdiv(ntiles, g)
    return cdiv(ntiles, tpb), tpb


def lp_box(W, rin_p, nvox):
    """conv3d_lp.hip lp_box: (th, bw) of a 16-bit forward / data-gradient box (depth 4)."""
    nch = min(rin_p, LP_SC) >> 3
    if nvox <= 4096:
        return 4, 8
    if W < 16:
        return 8, 8
    if nch <= 2:
        return 8, 16
    return 4, 16


def lp_wg_box_w(W):
    return 32 if W >= 32 else (16 if W >= 16 else 8)


def up_ny(nout_p, ntiles):
    """upconv_fused.hip up_plan: parity groups (blockIdx.y) of the fp32 fused up-convolution forward."""
    if nout_p == 16 and ntiles < 256:
        return 2
    return 1 if nout_p <= 16 else (2 if nout_p <= 32 else 4)


def up_bwd_nt(cin_p, ntiles):
    """upconv_fused.hip up_plan: the nt loop of the data gradient (input-channel tiles per block)."""
    n16 = cdiv(cin_p, 16)
    nt = 4 if n16 >= 4 else (2 if n16 >= 2 else 1)
    while nt > 1 and ntiles * cdiv(n16, nt) < 256:
        nt >>= 1
    return nt


def _boxes(N, D, H, W, box):
    return N * cdiv(D, box[0]) * cdiv(H, box[1]) * cdiv(W, box[2])


def _capped(name, N, D, H, W, box, cap, suffix=""):
    n = _boxes(N, D, H, W, box)
    return Route(name + suffix, True, box, n, cdiv(n, max(1, min(cap, n))))


def route(c):
    """The kernel a per-op case runs, its box, its number of boxes and boxes per block."""
    L = _lib()
    N, D, H, W, k = c.N, c.D, c.H, c.W, c.k
    cip, cop = pad8(c.Ci), pad8(c.Co)
    lp = c.dtype != "fp32"
    op = c.op
    lz = "+LZ" if op.endswith("_bn") else ""
    if op in ("fwd", "dgrad"):
        rin, nout = (cip, cop) if op == "fwd" else (cop, cip)
        if not lp:
            lay = L.ctu_conv3d_layout(k, nout, W)
            name = L.ctu_conv3d_fwd_kernel_name(N, D, H, W, k, nout, lay).decode()
            if "persist" not in name:
                return Route(name, False, None, None, 1)
            box = (4, 4, 32 if lay == 1 else 16)
            n = _boxes(N, D, H, W, box)
            return Route(name, True, box, n, cdiv(n, L.ctu_conv3d_num_blocks(N, D, H, W, k, nout, lay)))
        lay = L.ctu_lp_conv3d_layout(k, rin, nout, W)
        name = L.ctu_lp_conv3d_fwd_kernel_name(N, D, H, W, k, rin, nout, lay).decode()
        if lay == 1:
            box = (4, 8, 32)
        elif name == "lp_conv_fwd_p1_kernel":
            th, bw = lp_box(W, rin, N * D * H * W)
            box = (4, th, bw)
            name += f"<{th}x{bw}>"
        else:
            return Route(name, False, None, None, 1)
        n = _boxes(N, D, H, W, box)
        return Route(name, True, box, n, cdiv(n, L.ctu_lp_conv3d_num_blocks(N, D, H, W, k, rin, nout, lay)))
    if op in ("wgrad", "wgrad_bn"):
        if not lp:
            name = L.ctu_conv3d_wgrad_kernel_name(W, k, cip, cop).decode()
            if name.startswith("conv3d_wgrad_k3s") or name.startswith("conv3d_wgrad_k5s"):
                sm, sn = (2 if cip == 8 else 1), (2 if cop == 8 else 1)
                box = (4, 4, 16 if sm == 2 and sn == 2 else 8)
                groups = cdiv(cip, 16 // sm) * cdiv(cop, 16 // sn) * (5 if "k5s" in name else 1)
            else:
                box = (4, 4, 16) if W >= 16 else ((4, 8, 8) if W >= 8 else (4, 4, 4))
                groups = cdiv(cip, 16) * cdiv(cop, 16) * (1 if k == 3 else 5)
            return _capped(name, N, D, H, W, box, max(1, WG_BLOCKS // groups), lz)
        name = L.ctu_lp_conv3d_wgrad_kernel_name(D, H, W, k, cip, cop).decode()
        if name == "lp_wgrad8_kernel":
            return _capped(name, N, D, H, W, (4, 8, 32), LP_WG8_CAP, lz)
        pairs = cdiv(cip, 16) * cdiv(cop, 16)
        if name == "lp_wgrad16_kernel":
            return _capped(name, N, D, H, W, (4, 8, 32), max(8, LP_WG16_CAP // pairs), lz)
        bw = lp_wg_box_w(W)
        return _capped(name, N, D, H, W, (4, 4 * (32 // bw), bw), max(16, LP_WG_CAP // (pairs * (1 if k == 3 else 5))), lz)
    # fused up-convolution: N, D, H, W are the COARSE dims, Ci = C (transposed conv channels), Co = the 3x3x3 conv's outputs
    if op == "up_fwd":
        box = (4, 4, 16)
        n = _boxes(N, D, H, W, box)
        if lp:
            gx, tpb = persist_grid(n, UL_CAP)
            return Route("lp_upconv_fwd_kernel", True, box, n, tpb)
        ny = up_ny(cop, n)
        gx, tpb = persist_grid(n, UP_CAP // ny)
        if cop == 16 and ny == 2:
            name = "upconv_fused_fwd_kernel<4, 1>"
        elif cop == 8:
            name = "upconv_fused_fwd_kernel<4, 1, true>"
        else:
            name = {1: "upconv_fused_fwd_kernel<8, 1>", 2: "upconv_fused_fwd_kernel<4, 2>", 4: "upconv_fused_fwd_kernel<2, 4>"}[ny]
        return Route(name, True, box, n, tpb)
    if op == "up_dgrad":
        box = (4, 4, 16)
        n = _boxes(N, D, H, W, box)
        if lp:
            gx, tpb = persist_grid(n, UL_CAP)
            return Route(f"lp_upconv_bwd_data_kernel<{4 if cip >= 64 else 2}>", True, box, n, tpb)
        nt = up_bwd_nt(cip, n)
        gx, tpb = persist_grid(n, max(1, UP_CAP // cdiv(cdiv(cip, 16), nt)))
        return Route(f"upconv_fused_bwd_data_kernel<{nt}>", True, box, n, tpb)
    if op in ("up_wgrad", "up_wgrad_bn"):
        if lp:
            if not lz and cip % 32 == 0 and D % 4 == 0 and H % 4 == 0 and W % 32 == 0:
                return _capped("lp_upwg4_kernel", N, D, H, W, (4, 4, 32), LP_UPWG4_CAP)
            bw = lp_wg_box_w(W)
            return _capped(f"lp_upwg_kernel<{bw}>", N, D, H, W, (4, 4 * (32 // bw), bw), max(16, LP_WG_CAP // (4 * (cip // 16))), lz)
        if cop == 8:      # upwg_plan(pw): the (w-parity, c_out) tile
            return _capped("conv3d_wgrad_k3s_kernel<1, 1, 2>", N, D, H, W, (4, 4, 8), max(1, WG_BLOCKS // (4 * cdiv(cip, 16))), lz)
        return _capped("conv3d_wgrad_k3s_kernel<1, 1, 1>", N, D, H, W, (4, 4, 8),
                       max(1, WG_BLOCKS // (8 * cdiv(cip, 16) * cdiv(cop, 16))), lz)
    if op.startswith("first_"):      # C_in <= 2 first layer, 8 padded outputs, 4 x 4 x 32 boxes
        part = op[len("first_"):].replace("_bn", "")
        forced = part == "wgrad_mfma"                      # a GPU case that sets ops.FIRST_WGRAD_MFMA_MIN_VOX to 0
        part = part.replace("_mfma", "")
        if lp and part == "dgrad" and L.ctu_lp_conv3d_first_bwd_data_pair_supported(c.Ci, W):
            # ops.conv_first_bwd_data: the 8 -> 8 pair-layout kernel with the float32-plane epilogue
            return _capped("lp_conv_fwd_pair_kernel<OUT32>", N, D, H, W, (4, 8, 32), LP_PAIR_CAP)
        if lp and part == "wgrad":
            # ops.conv_first_wgrad: large volumes take a 16-bit copy of the input + the 8 -> 8 matrix-pipe weight gradient
            from ctunet_amd import ops as O
            if (forced or N * D * H * W >= O.FIRST_WGRAD_MFMA_MIN_VOX) \
                    and L.ctu_lp_conv3d_wgrad_kernel_name(D, H, W, 3, 8, 8) == b"lp_wgrad8_kernel":
                return _capped("lp_wgrad8_kernel<first>", N, D, H, W, (4, 8, 32), LP_WG8_CAP)
        box = (4, 4, 32)
        n = _boxes(N, D, H, W, box)
        gx, tpb = persist_grid(n, 256 * FIRST_PER_CU[part])
        kern = {"fwd": "first_fwd_kernel", "dgrad": "first_bwd_data_kernel", "wgrad": "first_wgrad_kernel"}[part]
        return Route(f"{kern}<{c.Ci}, T>" if lp else f"{kern}<{c.Ci}>{lz}", True, box, n, tpb)
    raise ValueError(f"unknown op {op}")


def family(c):
    """Forward and data gradient of a conv share the forward kernels; every other op is a family of its own (the forced
    matrix-pipe spelling of the first layer's weight gradient belongs to that weight gradient's family)."""
    op = "fwd" if c.op == "dgrad" else c.op.replace("_bn", "").replace("_mfma", "")
    return ("fp32" if c.dtype == "fp32" else "lp") + ":" + op


# ------------------------------------------------------------------ the sweep
SIZES = (32, 48, 64, 96, 128, 192, 256)
NON_CUBIC = ((64, 64, 32), (96, 96, 64), (128, 128, 96), (30, 34, 70), (48, 64, 80), (40, 56, 72))   # patches, test_non_cubic_volumes


def class_geometries():
    """(k, cin, cout, level, kind) of every conv / fused up-conv layer of the shipped classes (engine plans)."""
    from ctunet_amd import models
    from util import CLASS_INPUT
    out = set()
    for name in CLASS_INPUT:
        plan = getattr(models, name)()._plan
        n = len(plan.enc)
        for i, b in enumerate(plan.enc):
            out.add((plan.k, b.cin, b.cout, i, "conv"))
            out.add((plan.k, b.cout, b.cout, i, "conv"))
        out.add((plan.k, plan.center.cin, plan.center.cout, n, "conv"))
        out.add((plan.k, plan.center.cout, plan.center.cout, n, "conv"))
        for j, b in enumerate(plan.dec):
            fine = n - 1 - j
            out.add((plan.k, b.cin, b.cout, fine + 1, "up"))          # coarse level of the fused up-convolution
            out.add((plan.k, b.cin, b.cout, fine, "conv"))            # unfused form: the conv after the transposed conv
            out.add((plan.k, b.cout, b.cout, fine, "conv"))
    return sorted(out)


def sweep_cases():
    vols = [(s, s, s) for s in SIZES] + list(NON_CUBIC)
    cases = []
    for (k, ci, co, lev, kind) in class_geometries():
        for (d, h, w) in vols:
            dd, hh, ww = d >> lev, h >> lev, w >> lev
            if min(dd, hh, ww) < 2:
                continue
            for n in (1, 2):
                for dt in ("fp32", "bf16"):
                    if kind == "up":
                        cip, cop = pad8(ci), pad8(co)
                        if dt == "fp32" and _lib().ctu_upconv_fused_supported(3, dd, hh, ww, cip, cop) and k == 3:
                            ops = ("up_fwd", "up_dgrad", "up_wgrad") + (
                                ("up_wgrad_bn",) if _lib().ctu_upconv_fused_wgrad_bn_supported(n, dd, hh, ww, cip, cop) else ())
                        elif dt != "fp32" and _lib().ctu_lp_upconv_fused_supported(3, dd, hh, ww, cip, cop) and k == 3:
                            ops = ("up_fwd", "up_dgrad", "up_wgrad") + (
                                ("up_wgrad_bn",) if _lib().ctu_lp_upconv_fused_wgrad_bn_supported(n, dd, hh, ww, cip) else ())
                        else:
                            continue
                        cases += [Case("", o, dt, n, ci, co, dd, hh, ww, 3, True, 0, 0) for o in ops]
                        continue
                    if ci <= 2 and _lib().ctu_conv3d_first_supported(k, ci, pad8(co), ww):
                        # (ops.conv_first_wgrad_bn is fp32 only: the 16-bit first layer has no lazy weight gradient)
                        ops = ("first_fwd", "first_dgrad", "first_wgrad") + (("first_wgrad_bn",) if dt == "fp32" else ())
                        cases += [Case("", o, dt, n, ci, co, dd, hh, ww, k, False, 0, 0) for o in ops]
                        continue
                    # (a first layer with k = 5 or W < 16 falls through: the generic kernels on 8 padded input channels)
                    ops = ["fwd", "dgrad", "wgrad"]
                    cip, cop = pad8(ci), pad8(co)
                    if dt == "fp32" and _lib().ctu_conv3d_wgrad_bn_supported(n, dd, hh, ww, k, cip, cop):
                        ops.append("wgrad_bn")
                    if dt != "fp32" and _lib().ctu_lp_conv3d_wgrad_bn_supported(n, dd, hh, ww, k, cip, cop):
                        ops.append("wgrad_bn")
                    cases += [Case("", o, dt, n, ci, co, dd, hh, ww, k, False, 0, 0) for o in ops]
    return cases


# ------------------------------------------------------------------ the per-op GPU tables, as plain lists of Case
def table_cases():
    """Every per-op GPU case of the existing suites and of test_routes_gpu, as Case tuples."""
    import test_lowp_gpu as LP
    import test_ops_gpu as OP
    import test_routes_gpu as RG
    out = list(RG.CASES)
    for (n, ci, co, d, h, w, k, xf, _b) in OP.CONV_CASES:
        out += [Case("", o, "fp32", n, ci, co, d, h, w, k, xf, 0, 0) for o in ("fwd", "dgrad", "wgrad")]
    for (k, ci, co, (n, d, h, w), xf) in LP.CONV_CASES:
        out += [Case("", o, "bf16", n, ci, co, d, h, w, k, xf, 0, 0) for o in ("fwd", "dgrad", "wgrad")]
    return out


ALLOWED_UNCOVERED = {}   # route -> reason; empty: every swept route has a GPU case


def _reached():
    reached = {}
    for c in sweep_cases():
        r = route(c)
        key = (family(c), r.name)
        if key not in reached:
            reached[key] = (c, r)
    return reached


def test_restated_grids_match_the_library():
    """The Python restatement of the grids without a name query agrees with the library's *_num_blocks queries."""
    L = _lib()
    seen = 0
    for c in sweep_cases():
        N, D, H, W = c.N, c.D, c.H, c.W
        if c.op == "up_fwd" and c.dtype == "fp32":
            r = route(c)
            ny = up_ny(pad8(c.Co), r.boxes)
            gx, _ = persist_grid(r.boxes, UP_CAP // ny)
            assert gx * ny == L.ctu_upconv_fused_num_blocks(N, D, H, W, pad8(c.Co)), c
        elif c.op == "up_fwd":
            r = route(c)
            assert persist_grid(r.boxes, UL_CAP)[0] == L.ctu_lp_upconv_fused_num_blocks(N, D, H, W), c
        elif c.op == "first_fwd":                                # fp32 and 16-bit: one template, one grid
            r = route(c)
            assert r.name.startswith("first_fwd_kernel<") and r.name.endswith(", T>") == (c.dtype != "fp32"), c
            assert persist_grid(r.boxes, 256 * FIRST_PER_CU["fwd"])[0] == L.ctu_conv3d_first_num_blocks(N, D, H, W), c
        elif c.op == "first_dgrad" and c.dtype != "fp32":
            r = route(c)
            if r.name != "lp_conv_fwd_pair_kernel<OUT32>":
                continue
            assert persist_grid(r.boxes, LP_PAIR_CAP)[0] == L.ctu_lp_conv3d_num_blocks(N, D, H, W, 3, 8, 8, 1), c
        elif c.op in ("fwd", "dgrad") and c.dtype != "fp32":
            r = route(c)
            if r.name.startswith("lp_conv_fwd_p1_kernel"):     # the restated lp_box gives the library's grid
                gx = L.ctu_lp_conv3d_num_blocks(N, D, H, W, c.k, pad8(c.Ci if c.op == "fwd" else c.Co), 8, 0)
                assert persist_grid(r.boxes, LP_P1_CAP)[0] == gx, c
        else:
            continue
        seen += 1
    assert seen > 100


def test_every_swept_route_has_a_gpu_case():
    cov = {}
    for c in table_cases():
        r = route(c)
        cov.setdefault((family(c), r.name), []).append((c, r))
    missing = [f"{fam} {name}  e.g. {c.dtype} {c.op} N={c.N} {c.Ci}->{c.Co} {c.D}x{c.H}x{c.W} k={c.k}"
               for (fam, name), (c, r) in sorted(_reached().items()) if (fam, name) not in cov and name not in ALLOWED_UNCOVERED]
    assert not missing, "routes without a per-op GPU case:\n  " + "\n  ".join(missing)


def _multi_box_possible(fam, name):
    """Whether the sweep reaches this route with >= 2 boxes per block (up_ny splits 16-channel layers only below 256 boxes,
    so upconv_fused_fwd_kernel<4, 1> never loops) and with partial boxes (the lazy BatchNorm routes, lp_wgrad8_kernel and
    lp_upwg4_kernel take only volumes that are multiples of their box)."""
    multi = partial = False
    for c in sweep_cases():
        if family(c) != fam:
            continue
        r = route(c)
        if r.name != name:
            continue
        multi |= r.tpb >= 2
        partial |= bool(c.D % r.box[0] or c.H % r.box[1] or c.W % r.box[2])
    return multi, partial


def test_every_persistent_route_runs_several_boxes_per_block_and_partial_boxes():
    cov = {}
    for c in table_cases():
        r = route(c)
        cov.setdefault((family(c), r.name), []).append((c, r))
    bad = []
    for (fam, name), (c, r) in sorted(_reached().items()):
        if not r.persistent or name in ALLOWED_UNCOVERED:
            continue
        got = cov.get((fam, name), [])
        eg = f"e.g. {c.dtype} {c.op} N={c.N} {c.Ci}->{c.Co} {c.D}x{c.H}x{c.W} k={c.k}"
        multi, partial = _multi_box_possible(fam, name)
        if multi and not any(rr.tpb >= 2 for _, rr in got):
            bad.append(f"{fam} {name}: no case with >= 2 boxes per block ({eg})")
        if partial and not any(cc.D % rr.box[0] or cc.H % rr.box[1] or cc.W % rr.box[2] for cc, rr in got):
            bad.append(f"{fam} {name}: no case with partial boxes ({eg})")
    assert not bad, "persistent routes without a multi-box / partial-box case:\n  " + "\n  ".join(bad)


def test_every_new_case_lands_on_its_route():
    import test_routes_gpu as RG
    wrong = [f"{c}: runs {route(c).name}" for c in RG.CASES if route(c).name != c.route]
    assert not wrong, "cases off their route (a dispatcher retune moved them):\n  " + "\n  ".join(wrong)


def test_new_persistent_cases_run_several_boxes_per_block():
    """Each new case of a persistent route runs >= 2 boxes per block, unless no swept geometry makes that route loop."""
    import test_routes_gpu as RG
    single = [f"{c}: {route(c).tpb} box per block" for c in RG.CASES if route(c).persistent and route(c).tpb < 2
              and _multi_box_possible(family(c), route(c).name)[0]]
    assert not single, "\n  ".join(single)


def test_unreachable_lp_box():
    """lp_box never returns a 32-wide box, so lp_conv_launch has no 8 x 32 persistent branch to reach."""
    for w in (8, 16, 24, 32, 48, 64, 96, 128, 256):
        for rin in (8, 16, 24, 32, 64, 128):
            for nvox in (1024, 8192, 1 << 20, 1 << 24):
                assert lp_box(w, rin, nvox)[1] != 32
