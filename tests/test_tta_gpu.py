"""Mirrored passes, ensembles and uncertainty maps of predict_volume on the MI355X: the three flip kernels against
torch.flip and the float64 restatement tests/tta_ref.py, the statistics of the finalize pass, the whole path for one- and
two-output nets, the default-argument equivalences, ensembles across precisions, graph replay and side effects.

u = 2^-24 below is the unit roundoff of float32."""
import functools

import numpy as np
import pytest
import torch

import tta_ref as R
from util import gen, rel_err

pytestmark = pytest.mark.gpu

U = 2.0 ** -24

# name -> shape, patch, overlap, batch, K, masks of the passes.  The first three are the shape cases of
# test_sliding_window_gpu.test_accumulate_and_finalize_kernels_against_float64 (odd W / origins off a multiple of 4 / one
# tile overhanging the volume on every axis); "aligned" has W % 4 == 0 and every tile origin a multiple of 4 inside the
# row, so the 16-byte paths of all three kernels run (asserted from the plan in _check_cases).
CASES = {
    "odd_w": ((20, 45, 70), (32, 16, 32), (8, 4, 12), 5, 3, (0, 1, 6)),
    "off4": ((40, 37, 64), (16, 32, 16), (4, 0, 6), 5, 2, (0, 3, 4)),
    "overhang": ((18, 20, 22), (32, 32, 32), (8, 8, 8), 2, 1, (0, 7, 2)),
    "aligned": ((24, 40, 72), (16, 32, 32), (4, 8, 12), 5, 4, (0, 5, 2)),
}


def _dims(mask):
    return [d for bit, d in ((1, -1), (2, -2), (4, -3)) if mask & bit]


def _flip(t, mask):
    return torch.flip(t, _dims(mask)) if mask else t


def _plan(name):
    from ctunet_amd.inference import plan_batches, tile_grid
    shape, patch, overlap, batch, k, masks = CASES[name]
    tiles = tile_grid(shape, patch, overlap)
    return tiles, plan_batches(tiles, batch, shape, patch)


def _perturb_bn(net, seed):
    """Non-trivial running statistics, so the eval forward's BatchNorm does something (as test_sliding_window_gpu)."""
    g = gen(seed)
    for name, b in net.named_buffers():
        if name.endswith("running_mean"):
            b.copy_(0.1 * torch.randn(b.shape, generator=g))
        elif name.endswith("running_var"):
            b.copy_(0.5 + torch.rand(b.shape, generator=g))
    return net


def _check_cases():
    """What the shape cases are there for, asserted from their plans."""
    for name in CASES:
        tiles, bp = _plan(name)
        assert not bp.valid.all(), name
    shape, patch = CASES["aligned"][:2]
    tiles, bp = _plan("aligned")
    # extraction: 16-byte reads need W % 4 == 0 and source quads at multiples of 4 inside the row, mirrored or not:
    # x0 % 4 == 0, pw % 4 == 0 and no tile past the row's end; accumulation / finalize: box origins at multiples of 4, V % 4
    assert shape[2] % 4 == 0 and patch[2] % 4 == 0 and (tiles[:, 2] % 4 == 0).all()
    assert (tiles[:, 2] + patch[2] <= shape[2]).all() and (bp.box[:, 2] % 4 == 0).all() and int(np.prod(shape)) % 4 == 0
    assert tiles.shape[0] > 1 and len(set(tiles[:, 2])) > 2
    # ... and the other three leave them: an odd row, origins off a multiple of 4, a tile overhanging the volume
    assert CASES["odd_w"][0][2] % 4 and (_plan("off4")[0][:, 2] % 4 != 0).any()
    assert all(s < p for s, p in zip(*CASES["overhang"][:2]))


# ------------------------------------------------------------------------------------------------ 1. extraction
@pytest.mark.parametrize("name", list(CASES))
def test_mirrored_extraction_is_torch_flip_of_the_plain_extraction(name):
    from ctunet_amd import ops
    _check_cases()
    shape, patch = CASES[name][:2]
    tiles, _ = _plan(name)
    coords = torch.from_numpy(tiles).cuda()
    flip = torch.zeros(1, dtype=torch.int32, device="cuda")
    for c in (1, 2):
        vol = torch.randn((c,) + shape, generator=gen(3 + c)).cuda()
        ref = ops.extract_patches(vol, coords, patch)
        for mask in range(8):
            flip.fill_(mask if mask != 5 else 5 + 8 + 1024)          # only the low 3 bits count
            got = ops.extract_patches_flip(vol, coords, patch, flip)
            assert got.shape == ref.shape
            assert torch.equal(got, _flip(ref, mask)), (name, c, mask)
    # tiles wholly or partly outside the volume, before its start too: zero-filled like the plain extraction
    odd = torch.tensor([[-5, -3, -6], [shape[0] - 1, shape[1] - 2, shape[2] - 3], [0, 0, shape[2]]], dtype=torch.int32).cuda()
    ref = ops.extract_patches(vol, odd, patch)
    for mask in (0, 1, 7):
        flip.fill_(mask)
        assert torch.equal(ops.extract_patches_flip(vol, odd, patch, flip), _flip(ref, mask)), (name, mask)


def test_volume_views_off_16_byte_alignment_extract_and_predict_like_a_copy():
    """A contiguous volume whose first voxel is not 16-byte aligned -- item 1 of a stack of odd-sized volumes, or a view
    into a flat buffer -- is read with scalar loads; a plain predict_volume takes it as it always did."""
    import ctunet_amd as A
    from ctunet_amd import ops
    from ctunet_amd.inference import tile_grid
    stack = torch.randn((2, 1, 33, 35, 37), generator=gen(7)).cuda()              # 33 * 35 * 37 voxels: odd
    flat = torch.randn(1 + 34 * 33 * 40, generator=gen(8)).cuda()
    views = [stack[1], flat[1:].view(1, 34, 33, 40)]                               # odd W; W % 4 == 0, one float off
    torch.manual_seed(9)
    net = _perturb_bn(A.UNet(), 10).cuda()
    flip = torch.zeros(1, dtype=torch.int32, device="cuda")
    for vol in views:
        assert vol.is_contiguous() and vol.data_ptr() % 16 != 0
        copy = vol.clone()
        assert copy.data_ptr() % 16 == 0
        coords = torch.from_numpy(tile_grid(tuple(vol.shape[1:]), (32,) * 3, (8,) * 3)).cuda()
        ref = ops.extract_patches(vol, coords, (32,) * 3)
        for mask in (0, 1, 6, 7):
            flip.fill_(mask)
            got = ops.extract_patches_flip(vol, coords, (32,) * 3, flip)
            assert torch.equal(got, _flip(ref, mask)), mask
            assert torch.equal(got, ops.extract_patches_flip(copy, coords, (32,) * 3, flip)), mask
        a = A.predict_volume(net, vol, patch=32, overlap=8, batch=2)
        b = A.predict_volume(net, copy, patch=32, overlap=8, batch=2)
        assert torch.equal(a.probs, b.probs) and torch.equal(a.labels, b.labels)
        c = A.predict_volume(net, vol, patch=32, overlap=8, batch=2, flips=("x",), uncertainty="variance")
        d = A.predict_volume(net, copy, patch=32, overlap=8, batch=2, flips=("x",), uncertainty="variance")
        assert torch.equal(c.probs, d.probs) and torch.equal(c.uncertainty["variance"], d.uncertainty["variance"])


# ------------------------------------------------------------------------------------------------ 2. accumulate
@functools.lru_cache(maxsize=None)
def _kernels(name, blend):
    """One run of the mirrored accumulation per case and blend (the device's float32 accumulators, on the CPU) and its
    float64 restatement, shared by the tests below."""
    from ctunet_amd import ops
    from ctunet_amd.inference import WEIGHT_FLOOR, window_tables
    _check_cases()
    shape, patch, overlap, batch, k, masks = CASES[name]
    tiles, bp = _plan(name)
    nt = tiles.shape[0]
    ys = torch.rand((len(masks), nt, k) + patch, generator=gen(5))        # float32: the reference reads the same values
    dev = "cuda"
    tabs = tuple(torch.from_numpy(t).to(dev) for t in window_tables(patch, blend, 0.125))
    num, ws = torch.zeros((k,) + shape, device=dev), torch.zeros(shape, device=dev)
    sq, sh = torch.zeros_like(num), torch.zeros_like(ws) if k > 1 else None
    num0, ws0 = torch.zeros_like(num), torch.zeros_like(ws)
    flip = torch.zeros(1, dtype=torch.int32, device=dev)
    for f, mask in enumerate(masks):
        flip.fill_(mask)
        for b in range(bp.coords.shape[0]):
            sel = [min(i, nt - 1) for i in range(b * batch, (b + 1) * batch)]      # padding slots: real data
            yb = ys[f, sel].to(dev)
            meta = torch.from_numpy(bp.meta()[b]).to(dev)
            args = (yb, meta[:3 * batch].view(batch, 3), meta[3 * batch:4 * batch], meta[4 * batch:], flip, tabs, WEIGHT_FLOOR,
                    bp.extent)
            ops.window_accumulate_flip(*args, num, ws, sq, sh)
            ops.window_accumulate_flip(*args, num0, ws0)                            # the same sums without the moments
    ref = R.accumulate(ys.double().numpy()[None], masks, [tuple(t) for t in tiles], shape, patch, blend)
    return dict(num=num, ws=ws, sq=sq, sh=sh, num0=num0, ws0=ws0, ref=ref, n_max=int(ref["n"].max()))


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("blend", ["gaussian", "constant"])
def test_mirrored_accumulate_and_finalize_against_float64(name, blend):
    from ctunet_amd import ops
    shape, patch, overlap, batch, k, masks = CASES[name]
    r = _kernels(name, blend)
    ref, n_max = r["ref"], r["n_max"]
    assert (ref["S0"] > 0).all() and n_max >= len(masks)
    # 1e-6 is the project's figure for these accumulators.  With three passes a voxel gets up to n_max = 24 contributions
    # here; measured on an MI355X the largest rel_err of any sum in any case is 2.9e-7, so the figure stands as it is.
    tol = 1e-6
    print(f"{name}/{blend}: n_max {n_max}")
    errs = dict(S0=rel_err(r["ws"], torch.from_numpy(ref["S0"])), S1=rel_err(r["num"], torch.from_numpy(ref["S1"])),
                S2=rel_err(r["sq"], torch.from_numpy(ref["S2"])))
    if k > 1:
        errs["SH"] = rel_err(r["sh"], torch.from_numpy(ref["SH"]))
    print("   rel_err", {n: f"{e:.2e}" for n, e in errs.items()})
    assert all(e <= tol for e in errs.values()), errs
    # the moments are extra sums: S0 and S1 do not depend on whether they are accumulated
    assert torch.equal(r["num0"], r["num"]) and torch.equal(r["ws0"], r["ws"])
    probs = torch.empty_like(r["num"])
    lab = torch.empty(shape, dtype=torch.uint8, device="cuda")
    ops.window_finalize_stats(r["num"], r["ws"], probs, lab)
    assert rel_err(probs, torch.from_numpy(ref["S1"] / ref["S0"])) <= tol
    assert torch.equal(lab.cpu(), torch.argmax(probs, 0).to(torch.uint8).cpu())      # exactly the first argmax
    # without statistics it is window_finalize
    p2 = torch.empty_like(probs)
    l2 = torch.empty_like(lab)
    ops.window_finalize(r["num"], r["ws"], p2, l2)
    assert torch.equal(p2, probs) and torch.equal(l2, lab)


# ------------------------------------------------------------------------------------------------ 3. statistics
@pytest.mark.parametrize("name", list(CASES))
def test_finalize_statistics(name):
    from ctunet_amd import ops
    shape, patch, overlap, batch, k, masks = CASES[name]
    r = _kernels(name, "gaussian")
    n_max = r["n_max"]
    num, ws, sq, sh = r["num"], r["ws"].clone(), r["sq"], r["sh"]
    ws[0, 0, 0] = 0                                   # one uncovered voxel
    probs, var = torch.empty_like(num), torch.empty_like(sq)
    ent, mi = (torch.empty_like(ws), torch.empty_like(ws)) if k > 1 else (None, None)
    lab = torch.empty(shape, dtype=torch.uint8, device="cuda")
    ops.window_finalize_stats(num, ws, probs, lab, sq, sh, var, ent, mi)
    # the float64 finalize of the device's own float32 accumulators: only the finalize arithmetic is under test
    own = R.finalize(dict(S0=ws.double().cpu().numpy(), S1=num.double().cpu().numpy(), S2=sq.double().cpu().numpy(),
                          SH=(sh if k > 1 else ws).double().cpu().numpy()))
    full = R.finalize(dict(r["ref"], S0=np.where(ws.cpu().numpy() > 0, r["ref"]["S0"], 0.0)))
    # variance against the full float64 restatement: S2/S0 and probs^2 are both <= 1 for inputs in [0,1] and each carries
    # about n_max sequential roundings plus the division, the square and the subtraction
    e_var = np.abs(var.cpu().numpy() - full["variance"]).max()
    print(f"{name}: n_max {n_max}, variance abs err {e_var:.2e} (bound {4 * (n_max + 3) * U:.2e})")
    assert e_var <= 4 * (n_max + 3) * U
    assert (var >= 0).all() and (var[:, 0, 0, 0] == 0).all() and (probs[:, 0, 0, 0] == 0).all() and lab[0, 0, 0] == 0
    assert var.max() > 1e-3                            # (it is a variance of something)
    if k > 1:
        # entropy: K terms q ln q of magnitude <= 1/e, each a few roundings and one logf, over ln K >= ln 2
        e_ent = np.abs(ent.cpu().numpy() - own["entropy"]).max()
        # mutual information: the entropy's error, plus the division SH/S0 (a value <= 1: 2 u with the quotient's own
        # rounding) and the subtraction (u), rounded up to 4 u
        e_mi = np.abs(mi.cpu().numpy() - own["mutual_information"]).max()
        print(f"   entropy abs err {e_ent:.2e} (bound {16 * k * U:.2e}), mutual information {e_mi:.2e} "
              f"(bound {(16 * k + 4) * U:.2e})")
        assert e_ent <= 16 * k * U and e_mi <= (16 * k + 4) * U
        assert (mi >= 0).all() and (ent >= 0).all() and ent[0, 0, 0] == 0 and mi[0, 0, 0] == 0
        assert mi.max() > 1e-3
    # each statistic alone and the variance in place over S2 give the same bits
    sq2, p2 = sq.clone(), torch.empty_like(num)
    ops.window_finalize_stats(num, ws, p2, None, sq2, None, sq2)
    assert torch.equal(sq2, var) and torch.equal(p2, probs)
    if k > 1:
        e2, m2 = torch.empty_like(ws), torch.empty_like(ws)
        ops.window_finalize_stats(num, ws, p2, None, ent=e2)
        ops.window_finalize_stats(num, ws, p2, None, sh=sh, mi=m2)
        assert torch.equal(e2, ent) and torch.equal(m2, mi)


# ------------------------------------------------------------------------------------------------ 4. end to end
SHAPE, PATCH, OVERLAP, BATCH = (40, 52, 70), (32, 32, 32), (8, 8, 8), 5     # 2 x 2 x 3 = 12 tiles: a partial last batch


def _contributions(models, vol, masks):
    """float64 [M, F, T, K, ...] per head: every model's own eval output on the torch.flip-ed extracted patches."""
    from ctunet_amd import ops
    from ctunet_amd.inference import tile_grid
    tiles = tile_grid(SHAPE, PATCH, OVERLAP)
    patches = ops.extract_patches(vol, torch.from_numpy(tiles).cuda(), PATCH)
    heads = None
    with torch.no_grad():
        for m in models:
            was = m.training
            m.eval()
            per_model = None
            for mask in masks:
                x = _flip(patches, mask).contiguous()
                outs = [m(x[i:i + BATCH].contiguous()) for i in range(0, x.shape[0], BATCH)]
                outs = [o if isinstance(o, tuple) else (o,) for o in outs]
                ys = [torch.cat([o[h] for o in outs]).double().cpu().numpy() for h in range(len(outs[0]))]
                per_model = [[y] for y in ys] if per_model is None else [p + [y] for p, y in zip(per_model, ys)]
            m.train(was)
            heads = [[p] for p in per_model] if heads is None else [a + [p] for a, p in zip(heads, per_model)]
    return [np.array(h) for h in heads], [tuple(t) for t in tiles]


def _reference(models, vol, masks):
    ys, tiles = _contributions(models, vol, masks)
    accs = [R.accumulate(y, masks, tiles, SHAPE, PATCH, "gaussian") for y in ys]
    return accs, [R.finalize(a) for a in accs], [float(np.abs(y).max()) for y in ys]


def _as_tuple(v):
    return v if isinstance(v, tuple) else (v,)


@pytest.mark.parametrize("cls", ["UNet", "UNetSP"])
def test_end_to_end_mirrored_passes_against_the_restatement(cls):
    import ctunet_amd as A
    torch.manual_seed(21)
    net = _perturb_bn(getattr(A, cls)(), 22).cuda()
    vol = torch.randn((net._plan.in_ch,) + SHAPE, generator=gen(23)).cuda()
    pred = A.predict_volume(net, vol, patch=32, overlap=8, batch=BATCH, flips=("x", "zy"))
    assert pred.uncertainty is None
    _, refs, _ = _reference([net], vol, (0, 1, 6))
    probs, labs = _as_tuple(pred.probs), _as_tuple(pred.labels)
    assert len(probs) == len(refs) == (2 if cls == "UNetSP" else 1)
    for p, lab, ref in zip(probs, labs, refs):
        e = rel_err(p, torch.from_numpy(ref["probs"]))
        print(f"{cls}: probs rel_err {e:.2e}")
        assert e <= 1e-6
        assert lab.dtype == torch.uint8 and torch.equal(lab, torch.argmax(p, 0).to(torch.uint8))
    # the mirrored passes did something: the plain prediction differs
    plain = A.predict_volume(net, vol, patch=32, overlap=8, batch=BATCH)
    assert not torch.equal(_as_tuple(plain.probs)[0], probs[0])


# ------------------------------------------------------------------------------------------------ 5. defaults
def test_default_arguments_return_the_bits_of_the_old_ops():
    import ctunet_amd as A
    from ctunet_amd import ops
    from ctunet_amd.inference import WEIGHT_FLOOR, plan_batches, tile_grid, window_tables
    torch.manual_seed(31)
    net = _perturb_bn(A.UNetSP(), 32).cuda().eval()
    vol = torch.randn((2,) + SHAPE, generator=gen(33)).cuda()
    # the call as it ran before the mirrored kernels existed: extract_patches -> forward -> window_accumulate -> finalize
    tiles = tile_grid(SHAPE, PATCH, OVERLAP)
    bp = plan_batches(tiles, BATCH, SHAPE, PATCH)
    tabs = tuple(torch.from_numpy(t).cuda() for t in window_tables(PATCH, "gaussian", 0.125))
    nums = [torch.zeros((2,) + SHAPE, device="cuda") for _ in range(2)]
    ws = torch.zeros(SHAPE, device="cuda")
    with torch.no_grad():
        for b in range(bp.coords.shape[0]):
            meta = torch.from_numpy(bp.meta()[b]).cuda()
            coords, valid, box = meta[:3 * BATCH].view(BATCH, 3), meta[3 * BATCH:4 * BATCH], meta[4 * BATCH:]
            for j, (y, num) in enumerate(zip(net(ops.extract_patches(vol, coords, PATCH)), nums)):
                ops.window_accumulate(y, coords, valid, box, tabs, WEIGHT_FLOOR, bp.extent, num, ws if j == 0 else None)
    labs = [torch.empty(SHAPE, dtype=torch.uint8, device="cuda") for _ in nums]
    for num, lab in zip(nums, labs):
        ops.window_finalize(num, ws, num, lab)
    kw = dict(patch=32, overlap=8, batch=BATCH)
    for pred in (A.predict_volume(net, vol, **kw), A.predict_volume(net, vol, flips=None, uncertainty=None, **kw),
                 A.predict_volume(net, vol, flips=(), **kw), A.predict_volume([net], vol, **kw),
                 A.predict_volume((net,), vol, flips=[], graph=True, **kw)):
        assert pred.uncertainty is None
        assert all(torch.equal(a, b) for a, b in zip(pred.probs, nums))
        assert all(torch.equal(a, b) for a, b in zip(pred.labels, labs))


# ------------------------------------------------------------------------------------------------ 6. ensembles
@pytest.mark.parametrize("precisions", [("fp32", "fp32"), ("bf16", "fp32")])
def test_ensemble_against_the_restatement(precisions):
    import ctunet_amd as A
    nets = []
    for seed, prec in zip((41, 42), precisions):
        torch.manual_seed(seed)
        nets.append(_perturb_bn(A.UNet(), seed + 10).cuda().set_precision(prec))
    vol = torch.randn((1,) + SHAPE, generator=gen(43)).cuda()
    stats = ("entropy", "variance", "mutual_information")
    pred = A.predict_volume(nets, vol, patch=32, overlap=8, batch=BATCH, flips=("y",), uncertainty=stats)
    (acc,), (ref,), (ymax,) = _reference(nets, vol, (0, 2))
    n_max = int(acc["n"].max())
    e = rel_err(pred.probs, torch.from_numpy(ref["probs"]))
    assert set(pred.uncertainty) == set(stats)
    var, ent, mi = (pred.uncertainty[n] for n in ("variance", "entropy", "mutual_information"))
    assert var.shape == pred.probs.shape and ent.shape == mi.shape == SHAPE
    assert all(t.dtype == torch.float32 for t in (var, ent, mi))
    # variance: the bound of test_finalize_statistics for inputs in [0,1], scaled by the largest y^2 of this net
    e_var = np.abs(var.cpu().numpy() - ref["variance"]).max()
    b_var = 4 * (n_max + 3) * U * max(1.0, ymax * ymax)
    # entropy and mutual information against float64 on the returned probabilities / the restatement's contribution entropy
    own_ent = R.entropy(pred.probs.double().cpu().numpy())
    e_ent = np.abs(ent.cpu().numpy() - own_ent).max()
    e_mi = np.abs(mi.cpu().numpy() - np.maximum(own_ent - acc["SH"] / acc["S0"], 0)).max()
    # finalize (16 K + 4) u as in test_finalize_statistics; SH / S0 <= 1 from two float32 sums of (n_max + 8) u each
    b_mi = (16 * 2 + 4 + 2 * (n_max + 8)) * U
    print(f"ensemble {precisions}: n_max {n_max}, max |y| {ymax:.2f}, probs rel_err {e:.2e}, variance {e_var:.2e} (bound "
          f"{b_var:.2e}), entropy {e_ent:.2e} (bound {32 * U:.2e}), mutual information {e_mi:.2e} (bound {b_mi:.2e})")
    assert e <= 1e-6
    assert e_var <= b_var and e_ent <= 16 * 2 * U and e_mi <= b_mi
    assert (var >= 0).all() and (mi >= 0).all() and (ent >= 0).all() and ent.max() <= 1 + 32 * U
    # two different nets disagree somewhere: the ensemble is not one of its members, and the statistics see it
    single = A.predict_volume(nets[1], vol, patch=32, overlap=8, batch=BATCH, flips=("y",))
    assert not torch.equal(single.probs, pred.probs) and var.max() > 0 and mi.max() > 0
    for n in nets:
        n.set_precision("fp32")


# ------------------------------------------------------------------------------------------------ 7. graph
def test_graph_replay_with_flips_ensemble_and_statistics():
    import ctunet_amd as A
    nets = []
    for seed in (51, 52):
        torch.manual_seed(seed)
        nets.append(_perturb_bn(A.UNetSP(), seed + 10).cuda())
    vol = torch.randn((2,) + SHAPE, generator=gen(53)).cuda()
    stats = ("entropy", "variance", "mutual_information")
    kw = dict(patch=32, overlap=8, batch=BATCH)

    def same(a, b):
        ok = all(torch.equal(x, y) for x, y in zip(a.probs, b.probs)) and all(torch.equal(x, y) for x, y in zip(a.labels, b.labels))
        if a.uncertainty is None or b.uncertainty is None:
            return ok and a.uncertainty is b.uncertainty
        return ok and set(a.uncertainty) == set(b.uncertainty) and all(
            torch.equal(x, y) for n in a.uncertainty for x, y in zip(a.uncertainty[n], b.uncertainty[n]))

    e1 = A.predict_volume(nets, vol, flips=("x", "zy"), uncertainty=stats, **kw)
    g1 = A.predict_volume(nets, vol, flips=("x", "zy"), uncertainty=stats, graph=True, **kw)
    assert same(g1, e1)
    assert same(A.predict_volume(nets, vol, flips=("x", "zy"), uncertainty=stats, **kw), e1)        # and between two calls
    for n in stats:
        assert isinstance(e1.uncertainty[n], tuple) and len(e1.uncertainty[n]) == 2
    caps = [n.__dict__["_window_graph"] for n in nets]
    assert caps[0][2] is caps[1][2] and caps[0][3] is not caps[1][3]          # one window, one captured step per model
    # other flips, the same statistics: the captures are replayed, not rebuilt
    e2 = A.predict_volume(nets, vol, flips=("zyx", "y", "x"), uncertainty=stats, **kw)
    g2 = A.predict_volume(nets, vol, flips=("zyx", "y", "x"), uncertainty=stats, graph=True, **kw)
    assert all(n.__dict__["_window_graph"][3] is c[3] for n, c in zip(nets, caps))
    assert same(g2, e2) and not same(g2, g1)
    assert same(g1, e1)                                                       # the first result was not overwritten
    # no flips at all is one more set of flips for the same captures
    g3 = A.predict_volume(nets, vol, uncertainty=stats, graph=True, **kw)
    assert all(n.__dict__["_window_graph"][3] is c[3] for n, c in zip(nets, caps))
    assert same(g3, A.predict_volume(nets, vol, uncertainty=stats, **kw))
    # an ensemble that swaps a member rebuilds, and the member left out does not keep the old window and its capture
    torch.manual_seed(54)
    third = _perturb_bn(A.UNetSP(), 64).cuda()
    g4 = A.predict_volume([nets[0], third], vol, uncertainty=stats, graph=True, **kw)
    assert same(g4, A.predict_volume([nets[0], third], vol, uncertainty=stats, **kw))
    assert "_window_graph" not in nets[1].__dict__
    assert nets[0].__dict__["_window_graph"][2] is third.__dict__["_window_graph"][2] is not caps[0][2]
    # a plain call afterwards still returns the plain bits, graphed (its own capture) or not
    plain = A.predict_volume(nets[0], vol, **kw)
    assert same(A.predict_volume(nets[0], vol, graph=True, **kw), plain)
    assert nets[0].__dict__["_window_graph"][3] is not caps[0][3]
    assert same(A.predict_volume(nets[0], vol, graph=True, **kw), plain)


# ------------------------------------------------------------------------------------------------ 8. side effects
@pytest.mark.parametrize("graph", [False, True])
def test_no_side_effects_on_any_model(graph, monkeypatch):
    import ctunet_amd as A
    from ctunet_amd import ops
    torch.manual_seed(61)
    a = _perturb_bn(A.UNet(), 62).cuda().train()
    b = _perturb_bn(A.UNet(), 63).cuda().eval()
    before = [{k: v.clone() for k, v in n.state_dict().items()} for n in (a, b)]
    vol = torch.randn((1, 40, 40, 40), generator=gen(64)).cuda()
    A.predict_volume([a, b], vol, patch=32, overlap=8, batch=2, flips="all", uncertainty=("variance", "entropy"), graph=graph)
    assert a.training and not b.training
    for n, sd in zip((a, b), before):
        for k, v in n.state_dict().items():
            assert torch.equal(v, sd[k]), k

    def boom(*args, **kwargs):
        raise RuntimeError("boom")

    monkeypatch.setattr(ops, "window_finalize_stats", boom)
    with pytest.raises(RuntimeError, match="boom"):
        A.predict_volume([a, b], vol, patch=32, overlap=8, batch=2, uncertainty="variance", graph=graph)
    assert a.training and not b.training                    # restored on an exception too
