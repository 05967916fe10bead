"""ctunet_amd.metrics on the GPU against a float64 scipy restatement of the definitions pinned in its module docstring:
surface = mask & ~binary_erosion(mask) (6-neighbourhood, background outside), directed distances = distance_transform_edt
of the other surface's complement (with sampling = spacing) at the surface voxels, numpy's linear percentile."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

pytestmark = pytest.mark.gpu

PCTS = (0.0, 50.0, 95.0, 100.0)
STRUCT = ndi.generate_binary_structure(3, 1)


# ---------------------------------------------------------------------------------------------- scipy restatement
def _surface(mask):
    return mask & ~ndi.binary_erosion(mask, structure=STRUCT, border_value=0)


def _directed(ea, eb, sp):
    """distances from the surface voxels of ea to the surface eb (None when eb is empty)."""
    if not eb.any():
        return None
    return ndi.distance_transform_edt(~eb, sampling=sp)[ea]


def _ref_pair(p, g, sp, tau):
    """float64 metrics of one pair of boolean masks."""
    ep, eg = _surface(p), _surface(g)
    n_p, n_g = int(ep.sum()), int(eg.sum())
    tot = int(p.sum()) + int(g.sum())
    r = {"dice": 2.0 * int((p & g).sum()) / tot if tot else 1.0}
    nan = float("nan")
    if n_p and n_g:
        dpg, dgp = _directed(ep, eg, sp), _directed(eg, ep, sp)
        r.update(hd=max(dpg.max(), dgp.max()), hd_dir=dpg.max(), assd=(dpg.sum() + dgp.sum()) / (n_p + n_g),
                 asd=dpg.mean())
        for q in PCTS:
            r[("hdp", q)] = max(np.percentile(dpg, q), np.percentile(dgp, q))
            r[("hdp_dir", q)] = np.percentile(dpg, q)
        r["nsd"] = nan if tau is None else ((dpg <= tau).sum() + (dgp <= tau).sum()) / (n_p + n_g)
        r["dists"] = np.concatenate([dpg, dgp])
    else:
        r.update(hd=nan, hd_dir=nan, assd=nan, asd=nan)
        for q in PCTS:
            r[("hdp", q)] = r[("hdp_dir", q)] = nan
        r["nsd"] = nan if (tau is None or n_p + n_g == 0) else 0.0
        r["dists"] = np.zeros(0)
    return r


def _ref(pm, gm, classes, spacing, tau=None):
    """pm, gm: bool [N, C, D, H, W] numpy masks; classes: scored channel indices; spacing: N triples -> {key: [N, C']}"""
    out = {}
    for i in range(pm.shape[0]):
        for j, c in enumerate(classes):
            r = _ref_pair(pm[i, c], gm[i, c], spacing[i], None if tau is None else tau[j])
            for k, v in r.items():
                out.setdefault(k, [[None] * len(classes) for _ in range(pm.shape[0])])[i][j] = v
    return {k: (np.array(v, dtype=np.float64) if k != "dists" else v) for k, v in out.items()}


def _close(got, ref):
    got = got.detach().cpu().double().numpy()
    assert got.shape == ref.shape
    assert np.allclose(got, ref, rtol=1e-6, atol=0, equal_nan=True), (got, ref)


def _exact(got, ref):
    got = got.detach().cpu().numpy()
    assert np.array_equal(got, ref.astype(np.float32), equal_nan=True), (got, ref)


# ---------------------------------------------------------------------------------------------- cases
def _labels(n, c, d, h, w, seed, side):
    """int64 [N, D, H, W] label maps: balls touching the border, boxes, parallel slabs (many tied distances) and single
    voxels; side 1 (target) is a shifted variant of side 0 (prediction)."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((n, d, h, w), np.int64)
    zz, yy, xx = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    for i in range(n):
        for k in range(1, c):
            kind = (i + k) % 3
            sh = side * (1 + k % 2)
            if kind == 0:          # ball clipped by the volume border
                cz, cy, cx = rng.integers(0, d), 0, rng.integers(0, w)
                r = 3 + k + sh
                lab[i][((zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2) <= r * r] = k
            elif kind == 1:        # parallel slabs: every distance between them ties
                z0 = 2 + 3 * k + 2 * sh
                lab[i, z0:z0 + 2] = k
            else:                  # a box touching the far corner
                lab[i, d - 6 - sh:, h - 5:, w - 7 + sh:] = k
            # a single isolated voxel is its own surface
            lab[i, rng.integers(0, d), rng.integers(0, h), rng.integers(0, w)] = k
    return lab


def _onehot_np(lab, c):
    return np.stack([lab == k for k in range(c)], 1)


def _spacings(kind, n):
    if kind == "unit":
        return None, [(1.0, 1.0, 1.0)] * n
    if kind == "aniso":
        return (3.0, 0.8, 0.65), [(3.0, 0.8, 0.65)] * n
    per = [(1.5 + 0.5 * i, 0.7 + 0.1 * i, 1.25 - 0.2 * i) for i in range(n)]
    return per, per


def _safe_tau(dists, sp_unit):
    """a tolerance no distance of the case lies within 1e-5 (relative) of, near the median distance (fp32 rounding of
    the device distances cannot move a voxel across it); with unit spacing integer tolerances are exact anyway."""
    d = np.unique(np.concatenate([x for x in dists if len(x)]))
    if sp_unit:
        return 2.0
    med = np.median(d)
    for gap_lo, gap_hi in zip(d[:-1], d[1:]):
        if gap_hi >= med and (gap_hi - gap_lo) > 4e-5 * gap_hi:
            return float((gap_lo + gap_hi) / 2)
    return float(d[-1] * 1.5)


@pytest.mark.parametrize("shape", [(2, 3, 33, 17, 40), (1, 4, 24, 31, 20)])
@pytest.mark.parametrize("sp_kind", ["unit", "aniso", "per_item"])
def test_onehot_functions_match_scipy(shape, sp_kind):
    from ctunet_amd import metrics
    n, c, d, h, w = shape
    pl, gl = _labels(n, c, d, h, w, 1, 0), _labels(n, c, d, h, w, 1, 1)
    pm, gm = _onehot_np(pl, c), _onehot_np(gl, c)
    spacing, sp = _spacings(sp_kind, n)
    yp = torch.from_numpy(pm.astype(np.float32)).cuda()
    yg = torch.from_numpy(gm.astype(np.uint8)).cuda()            # mixed input dtypes are allowed
    for inc_bg in (False, True):
        classes = list(range(0 if inc_bg else 1, c))
        ref = _ref(pm, gm, classes, sp)
        _close(metrics.compute_hausdorff_distance(yp, yg, include_background=inc_bg, spacing=spacing), ref["hd"])
        _close(metrics.compute_hausdorff_distance(yp, yg, inc_bg, directed=True, spacing=spacing), ref["hd_dir"])
        for q in PCTS:
            _close(metrics.compute_hausdorff_distance(yp, yg, inc_bg, percentile=q, spacing=spacing), ref[("hdp", q)])
            _close(metrics.compute_hausdorff_distance(yp, yg, inc_bg, percentile=q, directed=True, spacing=spacing),
                   ref[("hdp_dir", q)])
        _close(metrics.compute_average_surface_distance(yp, yg, inc_bg, symmetric=True, spacing=spacing), ref["assd"])
        _close(metrics.compute_average_surface_distance(yp, yg, inc_bg, symmetric=False, spacing=spacing), ref["asd"])
        tau = [_safe_tau([ref["dists"][i][j] for i in range(n)], sp_kind == "unit") for j in range(len(classes))]
        ref_t = _ref(pm, gm, classes, sp, tau)
        _exact(metrics.compute_surface_dice(yp, yg, tau, inc_bg, spacing=spacing), ref_t["nsd"])
        # the label-map route: dice exact, nsd exact, distances as above
        res = metrics.surface_metrics(torch.from_numpy(pl.astype(np.uint8)).cuda(), torch.from_numpy(gl).cuda(), c,
                                      spacing=spacing, percentile=95.0, tolerance=tau, include_background=inc_bg)
        _exact(res["dice"], ref_t["dice"])
        _exact(res["nsd"], ref_t["nsd"])
        _close(res["hd"], ref["hd"])
        _close(res["hd_p"], ref[("hdp", 95.0)])
        _close(res["assd"], ref["assd"])


def test_hd_equals_the_existing_kernel_bit_for_bit():
    from ctunet_amd import metrics, ops
    g = torch.Generator().manual_seed(5)
    for shape in [(2, 3, 33, 17, 40), (1, 4, 24, 31, 20), (2, 2, 40, 40, 40)]:
        n, c = shape[:2]
        pred = torch.rand(shape, generator=g)
        lab = torch.from_numpy(_labels(n, c, *shape[2:], seed=7, side=1))
        target = torch.nn.functional.one_hot(lab, c).movedim(-1, 1).float().contiguous()
        pred, target = pred.cuda(), target.cuda()
        hard = torch.nn.functional.one_hot(pred.argmax(1), c).movedim(-1, 1).float()
        hd = metrics.compute_hausdorff_distance(hard, target)
        old = ops.hausdorff(pred, target)
        assert torch.equal(hd.nan_to_num(-1), old.nan_to_num(-1))
        assert torch.equal(metrics.compute_hausdorff_distance(hard, target, percentile=100).nan_to_num(-1),
                           hd.nan_to_num(-1))
        sp = (3.0, 0.8, 0.65)
        assert torch.equal(metrics.compute_hausdorff_distance(hard, target, percentile=100, spacing=sp).nan_to_num(-1),
                           metrics.compute_hausdorff_distance(hard, target, spacing=sp).nan_to_num(-1))


def _all_rows(res):
    return torch.stack([res[k] for k in sorted(res)]).nan_to_num(-7.0)


@pytest.mark.parametrize("spacing", [None, (3.0, 0.8, 0.65)])
def test_routes_and_batching_agree_bit_for_bit(spacing):
    from ctunet_amd import metrics
    n, c, d, h, w = 3, 4, 29, 23, 37
    pl, gl = _labels(n, c, d, h, w, 3, 0), _labels(n, c, d, h, w, 3, 1)
    p64, g64 = torch.from_numpy(pl).cuda(), torch.from_numpy(gl).cuda()
    p8, g8 = p64.to(torch.uint8), g64.to(torch.uint8)
    kw = dict(spacing=spacing, percentile=95.0, tolerance=[1.5, 2.5, 4.0])
    a = metrics.surface_metrics(p8, g8, c, **kw)
    b = metrics.surface_metrics(p64, g64, c, **kw)
    assert torch.equal(_all_rows(a), _all_rows(b))
    ohp = torch.nn.functional.one_hot(p64, c).movedim(-1, 1).contiguous()
    ohg = torch.nn.functional.one_hot(g64, c).movedim(-1, 1).contiguous()
    for yp, yg in ((ohp.float(), ohg.float()), (ohp.to(torch.uint8), ohg.to(torch.uint8))):
        assert torch.equal(metrics.compute_hausdorff_distance(yp, yg, percentile=95.0, spacing=spacing).nan_to_num(-7),
                           a["hd_p"].nan_to_num(-7))
        assert torch.equal(metrics.compute_hausdorff_distance(yp, yg, spacing=spacing).nan_to_num(-7), a["hd"].nan_to_num(-7))
        assert torch.equal(metrics.compute_average_surface_distance(yp, yg, symmetric=True, spacing=spacing).nan_to_num(-7),
                           a["assd"].nan_to_num(-7))
        assert torch.equal(metrics.compute_surface_dice(yp, yg, [1.5, 2.5, 4.0], spacing=spacing).nan_to_num(-7),
                           a["nsd"].nan_to_num(-7))
    for i in range(n):
        one = metrics.surface_metrics(p8[i], g8[i], c, **kw)
        assert torch.equal(_all_rows(one), _all_rows(a)[:, i:i + 1])
    # per-item spacing triples: each item as if scored alone with its own spacing
    per = [(1.0, 1.0, 1.0), (2.0, 0.5, 0.75), (0.9, 1.1, 1.3)]
    batch = metrics.surface_metrics(p8, g8, c, spacing=per, tolerance=2.0)
    for i in range(n):
        one = metrics.surface_metrics(p8[i:i + 1], g8[i:i + 1], c, spacing=per[i], tolerance=2.0)
        assert torch.equal(_all_rows(one), _all_rows(batch)[:, i:i + 1])


def test_empty_surface_conventions():
    from ctunet_amd import metrics
    d = h = w = 12
    lab_p = torch.zeros(3, d, h, w, dtype=torch.uint8)
    lab_g = torch.zeros(3, d, h, w, dtype=torch.uint8)
    lab_p[0, 2:5, 2:5, 2:5] = 1            # item 0: target empty
    lab_p[2, 3:6, 3:9, 1:4] = 1            # item 2: both present
    lab_g[2, 4:8, 3:9, 1:4] = 1            # item 1: both empty
    r = metrics.surface_metrics(lab_p.cuda(), lab_g.cuda(), 2, percentile=50.0, tolerance=1.0)
    hd, hdp, assd, nsd, dice = (r[k][:, 0].cpu() for k in ("hd", "hd_p", "assd", "nsd", "dice"))
    assert torch.isnan(hd[:2]).all() and torch.isnan(hdp[:2]).all() and torch.isnan(assd[:2]).all()
    assert float(nsd[0]) == 0.0 and math.isnan(float(nsd[1]))
    assert float(dice[0]) == 0.0 and float(dice[1]) == 1.0
    assert torch.isfinite(torch.stack([hd[2], hdp[2], assd[2], nsd[2], dice[2]])).all()
    # the one-hot functions follow the same rules; percentile=None leaves hd_p undefined in surface_metrics
    oh = lambda t: torch.nn.functional.one_hot(t.long(), 2).movedim(-1, 1).float().cuda()
    assert float(metrics.compute_surface_dice(oh(lab_g), oh(lab_p), [1.0])[0, 0]) == 0.0
    assert torch.isnan(metrics.surface_metrics(lab_p.cuda(), lab_g.cuda(), 2, percentile=None)["hd_p"]).all()
    assert "nsd" not in metrics.surface_metrics(lab_p.cuda(), lab_g.cuda(), 2)


def test_deterministic_graph_capture_and_no_side_effects():
    from ctunet_amd import metrics
    n, c, d, h, w = 2, 3, 40, 36, 44
    pl, gl = _labels(n, c, d, h, w, 9, 0), _labels(n, c, d, h, w, 9, 1)
    p = torch.from_numpy(pl.astype(np.uint8)).cuda()
    g = torch.from_numpy(gl.astype(np.uint8)).cuda()
    p0, g0 = p.clone(), g.clone()
    kw = dict(spacing=(3.0, 0.8, 0.65), percentile=95.0, tolerance=[2.0, 3.0])
    a = _all_rows(metrics.surface_metrics(p, g, c, **kw))
    b = _all_rows(metrics.surface_metrics(p, g, c, **kw))
    assert torch.equal(a, b)
    assert torch.equal(p, p0) and torch.equal(g, g0)
    yp = torch.nn.functional.one_hot(p.long(), c).movedim(-1, 1).float().contiguous()
    yg = torch.nn.functional.one_hot(g.long(), c).movedim(-1, 1).float().contiguous()
    yp0, yg0 = yp.clone(), yg.clone()
    metrics.compute_hausdorff_distance(yp, yg, percentile=95.0)
    assert torch.equal(yp, yp0) and torch.equal(yg, yg0)

    # graph: capture once on a side stream, replay after copying new inputs into the static tensors
    sp_, sg_ = p.clone(), g.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.surface_metrics(sp_, sg_, c, **kw)           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = metrics.surface_metrics(sp_, sg_, c, **kw)
    pl2, gl2 = _labels(n, c, d, h, w, 10, 0), _labels(n, c, d, h, w, 10, 1)
    sp_.copy_(torch.from_numpy(pl2.astype(np.uint8)))
    sg_.copy_(torch.from_numpy(gl2.astype(np.uint8)))
    graph.replay()
    torch.cuda.synchronize()
    eager = metrics.surface_metrics(sp_.clone(), sg_.clone(), c, **kw)
    assert torch.equal(_all_rows(static), _all_rows(eager))
    assert not torch.equal(_all_rows(static), a)


def _shell(d, h, w, centre, radii, thick):
    zz, yy, xx = torch.meshgrid(torch.arange(d, dtype=torch.float32), torch.arange(h, dtype=torch.float32),
                                torch.arange(w, dtype=torch.float32), indexing="ij")
    r = (((zz - centre[0]) / radii[0]) ** 2 + ((yy - centre[1]) / radii[1]) ** 2 + ((xx - centre[2]) / radii[2]) ** 2).sqrt()
    return (r <= 1.0) & (r >= 1.0 - thick)


def test_whole_volume_skull_shells_with_spacing():
    from ctunet_amd import metrics
    d, h, w = 224, 304, 304
    sp = (1.25, 0.7, 0.7)
    g = _shell(d, h, w, (112, 150, 152), (100, 140, 135), 0.06)
    p = _shell(d, h, w, (114, 149, 150), (98, 141, 136), 0.055)
    p[150:200, 100:200, 200:] = False                 # a missing flap in the prediction
    lab_p, lab_g = p.to(torch.uint8), g.to(torch.uint8)
    ref = _ref(p.numpy()[None, None], g.numpy()[None, None], [0], [sp], None)
    tau = _safe_tau([ref["dists"][0][0]], False)
    ref = _ref(p.numpy()[None, None], g.numpy()[None, None], [0], [sp], [tau])
    r = metrics.surface_metrics(lab_p.cuda(), lab_g.cuda(), 2, spacing=sp, percentile=95.0, tolerance=tau)
    _close(r["hd"], ref["hd"])
    _close(r["hd_p"], ref[("hdp", 95.0)])
    _close(r["assd"], ref["assd"])
    _exact(r["nsd"], ref["nsd"])
    _exact(r["dice"], ref["dice"])


def test_scores_a_predict_volume_result_directly():
    import ctunet_amd as A
    from ctunet_amd import metrics
    torch.manual_seed(3)
    net = A.UNetSP().cuda().eval()
    vol = torch.randn(2, 48, 40, 56, generator=torch.Generator().manual_seed(4)).cuda()
    pr = A.predict_volume(net, vol, patch=32, overlap=8, batch=2)
    flap = torch.zeros(48, 40, 56, dtype=torch.uint8, device="cuda")
    flap[10:30, 5:25, 20:50] = 1
    r = metrics.surface_metrics(pr.labels[1], flap, 2, spacing=(1.0, 0.5, 0.5), tolerance=2.0)
    assert set(r) == {"dice", "hd", "hd_p", "assd", "nsd"}
    lab = pr.labels[1].cpu().numpy().astype(bool)
    ref = _ref(lab[None, None], flap.cpu().numpy().astype(bool)[None, None], [0], [(1.0, 0.5, 0.5)], [2.0])
    for k in ("hd", "assd"):
        _close(r[k], ref[k])
    _close(r["hd_p"], ref[("hdp", 95.0)])
    _exact(r["dice"], ref["dice"])
