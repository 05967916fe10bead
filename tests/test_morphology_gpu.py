"""Binary morphology, hole filling and implant extraction of ctunet_amd.postprocess on the GPU, every result bit-equal to
scipy.ndimage computed here on the host (the definitions are pinned in the module docstring and, on scipy itself, in
test_morphology_cpu.py).  There are no tolerances."""
import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

pytestmark = pytest.mark.gpu

OPS = ("erosion", "dilation", "opening", "closing")
ITERATIONS = (1, 2, 3, 5)
SHAPES = ((5, 7, 31), (9, 30, 32), (17, 33, 33), (12, 31, 63), (40, 48, 64), (17, 33, 65), (14, 30, 127), (3, 70, 129),
          (1, 1, 1), (1, 1, 200))
# Degenerate shapes: the scipy result may be all-zero or all-one there, everywhere else each case asserts it is neither.
# shape -> the first iteration count from which the steps that the border feeds (erosion with border 0, dilation with
# border 1, opening, closing) sweep the whole of the volume's shortest axis (0: every case of the shape is exempt).
DEGENERATE = {(1, 1, 1): 0, (1, 1, 200): 0, (3, 70, 129): 2, (5, 7, 31): 3, (9, 30, 32): 5}
DTYPES = (torch.bool, torch.uint8, torch.int64)
_SCIPY = {"erosion": ndi.binary_erosion, "dilation": ndi.binary_dilation, "opening": ndi.binary_opening,
          "closing": ndi.binary_closing}


def _pp():
    from ctunet_amd import postprocess
    return postprocess


def _blob(shape, seed):
    """A smooth blob filling roughly the low-x half of the volume: a wobbling interface, thick foreground and thick
    background, so five steps of any structure leave both."""
    rng = np.random.default_rng(seed)
    g = ndi.gaussian_filter(rng.standard_normal(shape), 3.0, mode="nearest")
    g = g / (np.abs(g).max() + 1e-12)
    x = np.arange(shape[2], dtype=np.float64) / max(shape[2] - 1, 1)
    return (g * 0.15 + (0.5 - x)) > 0


def _shell(shape, thickness=0.07, centre=(0.5, 0.5, 0.5), radii=(0.45, 0.46, 0.44)):
    """The ellipsoidal skull shell of scripts/bench_components.py."""
    d, h, w = shape
    zz, yy, xx = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    r = np.sqrt(((zz - d * centre[0]) / (radii[0] * d)) ** 2 + ((yy - h * centre[1]) / (radii[1] * h)) ** 2
                + ((xx - w * centre[2]) / (radii[2] * w)) ** 2)
    return (r <= 1.0) & (r >= 1.0 - thickness)


def _exempt(shape, op, k, border):
    if shape not in DEGENERATE:
        return False
    border_fed = op in ("opening", "closing") or (op == "erosion" and border == 0) or (op == "dilation" and border == 1)
    return DEGENERATE[shape] == 0 or (border_fed and k >= DEGENERATE[shape])


def _ref(op, x, st, k, border):
    if op in ("erosion", "dilation"):
        return _SCIPY[op](x, st, iterations=k, border_value=border)
    return _SCIPY[op](x, st, iterations=k)


def _run(op, t, structure, k, border, label=None):
    pp = _pp()
    fn = getattr(pp, "binary_" + op)
    if op in ("erosion", "dilation"):
        return fn(t, structure=structure, iterations=k, border_value=border, label=label)
    return fn(t, structure=structure, iterations=k, label=label)


def _as(x, dtype):
    """The bool array as a device tensor of dtype; nonzero values vary for the integer dtypes."""
    t = torch.from_numpy(x)
    if dtype == torch.bool:
        return t.cuda()
    vals = torch.from_numpy(np.random.default_rng(x.size).integers(1, 200, x.shape)).to(dtype)
    if dtype == torch.int64:
        vals = vals * 1000003 - 7 * (vals % 2) * (1 << 40)       # large and negative labels are foreground too
    return (t.to(dtype) * vals).cuda()


def _check(got, ref, like):
    assert got.shape == like.shape and got.device == like.device
    assert got.dtype == (torch.bool if like.dtype == torch.bool else torch.uint8)
    g = got.cpu().numpy()
    assert g.max(initial=0) <= 1
    assert np.array_equal(g.astype(bool), ref)


# ---------------------------------------------------------------------------------------------- op x structure sweep
@pytest.mark.parametrize("structure", (1, 2, 3))
@pytest.mark.parametrize("op", OPS)
def test_ops_bit_equal_to_scipy(op, structure):
    st = ndi.generate_binary_structure(3, structure)
    for si, shape in enumerate(SHAPES):
        x = _blob(shape, 100 + si)
        tensors = [_as(x, dt) for dt in DTYPES]
        for k in ITERATIONS:
            for border in ((0, 1) if op in ("erosion", "dilation") else (0,)):
                ref = _ref(op, x, st, k, border)
                if not _exempt(shape, op, k, border):
                    assert ref.any() and not ref.all(), (shape, op, structure, k, border)
                for t in tensors:
                    _check(_run(op, t, structure, k, border), ref, t)


@pytest.mark.parametrize("op", OPS)
def test_batch_items_do_not_leak(op):
    shape = (17, 33, 65)
    items = [_blob(shape, 7), _shell(shape, 1.0), ~_blob(shape, 9)[:, :, ::-1]]      # blob, solid ellipsoid, blob
    x = np.stack(items)
    for dt in (torch.uint8, torch.int64):
        t = _as(x, dt)
        for structure in (1, 3):
            st = ndi.generate_binary_structure(3, structure)
            for k in (1, 3):
                for border in ((0, 1) if op in ("erosion", "dilation") else (0,)):
                    ref = np.stack([_ref(op, it, st, k, border) for it in items])
                    assert all(r.any() and not r.all() for r in ref)
                    _check(_run(op, t, structure, k, border), ref, t)
    # a full item next to an empty one: nothing crosses the batch boundary
    x = np.stack([np.ones(shape, bool), np.zeros(shape, bool), np.ones(shape, bool)])
    t = torch.from_numpy(x).cuda()
    ref = np.stack([_ref(op, it, ndi.generate_binary_structure(3, 3), 2, 0) for it in x])
    _check(_run(op, t, 3, 2, 0), ref, t)


@pytest.mark.parametrize("seed", range(8))
def test_custom_asymmetric_structures(seed):
    rng = np.random.default_rng(seed)
    st = rng.random((3, 3, 3)) < (0.25 if seed % 2 else 0.5)
    st[1, 1, 1] = seed % 4 >= 2                                  # with and without the centre
    st[tuple(rng.integers(0, 3, 3))] = True
    assert not np.array_equal(st, st[::-1, ::-1, ::-1]) or seed == 0
    for shape in ((17, 33, 65), (12, 31, 63)):
        x = _blob(shape, 40 + seed)
        t = torch.from_numpy(x).cuda()
        for form in (st, torch.from_numpy(st), torch.from_numpy(st).cuda()):
            _check(_pp().binary_dilation(t, structure=form), ndi.binary_dilation(x, st), t)
        for op in OPS:
            for k in (1, 2, 3):
                for border in ((0, 1) if op in ("erosion", "dilation") else (0,)):
                    _check(_run(op, t, st, k, border), _ref(op, x, st, k, border), t)
    # one off-centre voxel: dilation shifts by +s, erosion by -s (a missing reflection swaps them)
    one = np.zeros((3, 3, 3), bool)
    one[0, 2, 2] = True
    x = _blob((9, 30, 70), 3)
    t = torch.from_numpy(x).cuda()
    d, e = ndi.binary_dilation(x, one), ndi.binary_erosion(x, one)
    assert not np.array_equal(d, e)
    _check(_pp().binary_dilation(t, structure=one), d, t)
    _check(_pp().binary_erosion(t, structure=one), e, t)


def test_skull_shell_survives_two_erosions():
    shape = (56, 76, 76)
    x = _shell(shape, 0.2)
    t = torch.from_numpy(x.astype(np.uint8)).cuda()
    ref = ndi.binary_erosion(x, iterations=2)
    assert ref.sum() > 1000 and not ref.all()
    _check(_pp().binary_erosion(t, iterations=2), ref, t)
    _check(_pp().binary_opening(t, structure=2, iterations=2), ndi.binary_opening(x, ndi.generate_binary_structure(3, 2), 2), t)
    k = _pp().MAX_ITERATIONS
    _check(_pp().binary_dilation(t, iterations=k), ndi.binary_dilation(x, iterations=k), t)
    _check(_pp().binary_erosion(t, iterations=k, border_value=1), ndi.binary_erosion(x, iterations=k, border_value=1), t)


@pytest.mark.parametrize("dtype", (torch.uint8, torch.int64))
def test_label_selects_one_class_in_the_kernel(dtype):
    shape = (17, 33, 65)
    lab = np.zeros(shape, np.int64)
    lab[_blob(shape, 1)] = 1
    lab[_shell(shape, 0.3) & (lab == 0)] = 2
    lab[~_blob(shape, 2) & (lab == 0)] = 5
    t = torch.from_numpy(lab).to(dtype).cuda()
    pp = _pp()
    st = ndi.generate_binary_structure(3, 2)
    for k in (1, 2, 5, 0, 9):
        x = lab == k
        assert x.any() == (k in (0, 1, 2, 5))
        _check(pp.binary_erosion(t, structure=2, label=k), ndi.binary_erosion(x, st), t)
        _check(pp.binary_dilation(t, structure=2, iterations=2, label=k), ndi.binary_dilation(x, st, 2), t)
        _check(pp.binary_opening(t, structure=2, label=k), ndi.binary_opening(x, st), t)
        _check(pp.binary_closing(t, structure=2, label=k), ndi.binary_closing(x, st), t)
        _check(pp.binary_fill_holes(t, label=k), ndi.binary_fill_holes(x), t)
    if dtype == torch.int64:
        big = torch.from_numpy(lab).cuda() * ((1 << 40) + 3)
        _check(pp.binary_erosion(big, label=2 * ((1 << 40) + 3)), ndi.binary_erosion(lab == 2), big)
    else:
        _check(pp.binary_erosion(t, label=300), np.zeros(shape, bool), t)     # no uint8 voxel equals 300


# ---------------------------------------------------------------------------------------------- fill holes
def _fill_cases():
    shape = (40, 48, 72)
    closed = _shell(shape, 0.25)
    cut = closed.copy()
    cut[18:22, 22:26, :40] = False                                # a tunnel from the cavity to the outside
    nested = _shell(shape, 0.15) | _shell(shape, 0.2, radii=(0.25, 0.26, 0.24)) | _shell(shape, 0.5, radii=(0.08, 0.08, 0.08))
    touching = _shell(shape, 0.25, centre=(0.5, 0.5, 0.12))       # the cavity is cut open by the x = 0 face
    diag = np.ones((9, 9, 9), bool)                               # a cavity joined to the outside only through a corner
    diag[4, 4, 4] = False
    diag[:4, :4, :4] = ~np.eye(4, dtype=bool)[:, :, None] | ~np.eye(4, dtype=bool)[None, :, :]
    rng = np.random.default_rng(5)
    noise = ndi.gaussian_filter(rng.standard_normal(shape), 1.2) > 0.02
    return {"closed": closed, "cut": cut, "nested": nested, "touching": touching, "diagonal": diag, "noise": noise,
            "empty": np.zeros((5, 6, 7), bool), "full": np.ones((5, 6, 7), bool), "one": np.zeros((1, 1, 1), bool),
            "row": np.array([1, 0, 0, 1, 0, 1] * 30, bool).reshape(1, 1, 180)}


@pytest.mark.parametrize("connectivity", (1, 2, 3))
def test_fill_holes_bit_equal_to_scipy(connectivity):
    pp = _pp()
    st = ndi.generate_binary_structure(3, connectivity)
    cases = _fill_cases()
    closed, cut, touching = cases["closed"], cases["cut"], cases["touching"]
    filled = ndi.binary_fill_holes(closed, st)
    assert filled.sum() > closed.sum() and filled[20, 24, 36] and not closed[20, 24, 36]
    assert np.array_equal(ndi.binary_fill_holes(cut, st), cut)                # nothing to fill
    assert np.array_equal(ndi.binary_fill_holes(touching, st), touching)
    assert ndi.binary_fill_holes(cases["nested"], st).sum() > cases["nested"].sum()
    for name, x in cases.items():
        ref = ndi.binary_fill_holes(x, st)
        for dt in DTYPES:
            t = _as(x, dt)
            _check(pp.binary_fill_holes(t, connectivity=connectivity), ref, t)
    # the default is scipy's default
    t = torch.from_numpy(cases["diagonal"]).cuda()
    _check(pp.binary_fill_holes(t), ndi.binary_fill_holes(cases["diagonal"]), t)
    assert not np.array_equal(ndi.binary_fill_holes(cases["diagonal"]),
                              ndi.binary_fill_holes(cases["diagonal"], ndi.generate_binary_structure(3, 3)))
    # a batch: each item on its own
    x = np.stack([closed, cut, touching])
    t = torch.from_numpy(x.astype(np.uint8)).cuda()
    _check(pp.binary_fill_holes(t, connectivity=connectivity), np.stack([ndi.binary_fill_holes(i, st) for i in x]), t)


# ---------------------------------------------------------------------------------------------- implant extraction
def _implant_scene(shape, seed=0):
    """(full skull prediction, defective skull prediction, the true flap)."""
    d, h, w = shape
    rng = np.random.default_rng(seed)
    skull = _shell(shape, 0.3)
    zz, yy, xx = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    hole = ((zz - 0.5 * d) ** 2 + (yy - 0.5 * h) ** 2 + (xx - 0.92 * w) ** 2) <= (0.22 * min(shape)) ** 2
    flap = skull & hole
    defective = skull & ~hole
    # the two outputs disagree on a one-voxel layer of the bone surface, at random
    surface = skull & ~ndi.binary_erosion(skull)
    full = skull & ~(surface & (rng.random(shape) < 0.3))
    defective = defective & ~(surface & (rng.random(shape) < 0.3))
    for i in range(6):                                            # stray islands in the full-skull prediction
        z, y, x = (int(rng.integers(1, s - 4)) for s in shape)
        e = 1 + i % 3
        if not skull[z - 1:z + e + 1, y - 1:y + e + 1, x - 1:x + e + 1].any():
            full[z:z + e, y:y + e, x:x + e] = True
    return full, defective, flap


def _ref_implant(full, defective, k, structure, connectivity, num, fill):
    st = structure if isinstance(structure, np.ndarray) else ndi.generate_binary_structure(3, structure)
    m = (full != 0) & (defective == 0)
    if k > 0:
        m = ndi.binary_opening(m, st, iterations=k)
    if fill:
        m = ndi.binary_fill_holes(m)
    lab, n = ndi.label(m, ndi.generate_binary_structure(3, connectivity))
    if n:
        sizes = np.bincount(lab.ravel())[1:]
        keep = np.zeros(n + 1, bool)
        keep[1 + np.argsort(-sizes, kind="stable")[:num]] = True
        m = keep[lab]
    return m.astype(np.uint8)


def test_extract_implant_equals_the_four_steps():
    pp = _pp()
    shape = (48, 56, 72)
    full, defective, flap = _implant_scene(shape)
    raw = full & ~defective
    assert ndi.label(raw, np.ones((3, 3, 3)))[1] > 3              # the disagreement shell and the islands are there
    f8, d8 = torch.from_numpy(full.astype(np.uint8)).cuda(), torch.from_numpy(defective.astype(np.uint8)).cuda()
    got = pp.extract_implant(f8, d8)
    assert got.dtype == torch.uint8 and got.shape == f8.shape
    ref = _ref_implant(full, defective, 1, 1, 3, 1, False)
    assert np.array_equal(got.cpu().numpy(), ref)
    # one component, the cut-out bone up to the opening
    assert ndi.label(ref, np.ones((3, 3, 3)))[1] == 1
    # (the rim of the cut keeps a few disagreement voxels that the cross still fits; the opening rounds the flap's edges)
    assert (ref.astype(bool) & ~flap).sum() <= 0.01 * flap.sum()
    assert (ref.astype(bool) & flap).sum() >= 0.85 * flap.sum()
    combos = [(0, 1, 3, 1, False), (1, 3, 1, 1, False), (2, 1, 2, 2, False), (1, 2, 3, 2, True), (0, 1, 1, 8, True),
              (3, 1, 3, 1, True)]
    for k, structure, conn, num, fill in combos:
        ref = _ref_implant(full, defective, k, structure, conn, num, fill)
        for a, b in ((f8, d8), (f8.bool(), d8.long() * 7), (f8.long() * -3, d8.bool())):
            got = pp.extract_implant(a, b, opening_iterations=k, structure=structure, connectivity=conn,
                                     num_components=num, fill_holes=fill)
            assert got.dtype == torch.uint8
            assert np.array_equal(got.cpu().numpy(), ref), (k, structure, conn, num, fill)
    assert _ref_implant(full, defective, 0, 1, 3, 2, False).sum() > _ref_implant(full, defective, 0, 1, 3, 1, False).sum()
    # fill_holes matters: a flap with a cavity
    full2 = full.copy()
    cz, cy, cx = (int(c) for c in np.argwhere(ndi.binary_erosion(flap, iterations=2))[0])
    full2[cz, cy, cx] = False
    r0, r1 = (_ref_implant(full2, defective, 1, 1, 3, 1, f) for f in (False, True))
    assert r1.sum() == r0.sum() + 1
    t2 = torch.from_numpy(full2).cuda()
    for f, r in ((False, r0), (True, r1)):
        assert np.array_equal(pp.extract_implant(t2, d8, fill_holes=f).cpu().numpy(), r)
    # an asymmetric structure and a batch of different scenes
    st = np.random.default_rng(3).random((3, 3, 3)) < 0.3
    st[1, 1, 1] = True
    scenes = [_implant_scene(shape, s) for s in (1, 2)]
    fb = torch.from_numpy(np.stack([s[0] for s in scenes])).cuda()
    db = torch.from_numpy(np.stack([s[1] for s in scenes])).cuda()
    ref = np.stack([_ref_implant(s[0], s[1], 1, st, 3, 1, True) for s in scenes])
    assert np.array_equal(pp.extract_implant(fb, db, structure=st, fill_holes=True).cpu().numpy(), ref)


def test_extract_implant_feeds_surface_metrics():
    from ctunet_amd import metrics
    pp = _pp()
    shape = (48, 56, 72)
    full, defective, flap = _implant_scene(shape, 4)
    got = pp.extract_implant(torch.from_numpy(full).cuda(), torch.from_numpy(defective).cuda())
    host = torch.from_numpy(_ref_implant(full, defective, 1, 1, 3, 1, False)).cuda()
    target = torch.from_numpy(flap.astype(np.uint8)).cuda()
    kw = dict(num_classes=2, spacing=(1.0, 0.5, 0.5), percentile=95.0, tolerance=1.0)
    a = metrics.surface_metrics(got, target, **kw)                # the device result goes in as it is
    b = metrics.surface_metrics(host, target, **kw)
    assert set(a) == set(b) and len(a) > 0
    for key in a:
        assert torch.equal(a[key], b[key]), key
        assert torch.isfinite(a[key]).all(), key


# ---------------------------------------------------------------------------------------------- determinism, capture
def test_two_calls_are_bit_equal():
    pp = _pp()
    x = torch.from_numpy(_blob((3, 40, 48, 72)[1:], 1)).cuda()
    full, defective, _ = _implant_scene((48, 56, 72))
    f, d = torch.from_numpy(full).cuda(), torch.from_numpy(defective).cuda()
    for fn in (lambda: pp.binary_opening(x, structure=3, iterations=5), lambda: pp.binary_erosion(x, iterations=7),
               lambda: pp.binary_fill_holes(~x), lambda: pp.extract_implant(f, d, fill_holes=True)):
        assert torch.equal(fn(), fn())


def test_graph_capture_replays_on_new_contents():
    pp = _pp()
    shape = (40, 48, 72)
    first, second = _blob(shape, 1), ~_blob(shape, 2)
    holes1, holes2 = _shell(shape, 0.25), _shell(shape, 0.3, radii=(0.3, 0.3, 0.3))
    full1, def1, _ = _implant_scene(shape, 1)
    full2, def2, _ = _implant_scene(shape, 2)
    buf = torch.from_numpy(first.astype(np.uint8)).cuda()
    hb = torch.from_numpy(holes1).cuda()
    fb, db = torch.from_numpy(full1).cuda(), torch.from_numpy(def1).cuda()
    st = np.random.default_rng(1).random((3, 3, 3)) < 0.4

    def tail():
        return (pp.binary_opening(buf, structure=2, iterations=3), pp.binary_erosion(buf, structure=st, border_value=1),
                pp.binary_fill_holes(hb), pp.extract_implant(fb, db, fill_holes=True, num_components=2))

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        tail()                                                    # warm-up: library loaded, kernels resident
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                 # outputs and workspaces: the graph's private pool
        outs = tail()
    buf.copy_(torch.from_numpy(second.astype(np.uint8)))
    hb.copy_(torch.from_numpy(holes2))
    fb.copy_(torch.from_numpy(full2))
    db.copy_(torch.from_numpy(def2))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in outs]
    eager = tail()
    for r, e in zip(replayed, eager):
        assert torch.equal(r, e)
    s2 = ndi.generate_binary_structure(3, 2)
    assert np.array_equal(replayed[0].cpu().numpy().astype(bool), ndi.binary_opening(second, s2, iterations=3))
    assert np.array_equal(replayed[1].cpu().numpy().astype(bool), ndi.binary_erosion(second, st, border_value=1))
    assert np.array_equal(replayed[2].cpu().numpy(), ndi.binary_fill_holes(holes2))
    assert np.array_equal(replayed[3].cpu().numpy(), _ref_implant(full2, def2, 1, 1, 3, 2, True))
    assert not np.array_equal(ndi.binary_opening(second, s2, iterations=3), ndi.binary_opening(first, s2, iterations=3))


# ---------------------------------------------------------------------------------------------- full size
def test_full_size_volume_opening_and_fill_holes():
    pp = _pp()
    shape = (224, 512, 512)
    x = _shell(shape)
    x[100:124, 250:262, 256:] = False                             # a tunnel on one side, a closed cavity is left
    x[:, :, :256] |= _shell((224, 512, 256), 0.3, radii=(0.2, 0.2, 0.2))
    t = torch.from_numpy(x.astype(np.uint8)).cuda()
    ref = ndi.binary_opening(x, iterations=2)
    assert ref.any() and not ref.all() and not np.array_equal(ref, x)
    _check(pp.binary_opening(t, iterations=2), ref, t)
    ref = ndi.binary_fill_holes(x)
    assert ref.sum() > x.sum()
    _check(pp.binary_fill_holes(t), ref, t)
