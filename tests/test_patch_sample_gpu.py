"""Random patch sampling on the MI355X (csrc/patch_sample.hip): the chunk index against np.add.reduceat, the draw's records
and coords field for field against the NumPy restatement (tests/patch_sample_ref.py), the typed crop bit for bit against
NumPy slicing with padding and against ops.extract_patches, graph replay against an eager twin, state-dict resume and the
patch dataset through StepRunner."""
import functools

import numpy as np
import pytest
import torch

import patch_sample_ref as R

pytestmark = pytest.mark.gpu

SHAPES = {"odd": (3, (37, 45, 53)), "aligned": (1, (64, 128, 128))}
CLASS_SETS = {"nonzero": (None, 0.67), "four": ((1, 2, 7, 5), (0.2, 0.3, 0.2, 0.1))}


def _t(a):
    return torch.from_numpy(np.array(a)).cuda()                     # a copy: the shared fixtures are read-only


@functools.lru_cache(maxsize=None)
def _labels(shape):
    """uint8 [M, D, H, W] in {0, 1, 2, 7}; class 5 is absent everywhere.  Of the odd shape, item 1 holds no 2 and no 7 and
    item 2 is empty, so every class set meets an item where a chosen class is absent.  Shared and left unchanged."""
    m, dims = SHAPES[shape]
    g = np.random.RandomState(17 + m)
    lab = np.array([0, 1, 2, 7], np.uint8)[g.choice(4, size=(m,) + dims, p=[0.7, 0.15, 0.1, 0.05])]
    if m == 3:
        lab[1][lab[1] > 1] = 0
        lab[2] = 0
    lab.setflags(write=False)
    return lab


def _sampler(classes, class_p, patch, jitter, seed):
    from ctunet_amd.sampling import PatchSampler
    return PatchSampler(patch, classes=classes, class_p=class_p, jitter=jitter, seed=seed)


# ----------------------------------------------------------------------------------------------------------------- index
@pytest.mark.parametrize("classes", list(CLASS_SETS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_index_equals_reduceat(shape, classes):
    lab = _labels(shape)
    cl, cp = CLASS_SETS[classes]
    s = _sampler(cl, cp, (8, 8, 8), 0, 1)
    idx = s.index(_t(lab))
    want = R.index(lab, cl)
    assert idx.shape == lab.shape and idx.classes == cl
    assert idx.counts.dtype == torch.int32 and tuple(idx.counts.shape) == want.shape
    assert np.array_equal(idx.counts.cpu().numpy(), want)
    if cl is not None:
        assert want[:, 3].sum() == 0 and want[:, :3].sum() > 0            # class 5 is absent
    if shape == "odd":
        # a view that starts at an odd byte, and a bool tensor as its bytes
        sub = _t(lab)[1:]
        assert sub.data_ptr() % 2 == 1
        assert np.array_equal(s.index(sub).counts.cpu().numpy(), want[1:])
        assert np.array_equal(_sampler(None, 0.5, (8, 8, 8), 0, 1).index(_t(lab) != 0).counts.cpu().numpy(), R.index(lab, None))


# ------------------------------------------------------------------------------------------------------------------ draw
@pytest.mark.parametrize("full_jitter", [False, True])
@pytest.mark.parametrize("patch", [(8, 12, 20), (40, 16, 64)])
@pytest.mark.parametrize("classes", list(CLASS_SETS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_draw_equals_restatement(shape, classes, patch, full_jitter):
    lab = _labels(shape)
    m, dims = SHAPES[shape]
    cl, cp = CLASS_SETS[classes]
    jitter = tuple((p - 1) // 2 for p in patch) if full_jitter else (0, 0, 0)
    seed = 1000 + 7 * len(patch) + sum(patch) + full_jitter
    s = _sampler(cl, cp, patch, jitter, seed)
    idx = s.index(_t(lab))
    n = 256
    items = np.random.RandomState(3).randint(0, m, size=n).astype(np.int32)      # out of order, every item many times
    probs = (cp,) if cl is None else cp
    counter = 0
    for given in (items.tolist(), _t(items[:32])):                               # host items, then device items
        coords = s.draw(idx, items=given)
        host = items.tolist() if isinstance(given, list) else items[:32].tolist()
        want = R.draw(lab, cl, host, seed, counter, patch, jitter, probs)
        got = s.last_records
        assert len(got) == len(want)
        for j, (a, b) in enumerate(zip(got, want)):
            assert a == b, (j, a, b)
        assert np.array_equal(coords.cpu().numpy(), R.coords_of(want))
        counter += len(host)
        assert s.state_dict() == {"seed": seed, "counter": counter}              # advanced by P
    got = R.draw(lab, cl, items.tolist(), seed, 0, patch, jitter, probs)
    kinds = {(r["class_index"] >= 0, r["fallback"]) for r in got}
    assert (False, False) in kinds and (True, False) in kinds                    # uniform and class patches both occur
    if shape == "odd" or cl is not None:
        assert (True, True) in kinds                                             # a chosen class absent from its volume
    for r in got:
        if r["class_index"] >= 0 and not r["fallback"]:
            pred = R.predicates(lab[r["item"]], cl)[r["class_index"]]
            assert r["count"] == pred.sum() and r["centre"] == tuple(np.argwhere(pred)[r["k"]])
            assert all(s0 <= c < s0 + p for s0, c, p in zip(r["start"], r["centre"], patch))
        assert all(0 <= s0 <= max(0, nn - p) for s0, nn, p in zip(r["start"], dims, patch))


def test_draw_default_items_and_device_items_out_of_range():
    lab = _labels("odd")
    s = _sampler(None, 0.67, (8, 12, 20), (1, 2, 3), 77)
    idx = s.index(_t(lab))
    coords = torch.full((6, 4), -9, dtype=torch.int32, device="cuda")
    assert s.draw(idx, patches_per_volume=2, coords=coords) is coords
    want = R.draw(lab, None, [0, 0, 1, 1, 2, 2], 77, 0, (8, 12, 20), (1, 2, 3), (0.67,))
    assert s.last_records == want and np.array_equal(coords.cpu().numpy(), R.coords_of(want))
    # device items are the caller's: an entry outside [0, M) reads nothing and is marked
    bad = [1, 3, -1, 0, 2 ** 31 - 1, -2 ** 31]
    coords = s.draw(idx, items=torch.tensor(bad, dtype=torch.int32).cuda())
    want = R.draw(lab, None, bad, 77, 6, (8, 12, 20), (1, 2, 3), (0.67,))
    assert s.last_records == want and [r["item"] for r in want] == [1, -1, -1, 0, -1, -1]
    assert np.array_equal(coords.cpu().numpy(), R.coords_of(want))
    assert s.state_dict()["counter"] == 12


# ------------------------------------------------------------------------------------------------------------------ crop
def _source(dtype, ms, c, w, seed):
    g = np.random.RandomState(seed)
    shape = (ms, c, 9, 11, w)
    if dtype == "float32":
        return g.standard_normal(shape).astype(np.float32)
    return g.randint(0, 256, shape).astype(np.uint8) if dtype == "uint8" else g.randint(-32768, 32768, shape).astype(np.int16)


def _coords(dims, patch):
    d, h, w = dims
    pd, ph, pw = patch
    big = 2 ** 31 - 1
    rows = [(0, -2, 1, 1), (1, 1, -3, 2), (2, 1, 2, -5),                        # over the low face of each axis
            (0, d - pd + 3, 0, 0), (1, 0, h - ph + 4, 1), (2, 0, 0, w - pw + 7),   # over the high faces
            (0, -1, -1, -1), (1, d - 2, h - 3, w - 4),                             # a negative start; three faces at once
            (2, 1, 1, 0), (0, 0, 2, 1), (1, 2, 0, 2), (2, 0, 1, 3), (0, 1, 0, 5),  # rows starting at every byte alignment
            (1, 100, 0, 0), (0, 0, 0, -1000), (2, 0, -h - ph, 0),                  # wholly outside
            (0, big, -big - 1, big), (1, -big - 1, 0, 0),                          # any int32
            (-1, 0, 0, 0), (3, 1, 1, 1), (-big - 1, 0, 0, 0)]                      # items outside [0, Ms)
    return np.array(rows, np.int32)


@pytest.mark.parametrize("w", [23, 53, 128])
@pytest.mark.parametrize("dtype", ["uint8", "int16", "float32"])
def test_crop_bit_equal_to_numpy(dtype, w):
    from ctunet_amd import ops
    from ctunet_amd.sampling import crop
    fill = {"uint8": 7, "int16": -5, "float32": 2.5}[dtype]
    tdt = getattr(torch, dtype)
    for c in (1, 2):
        for ms in (3, 1):
            src = _source(dtype, ms, c, w, 31 * c + ms)
            dev = _t(src)
            for patch in ((5, 7, 20), (8, 12, 33), (16, 16, 64)):
                co = _coords(src.shape[2:], patch)
                cod = _t(co)
                got = crop(dev, cod, patch, fill=fill)
                assert got.dtype == tdt and np.array_equal(got.cpu().numpy(), R.crop(src, co, patch, fill)), (c, ms, patch)
                if dtype != "float32":                                           # exact conversion to float32
                    got = crop(dev, cod, patch, fill=fill + 0.5, dtype=torch.float32)
                    assert got.dtype == torch.float32
                    assert np.array_equal(got.cpu().numpy(), R.crop(src.astype(np.float32), co, patch, fill + 0.5))
                # into channels [1, 1 + c) of a wider output; channel 0 and the channels behind stay as they were
                out = torch.full((len(co), c + 2) + patch, 3, dtype=tdt, device="cuda")
                assert crop(dev, cod, patch, fill=fill, out=out, out_channel=1) is out
                o = out.cpu().numpy()
                assert np.array_equal(o[:, 1:1 + c], R.crop(src, co, patch, fill)) and (o[:, 0] == 3).all() and (o[:, -1] == 3).all()
                if dtype == "float32" and ms == 1:                               # the existing float32 gather, same windows
                    ok = co[co[:, 0] >= 0]
                    small = np.abs(ok[:, 1:].astype(np.int64)).max(1) < 2 ** 20   # extract_patches adds in int32
                    ok = ok[small]
                    old = ops.extract_patches(dev[0], _t(ok[:, 1:]), patch)
                    assert torch.equal(crop(dev, _t(ok), patch), old)


def test_crop_many_channels_and_bool():
    """P * C * pd above 65 535 (the cap of ctu_extract_patches_flip's grid), a bool source, misaligned out."""
    from ctunet_amd.sampling import crop
    g = np.random.RandomState(5)
    src = g.randint(0, 2, (2, 3, 6, 7, 9)).astype(bool)
    co = np.stack([g.randint(0, 2, 7000), g.randint(-2, 4, 7000), g.randint(-2, 4, 7000), g.randint(-3, 6, 7000)], 1).astype(np.int32)
    patch = (4, 3, 5)
    assert len(co) * 3 * patch[0] > 65535
    got = crop(_t(src), _t(co), patch, fill=1)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), R.crop(src.view(np.uint8), co, patch, 1))
    base = torch.zeros(7000 * 3 * 60 + 1, dtype=torch.uint8, device="cuda")
    out = base[1:].view(7000, 3, *patch)                                        # every row at an odd address
    crop(_t(src), _t(co), patch, fill=1, out=out)
    assert torch.equal(out, got) and base[0] == 0


# ----------------------------------------------------------------------------------------------------------------- graph
@pytest.mark.parametrize("index_inside", [False, True])
def test_graph_replay_equals_eager_twin(index_inside):
    from ctunet_amd.sampling import crop
    lab = _labels("odd")
    dev = _t(lab)
    vol = dev.view(3, 1, *lab.shape[1:])
    atlas = torch.rand((1, 1) + lab.shape[1:], device="cuda")
    patch, jitter = (8, 12, 20), (3, 5, 9)
    s, twin = (_sampler(None, 0.67, patch, jitter, 91).to("cuda") for _ in range(2))
    warm = _sampler(None, 0.67, patch, jitter, 5)                                # loads the three kernels before the capture
    crop(vol, warm.draw(warm.index(dev), patches_per_volume=2), patch)
    x = torch.zeros((6, 2) + patch, device="cuda")
    idx = None if index_inside else s.index(dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gi = s.index(dev) if index_inside else idx
        coords = s.draw(gi, patches_per_volume=2)
        crop(vol, coords, patch, dtype=torch.float32, out=x)
        crop(atlas, coords, patch, out=x, out_channel=1)
    assert s.state_dict()["counter"] == 0                                        # capturing runs nothing
    ti = twin.index(dev)
    for _ in range(3):
        g.replay()
        ce = twin.draw(ti, patches_per_volume=2)
        xe = torch.cat((crop(vol, ce, patch, dtype=torch.float32), crop(atlas, ce, patch)), 1)
        assert torch.equal(coords, ce) and torch.equal(x, xe)
    assert s.state_dict() == twin.state_dict() == {"seed": 91, "counter": 18}


def test_state_dict_resume():
    lab = _labels("odd")
    a = _sampler(None, 0.67, (8, 12, 20), (1, 1, 1), 51)
    idx = a.index(_t(lab))
    a.draw(idx, patches_per_volume=3)
    a.draw(idx)
    b = _sampler(None, 0.67, (8, 12, 20), (1, 1, 1), 2)
    b.load_state_dict(a.state_dict())
    assert b.seed == 51 and b.state_dict()["counter"] == 12
    assert torch.equal(a.draw(idx, patches_per_volume=2), b.draw(idx, patches_per_volume=2))
    assert a.last_records == b.last_records


# --------------------------------------------------------------------------------------------------------------- dataset
def test_patch_dataset_drives_step_runner():
    from torch.utils.data import DataLoader
    from ctunet_amd.datasets import FlapRecPatchDataset
    from ctunet_amd.sampling import PatchSampler
    from ctunet_amd.trainer import StepRunner
    from ctunet_amd.transforms import FlapRecTransform, SaltAndPepper, SkullRandomHole
    dims, patch = (48, 48, 48), (32, 32, 32)
    g = np.random.RandomState(8)
    skulls = torch.from_numpy((g.rand(4, *dims) < 0.2).astype(np.float32))       # [M,D,H,W] on the host
    atlas = torch.rand(dims)
    tr = FlapRecTransform(SkullRandomHole(double_output=True, seed=61), SaltAndPepper(p=1.0, noise_density=0.3, seed=62))
    sampler = PatchSampler(patch, class_p=0.67, jitter=8, seed=63)
    ds = FlapRecPatchDataset(skulls, sampler, atlas, transform=tr, patches_per_volume=2)
    assert len(ds) == 8
    s = ds[3]
    assert set(s) == {"image", "target", "filepath", "coords"} and s["image"].shape == (2,) + patch and s["image"].is_cuda
    assert s["image"].dtype == torch.float32 and s["filepath"] == "memory://1#1"
    full, flap = s["target"]
    assert full.shape == flap.shape == (2,) + patch and full.dtype == flap.dtype == torch.float32
    item, z, y, x = s["coords"].tolist()
    assert item == 1 and sampler.last_records[0]["start"] == (z, y, x) and tr.hole.state_dict()["counter"] == 1
    win = (slice(z, z + 32), slice(y, y + 32), slice(x, x + 32))
    assert torch.equal(s["image"][1].cpu(), atlas[win])
    assert torch.equal(full[1].cpu(), skulls[1][win]) and torch.equal(full[0].cpu(), 1 - skulls[1][win])
    assert torch.equal(flap[1].cpu() * full[1].cpu(), flap[1].cpu())            # the flap is bone
    runner = StepRunner({"problem_handler": "FlapRecWithShapePriorDoubleOut", "model_class": "UNetSP",
                         "learning_rate": 1e-4, "ce_lambda": 1.0, "dice_lambda": 1.0})
    before = [p.detach().clone() for p in runner.models["main"].parameters()]
    runner.forward_pass("train", DataLoader(ds, batch_size=2))
    assert any(not torch.equal(a, b) for a, b in zip(before, runner.models["main"].parameters()))
    avg = runner.epoch_averages()
    assert avg and all(np.isfinite(v) for v in avg.values())
    assert sampler.state_dict()["counter"] == 9
