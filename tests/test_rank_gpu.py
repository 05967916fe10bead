"""The rank filters of ctunet_amd.preprocess on the GPU: every result is bit-equal to the numpy restatement (tests/rank_ref.py)."""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import rank_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODES = ("nearest", "reflect", "constant")
SIZES = ((3, 3, 3), (5, 5, 5), (1, 3, 7), (7, 1, 3), (3, 1, 1), (1, 1, 1))
SHAPES = ((1, 1, 6), (2, 3, 4), (5, 7, 9), (9, 17, 33), (4, 18, 70), (2, 3, 5, 16, 31))
KINDS = {"mask": 1, "u1": 1, "i2": -1000, "f4": -1.5}              # the constant of mode "constant" per input kind


def _values(shape, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "mask":
        return (rng.random(shape) < 0.4).astype(np.uint8)
    if kind == "u1":
        return rng.integers(0, 256, shape).astype(np.uint8)
    if kind == "i2":
        return rng.integers(-1024, 3072, shape).astype(np.int16)
    return (rng.integers(-40, 41, shape) * 0.37).astype(np.float32)     # repeated values, both signs


def _dev(x: np.ndarray) -> torch.Tensor:
    return torch.tensor(x, device=DEV)


def _same_bits(got: torch.Tensor, want: np.ndarray, what=""):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    a, b = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    assert np.array_equal(a, b), f"{what}: {np.count_nonzero(a != b)} of {a.size} bytes differ"


def _ranks(n):
    """(label, public call, 0-based rank) of the grid's five ranks for a box of n elements."""
    from ctunet_amd import preprocess as pp
    calls = [("median", lambda x, s, **k: pp.median_filter(x, s, **k), n // 2),
             ("min", lambda x, s, **k: pp.minimum_filter(x, s, **k), 0),
             ("max", lambda x, s, **k: pp.maximum_filter(x, s, **k), n - 1),
             ("p25", lambda x, s, **k: pp.percentile_filter(x, 25, s, **k), R.percentile_rank(25, n))]
    if n >= 2:
        calls.append(("rank-2", lambda x, s, **k: pp.rank_filter(x, -2, s, **k), n - 2))
    return calls


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", MODES)
def test_grid_is_the_rule(shape, mode):
    from ctunet_amd import preprocess as pp
    for seed, (kind, cval) in enumerate(KINDS.items()):
        x = _values(shape, kind, seed)
        xd = _dev(x)
        for size in SIZES:
            n = size[0] * size[1] * size[2]
            calls = _ranks(n)
            wants = R.rank_filters(x, [c[2] for c in calls], size, mode, cval)
            for (label, call, rank), want in zip(calls, wants):
                got = call(xd, size, mode=mode, cval=cval)
                _same_bits(got, want, f"{kind} {size} {label}")
            if n == 1:
                with pytest.raises(ValueError):
                    pp.rank_filter(xd, -2, size)
    assert torch.equal(pp.median_filter(xd, 3), pp.median_filter(xd, (3, 3, 3), mode="nearest", cval=0))


@pytest.mark.parametrize("kind", ("i2", "f4"))
def test_every_rank_of_the_3x3x3_box(kind):
    """27 ranks: the separable kernel at 0 and 26, the 13 instantiations of the register kernel plain and on flipped keys."""
    from ctunet_amd import preprocess as pp
    x = _values((9, 6, 70), kind, 21) if kind == "i2" else R.specials()
    xd = _dev(x)
    for mode in MODES:
        wants = R.rank_filters(x, range(27), 3, mode, 2)
        for rank in range(27):
            _same_bits(pp.rank_filter(xd, rank, 3, mode=mode, cval=2), wants[rank], f"{mode} rank {rank}")


def test_float32_specials():
    from ctunet_amd import preprocess as pp
    x = R.specials()
    xd = _dev(x)
    for size, mode in (((3, 3, 3), "nearest"), ((1, 3, 3), "reflect"), ((3, 1, 5), "constant"), ((5, 5, 5), "reflect")):
        n = size[0] * size[1] * size[2]
        ranks = (0, n // 2, n - 1, 1)
        for rank, want in zip(ranks, R.rank_filters(x, ranks, size, mode, 2.0)):
            _same_bits(pp.rank_filter(xd, rank, size, mode=mode, cval=2.0), want, f"{size} {mode} {rank}")


@pytest.mark.parametrize("path,size,ranks", (("fast3", (3, 3, 3), (13, 20)), ("separable", (5, 3, 7), (0, 104)),
                                             ("generic", (3, 5, 3), (17, 22))))
def test_tile_seams(path, size, ranks):
    """More than one tile along every axis, none of them whole."""
    from ctunet_amd import preprocess as pp
    tz, ty, tx = pp.TILE[path]
    shape = (tz + 3, 2 * ty + 1, tx + 7)
    for kind, cval in KINDS.items():
        x = _values(shape, kind, 31)
        xd = _dev(x)
        for mode in ("reflect", "constant"):
            for rank, want in zip(ranks, R.rank_filters(x, ranks, size, mode, cval)):
                assert pp.path_of(size, rank) == path
                _same_bits(pp.rank_filter(xd, rank, size, mode=mode, cval=cval), want, f"{kind} {mode} {rank}")


@pytest.mark.parametrize("off", (1, 2, 6))
def test_views_off_the_16_byte_grid(off):
    from ctunet_amd import preprocess as pp
    shape = (4, 6, 75)
    nvox = shape[0] * shape[1] * shape[2]
    for kind in ("u1", "i2", "f4"):
        x = _values(shape, kind, 41)
        flat = torch.zeros(nvox + 64, dtype=_dev(x).dtype, device=DEV)
        assert flat.data_ptr() % 16 == 0
        xd = flat[off:off + nvox].view(shape)
        xd.copy_(_dev(x))
        assert xd.is_contiguous() and (xd.data_ptr() - flat.data_ptr()) == off * flat.element_size()
        for size, rank in (((3, 3, 3), 13), ((5, 5, 5), 124), ((1, 3, 7), 10)):
            want = R.rank_filter(x, rank, size, "reflect")
            guard = torch.tensor(np.random.default_rng(off).integers(1, 100, nvox + 64), device=DEV).to(flat.dtype)
            buf = guard.clone()
            od = buf[off:off + nvox].view(shape)
            got = pp.rank_filter(xd, rank, size, mode="reflect", out=od)
            assert got is od
            _same_bits(od, want, f"{kind} {size}")
            assert torch.equal(buf[:off], guard[:off]) and torch.equal(buf[off + nvox:], guard[off + nvox:])
            _same_bits(pp.rank_filter(xd, rank, size, mode="reflect"), want, f"{kind} {size} (aligned out)")


def _capture(run):
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    return graph


def test_determinism_capture_and_out():
    from ctunet_amd import preprocess as pp
    shape = (9, 10, 70)
    x0, x1 = _values(shape, "i2", 51), _values(shape, "i2", 52)
    xd = _dev(x0)
    cases = (((3, 3, 3), 13), ((5, 5, 5), 0), ((3, 5, 3), 22))
    outs = [torch.empty_like(xd) for _ in cases]
    for (size, rank), od in zip(cases, outs):
        a, b = pp.rank_filter(xd, rank, size), pp.rank_filter(xd, rank, size)
        assert torch.equal(a, b)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        pp.rank_filter(xd, rank, size, out=od)
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == before      # out=: nothing is allocated
        assert torch.equal(od, a)

    def run():
        count = torch.cuda.memory_stats()["allocation.all.allocated"]
        for (size, rank), od in zip(cases, outs):
            pp.rank_filter(xd, rank, size, mode="reflect", out=od)
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == count        # also while capturing
    graph = _capture(run)
    xd.copy_(_dev(x1))
    for od in outs:
        od.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for (size, rank), od in zip(cases, outs):
        _same_bits(od, R.rank_filter(x1, rank, size, "reflect"), f"replay {size}")
    with pytest.raises(ValueError, match="shares memory"):
        pp.median_filter(xd, 3, out=xd)


@functools.lru_cache(maxsize=None)
def _head():
    x = R.synthetic_head()
    x.setflags(write=False)
    return x


def test_extract_skull_takes_the_median_first():
    from ctunet_amd import preprocess as pp
    ct = _head()
    xd = _dev(ct)
    kw = dict(spacing=(0.8, 0.45, 0.45), sigma=0.4, closing_radius=1.0)
    med = pp.median_filter(xd, 3)
    _same_bits(med, R.median_filter(ct, 3))
    got = pp.extract_skull(xd, 300, median=3, **kw)
    assert got.dtype == torch.uint8 and torch.equal(got, pp.extract_skull(med, 300, **kw))
    assert torch.equal(pp.extract_skull(xd, 300, median=(1, 3, 3), components=0),
                       pp.extract_skull(pp.median_filter(xd, (1, 3, 3)), 300, components=0))
    plain = pp.extract_skull(xd, 300, **kw)
    assert torch.equal(pp.extract_skull(xd, 300, median=0, **kw), plain)
    assert torch.equal(pp.extract_skull(xd, 300, median=1, **kw), plain)
    # the specks are bone-valued single voxels: the threshold alone keeps them, the median removes them
    specks = (ct == 3000) & (ndi.uniform_filter((ct > 300).astype(np.float32), 3) < 0.2)
    assert specks.sum() > 20
    raw, cleaned = pp.extract_skull(xd, 300, components=0).cpu().numpy(), pp.extract_skull(xd, 300, median=3, components=0).cpu().numpy()
    assert raw[specks].all() and not cleaned[specks].any()


def test_median_undoes_salt_and_pepper_like_scipy():
    from ctunet_amd import preprocess as pp
    clean, noisy = R.shell_with_flips()
    assert clean.shape == (24, 40, 40) and 200 < np.count_nonzero(clean != noisy) < 2000
    got = pp.median_filter(_dev(noisy), size=3).cpu().numpy()
    want = ndi.median_filter(noisy, size=3, mode="nearest")
    assert np.array_equal(got, want)
    assert np.count_nonzero(got != clean) <= np.count_nonzero(want != clean) < np.count_nonzero(noisy != clean)
