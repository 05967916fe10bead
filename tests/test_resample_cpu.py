"""Resampling of ctunet_amd.resample without a GPU: the pinned rule (tests/resample_ref.py) against scipy and torch, the
spacing geometry, argument validation (which must raise before anything is launched) and the C-ABI entry point in the
header, the ctypes table and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy import ndimage as ndi

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = (((7, 9, 11), (13, 8, 20)), ((5, 1, 6), (9, 3, 4)), ((40, 48, 56), (31, 64, 45)), ((12, 10, 9), (12, 10, 9)))


@pytest.mark.parametrize("shape,size", CASES)
def test_linear_rule_is_scipys_zoom(shape, size):
    """float32 rule against zoom(order=1, mode="nearest", grid_mode=True) in float64: seven lerps of three roundings each
    plus the weight's rounding stay inside 2^-18 max|x|."""
    x = np.random.default_rng(3).standard_normal(shape)
    _, a = R.scales(shape, size)
    want = ndi.zoom(x, [m / n for n, m in zip(shape, size)], order=1, mode="nearest", grid_mode=True)
    assert want.shape == size and want.dtype == np.float64
    got = R.linear(x.astype(np.float32), size, a)
    assert got.dtype == np.float32 and got.shape == size
    err = np.abs(got.astype(np.float64) - R.linear(x.astype(np.float32).astype(np.float64), size, a, np.float64,
                                                   R.exact_weights(shape, size, a))).max()
    err_scipy = np.abs(got.astype(np.float64) - want).max()
    print(f"{shape}->{size}: |rule32 - rule64| {err:.3g}, |rule32 - zoom| {err_scipy:.3g}, bound {2.0 ** -18 * np.abs(x).max():.3g}")
    assert err_scipy <= 2.0 ** -18 * np.abs(x).max()
    # and torch's trilinear, whose coordinate is float32: a coordinate below 64 is off by at most 2 ulp = 2^-17, which
    # moves a lerp between two neighbours (at most 2 max|x| apart) by 2^-16 max|x| per axis
    t = F.interpolate(torch.from_numpy(x.astype(np.float32))[None, None], size=size, mode="trilinear", align_corners=False)
    assert np.abs(t[0, 0].numpy() - got).max() <= (3 * 2.0 ** -16 + 2.0 ** -18) * np.abs(x).max()


@pytest.mark.parametrize("n,m", ((7, 13), (9, 8), (1, 3), (6, 4), (56, 45), (48, 64), (512, 230), (230, 512), (256, 16),
                                 (33, 33), (511, 512), (3, 1000)))
def test_near_table_is_torchs_nearest_exact(n, m):
    want = F.interpolate(torch.arange(n, dtype=torch.float32)[None, None], size=m, mode="nearest-exact")[0, 0]
    near = R.axis_tables(n, m, n / m)[3]
    # torch forms the coordinate in float32: where (j + 0.5) n / m is an integer exactly (512 -> 230 has two such j, at
    # 128 and 384) its product can fall just below it; there the float64 table holds that integer, and it is torch's everywhere else
    off = (2 * np.arange(m) + 1) * n % (2 * m) != 0
    assert near.dtype == np.int32 and np.array_equal(near[off], want.numpy().astype(np.int32)[off])
    assert np.array_equal(near[~off], ((2 * np.arange(m) + 1) * n // (2 * m))[~off])
    from ctunet_amd import resample as rs
    i0, w, near2 = rs.axis_tables(n, m, n / m)
    r0, r1, rw, _, _ = R.axis_tables(n, m, n / m)
    assert np.array_equal(near2, near) and np.array_equal(i0, r0) and np.array_equal(w.view(np.int32), rw.view(np.int32))
    assert i0.dtype == np.int32 and w.dtype == np.float32 and near2.dtype == np.int32
    assert i0.min() >= 0 and r1.max() <= n - 1 and (np.diff(i0) >= 0).all() and (np.diff(near) >= 0).all()
    assert w.min() >= 0.0 and w.max() <= 1.0


@pytest.mark.parametrize("k", (2, 3, 16))
@pytest.mark.parametrize("shape,size", CASES[:3])
def test_label_rule_is_the_float64_composite(shape, size, k):
    """one_hot -> linear per class -> first argmax in float64, on the voxels whose two best scores differ by more than
    1e-5; at most 6 % of the voxels of random labels are left out."""
    x = np.random.default_rng(k).integers(0, k, shape).astype(np.uint8)
    _, a = R.scales(shape, size)
    got = R.label_linear(x, size, a, k)
    assert got.dtype == np.uint8 and got.shape == size
    s = R.label_scores(x, size, a, k, np.float64, R.exact_weights(shape, size, a))
    top = np.sort(s, axis=0)
    clear = top[-1] - top[-2] > 1e-5
    left_out = 1.0 - clear.mean()
    print(f"{shape}->{size} K={k}: {left_out:.4f} of the voxels within 1e-5 of a tie")
    assert left_out <= 0.06
    assert np.array_equal(got[clear], np.argmax(s, axis=0).astype(np.uint8)[clear])


def test_label_rule_edge_cases():
    _, a = R.scales((4, 4, 4), (8, 8, 8))
    x = np.full((4, 4, 4), 7, np.uint8)                         # >= K everywhere: no class scores, class 0 wins
    assert (R.label_linear(x, (8, 8, 8), a, 3) == 0).all()
    x = np.random.default_rng(0).integers(0, 3, (4, 5, 6)).astype(np.int64)
    assert np.array_equal(R.label_linear(x, x.shape, (1.0, 1.0, 1.0), 3), x)
    assert np.array_equal(R.nearest(x, x.shape, (1.0, 1.0, 1.0)), x)
    c = np.full((3, 4, 5), np.float32(-1234.567))
    assert (R.linear(c, (5, 3, 9), R.scales(c.shape, (5, 3, 9))[1]) == np.float32(-1234.567)).all()


def test_spacing_geometry():
    from ctunet_amd import resample as rs
    n, m, a = rs.geometry((224, 512, 512), spacing=(0.8, 0.45, 0.45), new_spacing=1.0)
    assert m == (179, 230, 230) and n == (224, 512, 512)
    assert a == (1.0 / 0.8, 1.0 / 0.45, 1.0 / 0.45)
    assert R.scales((224, 512, 512), None, (0.8, 0.45, 0.45), 1.0) == (m, a)
    r = rs.Resampler((224, 512, 512), in_spacing=(0.8, 0.45, 0.45), out_spacing=1.0)
    assert r.out_shape == (179, 230, 230) and r.out_spacing == (1.0, 1.0, 1.0) and r.in_shape == (224, 512, 512)
    assert r.inverse_scale == (0.8, 0.45, 0.45)
    # the inverse is pinned on in_shape, not on a rounding of m * s_new / s: 230 / 0.45 = 511.1 rounds to 511
    assert int(np.floor(230 * 1.0 / 0.45 + 0.5)) == 511
    for t, length in zip(r._host[1], (3,) * 3):
        assert t.shape == (224 + 512 + 512,)
    i0, w, near = r._host[1]
    want = R.axis_tables(230, 512, 0.45)
    assert np.array_equal(i0[224 + 512:], want[0]) and np.array_equal(near[224 + 512:], want[3])
    assert np.array_equal(w[224 + 512:], want[2])
    assert r._host[0][0].shape == (179 + 230 + 230,)
    # size mode: a = n / m, the inverse m / n; no spacing to report
    r = rs.Resampler((7, 9, 11), (13, 8, 20))
    assert r.out_shape == (13, 8, 20) and r.out_spacing is None
    assert r.scale == (7 / 13, 9 / 8, 11 / 20) and r.inverse_scale == (13 / 7, 8 / 9, 20 / 11)
    # size with both spacings: the grid is the size, the scale the spacings'
    n, m, a = rs.geometry((10, 10, 10), (7, 7, 7), 1.0, (2.0, 2.0, 2.0))
    assert m == (7, 7, 7) and a == (2.0, 2.0, 2.0)
    assert rs.geometry((3, 3, 3), spacing=1.0, new_spacing=100.0)[1] == (1, 1, 1)          # m = max(1, .)
    assert rs.geometry((3, 4, 5), spacing=(1, 1, 1), new_spacing=(2, 2, 2))[1] == (2, 2, 3)   # floor(x + 0.5): 1.5 -> 2, 2.5 -> 3


def test_arguments_are_validated_before_any_launch():
    from ctunet_amd import resample as rs
    x = torch.zeros(4, 5, 6)
    lab = torch.zeros(4, 5, 6, dtype=torch.uint8)
    for make in (lambda t: t, lambda t: t.to("meta")):
        xf, xl = make(x), make(lab)
        for mode in ("cubic", "bilinear", None, 1, "Linear"):
            with pytest.raises(ValueError, match="resample.*mode"):
                rs.resample(xf, (4, 5, 6), mode=mode)
        with pytest.raises(TypeError, match="resample.*num_classes"):
            rs.resample(xl, (4, 5, 6), mode="label_linear")
        for k in (2.0, True, "2"):
            with pytest.raises(TypeError, match="resample.*num_classes"):
                rs.resample(xl, (4, 5, 6), mode="label_linear", num_classes=k)
        for k in (0, 1, 17, -3):
            with pytest.raises(ValueError, match="resample.*num_classes"):
                rs.resample(xl, (4, 5, 6), mode="label_linear", num_classes=k)
        for mode in ("nearest", "linear"):
            with pytest.raises(ValueError, match="resample.*num_classes"):
                rs.resample(xl, (4, 5, 6), mode=mode, num_classes=2)
        for mode, bad in (("nearest", (torch.float64, torch.float16, torch.int8)),
                          ("linear", (torch.bool, torch.int32, torch.int64, torch.float64, torch.bfloat16)),
                          ("label_linear", (torch.float32, torch.int16, torch.int32))):
            for dt in bad:
                with pytest.raises(TypeError, match="resample.*takes"):
                    rs.resample(make(torch.zeros(4, 5, 6, dtype=dt)), (4, 5, 6), mode=mode,
                                num_classes=2 if mode == "label_linear" else None)
        with pytest.raises(ValueError, match="resample.*three dimensions"):
            rs.resample(make(torch.zeros(5, 6)), (4, 5, 6))
        with pytest.raises(TypeError, match="resample.*tensor"):
            rs.resample(np.zeros((4, 5, 6), np.float32), (4, 5, 6))
        for size in ((0, 5, 6), (4, -1, 6), (2048, 1024, 1024)):
            with pytest.raises(ValueError, match="resample.*size"):
                rs.resample(xf, size)
        for size in ((4, 5), (4, 5, 6, 7), (4.0, 5, 6), 4, (True, 5, 6)):
            with pytest.raises(TypeError, match="resample.*size"):
                rs.resample(xf, size)
        for sp in (0, -1.0, (1, 1, 0), float("nan"), float("inf")):
            with pytest.raises(ValueError, match="resample.*spacing"):
                rs.resample(xf, spacing=sp, new_spacing=1.0)
            with pytest.raises(ValueError, match="resample.*new_spacing"):
                rs.resample(xf, spacing=1.0, new_spacing=sp)
        for sp in ((1, 1), "1", (1, 1, "1"), True):
            with pytest.raises(TypeError, match="resample.*spacing"):
                rs.resample(xf, spacing=sp, new_spacing=1.0)
        with pytest.raises(ValueError, match="resample.*go together"):
            rs.resample(xf, (4, 5, 6), spacing=1.0)
        with pytest.raises(ValueError, match="resample.*go together"):
            rs.resample(xf, (4, 5, 6), new_spacing=1.0)
        with pytest.raises(ValueError, match="resample.*go together"):
            rs.resample(xf, new_spacing=1.0)
        with pytest.raises(ValueError, match="resample.*give size"):
            rs.resample(xf)
        for out in (make(torch.zeros(8, 5, 7)), make(torch.zeros(1, 8, 5, 6)), make(torch.zeros(8, 5, 6, dtype=torch.float64)),
                    make(torch.zeros(8, 5, 12))[:, :, ::2]):
            with pytest.raises(ValueError, match="resample.*out must"):
                rs.resample(xf, (8, 5, 6), out=out)
        with pytest.raises(ValueError, match="resample.*out must"):            # nearest keeps the dtype, linear does not
            rs.resample(xl, (8, 5, 6), mode="nearest", out=make(torch.zeros(8, 5, 6)))
        with pytest.raises(ValueError, match="resample.*out must"):
            rs.resample(xl, (8, 5, 6), mode="linear", out=make(torch.zeros(8, 5, 6, dtype=torch.uint8)))
        with pytest.raises(TypeError, match="resample.*out must"):
            rs.resample(xf, (8, 5, 6), out=np.zeros((8, 5, 6), np.float32))
        # valid arguments on a host / meta tensor: refused as such, still before any launch
        with pytest.raises(ValueError, match="resample.*GPU"):
            rs.resample(xf, (8, 5, 6), out=make(torch.zeros(8, 5, 6)))
        with pytest.raises(ValueError, match="resample.*GPU"):
            rs.resample(xl, spacing=(1, 2, 3), new_spacing=0.7, mode="label_linear", num_classes=16)
        with pytest.raises(ValueError, match="resample.*GPU"):
            rs.resample(make(torch.zeros(2, 3, 4, 5, 6, dtype=torch.int16)), (3, 3, 3), mode="nearest")
        r = rs.Resampler((4, 5, 6), (8, 5, 6))
        with pytest.raises(ValueError, match="Resampler.*GPU"):
            r(xf)
        with pytest.raises(ValueError, match="Resampler.inverse.*GPU"):
            r.inverse(make(torch.zeros(3, 8, 5, 6, dtype=torch.int64)), mode="label_linear", num_classes=3)
        with pytest.raises(ValueError, match="Resampler.inverse.*grid"):
            r.inverse(xf)
        with pytest.raises(ValueError, match="Resampler.*mode"):
            r(xf, mode="cubic")
        with pytest.raises(ValueError, match="Resampler.*out must"):
            r(xf, out=make(torch.zeros(4, 5, 6)))
    with pytest.raises(ValueError, match="Resampler.*give size"):
        rs.Resampler((4, 5, 6))
    with pytest.raises(ValueError, match="Resampler.*go together"):
        rs.Resampler((4, 5, 6), (4, 5, 6), in_spacing=1.0)
    with pytest.raises(ValueError, match="Resampler.*input grid"):
        rs.Resampler((4, 0, 6), (4, 5, 6))
    with pytest.raises(ValueError, match="Resampler.*GPU"):
        rs.Resampler((4, 5, 6), (4, 5, 6)).to("cpu")


def test_entry_point_declared_bound_and_exported():
    import ctunet_amd
    from ctunet_amd import _lib, ops, resample
    assert ctunet_amd.resample is resample and "resample" in ctunet_amd.__all__
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctunet_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bctu_resample\s*\(", src)
    assert "ctu_resample" in _lib.SIGNATURES and len(_lib.SIGNATURES["ctu_resample"][1]) == 16
    assert hasattr(lib, "ctu_resample")
    for name, val in (("CTU_RESAMPLE_NEAREST", ops.RESAMPLE_NEAREST), ("CTU_RESAMPLE_LINEAR", ops.RESAMPLE_LINEAR),
                      ("CTU_RESAMPLE_LABEL_LINEAR", ops.RESAMPLE_LABEL_LINEAR), ("CTU_I16", ops.RESAMPLE_CODE[torch.int16]),
                      ("CTU_I32", ops.RESAMPLE_CODE[torch.int32]), ("CTU_U8", ops.RESAMPLE_CODE[torch.uint8]),
                      ("CTU_I64", ops.RESAMPLE_CODE[torch.int64]), ("CTU_F32", ops.RESAMPLE_CODE[torch.float32])):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), src), name
    assert callable(ops.resample) and callable(resample.resample) and callable(resample.Resampler)
    # adding an entry point changes no signature: the ABI version stays
    assert _lib.load().ctu_abi_version() == _lib.ABI_VERSION


def test_bad_arguments_fail_in_the_library_before_any_launch():
    from ctunet_amd import _lib
    L = _lib.load()
    fake = 4096                      # never dereferenced: every check below fails on the host first

    def call(dtype=3, mode=0, k=0, n=1, src=(4, 5, 6), dst=(8, 5, 6), ptr=fake):
        return L.ctu_resample(ptr, dtype, mode, k, n, *src, *dst, fake, fake, fake, fake, None)

    for kw, what in ((dict(mode=3), "mode"), (dict(mode=-1), "mode"), (dict(n=0), "shape"), (dict(src=(0, 5, 6)), "shape"),
                     (dict(dst=(8, 5, -1)), "shape"), (dict(src=(2048, 1024, 1024)), "shape"),
                     (dict(dst=(1024, 2048, 1024)), "shape"), (dict(dtype=1), "dtype"), (dict(dtype=7), "dtype"),
                     (dict(mode=1, dtype=4), "dtype"), (dict(mode=1, dtype=6), "dtype"), (dict(mode=2, k=2, dtype=0), "dtype"),
                     (dict(mode=2, k=2, dtype=5), "dtype"), (dict(mode=2, k=1), "num_classes"),
                     (dict(mode=2, k=17), "num_classes"), (dict(ptr=None), "null")):
        assert call(**kw) == -1, kw
        assert what in L.ctu_last_error().decode(), (kw, L.ctu_last_error())
    with pytest.raises(_lib.CtuError, match="num_classes"):
        _lib.check(call(mode=2, k=0), "resample")
