"""Affine resampling of ctunet_amd.resample without a GPU: the restated rule (tests/affine_ref.py) against the axis-aligned
rule it extends and against scipy, argument validation (which must raise before anything is launched) and the C-ABI entry
point in the header, the ctypes table and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import affine_ref as A
import registration_ref as G
import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.eye(4)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def test_identity_on_equal_grids_is_the_axis_aligned_rule():
    """With the identity and equal grids u is the voxel index itself, every weight is 0 and the output is the input; the
    axis-aligned rule agrees bit for bit.  The grids' spacings and origins are dyadic, so that (origin + k spacing - origin)
    / spacing is k exactly.  The values are multiples of 1/4 below 2^13: at the last index of an axis the axis-aligned rule
    forms x[n-2] + 1 * (x[n-1] - x[n-2]), which is x[n-1] only where that difference is exact in float32."""
    shape = (6, 10, 33)
    rng = np.random.default_rng(11)
    _, a = R.scales(shape, shape)
    for sp, org in ((None, None), ((0.5, 2.0, 0.25), (-3.0, 12.5, 0.125))):
        kw = dict(spacing=sp, origin=org, out_spacing=sp, out_origin=org)
        for dtype in (np.float32, np.int16, np.uint8):
            x = (np.round(rng.standard_normal((2,) + shape) * 1000) / (4 if dtype == np.float32 else 1)).astype(dtype) \
                if dtype != np.uint8 else rng.integers(0, 256, (2,) + shape).astype(np.uint8)
            got = A.affine_resample(x, IDENTITY, shape, mode="linear", fill=7.0, **kw)
            want = R.linear(x, shape, a)
            assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want)), (dtype, sp)
            assert np.array_equal(got, x.astype(np.float32))
            near = A.affine_resample(x, IDENTITY, shape, mode="nearest", fill=3, **kw)
            assert near.dtype == x.dtype and np.array_equal(_bits(near), _bits(R.nearest(x, shape, a)))
        lab = rng.integers(0, 5, shape).astype(np.uint8)
        got = A.affine_resample(lab, IDENTITY, shape, mode="label_linear", num_classes=4, fill=1, **kw)
        assert np.array_equal(got, R.label_linear(lab, shape, a, 4))


# an irrational-looking rigid matrix: no output voxel lands on a half-integer input coordinate
W, T = (0.2113, -0.1371, 0.3049), (1.2345, -2.7182, 0.5772)
SHAPE, OUT_SHAPE = (21, 26, 31), (24, 23, 29)
SPACING, ORIGIN, OUT_SPACING, OUT_ORIGIN = (1.3, 0.9, 1.1), (-2.0, 1.5, 0.25), (1.0, 1.2, 0.8), (0.5, -1.0, 2.0)
# measured: largest |rule - scipy| / max|x| on this case = 7.44e-08 (linear); the gate is that value times 4.  About float32
# epsilon, as expected: the weights are rounded to float32 where scipy keeps them in float64.
MEASURED_LINEAR_GAP = 7.44e-08


def _scipy_matrix():
    """(matrix, offset) of scipy.ndimage.affine_transform in index space: u = diag(1/sp) (M (oorg + idx osp)) - org / sp."""
    M = G.rigid(W, T, (12.0, 11.0, 15.0))
    lin = M[:3, :3] * np.asarray(OUT_SPACING)[None, :] / np.asarray(SPACING)[:, None]
    off = (M[:3, :3] @ np.asarray(OUT_ORIGIN) + M[:3, 3] - np.asarray(ORIGIN)) / np.asarray(SPACING)
    return M, lin, off


def test_linear_and_nearest_are_scipys_affine_transform():
    rng = np.random.default_rng(13)
    x = rng.standard_normal(SHAPE).astype(np.float32)
    M, lin, off = _scipy_matrix()
    kw = dict(spacing=SPACING, origin=ORIGIN, out_spacing=OUT_SPACING, out_origin=OUT_ORIGIN)
    fill = 0.75
    want = ndi.affine_transform(x.astype(np.float64), lin, off, OUT_SHAPE, order=1, mode="grid-constant", cval=fill)
    got = A.affine_resample(x, M, OUT_SHAPE, mode="linear", fill=fill, **kw)
    assert got.dtype == np.float32 and got.shape == OUT_SHAPE
    gap = np.abs(got.astype(np.float64) - want).max() / np.abs(x).max()
    inside = np.count_nonzero(got != np.float32(fill)) / got.size
    print(f"linear: |rule - scipy| / max|x| = {gap:.3g}, {inside:.0%} of the output inside the input")
    assert inside > 0.4
    assert gap <= 4 * MEASURED_LINEAR_GAP
    # nearest: scipy's order 0 except where u + 0.5 is (nearly) an integer, where the two may round differently
    xi = rng.integers(-1000, 3000, SHAPE).astype(np.int16)
    want = ndi.affine_transform(xi, lin, off, OUT_SHAPE, order=0, mode="grid-constant", cval=-7)
    got = A.affine_resample(xi, M, OUT_SHAPE, mode="nearest", fill=-7, **kw)
    u = A.coordinates(OUT_SHAPE, M, SPACING, ORIGIN, OUT_SPACING, OUT_ORIGIN)
    tie = np.zeros(OUT_SHAPE, bool)
    for ua in u:
        h = ua + 0.5
        tie |= np.abs(h - np.round(h)) < 1e-9
    print(f"nearest: {np.count_nonzero(tie)} of {tie.size} voxels on a tie")
    assert np.count_nonzero(tie) < 0.01 * tie.size
    assert got.dtype == np.int16 and np.array_equal(got[~tie], want[~tie])


def test_fill_outside_and_nan_matrix():
    x = np.arange(4 * 5 * 6, dtype=np.float32).reshape(4, 5, 6) + 1
    far = np.eye(4)
    far[:3, 3] = (100.0, 0.0, 0.0)
    for mode, fill, xx in (("linear", 2.5, x), ("nearest", 9.0, x), ("label_linear", 1, (x % 3).astype(np.uint8))):
        kw = dict(num_classes=3) if mode == "label_linear" else {}
        assert (A.affine_resample(xx, far, (3, 4, 5), mode=mode, fill=fill, **kw) == fill).all()
        bad = np.eye(4)
        bad[1, 2] = np.nan
        assert (A.affine_resample(xx, bad, (3, 4, 5), mode=mode, fill=fill, **kw) == fill).all()
    # half a voxel outside the volume the linear rule blends with the fill (grid-constant), one voxel outside it is the fill
    shift = np.eye(4)
    shift[2, 3] = -0.5
    got = A.affine_resample(x, shift, (4, 5, 6), mode="linear", fill=0.0)
    assert np.array_equal(got[:, :, 0], x[:, :, 0] / 2) and np.array_equal(got[:, :, 1], (x[:, :, 0] + x[:, :, 1]) / 2)


def test_entry_point_declared_bound_and_exported():
    from ctunet_amd import _lib, ops, resample
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctunet_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    decl = re.search(r"\bctu_affine_resample\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert decl and len(decl.group(1).split(",")) == 19
    assert "ctu_affine_resample" in _lib.SIGNATURES and len(_lib.SIGNATURES["ctu_affine_resample"][1]) == 19
    assert hasattr(lib, "ctu_affine_resample")
    assert callable(ops.affine_resample) and callable(resample.affine_resample)
    # adding an entry point changes no signature: the ABI version stays
    assert _lib.load().ctu_abi_version() == _lib.ABI_VERSION


def test_bad_arguments_fail_in_the_library_before_any_launch():
    from ctunet_amd import _lib
    L = _lib.load()
    fake = 4096                      # never dereferenced: every check below fails on the host first
    three = ctypes.c_double * 3

    def call(dtype=3, mode=0, k=0, n=1, src=(4, 5, 6), dst=(8, 5, 6), ptr=fake, sp=None, org=None, fill=0.0):
        return L.ctu_affine_resample(ptr, dtype, mode, k, n, *src, *dst, fake, sp, org, None, None, fill, fake, None)

    for kw, what in ((dict(mode=3), "mode"), (dict(mode=-1), "mode"), (dict(n=0), "shape"), (dict(src=(0, 5, 6)), "shape"),
                     (dict(dst=(8, 5, -1)), "shape"), (dict(src=(2048, 1024, 1024)), "shape"), (dict(dtype=4), "dtype"),
                     (dict(dtype=6), "dtype"), (dict(mode=1, dtype=4), "dtype"), (dict(mode=2, k=2, dtype=0), "dtype"),
                     (dict(mode=2, k=2, dtype=5), "dtype"), (dict(mode=2, k=1), "num_classes"), (dict(mode=2, k=17), "num_classes"),
                     (dict(ptr=None), "null"), (dict(sp=three(1.0, 0.0, 1.0)), "spacing"),
                     (dict(sp=three(1.0, float("nan"), 1.0)), "spacing"), (dict(org=three(0.0, float("inf"), 0.0)), "origin"),
                     (dict(fill=256.0), "fill"), (dict(fill=0.5), "fill"), (dict(dtype=5, fill=40000.0), "fill"),
                     (dict(mode=1, fill=float("nan")), "fill"), (dict(mode=1, fill=1e39), "fill"),
                     (dict(mode=2, k=3, fill=-1.0), "fill")):
        assert call(**kw) == -1, kw
        assert what in L.ctu_last_error().decode(), (kw, L.ctu_last_error())


def test_bad_arguments_raise_before_any_launch():
    from ctunet_amd import resample as rs
    x, m = torch.zeros(4, 5, 6), torch.eye(4, dtype=torch.float64)
    with pytest.raises(ValueError, match="affine_resample.*GPU"):
        rs.affine_resample(x, m, (4, 5, 6))
    with pytest.raises(ValueError, match="affine_resample.*mode"):
        rs.affine_resample(x, m, (4, 5, 6), mode="cubic")
    with pytest.raises(TypeError, match="affine_resample.*takes"):
        rs.affine_resample(x.to(torch.int64), m, (4, 5, 6), mode="nearest")
    with pytest.raises(TypeError, match="affine_resample.*takes"):
        rs.affine_resample(x, m, (4, 5, 6), mode="label_linear", num_classes=2)
    with pytest.raises(ValueError, match="affine_resample.*num_classes"):
        rs.affine_resample(x.to(torch.uint8), m, (4, 5, 6), mode="label_linear", num_classes=17)
    with pytest.raises(ValueError, match="affine_resample.*out_shape"):
        rs.affine_resample(x, m, (4, 0, 6))
    with pytest.raises(ValueError, match="affine_resample.*spacing"):
        rs.affine_resample(x, m, (4, 5, 6), spacing=(1.0, -1.0, 1.0))
    with pytest.raises(ValueError, match="affine_resample.*out_origin"):
        rs.affine_resample(x, m, (4, 5, 6), out_origin=(0.0, float("nan"), 0.0))
    with pytest.raises(ValueError, match="affine_resample.*fill"):
        rs.affine_resample(x, m, (4, 5, 6), fill=float("inf"))
    with pytest.raises(ValueError, match="affine_resample.*fill"):
        rs.affine_resample(x.to(torch.uint8), m, (4, 5, 6), mode="nearest", fill=300)
    with pytest.raises(ValueError, match="affine_resample.*out must"):
        rs.affine_resample(x, m, (4, 5, 6), out=torch.zeros(4, 5, 7))
