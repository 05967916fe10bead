"""Distance transform and ball morphology of ctunet_amd.postprocess without a GPU: the host references of distance_ref.py
pinned on scipy itself, argument validation (which must raise before anything is launched) and the C-ABI entry points in
the header, the ctypes table and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import distance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANISO = ((0.8, 0.45, 0.45), (1.0, 2.5, 0.7))


def test_ball_margin_is_the_gap_to_the_nearest_offset_norm():
    # unit spacing: the norms are sqrt(k); 1.5 lies between sqrt(2) and sqrt(3), nearest sqrt(2)
    assert R.ball_margin(1.5, None, 3) == pytest.approx((1.5 - np.sqrt(2.0)) / 1.5, rel=1e-12)
    assert R.ball_margin(2.5, None, 4) == pytest.approx((2.5 - np.sqrt(6.0)) / 2.5, rel=1e-12)
    assert R.ball_margin(3.0, None, 4) == 0.0 and R.ball_margin(1.0, 1.0, 1) == 0.0     # an offset on the sphere
    assert R.ball_margin(3.0, None, 1) == pytest.approx((3.0 - np.sqrt(3.0)) / 3.0)      # ... unless it is out of range
    # anisotropic: (3, 0, 0) * (1.0, 2.5, 0.7) has length 3 exactly; brute force over the offsets otherwise
    assert R.ball_margin(3.0, ANISO[1], 4) == 0.0
    for r, s, ext in ((2.0, ANISO[0], (3, 5, 5)), (3.2, ANISO[1], (4, 2, 5))):
        sv = np.asarray(s)
        gaps = [abs(np.sqrt(((np.array(o) * sv) ** 2).sum()) - r) / r
                for o in np.ndindex(*(e + 1 for e in ext))]
        assert R.ball_margin(r, s, ext) == pytest.approx(min(gaps), rel=1e-12)
    # the structure holds exactly the offsets shorter than the radius
    for r, s in ((1.0, None), (1.5, None), (2.5, None), (3.2, None), (2.0, ANISO[0]), (3.2, ANISO[1])):
        b = R.ball(r, s)
        c = [k // 2 for k in b.shape]
        assert all(k % 2 == 1 for k in b.shape) and b[tuple(c)]
        sv = R.triple(s)
        for o in np.ndindex(*b.shape):
            assert b[o] == (np.sqrt((((np.array(o) - c) * sv) ** 2).sum()) <= r)
        assert not b[0].all() or min(b.shape) == 1
    assert R.ball(1.0).sum() == 7 and np.array_equal(R.ball(1.0), ndi.generate_binary_structure(3, 1))
    assert np.array_equal(R.ball(1.5), ndi.generate_binary_structure(3, 2))


CASES = ((1.0, None), (1.5, None), (2.5, None), (3.2, None), (2.0, ANISO[0]), (1.5, ANISO[0]), (3.2, ANISO[1]))


def test_the_references_are_scipys_ball_morphology():
    """Distance thresholds equal scipy's binary morphology with the float64 ball and border_value=0; the zero padding is
    the virtual border."""
    shape = (11, 14, 17)
    masks = [R.blob(shape, 1), R.blob(shape, 2, 1.0), R.random_mask(shape, 0.9, 3), np.ones(shape, bool), np.zeros(shape, bool)]
    for r, s in CASES:
        assert R.ball_decidable(r, s, shape), (r, s)
        assert R.ball_margin(r, s, shape) >= 1e-4 or (r, s) == (1.0, None), (r, s)
        st = R.ball(r, s)
        for m in masks:
            assert np.array_equal(R.ball_erosion(m, r, s), ndi.binary_erosion(m, st, border_value=0)), (r, s)
            assert np.array_equal(R.ball_dilation(m, r, s), ndi.binary_dilation(m, st, border_value=0)), (r, s)
            assert np.array_equal(R.ball_opening(m, r, s), ndi.binary_opening(m, st)), (r, s)
            assert np.array_equal(R.ball_closing(m, r, s), ndi.binary_closing(m, st)), (r, s)
    # a mask touching the faces: the border erodes it, and without the padding it would not
    m = np.ones((6, 7, 8), bool)
    e = R.ball_erosion(m, 1.5)
    assert np.array_equal(e, ndi.binary_erosion(m, R.ball(1.5), border_value=0)) and e.sum() == 4 * 5 * 6
    assert ndi.binary_erosion(m, R.ball(1.5), border_value=1).all()


def test_signed_map_is_antisymmetric_under_complement():
    for s in (None,) + ANISO:
        for seed in (1, 2):
            m = R.blob((9, 12, 15), seed)
            sd = R.signed(m, s)
            assert np.array_equal(sd, -R.signed(~m, s))
            assert (sd[m] < 0).all() and (sd[~m] > 0).all()
            assert np.array_equal(sd[m], -R.edt(m, s)[m]) and np.array_equal(sd[~m], R.edt(~m, s)[~m])


def test_arguments_are_validated_before_any_launch():
    from ctunet_amd import postprocess as pp
    m = torch.zeros(4, 5, 6, dtype=torch.bool)
    balls = (pp.ball_erosion, pp.ball_dilation, pp.ball_opening, pp.ball_closing)
    bad_masks = (torch.zeros(5, 6, dtype=torch.bool), torch.zeros(1, 1, 4, 5, 6, dtype=torch.uint8),
                 torch.zeros(4, 5, 6, dtype=torch.float32), torch.zeros(4, 5, 6, dtype=torch.int32), "mask", None)
    for bad in bad_masks:
        for op in balls:
            with pytest.raises(ValueError, match="mask"):
                op(bad, 1.5)
        with pytest.raises(ValueError, match="mask"):
            pp.distance_transform_edt(bad)
        with pytest.raises(ValueError, match="mask"):
            pp.signed_distance(bad)
    with pytest.raises(ValueError, match="side"):
        pp.distance_transform_edt(torch.zeros(0, 4, 4, dtype=torch.bool))
    for fn in (pp.distance_transform_edt, pp.signed_distance, lambda t: pp.ball_opening(t, 2.0)):
        with pytest.raises(ValueError, match="1024"):
            fn(torch.zeros(1, 2, 1025, dtype=torch.uint8))
    for r in (0, 0.0, -1.5, float("inf"), float("nan"), True, "2", None, 1e30):
        for op in balls:
            with pytest.raises(ValueError, match="radius"):
                op(m, r)
        with pytest.raises(ValueError, match="opening_radius"):
            pp.extract_implant(m, m, opening_radius=r) if r is not None else pp.extract_implant(m, m, opening_radius="x")
    for s in (0, -1.0, (1.0, 2.0), (1.0, 0.0, 1.0), float("inf"), "1", [(1, 1, 1), (1, 1, 1)]):
        for fn in (lambda: pp.distance_transform_edt(m, sampling=s), lambda: pp.signed_distance(m, s),
                   lambda: pp.ball_dilation(m, 1.5, s), lambda: pp.extract_implant(m, m, opening_radius=1.5, sampling=s)):
            with pytest.raises(ValueError, match="sampling"):
                fn()
    for lab in (1.0, True, "1", 1 << 64):
        for fn in (lambda: pp.distance_transform_edt(m.long(), label=lab), lambda: pp.signed_distance(m.long(), label=lab),
                   lambda: pp.ball_erosion(m.long(), 1.5, label=lab)):
            with pytest.raises(ValueError, match="label"):
                fn()
    with pytest.raises(ValueError, match="return_distances"):
        pp.distance_transform_edt(m, return_distances=False)
    for flag in ("return_distances", "return_indices", "squared"):
        with pytest.raises(ValueError, match=flag):
            pp.distance_transform_edt(m, **{flag: "yes"})
    with pytest.raises(ValueError, match="not both"):
        pp.extract_implant(m, m, opening_iterations=2, opening_radius=1.5)
    with pytest.raises(ValueError, match="not both"):
        pp.extract_implant(m, m, opening_iterations=0, opening_radius=1.5)
    with pytest.raises(ValueError, match="sampling"):
        pp.extract_implant(m, m, sampling=(0.8, 0.45, 0.45))
    with pytest.raises(TypeError):
        pp.extract_implant(m, m, 1, 1, 3, 1, False, 1.5)          # the new arguments are keyword-only
    # valid arguments on host tensors: refused as host inputs, still before any launch
    for op in balls:
        with pytest.raises(ValueError, match="GPU"):
            op(m, 2.5, sampling=ANISO[0])
        with pytest.raises(ValueError, match="GPU"):
            op(m.long(), 1, label=2)
    with pytest.raises(ValueError, match="GPU"):
        pp.distance_transform_edt(m.to(torch.uint8), sampling=2.0, return_indices=True, squared=True)
    with pytest.raises(ValueError, match="GPU"):
        pp.signed_distance(torch.zeros(2, 4, 5, 6, dtype=torch.int64), sampling=[ANISO[0], ANISO[1]], label=3)
    with pytest.raises(ValueError, match="GPU"):
        pp.extract_implant(m, m.long(), opening_radius=1.5, sampling=ANISO[0], fill_holes=True)


ENTRIES = (("ctu_distance_ws_bytes", 6), ("ctu_distance_transform", 17))


def test_entry_points_declared_bound_exported_and_sized():
    from ctunet_amd import _lib, postprocess
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctunet_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name)
    L = _lib.load()
    assert L.ctu_abi_version() == _lib.ABI_VERSION == 8
    for fn in ("distance_transform_edt", "signed_distance", "ball_erosion", "ball_dilation", "ball_opening", "ball_closing",
               "distance_workspace_bytes"):
        assert callable(getattr(postprocess, fn))
    for kind in (0, 1, 2, 3):
        for bad in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, -1, 8), (1, 8, 8, 1025), (1, 1025, 2, 2), (65536, 1, 1, 1)):
            assert L.ctu_distance_ws_bytes(*bad, kind, 0) == 0, bad
        assert L.ctu_distance_ws_bytes(1, 1, 1, 1, kind, 1) > 0
    assert L.ctu_distance_ws_bytes(1, 8, 8, 8, 4, 0) == 0 and L.ctu_distance_ws_bytes(1, 8, 8, 8, -1, 0) == 0
    # distances are computed inside the result; the signed map and the ball need one 4-byte plane, indices 3 int16 planes
    for n, shape in ((1, (224, 512, 512)), (3, (17, 33, 65)), (2, (5, 7, 31))):
        v = n * shape[0] * shape[1] * shape[2]
        assert postprocess.distance_workspace_bytes(n, shape) == L.ctu_distance_ws_bytes(n, *shape, 0, 0) <= 256
        assert 6 * v <= postprocess.distance_workspace_bytes(n, shape, True) <= 6 * v + 3 * 256
        for kind in (2, 3):
            assert 4 * v <= L.ctu_distance_ws_bytes(n, *shape, kind, 0) <= 4 * v + 256


def test_bad_arguments_fail_before_any_launch():
    from ctunet_amd import _lib
    L = _lib.load()
    fake = 4096                      # never dereferenced: every check below fails on the host first

    def run(dtype=3, shape=(1, 8, 8, 8), border=0, spacing=None, kind=0, idx=None, r2=-1.0, src=fake):
        sp = None if spacing is None else (ctypes.c_float * len(spacing))(*spacing)
        return L.ctu_distance_transform(src, dtype, *shape, 0, 0, 0, border, sp, kind, fake, idx, r2, fake, None)

    for kw, what in ((dict(shape=(1, 0, 8, 8)), "shape"), (dict(shape=(65536, 1, 1, 1)), "shape"),
                     (dict(shape=(1, 1024, 1024, 2048)), "shape"), (dict(shape=(1, 2, 1025, 2)), "side"),
                     (dict(dtype=0), "dtype"), (dict(dtype=5), "dtype"), (dict(kind=4), "out_kind"), (dict(kind=-1), "out_kind"),
                     (dict(kind=2, idx=fake), "indices"), (dict(kind=3, idx=fake, r2=1.0), "indices"),
                     (dict(border=1, idx=fake), "indices"), (dict(kind=3, r2=-1.0), "ball_r2"),
                     (dict(kind=3, r2=float("inf")), "ball_r2"), (dict(spacing=(1.0, 0.0, 1.0)), "spacing"),
                     (dict(spacing=(1.0, float("inf"), 1.0)), "spacing"), (dict(src=None), "null")):
        assert run(**kw) == -1, kw
        assert what in L.ctu_last_error().decode(), (kw, L.ctu_last_error())
    with pytest.raises(_lib.CtuError, match="side"):
        _lib.check(run(shape=(1, 1025, 1, 1)), "distance_transform")
