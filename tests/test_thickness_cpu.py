"""Local thickness of ctunet_amd.postprocess without a GPU: the numpy reference of thickness_ref.py on cases with a known
answer, the host-side entry points, and argument validation (which must raise before anything is launched)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import distance_ref as DR
import thickness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANISO = ((0.8, 0.45, 0.45), (1.0, 2.5, 0.7))


@pytest.mark.parametrize("k, want", ((1, 2.0), (2, 2.0), (3, 4.0), (4, 4.0), (5, 6.0)))
def test_reference_plates_read_two_ceil_half_k(k, want):
    """The voxel-centre convention: a plate of k voxels between two background layers reads 2 ceil(k / 2) everywhere."""
    m = np.zeros((k + 4, 9, 9), bool)
    m[2:2 + k] = True
    t = R.local_thickness(R.squared_edt(m))
    assert t.dtype == np.float32 and t.shape == m.shape
    assert (t[m] == np.float32(want)).all() and (t[~m] == 0).all()


def test_reference_ball_reads_its_diameter_at_the_centre():
    g = np.arange(17) - 8
    dd = g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2
    # the ball whose nearest background centre lies at distance 6, (6, 0, 0): 12 at the centre and nowhere more
    m = dd < 36
    d2 = R.squared_edt(m)
    assert d2[8, 8, 8] == 36
    t = R.local_thickness(d2)
    assert t[8, 8, 8] == 12 and t.max() == 12 and (t[~m] == 0).all() and (t[m] >= 2).all()
    # with the voxels at dd = 36 inside, the nearest background centre is (6, 1, 0) at dd = 37 and the pinned rule
    # (D2 of the centre, open ball) reads 2 sqrt(37) = 12.17 there: 12 plus the 0 to 1 voxel of the convention
    m = dd <= 36
    d2 = R.squared_edt(m)
    assert d2[8, 8, 8] == 37
    t = R.local_thickness(d2)
    assert t[8, 8, 8] == t.max() == np.float32(2) * np.sqrt(np.float32(37)) and 12 <= t.max() < 13
    assert (t[~m] == 0).all() and (t[m] >= 2).all()


def test_reference_dominates_the_voxels_own_ball_and_handles_the_edge_cases():
    m = DR.blob((12, 14, 16), 5)
    d2 = R.squared_edt(m)
    t = R.local_thickness(d2)
    assert (t >= np.float32(2) * np.sqrt(d2.astype(np.float32))).all()
    assert (t[~m] == 0).all() and (t[m] >= 2).all()
    # the same rule in float32 with sampling 1 gives the same map; a scaled grid scales the map
    f = R.local_thickness(d2.astype(np.float32), (1.0, 1.0, 1.0))
    assert np.array_equal(f, t)
    f2 = R.local_thickness((d2 * 4).astype(np.float32), (2.0, 2.0, 2.0))
    assert np.array_equal(f2, t * 2)
    # no background: +inf; no foreground: 0
    full = np.full((3, 4, 5), R.INT32_MAX, np.int64)
    assert np.isinf(R.local_thickness(full)).all()
    assert np.isinf(R.local_thickness(np.full((3, 4, 5), np.inf, np.float32), ANISO[0])).all()
    assert (R.local_thickness(np.zeros((3, 4, 5), np.int64)) == 0).all()
    # summary rows
    s = R.summary(t, 4.0)
    assert s[0] == m.sum() and s[1] == t[m].min() and s[2] == t.max() and s[4] == (t[m] < 4).sum()
    e = R.summary(np.zeros((2, 2, 2), np.float32), 1.0)
    assert e[0] == 0 and e[1] == np.inf and e[2] == 0 and np.isnan(e[3]) and e[4] == 0


ENTRIES = (("ctu_thickness_ws_bytes", 5), ("ctu_local_thickness", 10), ("ctu_thickness_summary_ws_bytes", 2),
           ("ctu_thickness_summary", 7))


def test_entry_points_declared_bound_exported_and_sized():
    from ctunet_amd import _lib, postprocess
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctunet_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name)
    L = _lib.load()
    for fn in ("local_thickness", "thickness_summary", "thickness_workspace_bytes"):
        assert callable(getattr(postprocess, fn))
    for flt in (0, 1):
        for bad in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, -1, 8), (1, 8, 8, 1025), (1, 1025, 2, 2), (65536, 1, 1, 1),
                    (1, 1024, 1024, 2048)):
            assert L.ctu_thickness_ws_bytes(*bad, flt) == 0, bad
        assert L.ctu_thickness_ws_bytes(1, 1, 1, 1, flt) > 0
        # monotone in every argument, and at least the 4 bytes per voxel of the candidate map
        prev = 0
        for n, shape in ((1, (1, 1, 1)), (1, (8, 8, 8)), (1, (9, 8, 8)), (1, (17, 33, 65)), (2, (17, 33, 65)),
                         (2, (20, 33, 70)), (3, (224, 512, 512))):
            b = L.ctu_thickness_ws_bytes(n, *shape, flt)
            v = n * shape[0] * shape[1] * shape[2]
            assert b > prev and 4 * v <= b <= 4 * v + 4 * v // 64 + 4 * n + 4096
            prev = b
    assert L.ctu_thickness_ws_bytes(1, 8, 8, 8, 2) == 0 and L.ctu_thickness_ws_bytes(1, 8, 8, 8, -1) == 0
    for bad in ((0, 10), (65536, 10), (1, 0), (1, -5)):
        assert L.ctu_thickness_summary_ws_bytes(*bad) == 0
    assert 0 < L.ctu_thickness_summary_ws_bytes(1, 1) <= L.ctu_thickness_summary_ws_bytes(1, 1 << 30) \
        <= L.ctu_thickness_summary_ws_bytes(3, 1 << 30)
    n, shape = 2, (20, 24, 70)
    v = n * 20 * 24 * 70
    for s in (None, ANISO[0]):
        assert postprocess.thickness_workspace_bytes(n, shape, s) == L.ctu_thickness_ws_bytes(n, *shape, int(s is not None)) \
            + 4 * v + L.ctu_distance_ws_bytes(n, *shape, 1, 0)
    with pytest.raises(ValueError, match="1024"):
        postprocess.thickness_workspace_bytes(1, (2, 2, 1025))


def test_bad_arguments_fail_before_any_launch():
    from ctunet_amd import _lib
    L = _lib.load()
    fake = 4096                      # never dereferenced: every check below fails on the host first

    def run(is_float=0, shape=(1, 8, 8, 8), spacing=None, src=fake):
        sp = None if spacing is None else (ctypes.c_float * len(spacing))(*spacing)
        return L.ctu_local_thickness(src, is_float, *shape, sp, fake, fake, None)

    for kw, what in ((dict(shape=(1, 0, 8, 8)), "shape"), (dict(shape=(65536, 1, 1, 1)), "shape"),
                     (dict(shape=(1, 1024, 1024, 2048)), "shape"), (dict(shape=(1, 2, 1025, 2)), "side"),
                     (dict(is_float=2), "is_float"), (dict(is_float=1, spacing=(1.0, 0.0, 1.0)), "spacing"),
                     (dict(is_float=1, spacing=(1.0, float("inf"), 1.0)), "spacing"),
                     (dict(is_float=1, spacing=(1.0, float("nan"), 1.0)), "spacing"),
                     (dict(is_float=0, spacing=(0.8, 0.45, 0.45)), "unit spacing"), (dict(src=None), "null")):
        assert run(**kw) == -1, kw
        assert what in L.ctu_last_error().decode(), (kw, L.ctu_last_error())
    for args, what in (((None, 1, 8, 0.0, fake, fake, None), "null"), ((fake, 0, 8, 0.0, fake, fake, None), "shape"),
                       ((fake, 1, 0, 0.0, fake, fake, None), "shape"), ((fake, 1, 8, -1.0, fake, fake, None), "min_thickness"),
                       ((fake, 1, 8, float("nan"), fake, fake, None), "min_thickness")):
        assert L.ctu_thickness_summary(*args) == -1, args
        assert what in L.ctu_last_error().decode(), (args, L.ctu_last_error())


def test_arguments_are_validated_before_any_launch():
    from ctunet_amd import postprocess as pp
    m = torch.zeros(4, 5, 6, dtype=torch.bool)
    t = torch.zeros(4, 5, 6, dtype=torch.float32)
    for bad in (torch.zeros(5, 6, dtype=torch.bool), torch.zeros(1, 1, 4, 5, 6, dtype=torch.uint8),
                torch.zeros(4, 5, 6, dtype=torch.float32), torch.zeros(4, 5, 6, dtype=torch.int32), "mask", None):
        with pytest.raises(ValueError, match="mask"):
            pp.local_thickness(bad)
    with pytest.raises(ValueError, match="side"):
        pp.local_thickness(torch.zeros(0, 4, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="1024"):
        pp.local_thickness(torch.zeros(1, 2, 1025, dtype=torch.uint8))
    for s in (0, -1.0, (1.0, 2.0), (1.0, 0.0, 1.0), float("inf"), "1", [(1, 1, 1), (1, 1, 1)]):
        with pytest.raises(ValueError, match="sampling"):
            pp.local_thickness(m, sampling=s)
        with pytest.raises(ValueError, match="sampling"):
            pp.thickness_workspace_bytes(1, (4, 5, 6), s)
    for lab in (1.0, True, "1", 1 << 64):
        with pytest.raises(ValueError, match="label"):
            pp.local_thickness(m.long(), label=lab)
    for bad in (torch.zeros(5, 6), torch.zeros(4, 5, 6, dtype=torch.float64), torch.zeros(4, 5, 6, dtype=torch.int32), m, None):
        with pytest.raises(ValueError, match="thickness"):
            pp.thickness_summary(bad)
    for mt in ("2", True, -0.5, float("nan"), [2.0], 1j):
        with pytest.raises(ValueError, match="min_thickness"):
            pp.thickness_summary(t, mt)
    # valid arguments on host tensors: refused as host inputs, in the module's words, still before any launch
    for call in (lambda: pp.local_thickness(m), lambda: pp.local_thickness(m.to(torch.uint8), sampling=ANISO[0]),
                 lambda: pp.local_thickness(torch.zeros(2, 4, 5, 6, dtype=torch.int64), sampling=[ANISO[0], ANISO[1]], label=2),
                 lambda: pp.thickness_summary(t), lambda: pp.thickness_summary(t, 2.0),
                 lambda: pp.thickness_summary(torch.zeros(2, 4, 5, 6), float("inf"))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == pp._ON_GPU
