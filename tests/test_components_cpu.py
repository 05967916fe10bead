"""ctunet_amd.postprocess without a GPU: the numbering rule pinned on scipy itself, argument validation (which must raise
before anything is launched) and the new C-ABI entry points in the header, the ctypes table and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rule_numbering(mask, connectivity):
    """scipy's components renumbered by the pinned rule: 1 + the C-order rank of each component's first voxel."""
    lab, n = ndi.label(mask, ndi.generate_binary_structure(3, connectivity))
    flat = lab.ravel()
    first = np.full(n + 1, flat.size, dtype=np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    order = np.argsort(first[1:], kind="stable")
    num = np.zeros(n + 1, dtype=np.int64)
    num[1 + order] = np.arange(1, n + 1)
    return lab, n, num[lab]


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_scipy_numbers_components_by_their_first_voxel_in_c_order(connectivity):
    rng = np.random.default_rng(connectivity)
    masks = [rng.random((9, 11, 13)) < d for d in (0.05, 0.3, 0.5, 0.7)]
    chk = (np.indices((6, 6, 6)).sum(0) % 2).astype(bool)
    masks += [chk, np.zeros((4, 5, 6), bool), np.ones((4, 5, 6), bool), rng.random((1, 1, 300)) < 0.5,
              rng.random((300, 1, 1)) < 0.5]
    for m in masks:
        lab, n, rule = _rule_numbering(m, connectivity)
        assert lab.dtype == np.int32
        assert np.array_equal(lab, rule)
        assert n == lab.max()
    # the checkerboard: all singletons at rank 1, one component at rank 3
    assert ndi.label(chk, ndi.generate_binary_structure(3, 1))[1] == int(chk.sum())
    assert ndi.label(chk, ndi.generate_binary_structure(3, 3))[1] == 1


def test_arguments_are_validated_before_any_launch():
    from ctunet_amd import postprocess as pp
    m = torch.zeros(4, 5, 6, dtype=torch.bool)
    lab = torch.zeros(2, 4, 5, 6, dtype=torch.uint8)
    # dims and dtypes
    for bad in (torch.zeros(5, 6, dtype=torch.bool), torch.zeros(1, 1, 4, 5, 6, dtype=torch.bool),
                torch.zeros(4, 5, 6, dtype=torch.float32), torch.zeros(4, 5, 6, dtype=torch.int64), "mask"):
        with pytest.raises(ValueError):
            pp.label(bad)
    for bad in (torch.zeros(5, 6, dtype=torch.uint8), torch.zeros(4, 5, 6, dtype=torch.int32),
                torch.zeros(4, 5, 6, dtype=torch.bool), torch.zeros(4, 5, 6)):
        with pytest.raises(ValueError):
            pp.keep_largest_connected_component(bad)
        with pytest.raises(ValueError):
            pp.remove_small_objects(bad, 5)
    with pytest.raises(ValueError, match="side"):
        pp.label(torch.zeros(0, 4, 4, dtype=torch.bool))
    # connectivity
    for c in (0, 4, -1, 1.0, True, "3", None):
        with pytest.raises(ValueError, match="connectivity"):
            pp.label(m, connectivity=c)
        with pytest.raises(ValueError, match="connectivity"):
            pp.keep_largest_connected_component(lab, connectivity=c)
        with pytest.raises(ValueError, match="connectivity"):
            pp.remove_small_objects(lab, 3, connectivity=c)
    # min_size and num_components
    for s in (-1, 2.5, 3.0, True, None, "4"):
        with pytest.raises(ValueError, match="min_size"):
            pp.remove_small_objects(lab, s)
    for k in (0, 9, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="num_components"):
            pp.keep_largest_connected_component(lab, num_components=k)
    # applied labels: 1 to 16 distinct nonzero values of the map's dtype
    for al in ([], [0], [1, 1], list(range(1, 18)), [256], [-1], [1.5], [True]):
        with pytest.raises(ValueError, match="applied_labels"):
            pp.keep_largest_connected_component(lab, applied_labels=al)
        with pytest.raises(ValueError, match="applied_labels"):
            pp.remove_small_objects(lab, 2, applied_labels=al)
    with pytest.raises(ValueError, match="applied_labels"):
        pp.remove_small_objects(lab.long(), 2, applied_labels=[3, 0])
    # valid arguments on the CPU: refused as CPU inputs (no fallback), still before any launch
    with pytest.raises(ValueError, match="GPU"):
        pp.label(m, connectivity=1)
    with pytest.raises(ValueError, match="GPU"):
        pp.label(lab)
    with pytest.raises(ValueError, match="GPU"):
        pp.keep_largest_connected_component(lab, applied_labels=[1, 2], num_components=8)
    with pytest.raises(ValueError, match="GPU"):
        pp.keep_largest_connected_component(lab.long(), applied_labels=[1 << 40], connectivity=2)
    with pytest.raises(ValueError, match="GPU"):
        pp.remove_small_objects(lab.long(), 0, applied_labels=16)
    with pytest.raises(ValueError, match="GPU"):
        pp.remove_small_objects(lab, 1 << 40)


def test_entry_points_declared_bound_exported_and_sized():
    from ctunet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctunet_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("ctu_components_ws_bytes", 4), ("ctu_label_components", 13), ("ctu_filter_components", 14)):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 8 and _lib.load().ctu_abi_version() == 8
    import ctunet_amd
    assert "postprocess" in ctunet_amd.__all__
    from ctunet_amd import postprocess
    for fn in ("label", "keep_largest_connected_component", "remove_small_objects"):
        assert callable(getattr(postprocess, fn))
    # workspace: about 8 bytes per voxel (parent + size) plus per-tile tables
    v = 224 * 512 * 512
    ws = postprocess.workspace_bytes(1, (224, 512, 512))
    assert 8 * v <= ws <= 9 * v
    assert postprocess.workspace_bytes(3, (17, 33, 65)) >= 3 * 8 * 17 * 33 * 65
    L = _lib.load()
    for bad in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, -1, 8), (1, 8, 8, 0), (1, 1024, 1024, 2048), (65536, 1, 1, 1)):
        assert L.ctu_components_ws_bytes(*bad) == 0, bad
    assert L.ctu_components_ws_bytes(1, 1, 1, 1) > 0


def test_bad_geometry_fails_before_any_launch():
    from ctunet_amd import _lib
    L = _lib.load()
    fake = 4096                      # never dereferenced: every check below fails on the host first
    cases = [((fake, 3, 1, 0, 8, 8, 3, None, 0, None, fake, fake, None), "shape"),
             ((fake, 3, 1, 1024, 1024, 2048, 3, None, 0, None, fake, fake, None), "shape"),
             ((fake, 3, 1, 8, 8, 8, 4, None, 0, None, fake, fake, None), "connectivity"),
             ((fake, 5, 1, 8, 8, 8, 3, None, 0, None, fake, fake, None), "dtype"),
             ((fake, 3, 1, 8, 8, 8, 3, None, 17, None, fake, fake, None), "applied")]
    for args, what in cases:
        assert L.ctu_label_components(*args) == -1
        assert what in L.ctu_last_error().decode()
    assert L.ctu_filter_components(fake, 4, 1, 8, 8, 8, 3, None, 0, 0, 9, fake, fake, None) == -1
    assert "largest" in L.ctu_last_error().decode()
    assert L.ctu_filter_components(fake, 4, 1, 8, 8, 8, 3, None, 0, 1, -1, fake, fake, None) == -1
    assert "min_size" in L.ctu_last_error().decode()
    with pytest.raises(_lib.CtuError, match="shape"):
        _lib.check(L.ctu_filter_components(fake, 4, 2, 8, 0, 8, 3, None, 0, 1, 3, fake, fake, None), "filter_components")
