"""Binary morphology of ctunet_amd.postprocess without a GPU: the definitions pinned on scipy itself, argument validation
(which must raise before anything is launched) and the C-ABI entry points in the header, the ctypes table and the built
library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blob(shape, seed, sigma=2.0):
    g = ndi.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), sigma)
    return g > np.median(g)


def _shift_read(x, s, border):
    """y[v] = x[v + s], `border` outside the volume."""
    p = np.pad(x, 1, constant_values=bool(border))
    d, h, w = x.shape
    return p[1 + s[0]:1 + s[0] + d, 1 + s[1]:1 + s[1] + h, 1 + s[2]:1 + s[2] + w]


def _rule(x, st, op, border):
    """The pinned rule over the offsets that the project's 27-bit code of `st` carries (what the kernels receive)."""
    from ctunet_amd import postprocess as pp
    code = pp._structure_code(st)
    offs = [(b // 9 - 1, b // 3 % 3 - 1, b % 3 - 1) for b in range(27) if code >> b & 1]
    assert len(offs) == int(np.count_nonzero(st))
    if op == "erosion":
        return np.logical_and.reduce([_shift_read(x, s, border) for s in offs])
    return np.logical_or.reduce([_shift_read(x, tuple(-c for c in s), border) for s in offs])


def test_the_pinned_definitions_are_scipys():
    """The module docstring's rules, applied to the offsets decoded from postprocess._structure_code, are scipy's."""
    rng = np.random.default_rng(11)
    x = _blob((9, 12, 14), 1, 1.5)
    structs = [ndi.generate_binary_structure(3, c) for c in (1, 2, 3)] + [rng.random((3, 3, 3)) < p for p in (0.2, 0.5)]
    for st in structs:
        assert st.any()
        for border in (0, 1):
            for k in (1, 2, 3):
                e, d = x, x
                for _ in range(k):
                    e, d = _rule(e, st, "erosion", border), _rule(d, st, "dilation", border)
                assert np.array_equal(e, ndi.binary_erosion(x, st, iterations=k, border_value=border))
                assert np.array_equal(d, ndi.binary_dilation(x, st, iterations=k, border_value=border))
        for k in (1, 2):
            o = c = x
            for _ in range(k):
                o, c = _rule(o, st, "erosion", 0), _rule(c, st, "dilation", 0)
            for _ in range(k):
                o, c = _rule(o, st, "dilation", 0), _rule(c, st, "erosion", 0)
            assert np.array_equal(o, ndi.binary_opening(x, st, iterations=k))
            assert np.array_equal(c, ndi.binary_closing(x, st, iterations=k))
    # fill holes: the background components that touch no face
    shell = np.zeros((9, 9, 9), bool)
    shell[2:7, 2:7, 2:7] = True
    shell[3:6, 3:6, 3:6] = False
    for conn in (1, 3):
        st = ndi.generate_binary_structure(3, conn)
        lab, n = ndi.label(~shell, st)
        faces = np.zeros_like(shell)
        for ax in range(3):
            idx = [slice(None)] * 3
            for side in (0, -1):
                idx[ax] = side
                faces[tuple(idx)] = True
        open_ = np.unique(lab[faces & ~shell])
        rule = shell | (~shell & ~np.isin(lab, open_))
        assert np.array_equal(rule, ndi.binary_fill_holes(shell, st)) and rule[4, 4, 4]


def test_structure_codes():
    from ctunet_amd import postprocess as pp
    for c in (1, 2, 3):
        st = ndi.generate_binary_structure(3, c)
        want = sum(1 << i for i, b in enumerate(st.ravel()) if b)
        assert pp._structure_code(c) == want == pp._structure_code(st) == pp._structure_code(torch.from_numpy(st))
    assert bin(pp._structure_code(1)).count("1") == 7 and bin(pp._structure_code(2)).count("1") == 19
    assert pp._structure_code(3) == (1 << 27) - 1
    one = np.zeros((3, 3, 3), bool)
    one[0, 1, 2] = True
    assert pp._structure_code(one) == 1 << 5


def test_arguments_are_validated_before_any_launch():
    from ctunet_amd import postprocess as pp
    m = torch.zeros(4, 5, 6, dtype=torch.bool)
    ops = (pp.binary_erosion, pp.binary_dilation, pp.binary_opening, pp.binary_closing)
    bad_masks = (torch.zeros(5, 6, dtype=torch.bool), torch.zeros(1, 1, 4, 5, 6, dtype=torch.uint8),
                 torch.zeros(4, 5, 6, dtype=torch.float32), torch.zeros(4, 5, 6, dtype=torch.int32), "mask", None)
    for bad in bad_masks:
        for op in ops + (pp.binary_fill_holes,):
            with pytest.raises(ValueError):
                op(bad)
        with pytest.raises(ValueError):
            pp.extract_implant(bad, m)
        with pytest.raises(ValueError):
            pp.extract_implant(m, bad)
    with pytest.raises(ValueError, match="side"):
        pp.binary_erosion(torch.zeros(0, 4, 4, dtype=torch.bool))
    bad_structs = (0, 4, -1, True, 1.5, "1", None, np.ones((3, 3), bool), np.ones((3, 3, 5), bool),
                   torch.ones(27, dtype=torch.bool), np.zeros((3, 3, 3), bool), torch.zeros(3, 3, 3, dtype=torch.bool))
    for st in bad_structs:
        for op in ops:
            with pytest.raises(ValueError, match="structure"):
                op(m, structure=st)
        with pytest.raises(ValueError, match="structure"):
            pp.extract_implant(m, m, structure=st)
    for it in (0, -1, pp.MAX_ITERATIONS + 1, True, 2.0, None, "2"):
        for op in ops:
            with pytest.raises(ValueError, match="iterations"):
                op(m, iterations=it)
    assert pp.MAX_ITERATIONS == 64
    for it in (-1, pp.MAX_ITERATIONS + 1, True, 1.0, None):
        with pytest.raises(ValueError, match="opening_iterations"):
            pp.extract_implant(m, m, opening_iterations=it)
    for bv in (2, -1, 0.5, "0", None):
        with pytest.raises(ValueError, match="border_value"):
            pp.binary_erosion(m, border_value=bv)
        with pytest.raises(ValueError, match="border_value"):
            pp.binary_dilation(m, border_value=bv)
    for lab in (1.0, True, "1", 1 << 64):
        with pytest.raises(ValueError, match="label"):
            pp.binary_erosion(m.to(torch.uint8), label=lab)
        with pytest.raises(ValueError, match="label"):
            pp.binary_fill_holes(m.to(torch.uint8), label=lab)
    for c in (0, 4, True, 1.0, None):
        with pytest.raises(ValueError, match="connectivity"):
            pp.binary_fill_holes(m, connectivity=c)
        with pytest.raises(ValueError, match="connectivity"):
            pp.extract_implant(m, m, connectivity=c)
    for k in (0, 9, True, 2.0, None):
        with pytest.raises(ValueError, match="num_components"):
            pp.extract_implant(m, m, num_components=k)
    with pytest.raises(ValueError, match="same shape"):
        pp.extract_implant(m, torch.zeros(4, 5, 7, dtype=torch.bool))
    with pytest.raises(ValueError, match="same shape"):
        pp.extract_implant(m, torch.zeros(1, 4, 5, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="iterations"):
        pp.morphology_workspace_bytes(1, (8, 8, 8), 0)
    # valid arguments on host tensors: refused as host inputs, still before any launch
    st = np.random.default_rng(0).random((3, 3, 3)) < 0.5
    for op in ops:
        with pytest.raises(ValueError, match="GPU"):
            op(m, structure=st, iterations=64)
        with pytest.raises(ValueError, match="GPU"):
            op(m.long(), structure=2, iterations=3, label=2)
    with pytest.raises(ValueError, match="GPU"):
        pp.binary_erosion(m.to(torch.uint8), border_value=1)
    with pytest.raises(ValueError, match="GPU"):
        pp.binary_fill_holes(m, connectivity=3, label=1)
    with pytest.raises(ValueError, match="GPU"):
        pp.extract_implant(m.long(), m.to(torch.uint8), opening_iterations=0, structure=3, connectivity=1,
                           num_components=2, fill_holes=True)


ENTRIES = (("ctu_morphology_ws_bytes", 5), ("ctu_binary_morphology", 15), ("ctu_fill_holes", 12), ("ctu_implant_mask", 16))


def test_entry_points_declared_bound_exported_and_sized():
    from ctunet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctunet_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 8 and _lib.load().ctu_abi_version() == 8
    from ctunet_amd import postprocess
    for fn in ("binary_erosion", "binary_dilation", "binary_opening", "binary_closing", "binary_fill_holes",
               "extract_implant", "morphology_workspace_bytes"):
        assert callable(getattr(postprocess, fn))
    L = _lib.load()
    for kind in (0, 1, 2):
        for bad in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, -1, 8), (1, 8, 8, 0), (1, 1024, 1024, 2048), (65536, 1, 1, 1)):
            assert L.ctu_morphology_ws_bytes(*bad, kind) == 0, bad
        assert L.ctu_morphology_ws_bytes(1, 1, 1, 1, kind) > 0
    assert L.ctu_morphology_ws_bytes(1, 8, 8, 8, 3) == 0 and L.ctu_morphology_ws_bytes(1, 8, 8, 8, -1) == 0
    # two bit images: a quarter byte per voxel plus the padding of rows to 64 voxels and of each image to 256 bytes
    for n, shape in ((1, (224, 512, 512)), (1, (224, 304, 304)), (3, (17, 33, 65)), (2, (5, 7, 31)), (1, (1, 1, 1))):
        d, h, w = shape
        image = n * d * h * ((w + 63) // 64) * 8
        for it in (1, 64):
            ws = postprocess.morphology_workspace_bytes(n, shape, it)
            assert 2 * image <= ws <= 2 * image + 512
        assert ws == L.ctu_morphology_ws_bytes(n, *shape, 0)
    v = 224 * 512 * 512
    assert postprocess.morphology_workspace_bytes(1, (224, 512, 512), 2) == v // 4
    fill = L.ctu_morphology_ws_bytes(1, 224, 512, 512, 1)
    assert postprocess.workspace_bytes(1, (224, 512, 512)) + v <= fill <= postprocess.workspace_bytes(1, (224, 512, 512)) + v + 512
    assert L.ctu_morphology_ws_bytes(1, 224, 512, 512, 2) == v // 4 + fill


def test_bad_arguments_fail_before_any_launch():
    from ctunet_amd import _lib
    L = _lib.load()
    fake = 4096                      # never dereferenced: every check below fails on the host first
    six = 0b000010000_010111010_000010000

    def morph(dtype=3, shape=(1, 8, 8, 8), mode=0, st=six, it=1, border=0):
        return L.ctu_binary_morphology(fake, dtype, *shape, mode, st, it, border, 0, 0, fake, fake, None)

    for kw, what in ((dict(shape=(1, 0, 8, 8)), "shape"), (dict(shape=(1, 1024, 1024, 2048)), "shape"),
                     (dict(shape=(65536, 1, 1, 1)), "shape"), (dict(dtype=5), "dtype"), (dict(dtype=0), "dtype"),
                     (dict(mode=4), "mode"), (dict(mode=-1), "mode"), (dict(st=0), "structure"),
                     (dict(st=1 << 27), "structure"), (dict(it=0), "iterations"), (dict(it=-1), "iterations"),
                     (dict(it=65), "iterations"), (dict(border=2), "border"), (dict(border=-1), "border")):
        assert morph(**kw) == -1, kw
        assert what in L.ctu_last_error().decode(), (kw, L.ctu_last_error())
    assert L.ctu_binary_morphology(None, 3, 1, 8, 8, 8, 0, six, 1, 0, 0, 0, fake, fake, None) == -1
    assert "null" in L.ctu_last_error().decode()

    def fill(dtype=3, shape=(1, 8, 8, 8), conn=1):
        return L.ctu_fill_holes(fake, dtype, *shape, conn, 0, 0, fake, fake, None)

    for kw, what in ((dict(shape=(1, 8, 0, 8)), "shape"), (dict(dtype=2), "dtype"), (dict(conn=0), "connectivity"),
                     (dict(conn=4), "connectivity")):
        assert fill(**kw) == -1, kw
        assert what in L.ctu_last_error().decode(), kw

    def implant(da=3, db=4, shape=(1, 8, 8, 8), st=six, it=1, fh=0, conn=3, k=1):
        return L.ctu_implant_mask(fake, da, fake, db, *shape, st, it, fh, conn, k, fake, fake, None)

    for kw, what in ((dict(shape=(1, 8, 8, -2)), "shape"), (dict(da=1), "dtype"), (dict(db=7), "dtype"),
                     (dict(st=0), "structure"), (dict(it=-1), "iterations"), (dict(it=65), "iterations"),
                     (dict(conn=4), "connectivity"), (dict(k=0), "num_components"), (dict(k=9), "num_components")):
        assert implant(**kw) == -1, kw
        assert what in L.ctu_last_error().decode(), kw
    with pytest.raises(_lib.CtuError, match="iterations"):
        _lib.check(morph(it=100), "binary_morphology")
