"""Random patch sampling without a GPU: the three entry points in the header, the ctypes table and the library; the argument
refusals of ctunet_amd.sampling, raised before any device call; and the properties of the NumPy restatement
(tests/patch_sample_ref.py) that the GPU tests compare the kernels with."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import patch_sample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, DRAWS = 1234, 4096


def test_symbols_header_and_abi():
    import ctunet_amd
    from ctunet_amd import _lib, sampling
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctunet_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("ctu_patch_index", 7), ("ctu_patch_draw", 18), ("ctu_patch_crop", 18)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name), name
    for macro, value in (("CTU_PATCH_CHUNK", sampling.CHUNK), ("CTU_PATCH_MAX_CLASSES", sampling.MAX_CLASSES),
                         ("CTU_PATCH_RECORD", sampling.RECORD)):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value
    assert sampling.CHUNK == R.CHUNK == 8192
    assert _lib.ABI_VERSION == 8 and _lib.load().ctu_abi_version() == 8
    assert "sampling" in ctunet_amd.__all__ and ctunet_amd.sampling is sampling
    assert "FlapRecPatchDataset" in ctunet_amd.__all__


def test_sampler_refusals():
    from ctunet_amd.sampling import PatchIndex, PatchSampler
    with pytest.raises(ValueError, match="above 1"):
        PatchSampler((8, 8, 8), classes=(1, 2), class_p=(0.6, 0.5))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        PatchSampler((8, 8, 8), class_p=1.025)
    with pytest.raises(ValueError, match="classes"):
        PatchSampler((8, 8, 8), classes=(1, 2, 3, 4, 5), class_p=(0.1,) * 5)
    with pytest.raises(ValueError, match="0..255"):
        PatchSampler((8, 8, 8), classes=(256,), class_p=(0.5,))
    with pytest.raises(ValueError, match="per class"):
        PatchSampler((8, 8, 8), classes=(1, 2), class_p=0.5)
    for patch, jitter in (((8, 12, 20), 4), ((8, 12, 20), (3, 6, 9)), ((7, 7, 7), (0, 0, 4)), ((8, 8, 8), -1)):
        with pytest.raises(ValueError, match="jitter"):
            PatchSampler(patch, jitter=jitter)
    PatchSampler((8, 12, 20), jitter=(3, 5, 9))                       # (p - 1) // 2 itself is allowed
    with pytest.raises(TypeError, match="patch"):
        PatchSampler((8, 8))
    s = PatchSampler((4, 4, 4), seed=3)
    assert s.state_dict() == {"seed": 3, "counter": 0}
    for bad in (torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 4, dtype=torch.int16), torch.zeros(1, 4, 4, 4, dtype=torch.int64)):
        with pytest.raises(TypeError, match="uint8"):
            s.index(bad)
    with pytest.raises(ValueError, match=r"\[M, D, H, W\]"):
        s.index(torch.zeros(4, 4, 4, dtype=torch.uint8))
    # host items are checked against [0, M) before anything touches a device
    idx = PatchIndex(torch.zeros(3, 1, 1, dtype=torch.int32), torch.zeros(3, 4, 4, 4, dtype=torch.uint8), (3, 4, 4, 4), None)
    for items in ([0, 3], [-1], torch.tensor([1, 5])):
        with pytest.raises(ValueError, match=r"\[0, 3\)"):
            s.draw(idx, items=items)
    with pytest.raises(ValueError, match="classes"):
        PatchSampler((4, 4, 4), classes=(1,), class_p=(0.5,)).draw(idx)
    with pytest.raises(ValueError, match="out must be"):
        s.draw(idx, items=[0, 1], coords=torch.zeros(2, 3, dtype=torch.int32))
    assert s.state_dict()["counter"] == 0


def test_crop_refusals():
    from ctunet_amd.sampling import crop
    src = torch.zeros(2, 1, 6, 6, 6, dtype=torch.uint8)
    co = torch.zeros(3, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="out must be"):
        crop(src, co, (4, 4, 4), out=torch.zeros(3, 1, 4, 4, 5, dtype=torch.uint8))            # wrong shape
    with pytest.raises(ValueError, match="out must be"):
        crop(src, co, (4, 4, 4), out=torch.zeros(3, 1, 4, 4, 4))                               # wrong dtype
    with pytest.raises(ValueError, match="out must be"):
        crop(src, co, (4, 4, 4), dtype=torch.float32, out=torch.zeros(3, 1, 4, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="channels"):
        crop(src, co, (4, 4, 4), out=torch.zeros(3, 1, 4, 4, 4, dtype=torch.uint8), out_channel=1)
    with pytest.raises(TypeError, match="dtype"):
        crop(src, co, (4, 4, 4), dtype=torch.int16)
    with pytest.raises(TypeError, match="uint8, int16 or float32"):
        crop(src.double(), co, (4, 4, 4))
    with pytest.raises(ValueError, match="coords"):
        crop(src, co[:, :3], (4, 4, 4))
    with pytest.raises(ValueError, match="fill"):
        crop(src, co, (4, 4, 4), fill=256)
    with pytest.raises(ValueError, match="fill"):
        crop(src, co, (4, 4, 4), fill=0.5)
    with pytest.raises(ValueError, match="MI355X"):                   # everything else in order: no CPU fallback
        crop(src, co, (4, 4, 4), fill=7)


def _words():
    return [R.words(SEED, seq) for seq in range(DRAWS)]


def test_restatement_class_shares():
    """class_p = (0.25, 0.5): shares 0.25 / 0.5 / 0.25 (uniform), each within 0.035 (>= 3.8 sigma of 4096 draws)."""
    cum = R.cumulative((0.25, 0.5))
    assert cum == [0.25, 0.75]
    got = np.bincount([R.choose_class(w[0], cum) + 1 for w in _words()], minlength=3) / DRAWS       # uniform, 0, 1
    print("shares (class 0, class 1, uniform):", got[1], got[2], got[0])
    assert abs(got[1] - 0.25) <= 0.035 and abs(got[2] - 0.5) <= 0.035 and abs(got[0] - 0.25) <= 0.035


def test_restatement_k_deciles():
    ks = np.array([R.draw_int(w[1], 0, 1000) for w in _words()])
    assert ks.min() >= 0 and ks.max() < 1000
    dec = np.bincount(ks // 100, minlength=10) / DRAWS
    print("deciles of k:", dec.min(), dec.max())
    assert dec.min() >= 0.08 and dec.max() <= 0.12


def test_restatement_uniform_starts():
    """hi = 11: each of the 12 starts has a share in [0.068, 0.098] (1/12 = 0.083)."""
    for axis in range(3):
        s = np.array([R.start_of(31, 20, w[2 + axis]) for w in _words()])
        share = np.bincount(s, minlength=12) / DRAWS
        print("uniform starts, axis", axis, share.min(), share.max())
        assert len(share) == 12 and share.min() >= 0.068 and share.max() <= 0.098
    assert R.start_of(5, 9, 0xFFFFFFFF) == 0                          # a patch larger than the volume starts at 0


def test_restatement_centre_stays_inside():
    """For every n, p < 30, centre c < n and jitter |j| <= (p - 1) // 2, the clamped start keeps c inside [s, s + p)."""
    checked = 0
    for n in range(1, 30):
        for p in range(1, 30):
            jm = (p - 1) // 2
            c, j = np.meshgrid(np.arange(n), np.arange(-jm, jm + 1), indexing="ij")
            s = R.clamp_start(n, p, c, j)
            assert ((s >= 0) & (s <= max(0, n - p)) & (s <= c) & (c < s + p)).all(), (n, p)
            checked += c.size
    assert checked > 150000
    s = R.clamp_start(29, 8, 14, -4)                                  # one past the bound (3) loses the centre: it is tight
    assert not s <= 14 < s + 8


def test_restatement_crop_and_index():
    lab = (np.arange(2 * 3 * 4 * 5).reshape(2, 3, 4, 5) % 3).astype(np.uint8)
    assert R.index(lab, None).shape == (2, 1, 1) and R.index(lab, None)[1, 0, 0] == (lab[1] != 0).sum()
    assert R.index(lab, (2, 9))[:, 1].sum() == 0
    src = lab[:, None]
    out = R.crop(src, [[1, -1, 2, 3], [0, 9, 0, 0], [-1, 0, 0, 0]], (3, 3, 4), fill=7)
    assert out.shape == (3, 1, 3, 3, 4) and (out[1:] == 7).all()
    assert np.array_equal(out[0, 0, 1:, :2, :2], lab[1, 0:2, 2:4, 3:5]) and (out[0, 0, 0] == 7).all()
    assert (out[0, 0, :, 2:] == 7).all() and (out[0, 0, :, :, 2:] == 7).all()
