"""Mirrored passes, ensembles and uncertainty maps of predict_volume, the parts that need no GPU: flip parsing, ensemble
and statistic validation (models on the CPU, nothing launched), the numpy restatement tests/tta_ref.py against the
properties of the rule, and the new C entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tta_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ flips
def test_all_is_the_seven_masks_in_ascending_order():
    from ctunet_amd.inference import parse_flips
    assert parse_flips("all") == (1, 2, 3, 4, 5, 6, 7)
    assert parse_flips(("x", "y", "yx", "z", "zx", "zy", "zyx")) == parse_flips("all")
    assert parse_flips(None) == () and parse_flips(()) == () and parse_flips([]) == ()
    assert parse_flips(("x", "zy")) == (1, 6) and parse_flips(["yz", "x"]) == (6, 1)       # order kept, letters in any order


@pytest.mark.parametrize("flips", [("x", "x"), ("zy", "yz"), ("",), ("xx",), ("zyz",), ("w",), ("xa",), "x", "zyx", (1,),
                                   (None,), 3, ("x", ("y",))])
def test_bad_flips_raise_value_error(flips):
    import ctunet_amd as A
    from ctunet_amd.inference import parse_flips
    with pytest.raises(ValueError):
        parse_flips(flips)
    torch.manual_seed(0)
    with pytest.raises(ValueError):                       # through the public call, on a CPU model: before the device check
        A.predict_volume(A.UNet(), torch.zeros(1, 40, 40, 40), patch=32, overlap=8, flips=flips)


# ------------------------------------------------------------------------------------------------ ensembles / statistics
def _call(models, in_ch=1, **kw):
    import ctunet_amd as A
    return A.predict_volume(models, torch.zeros(in_ch, 40, 40, 40), **{**dict(patch=32, overlap=8), **kw})


def test_ensemble_and_uncertainty_validation_without_a_gpu():
    import ctunet_amd as A
    torch.manual_seed(0)
    one, sp = A.UNet(), A.UNetSP()
    for bad in ([], (), [one, A.UNet4b2i3o()],               # empty; in_ch 1 against 2
                [one, A.UNet(out_channels=3)],               # out_ch
                [one, "net"], [one, None]):
        with pytest.raises(ValueError):
            _call(bad)
    with pytest.raises(ValueError):
        _call([sp, A.UNet4b2i3o()], in_ch=2)                 # same in_ch, different heads (two-output SP against one)
    with pytest.raises(ValueError):
        _call([A.UNet5b2i3o(), A.UNet4b2i3o()], in_ch=2, patch=64)          # levels
    k1 = A.UNet(out_channels=1)
    for u in ("entropy", "mutual_information", ("variance", "entropy")):
        with pytest.raises(ValueError):
            _call(k1, uncertainty=u)
    for u in ("std", ("entropy", "entropy"), (), 5, ("variance", "kl")):
        with pytest.raises(ValueError):
            _call(one, uncertainty=u)
    # what is valid passes validation and stops at the device check: nothing runs on a CPU model
    for kw in (dict(), dict(flips="all"), dict(flips=("x", "zy"), uncertainty=("mutual_information", "variance")),
               dict(uncertainty="entropy")):
        with pytest.raises(RuntimeError, match="MI355X"):
            _call([one, A.UNet()], **kw)
    with pytest.raises(RuntimeError, match="MI355X"):
        _call(k1, uncertainty="variance")
    assert one.training                                       # the failed calls left the mode alone
    from ctunet_amd.inference import parse_uncertainty
    assert parse_uncertainty(("mutual_information", "entropy"), 2) == ("entropy", "mutual_information")
    assert parse_uncertainty(None, 1) == () and parse_uncertainty("variance", 1) == ("variance",)


def test_prediction_has_a_last_uncertainty_field():
    import dataclasses
    from ctunet_amd.inference import Prediction
    assert [f.name for f in dataclasses.fields(Prediction)] == ["probs", "labels", "uncertainty"]
    assert Prediction(torch.zeros(1), None).uncertainty is None


# ------------------------------------------------------------------------------------------------ tta_ref
def test_mirroring_is_an_involution_also_on_a_padded_overhanging_tile():
    rng = np.random.default_rng(0)
    vol = rng.standard_normal((2, 10, 13, 9))
    for tile, patch in (((0, 0, 0), (8, 8, 8)), ((4, 8, 4), (8, 8, 8)), ((0, 0, 0), (16, 16, 16))):
        x = R.extract(vol, tile, patch)
        overhang = any(t + p > s for t, p, s in zip(tile, patch, vol.shape[1:]))
        assert (x == 0).any() == overhang
        for mask in range(8):
            m = R.mirror(x, mask)
            assert np.array_equal(R.mirror(m, mask), x)
            assert (mask == 0) == np.array_equal(m, x)
            # the padding is mirrored with the patch: a z-mirrored overhanging tile starts with its zero planes
            if mask & 4 and tile[0] + patch[0] > vol.shape[1]:
                assert (m[:, 0] == 0).all() and (x[:, 0] != 0).any()
        assert np.array_equal(R.mirror(x, 5), x[:, ::-1, :, ::-1])


@pytest.mark.parametrize("masks", [(0,), (0, 1), (0, 6, 1), tuple(range(8))])
def test_position_wise_model_is_reproduced_exactly_by_a_constant_blend(masks):
    from ctunet_amd.inference import tile_grid
    rng = np.random.default_rng(1)
    shape, patch, overlap = (12, 21, 38), (16, 16, 16), (4, 6, 5)           # every tile overhangs in z: mirrored padding
    vol = rng.standard_normal((1,) + shape)
    tiles = [tuple(t) for t in tile_grid(shape, patch, overlap)]
    a, b = np.array([1.5, -0.5])[:, None, None, None], np.array([0.25, 2.0])[:, None, None, None]
    out = R.predict(lambda m, x: a * x + b, vol, tiles, patch, masks, blend="constant")
    assert np.abs(out["probs"] - (a * vol + b)).max() <= 1e-12
    assert np.abs(out["variance"]).max() <= 1e-12        # every contribution of a voxel says the same


def test_statistics_of_the_restatement():
    from ctunet_amd.inference import tile_grid
    rng = np.random.default_rng(2)
    shape, patch, overlap, masks = (12, 20, 20), (8, 16, 16), (4, 8, 8), (0, 3, 4)
    tiles = [tuple(t) for t in tile_grid(shape, patch, overlap)]
    one = rng.random((3,) + patch)
    # identical contributions (up to the un-mirroring): y~ of pass f is the mirrored image of one fixed output
    ys = np.array([[[R.mirror(one, mask)] for mask in masks] for _ in range(2)])
    acc = R.accumulate(ys, masks, [(0, 0, 0)], patch, patch)                 # one tile: 2 models x 3 passes per voxel
    assert np.abs(R.finalize(acc)["variance"]).max() <= 1e-15
    assert (acc["n"] == 2 * 3).all()
    ys = rng.random((2, len(masks), len(tiles), 3) + patch)
    acc = R.accumulate(ys, masks, tiles, shape, patch)
    out = R.finalize(acc)
    assert (out["mutual_information"] >= 0).all() and out["mutual_information"].max() > 0        # Jensen: h is concave
    assert (out["variance"] >= 0).all() and (out["entropy"] <= 1 + 1e-12).all()
    assert acc["n"].max() == 2 * 3 * 2 * 2 * 2 and acc["n"].min() == 2 * 3
    # entropy: 1 for a uniform q (scaled by anything positive), 0 for one class, a zero sum and negative entries
    for k in (2, 3, 4):
        assert abs(R.entropy(np.full((k, 5), 0.7)) - 1).max() <= 1e-15
    assert (R.entropy(np.array([[0.0, 2.0, -1.0], [0.0, 0.0, 3.0]])) == 0).all()
    assert abs(R.entropy(np.array([[-5.0], [0.5], [0.5]]))[0] - np.log(2) / np.log(3)) <= 1e-15
    # uncovered voxels give 0 everywhere
    acc["S0"][0, 0, 0] = 0
    out = R.finalize(acc)
    assert all(np.all(out[n][..., 0, 0, 0] == 0) for n in ("probs", "variance", "entropy", "mutual_information", "labels"))


# ------------------------------------------------------------------------------------------------ symbols
def test_flip_entry_points_are_declared_bound_and_exported():
    from ctunet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctunet_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("ctu_extract_patches_flip", 13), ("ctu_window_accumulate_flip", 25),
                        ("ctu_window_finalize_stats", 12)):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name)
    from ctunet_amd import ops
    assert all(callable(getattr(ops, n)) for n in ("extract_patches_flip", "window_accumulate_flip", "window_finalize_stats"))
