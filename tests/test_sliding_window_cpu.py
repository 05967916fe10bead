"""Sliding-window inference, the parts that need no GPU: the blend tables against a float64 restatement of the rule,
the batching of the tile list, argument validation, and the C-ABI entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gauss64(p, sigma_scale):
    """g(i) = exp(-(i - (P-1)/2)^2 / (2 sigma^2)), sigma = sigma_scale * P, in float64."""
    i = np.arange(p, dtype=np.float64)
    s = sigma_scale * p
    return np.exp(-(i - (p - 1) / 2) ** 2 / (2 * s * s))


@pytest.mark.parametrize("patch,sigma_scale", [((32, 32, 32), 0.125), ((16, 32, 48), 0.125), ((192, 192, 192), 0.125),
                                               ((32, 16, 64), 0.3)])
def test_gaussian_tables_and_floor_match_a_float64_restatement(patch, sigma_scale):
    from ctunet_amd.inference import window_tables, window_weight
    tabs = window_tables(patch, "gaussian", sigma_scale)
    for p, t in zip(patch, tabs):
        assert t.dtype == np.float32 and t.shape == (p,)
        ref = _gauss64(p, sigma_scale)
        np.testing.assert_allclose(t, ref, rtol=1e-7, atol=0)
        assert np.array_equal(t, t[::-1]) and t.max() <= 1        # symmetric about (P-1)/2, peak 1 there
    w = window_weight(patch, "gaussian", sigma_scale)
    g = [_gauss64(p, sigma_scale) for p in patch]
    ref = np.maximum(g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :], 1e-3)
    assert w.dtype == np.float32 and w.shape == tuple(patch)
    np.testing.assert_allclose(w, ref, rtol=1e-6, atol=0)
    if sigma_scale == 0.125:
        # sigma = P/8: the corners sit 4 sigma out on every axis (product e^-24): the floor holds there
        assert w[0, 0, 0] == np.float32(1e-3) and (w >= np.float32(1e-3)).all()


def test_constant_blend_is_all_ones():
    from ctunet_amd.inference import window_tables, window_weight
    for t in window_tables((16, 32, 48), "constant"):
        assert (t == 1).all()
    assert (window_weight((16, 32, 48), "constant") == 1).all()


@pytest.mark.parametrize("shape,patch,overlap,batch", [((224, 512, 512), 192, 48, 2), ((40, 52, 70), 32, 8, 3),
                                                       ((56, 72, 88), 32, 8, 4), ((20, 33, 70), (16, 32, 32), (4, 8, 2), 5),
                                                       ((10, 10, 10), 32, 8, 2)])
def test_batches_cover_every_tile_once_in_order(shape, patch, overlap, batch):
    from ctunet_amd.inference import _triple, plan_batches, tile_grid
    from ctunet_amd.tiling import VolumeTiler
    p3, o3 = _triple(patch, "patch"), _triple(overlap, "overlap")
    tiles = tile_grid(shape, p3, o3)
    assert np.array_equal(tiles, VolumeTiler(patch, overlap).coords(shape, "cpu").numpy())      # z-major, same tiles
    bp = plan_batches(tiles, batch, shape, p3)
    nb = -(-tiles.shape[0] // batch)
    assert bp.coords.shape == (nb, batch, 3) and bp.valid.shape == (nb, batch)
    flat_c, flat_v = bp.coords.reshape(-1, 3), bp.valid.reshape(-1)
    assert np.array_equal(flat_c[flat_v == 1], tiles)                  # each tile exactly once, in tile order
    n_pad = nb * batch - tiles.shape[0]
    assert flat_v[:tiles.shape[0]].all() and not flat_v[tiles.shape[0]:].any() and (flat_v == 0).sum() == n_pad
    ext = np.array(bp.extent)
    assert ext[2] % 4 == 0
    for b in range(nb):
        tb = bp.coords[b][bp.valid[b] == 1]
        assert (bp.box[b] <= tb.min(0)).all() and bp.box[b][2] % 4 == 0
        hi = np.minimum(tb.max(0) + np.array(p3), np.array(shape))
        assert (bp.box[b] + ext >= hi).all()                           # the launch extent covers every batch's box
        # padding slots point at a real tile: extraction stays inside the volume's tile grid
        for c in bp.coords[b][bp.valid[b] == 0]:
            assert any((c == t).all() for t in tiles)
    meta = bp.meta()
    assert meta.shape == (nb, 4 * batch + 3) and meta.dtype == np.int32


def test_one_batch_for_2x4x4_tiles_at_full_size():
    from ctunet_amd.inference import plan_batches, tile_grid
    tiles = tile_grid((224, 512, 512), (192,) * 3, (48,) * 3)
    assert tiles.shape[0] == 32
    bp = plan_batches(tiles, 2, (224, 512, 512), (192,) * 3)
    assert bp.coords.shape[0] == 16 and bp.valid.all()


def _bad(model, **kw):
    from ctunet_amd import predict_volume
    args = dict(volume=torch.zeros(model._plan.in_ch, 40, 40, 40), patch=32, overlap=8)
    args.update(kw)
    with pytest.raises(ValueError):
        predict_volume(model, **args)


def test_invalid_arguments_raise_value_error_before_any_launch():
    import ctunet_amd as A
    torch.manual_seed(0)
    four = A.UNet()                 # 4 levels: patch % 16
    five = A.UNet5b2i3o()           # 5 levels: patch % 32
    _bad(four, patch=24)
    _bad(four, patch=(32, 32, 40))
    _bad(five, patch=48)
    _bad(five, patch=(64, 64, 16))
    _bad(four, patch=32, overlap=32)
    _bad(four, patch=32, overlap=(8, 40, 8))
    _bad(four, overlap=-1)
    _bad(four, blend="mean")
    _bad(four, batch=0)
    _bad(four, batch=-2)
    _bad(four, volume=torch.zeros(40, 40, 40))                 # 3-D
    _bad(four, volume=torch.zeros(2, 1, 40, 40, 40))           # a batch of volumes
    _bad(four, volume=torch.zeros(2, 40, 40, 40))              # channel count of the model: 1
    _bad(four, volume=torch.zeros(1, 40, 40, 40, dtype=torch.float64))
    _bad(four, sigma_scale=0.0)
    _bad(four, patch=32.0)
    # the 5-level class accepts what the 4-level one rejects only when divisible by 32; these do not raise on validation
    from ctunet_amd.inference import _validate
    _validate(five, torch.zeros(2, 40, 40, 40), 64, 16, 2, "gaussian", 0.125)
    _validate(four, torch.zeros(1, 1, 40, 40, 40), (16, 32, 48), (0, 8, 47), 1, "constant", 0.125)


def test_new_entry_points_are_declared_bound_and_exported():
    from ctunet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctunet_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("ctu_window_accumulate", 22), ("ctu_window_finalize", 7)):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name)
    import ctunet_amd
    assert "predict_volume" in ctunet_amd.__all__ and callable(ctunet_amd.predict_volume)
