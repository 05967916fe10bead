"""ctunet_amd.metrics without a GPU: argument parsing and validation (which must raise before anything is launched) and
the new C-ABI entry points in the header, the ctypes table and the built library."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spacing_parsing():
    from ctunet_amd.metrics import parse_spacing
    assert parse_spacing(None, 2) is None
    assert parse_spacing(0.5, 2) == [[0.5] * 3, [0.5] * 3]
    assert parse_spacing(2, 1) == [[2.0] * 3]
    assert parse_spacing((3.0, 0.8, 0.65), 2) == [[3.0, 0.8, 0.65]] * 2
    assert parse_spacing([(1, 2, 3), (4, 5, 6)], 2) == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
    assert parse_spacing(torch.tensor([1.0, 2.0, 3.0]), 1) == [[1.0, 2.0, 3.0]]
    # N == 3 triples of a batch of three
    assert parse_spacing([(1, 1, 1), (2, 2, 2), (3, 3, 3)], 3)[2] == [3.0, 3.0, 3.0]
    for bad in (0.0, -1.0, float("nan"), float("inf"), (1.0, 0.0, 1.0), (1.0, 2.0), [(1, 1, 1)], "1mm", True,
                (1.0, float("inf"), 1.0), [(1, 1, 1), (1, -1, 1)]):
        with pytest.raises(ValueError):
            parse_spacing(bad, 2)


def _cpu_onehot(n=1, c=3, d=8, h=8, w=8):
    return torch.zeros(n, c, d, h, w), torch.zeros(n, c, d, h, w)


def test_arguments_are_validated_before_any_launch():
    from ctunet_amd import metrics
    a, b = _cpu_onehot()
    with pytest.raises(ValueError, match="euclidean"):
        metrics.compute_hausdorff_distance(a, b, distance_metric="chessboard")
    with pytest.raises(ValueError, match="euclidean"):
        metrics.compute_average_surface_distance(a, b, distance_metric="taxicab")
    with pytest.raises(ValueError, match="euclidean"):
        metrics.compute_surface_dice(a, b, [1.0, 1.0], distance_metric="cityblock")
    for q in (-0.5, 100.5, float("nan"), "95"):
        with pytest.raises(ValueError, match="percentile"):
            metrics.compute_hausdorff_distance(a, b, percentile=q)
        with pytest.raises(ValueError, match="percentile"):
            metrics.surface_metrics(a[0, 0], b[0, 0], 2, percentile=q)
    with pytest.raises(ValueError, match="class_thresholds"):
        metrics.compute_surface_dice(a, b, [1.0])                      # two scored classes
    with pytest.raises(ValueError, match="class_thresholds"):
        metrics.compute_surface_dice(a, b, [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="class_thresholds"):
        metrics.compute_surface_dice(a, b, [1.0, 2.0, 3.0], include_background=False)
    with pytest.raises(ValueError, match="class_thresholds"):
        metrics.compute_surface_dice(a, b, [1.0, -2.0])
    with pytest.raises(ValueError, match="tolerance"):
        metrics.surface_metrics(a[0, 0].byte(), b[0, 0].byte(), 3, tolerance=[1.0])
    with pytest.raises(ValueError, match="spacing"):
        metrics.compute_hausdorff_distance(a, b, spacing=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="spacing"):
        metrics.surface_metrics(a[0, 0].byte(), b[0, 0].byte(), 2, spacing=-1.0)
    # shapes, dtypes, class counts and sides
    with pytest.raises(ValueError, match="shape"):
        metrics.compute_hausdorff_distance(a, b[:, :, :4])
    with pytest.raises(ValueError, match="shape"):
        metrics.surface_metrics(torch.zeros(4, 4, 4, dtype=torch.uint8), torch.zeros(4, 4, 5, dtype=torch.uint8), 2)
    with pytest.raises(ValueError):
        metrics.compute_hausdorff_distance(a[0], b[0])                  # 4-D
    with pytest.raises(ValueError):
        metrics.compute_hausdorff_distance(a.double(), b)
    with pytest.raises(ValueError):
        metrics.surface_metrics(a[0, 0], b[0, 0], 2)                    # float label maps
    with pytest.raises(ValueError):
        metrics.surface_metrics(a[0, 0].int(), b[0, 0].int(), 2)        # int32 label maps
    with pytest.raises(ValueError, match="classes"):
        metrics.surface_metrics(a[0, 0].byte(), b[0, 0].byte(), 18)
    with pytest.raises(ValueError, match="classes"):
        metrics.surface_metrics(a[0, 0].byte(), b[0, 0].byte(), 1)      # background only, not scored
    with pytest.raises(ValueError, match="classes"):
        metrics.compute_hausdorff_distance(torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(ValueError, match="side"):
        metrics.surface_metrics(torch.zeros(2, 2, 1025, dtype=torch.uint8), torch.zeros(2, 2, 1025, dtype=torch.uint8), 2)
    # valid arguments on the CPU: refused as CPU inputs (no fallback), still before any launch
    with pytest.raises(ValueError, match="GPU"):
        metrics.compute_hausdorff_distance(a, b, percentile=95, spacing=(3.0, 0.8, 0.65))
    with pytest.raises(ValueError, match="GPU"):
        metrics.compute_surface_dice(a.byte(), b.bool(), [1.0, 2.0])
    with pytest.raises(ValueError, match="GPU"):
        metrics.surface_metrics(torch.zeros(2, 4, 4, 4, dtype=torch.int64), torch.zeros(2, 4, 4, 4, dtype=torch.uint8), 3,
                                spacing=[(1, 1, 1), (2, 2, 2)], tolerance=1.0)


def test_entry_points_declared_bound_exported_and_sized():
    from ctunet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctunet_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("ctu_surface_ws_bytes", 5), ("ctu_surface_metrics", 19)):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 8 and _lib.load().ctu_abi_version() == 8
    import ctunet_amd
    assert "metrics" in ctunet_amd.__all__
    from ctunet_amd import metrics
    for fn in ("compute_hausdorff_distance", "compute_average_surface_distance", "compute_surface_dice",
               "surface_metrics"):
        assert callable(getattr(metrics, fn))
    # workspace: about 5 bytes per voxel per plane (edge byte + 4-byte distance) plus small per-pair tables
    v = 224 * 512 * 512
    ws = metrics.workspace_bytes(1, 1, (224, 512, 512))
    assert 10 * v <= ws <= 10 * v + (1 << 20)
    assert ws / (2 * v) <= 9.0
    assert metrics.workspace_bytes(1, 2, (224, 512, 512)) >= 20 * v
    assert _lib.load().ctu_surface_ws_bytes(1, 17, 8, 8, 8) == 0
    assert _lib.load().ctu_surface_ws_bytes(0, 1, 8, 8, 8) == 0
    assert math.isfinite(ws)
