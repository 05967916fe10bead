"""The shared 16-voxel row reader (csrc/voxel_rows.h: mask16 and its membership rules) through every kernel that reads a
map with it, at the widths where a lane's 16 voxels can go wrong, against the references the consumers' own test files use
(scipy.ndimage, distance_ref, the scipy restatement of test_surface_metrics_gpu, mesh_ref).

Volumes are 3 x 5 x W.  W = 1: one voxel in lane 0; 15: one short lane; 16: one full lane; 17: a full lane and a one-voxel
tail, and rows whose alignment changes from row to row; 40: two full lanes and a tail of 8; 1024: all 64 lanes full.  Every
width runs once from a tensor at the head of its storage and once from a view one element into it, so that the first row
starts off a 16-byte boundary with all 16 voxels present.  Label maps hold {0, 1, 2, 3}: the nonzero rule and label = 2.
Comparisons are bit-equal except where the consumer's own test states a tolerance (noted at the assertion)."""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import distance_ref as DR
import mesh_ref as MR
from test_morphology_gpu import _ref_implant
from test_surface_metrics_gpu import _ref as _ref_metrics

pytestmark = pytest.mark.gpu

D, H = 3, 5
WIDTHS = (1, 15, 16, 17, 40, 1024)
INT_DTYPES = (torch.uint8, torch.int64)
ALL_DTYPES = INT_DTYPES + (torch.float32,)
LABELS = (None, 2)
_ids = dict(ids=lambda v: str(v).replace("torch.", ""))


@functools.lru_cache(maxsize=None)
def _labels(w, seed=0):
    """int64 [D, H, w] label map with values 0..3 in runs along x (never modified); voxel 0 is background and the last
    voxel class 2, so every rule has a member and a non-member at every width."""
    rng = np.random.default_rng(100 * w + seed)
    a = np.repeat(rng.integers(0, 4, (D, H, (w + 2) // 3)), 3, axis=2)[:, :, :w]
    a = np.where(rng.random((D, H, w)) < 0.15, rng.integers(0, 4, (D, H, w)), a).astype(np.int64)
    a[0, 0, 0], a[-1, -1, -1] = 0, 2
    a.setflags(write=False)
    return a


def _member(a, label):
    return (a != 0) if label is None else (a == label)


def _dev(a, dtype, offset):
    """The array on the device as dtype: offset 0 at the head of its storage (16-byte aligned), offset 1 a contiguous view
    one element into a larger buffer."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    base = torch.zeros(t.numel() + 1, dtype=dtype, device="cuda")
    v = base[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == offset * v.element_size()
    return v


def _cases(dtypes):
    def deco(fn):
        for name, vals in (("offset", (0, 1)), ("w", WIDTHS), ("dtype", dtypes)):
            fn = pytest.mark.parametrize(name, vals, **_ids)(fn)
        return fn
    return deco


# ---------------------------------------------------------------------------------------------- morphology.hip, components.hip
@_cases(INT_DTYPES)
def test_morphology_pack(dtype, w, offset):
    from ctunet_amd import postprocess as pp
    a = _labels(w)
    t = _dev(a, dtype, offset)
    for label in LABELS:
        x = _member(a, label)
        assert np.array_equal(pp.binary_dilation(t, label=label).cpu().numpy() != 0, ndi.binary_dilation(x))
        # border value 1: the padding bits of the last word of a row carry the border into the volume
        assert np.array_equal(pp.binary_erosion(t, border_value=1, label=label).cpu().numpy() != 0,
                              ndi.binary_erosion(x, border_value=1))
        assert np.array_equal(pp.binary_fill_holes(t, label=label).cpu().numpy() != 0, ndi.binary_fill_holes(x))
    # the two-input pack: full AND NOT defective, the second map in the other dtype
    b = _labels(w, 1)
    other = _dev(b, INT_DTYPES[1 - INT_DTYPES.index(dtype)], offset)
    got = pp.extract_implant(t, other, opening_iterations=0, num_components=8)
    assert np.array_equal(got.cpu().numpy(), _ref_implant(a, b, 0, 1, 3, 8, False))


# ---------------------------------------------------------------------------------------------- distance.hip
@_cases(INT_DTYPES)
def test_distance_x_pass(dtype, w, offset):
    from ctunet_amd import postprocess as pp
    a = _labels(w)
    t = _dev(a, dtype, offset)
    for label in LABELS:
        x = _member(a, label)
        sq, idx = pp.distance_transform_edt(t, label=label, squared=True, return_indices=True)
        assert np.array_equal(sq.cpu().numpy(), np.rint(DR.edt(x) ** 2).astype(np.int32))      # unit sampling: exact
        i = idx.cpu().numpy().astype(np.int64)
        zz, yy, xx = np.indices(a.shape)
        assert not x[i[0], i[1], i[2]].any()
        assert np.array_equal((i[0] - zz) ** 2 + (i[1] - yy) ** 2 + (i[2] - xx) ** 2, sq.cpu().numpy())
        # both planes from one mask; float32 square roots of exact integers (test_distance_gpu's rtol for unit sampling)
        torch.testing.assert_close(pp.signed_distance(t, label=label).cpu(),
                                   torch.from_numpy(DR.signed(x).astype(np.float32)), rtol=1e-6, atol=0)
        assert DR.ball_decidable(1.5, None, 3)
        assert np.array_equal(pp.ball_dilation(t, 1.5, label=label).cpu().numpy() != 0, DR.ball_dilation(x, 1.5))


# ---------------------------------------------------------------------------------------------- surface.hip
def _close(got, ref):
    """test_surface_metrics_gpu's tolerance: float32 results against the float64 restatement."""
    got = got.detach().cpu().double().numpy()
    assert got.shape == ref.shape and np.allclose(got, ref, rtol=1e-6, atol=0, equal_nan=True), (got, ref)


@_cases(ALL_DTYPES)
def test_surface_metrics_rows(dtype, w, offset):
    from ctunet_amd import metrics, ops
    pl, gl = _labels(w), _labels(w, 1)
    onehot = lambda lab: np.stack([lab == k for k in range(4)])[None]              # bool [1, 4, D, H, w]
    ref = _ref_metrics(onehot(pl), onehot(gl), [1, 2, 3], [(1.0, 1.0, 1.0)])
    if dtype != torch.float32:                           # label maps: member = (v == c)
        res = metrics.surface_metrics(_dev(pl, dtype, offset), _dev(gl, dtype, offset), 4, percentile=None)
        assert np.array_equal(res["dice"].cpu().numpy(), ref["dice"].astype(np.float32))
        _close(res["hd"], ref["hd"])
        _close(res["assd"], ref["assd"])
    if dtype != torch.int64:                             # one-hot tensors: member = (v != 0)
        yp, yg = _dev(onehot(pl), dtype, offset), _dev(onehot(gl), dtype, offset)
        _close(metrics.compute_hausdorff_distance(yp, yg), ref["hd"])
        _close(metrics.compute_average_surface_distance(yp, yg, symmetric=True), ref["assd"])
    if dtype == torch.float32:                           # the float label map: member = (v == (float)c), under ops.hausdorff
        _close(ops.hausdorff(yp, yg), ref["hd"])


# ---------------------------------------------------------------------------------------------- mesh.hip
@_cases(ALL_DTYPES)
def test_mesh_count_rows(dtype, w, offset):
    from ctunet_amd import mesh
    if dtype == torch.float32:
        field = np.random.default_rng(w).random((D, H, w), dtype=np.float32)
        assert not (field == np.float32(0.37)).any()
        rv, rf = MR.extract(field, level=0.37)
        m = mesh.extract_surface(_dev(field, dtype, offset), level=0.37)
        v, f = m.vertices.cpu().numpy(), m.faces.cpu().numpy()
        assert np.array_equal(f, rf) and v.shape == rv.shape
        assert np.abs(v.astype(np.float64) - rv).max() <= 1e-6 * np.abs(rv).max()      # test_mesh_gpu.test_float_fields
        return
    a = _labels(w)
    t = _dev(a, dtype, offset)
    for label in LABELS:
        rv, rf = MR.extract(a, label=label)
        m = mesh.extract_surface(t, label=label)
        assert np.array_equal(m.faces.cpu().numpy(), rf)
        assert np.array_equal(m.vertices.cpu().numpy().view(np.uint32), rv.view(np.uint32))
