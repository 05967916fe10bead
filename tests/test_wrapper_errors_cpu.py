"""The refusals of the volume, mesh and metric wrappers, pinned: every row of the table below is one erroneous call (or a
valid one on CPU tensors, which must be refused for not living on the GPU), and ``tests/golden/wrapper_errors.json`` holds
the exception class and the full message each raised when the table was recorded.  The test replays the calls and
compares both exactly, so neither the wording nor the order of the checks can drift.  Validation runs before the GPU
check in these wrappers, so no row needs a GPU.  ``python tests/test_wrapper_errors_cpu.py`` records the fixture anew;
that is for a commit that means to change a message, never for one that means to keep them."""
import functools
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "wrapper_errors.json")
if __name__ == "__main__":
    for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "ct-unet_amd")):
        sys.path.insert(0, p)

from ctunet_amd import mesh, metrics, postprocess, preprocess, registration, resample, transforms  # noqa: E402

NAN, INF = float("nan"), float("inf")
# what a number-or-triple argument may wrongly be; "tensor", "zero" and "neg" are valid for some arguments, and the row then
# pins that the call gets as far as the GPU check
TRIPLES = {
    "not_iterable": 1j, "none": None, "len2": (1.0, 2.0), "len4": [1.0, 2.0, 3.0, 4.0], "bool_scalar": True,
    "bool": (1.0, True, 1.0), "str": (1.0, "a", 1.0), "text": "abc", "nan": (1.0, NAN, 1.0), "inf": INF,
    "zero": (1.0, 0.0, 1.0), "neg": -1.0, "neg_one": [1.0, 1.0, -2.5], "tensor": torch.tensor([1.0, 2.0, 3.0]),
    "tensor_bad": torch.tensor([1.0, -2.0, NAN]), "nested": [[1.0, 2.0, 3.0]], "tensor_nested": torch.tensor([[1.0, 2.0, 3.0]]),
    "f32_overflow": 1e39, "f32_underflow": (1.0, 1e-50, 1.0), "nan_then_bool": (NAN, True, 1.0), "good": (0.5, 1.0, 2.0),
}
# what a (D, H, W) grid argument may wrongly be
GRIDS = {
    "not_iterable": 5, "len2": (4, 5), "bool": (4, True, 6), "float": (4, 5.0, 6), "str": "456", "zero": (4, 0, 6),
    "neg": [4, -1, 6], "side_1025": (1025, 2, 2), "voxels_2_31": (2048, 1024, 1024), "cells_2_31": (1024, 1024, 1024),
    "tensor": torch.tensor([4, 5, 6]), "good": [4, 5, 6],
}

X = torch.zeros(4, 5, 6)                                   # one float32 volume
XB = torch.zeros(2, 4, 5, 6)                               # a batch of two
I16 = torch.zeros(4, 5, 6, dtype=torch.int16)
U8 = torch.zeros(4, 5, 6, dtype=torch.uint8)
U8B = torch.zeros(2, 4, 5, 6, dtype=torch.uint8)
HUGE = torch.zeros(1).expand(2048, 1024, 1024)             # 2^31 voxels without the memory
WIDE = torch.zeros(1).expand(1, 1, 1025)
EMPTY = torch.zeros(0, 4, 5, 6)
M44 = torch.eye(4, dtype=torch.float64)
PTS = torch.zeros(7, 3)
MESH = mesh.Mesh(torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32))
ONEHOT = torch.zeros(2, 3, 4, 5, 6)
X5 = torch.zeros(2, 1, 4, 5, 6)


def _outs(shape, dtype):
    """What an ``out=`` may wrongly be for a result of ``shape`` and ``dtype``."""
    other = torch.float64 if dtype != torch.float64 else torch.float32
    return {"not_tensor": [0.0], "shape": torch.zeros(shape + (1,), dtype=dtype), "dtype": torch.zeros(shape, dtype=other),
            "strided": torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=dtype)[..., ::2],
            "good": torch.zeros(shape, dtype=dtype)}


def _spatial(**kw):
    return transforms.RandomSpatial(seed=1, **kw)


ROWS = {}


def _add(name, call):
    assert name not in ROWS, name
    ROWS[name] = call


def _each(prefix, values, call):
    for kind, v in values.items():
        _add(f"{prefix}[{kind}]", lambda v=v: call(v))


# ---- resample
_each("resample.size", GRIDS, lambda v: resample.resample(X, v))
_each("resample.spacing", TRIPLES, lambda v: resample.resample(X, spacing=v, new_spacing=1.0))
_each("resample.new_spacing", TRIPLES, lambda v: resample.resample(X, spacing=1.0, new_spacing=v))
_each("resample.out", _outs((8, 8, 8), torch.float32), lambda v: resample.resample(X, (8, 8, 8), out=v))
_add("resample.input_grid[voxels_2_31]", lambda: resample.resample(HUGE, (4, 4, 4)))
_add("resample.output_grid[voxels_2_31]", lambda: resample.resample(X, spacing=1.0, new_spacing=(1 / 512, 1 / 1024, 1 / 1024)))
_add("resample.batch[empty]", lambda: resample.resample(EMPTY, (8, 8, 8)))
_add("resample[only_spacing]", lambda: resample.resample(X, spacing=1.0))
_add("resample[two_bad:size,out]", lambda: resample.resample(X, (4, 0, 6), out=[0.0]))
_add("resample[two_bad:spacing,new_spacing]", lambda: resample.resample(X, spacing="abc", new_spacing=-1.0))
_add("resample[two_bad:mode,size]", lambda: resample.resample(X, (4, 0, 6), mode="cubic"))
_add("resample[two_bad:empty,out]", lambda: resample.resample(EMPTY, (8, 8, 8), out=[0.0]))
_each("geometry.in_shape", GRIDS, lambda v: resample.geometry(v, (8, 8, 8)))
_each("geometry.size", GRIDS, lambda v: resample.geometry((4, 5, 6), v))
_each("geometry.spacing", TRIPLES, lambda v: resample.geometry((4, 5, 6), None, v, 1.0))
_add("geometry[two_bad:in_shape,size]", lambda: resample.geometry((4, 0, 6), "456"))
_each("Resampler.in_shape", GRIDS, lambda v: resample.Resampler(v, (8, 8, 8)))
_each("Resampler.out_shape", GRIDS, lambda v: resample.Resampler((4, 5, 6), v))
_each("Resampler.in_spacing", TRIPLES, lambda v: resample.Resampler((4, 5, 6), in_spacing=v, out_spacing=1.0))
_each("Resampler.out_spacing", TRIPLES, lambda v: resample.Resampler((4, 5, 6), in_spacing=1.0, out_spacing=v))
_add("Resampler[two_bad:in_shape,in_spacing]", lambda: resample.Resampler((4, 5), in_spacing=-1.0, out_spacing=1.0))
_each("Resampler.call.out", _outs((8, 8, 8), torch.float32), lambda v: resample.Resampler((4, 5, 6), (8, 8, 8))(X, out=v))
_each("Resampler.inverse.out", _outs((2, 4, 5, 6), torch.float32),
      lambda v: resample.Resampler((4, 5, 6), (8, 8, 8)).inverse(torch.zeros(2, 8, 8, 8), out=v))
_add("Resampler.call[two_bad:grid,out]", lambda: resample.Resampler((4, 5, 6), (8, 8, 8))(torch.zeros(4, 5, 7), out=[0.0]))
_add("Resampler.call.batch[empty]", lambda: resample.Resampler((4, 5, 6), (8, 8, 8))(EMPTY))
_add("Resampler.to[cpu]", lambda: resample.Resampler((4, 5, 6), (8, 8, 8)).to("cpu"))
_each("affine_resample.out_shape", GRIDS, lambda v: resample.affine_resample(X, M44, v))
for _arg in ("spacing", "origin", "out_spacing", "out_origin"):
    _each(f"affine_resample.{_arg}", TRIPLES, lambda v, a=_arg: resample.affine_resample(X, M44, (4, 5, 6), **{a: v}))
_each("affine_resample.out", _outs((4, 5, 6), torch.float32), lambda v: resample.affine_resample(X, M44, (4, 5, 6), out=v))
_each("affine_resample.out_u8", _outs((4, 5, 6), torch.uint8),
      lambda v: resample.affine_resample(U8, M44, (4, 5, 6), mode="nearest", out=v))
_add("affine_resample.input_grid[voxels_2_31]", lambda: resample.affine_resample(HUGE, M44, (4, 5, 6)))
_add("affine_resample.batch[empty]", lambda: resample.affine_resample(EMPTY, M44, (4, 5, 6)))
_add("affine_resample[two_bad:out_shape,spacing]", lambda: resample.affine_resample(X, M44, (4, 0, 6), spacing=-1.0))
_add("affine_resample[two_bad:spacing,origin]", lambda: resample.affine_resample(X, M44, (4, 5, 6), spacing=0.0, origin="abc"))
_add("affine_resample[two_bad:origin,fill]", lambda: resample.affine_resample(X, M44, (4, 5, 6), origin=NAN, fill="0"))
_add("affine_resample[two_bad:fill,out]", lambda: resample.affine_resample(X, M44, (4, 5, 6), fill=INF, out=[0.0]))
_add("affine_resample[two_bad:out,matrix]", lambda: resample.affine_resample(X, None, (4, 5, 6), out=[0.0]))

# ---- preprocess
_each("gaussian_filter.sigma", TRIPLES, lambda v: preprocess.gaussian_filter(X, v))
_each("gaussian_filter.spacing", TRIPLES, lambda v: preprocess.gaussian_filter(X, 1.0, spacing=v))
_each("gaussian_filter.out", _outs((4, 5, 6), torch.float32), lambda v: preprocess.gaussian_filter(X, 1.0, out=v))
_add("gaussian_filter.side[1025]", lambda: preprocess.gaussian_filter(WIDE, 1.0))
_add("gaussian_filter[two_bad:sigma,spacing]", lambda: preprocess.gaussian_filter(X, -1.0, spacing=0.0))
_add("gaussian_filter[two_bad:spacing,mode]", lambda: preprocess.gaussian_filter(X, 1.0, spacing="abc", mode="wrap"))
_add("gaussian_filter[two_bad:radius,side]", lambda: preprocess.gaussian_filter(WIDE, 100.0))
_add("gaussian_filter[two_bad:side,out]", lambda: preprocess.gaussian_filter(WIDE, 1.0, out=[0.0]))
_add("finite_range[cpu]", lambda: preprocess.finite_range(X))
_each("histogram.out", _outs((256,), torch.int64), lambda v: preprocess.histogram(X, out=v))
_each("histogram.out_with_range", _outs((16,), torch.int64), lambda v: preprocess.histogram(I16, 16, (0, 100), out=v))
_add("histogram[two_bad:bins,out]", lambda: preprocess.histogram(X, 1, out=[0.0]))
_add("histogram[two_bad:range,out]", lambda: preprocess.histogram(X, range=(1, 0), out=[0.0]))
_add("threshold_otsu[cpu]", lambda: preprocess.threshold_otsu(X))
_add("threshold_otsu[cpu,range]", lambda: preprocess.threshold_otsu(X, range=(0, 1)))
_add("threshold_otsu[cpu,hist]", lambda: preprocess.threshold_otsu(hist=torch.zeros(16, dtype=torch.int64), range=(0, 1)))
_each("binarize.out", _outs((4, 5, 6), torch.uint8), lambda v: preprocess.binarize(X, 0.5, out=v))
_add("binarize[two_bad:lower,out]", lambda: preprocess.binarize(X, NAN, out=[0.0]))
_add("binarize[two_bad:upper,out]", lambda: preprocess.binarize(X, 0.0, True, out=[0.0]))
_each("extract_skull.sigma", TRIPLES, lambda v: preprocess.extract_skull(I16, 300, sigma=v))
_each("extract_skull.spacing", TRIPLES, lambda v: preprocess.extract_skull(I16, 300, spacing=v))
_add("extract_skull[cpu,sigma]", lambda: preprocess.extract_skull(I16, 300, sigma=1.0, spacing=(0.8, 0.45, 0.45)))
_add("extract_skull[cpu,otsu]", lambda: preprocess.extract_skull(I16, "otsu", otsu_range=(-200, 3000)))
_add("extract_skull[two_bad:threshold,sigma]", lambda: preprocess.extract_skull(I16, NAN, sigma=-1.0))
_add("extract_skull[two_bad:sigma,components]", lambda: preprocess.extract_skull(I16, 300, sigma=-1.0, components=99))
_add("extract_skull[two_bad:closing_radius,spacing]", lambda: preprocess.extract_skull(I16, 300, closing_radius=-1, spacing=0))

# ---- registration
for _arg in ("spacing", "origin"):
    _each(f"register_points.{_arg}", TRIPLES, lambda v, a=_arg: registration.register_points(PTS, X, **{a: v}))
    _each(f"accumulate.{_arg}", TRIPLES, lambda v, a=_arg: registration.accumulate(PTS, X, M44, **{a: v}))
    _each(f"surface_points.{_arg}", TRIPLES, lambda v, a=_arg: registration.surface_points(U8, **{a: v}))
for _arg in ("moving_spacing", "moving_origin", "fixed_spacing", "fixed_origin"):
    _each(f"register.{_arg}", TRIPLES, lambda v, a=_arg: registration.register(U8, U8, **{a: v}))
_add("register_points[two_bad:iterations,spacing]", lambda: registration.register_points(PTS, X, iterations=-1, spacing=0.0))
_add("register_points[two_bad:max_distance,origin]", lambda: registration.register_points(PTS, X, max_distance=-1, origin=NAN))
_add("register_points[two_bad:spacing,origin]", lambda: registration.register_points(PTS, X, spacing=(1, 2), origin="abc"))
_add("register_points[two_bad:origin,init]", lambda: registration.register_points(PTS, X, origin=INF, init=0))
_add("accumulate[two_bad:max_distance,spacing]", lambda: registration.accumulate(PTS, X, M44, max_distance=NAN, spacing=-1))
_add("accumulate[two_bad:spacing,origin]", lambda: registration.accumulate(PTS, X, M44, spacing=-1, origin=(1, 2)))
_add("surface_points[two_bad:mask,spacing]", lambda: registration.surface_points(X, spacing=-1))
_add("surface_points[two_bad:spacing,origin]", lambda: registration.surface_points(U8, spacing=-1, origin=NAN))
_add("register[two_bad:moving_spacing,fixed_origin]", lambda: registration.register(U8, U8, moving_spacing=0, fixed_origin=INF))
_add("register[two_bad:fixed_spacing,init]", lambda: registration.register(U8, U8, fixed_spacing=-1, init="pca"))
_add("register_points[cpu,one_on_cpu]", lambda: registration.register_points(PTS, X, init=M44))

# ---- mesh
_each("extract_surface.spacing", TRIPLES, lambda v: mesh.extract_surface(U8, spacing=v))
_each("extract_surface.origin", TRIPLES, lambda v: mesh.extract_surface(U8, origin=v))
_add("extract_surface.volume[side_1025]", lambda: mesh.extract_surface(WIDE.to(torch.uint8)))
_add("extract_surface[two_bad:level,spacing]", lambda: mesh.extract_surface(U8, level=NAN, spacing=-1))
_add("extract_surface[two_bad:spacing,origin]", lambda: mesh.extract_surface(U8, spacing=1e-50, origin=1e39))
_add("extract_surface[two_bad:origin,label]", lambda: mesh.extract_surface(U8, origin="abc", label=1.5))
_add("extract_surface[cpu,field]", lambda: mesh.extract_surface(X, 0.25, spacing=torch.tensor([0.5, 1.0, 2.0]), origin=-3))
for _name in ("voxelize", "winding_number"):
    _fn = getattr(mesh, _name)
    _each(f"{_name}.shape", GRIDS, lambda v, f=_fn: f(MESH, v))
    _each(f"{_name}.spacing", TRIPLES, lambda v, f=_fn: f(MESH, (4, 5, 6), spacing=v))
    _each(f"{_name}.origin", TRIPLES, lambda v, f=_fn: f(MESH, (4, 5, 6), origin=v))
    _add(f"{_name}[two_bad:mesh,shape]", lambda f=_fn: f((X, X), (4, 0, 6)))
    _add(f"{_name}[two_bad:shape,spacing]", lambda f=_fn: f(MESH, (4, 0, 6), spacing=-1))
    _add(f"{_name}[two_bad:spacing,origin]", lambda f=_fn: f(MESH, (4, 5, 6), spacing=(1, True, 1), origin=(1, 2)))
_each("distance_field.shape", GRIDS, lambda v: mesh.distance_field(MESH, v, max_distance=2.0))
_each("distance_field.spacing", TRIPLES, lambda v: mesh.distance_field(MESH, (4, 5, 6), spacing=v, max_distance=2.0))
_each("distance_field.origin", TRIPLES, lambda v: mesh.distance_field(MESH, (4, 5, 6), origin=v, max_distance=2.0))
_add("distance_field[two_bad:shape,max_distance]", lambda: mesh.distance_field(MESH, (4, 5)))
_add("distance_field[two_bad:origin,max_distance]", lambda: mesh.distance_field(MESH, (4, 5, 6), origin=INF, max_distance=-1))
_add("distance_field[two_bad:spacing,origin]", lambda: mesh.distance_field(MESH, (4, 5, 6), 0.0, "abc", max_distance=2.0))
_each("mesh.workspace_bytes.shape", GRIDS, lambda v: mesh.workspace_bytes(v) and None)
_each("mesh.voxelize_workspace_bytes.shape", GRIDS, lambda v: mesh.voxelize_workspace_bytes(v) and None)
for _name in ("measure", "face_normals", "adjacency", "smooth", "build_face_grid"):
    _add(f"{_name}[cpu]", lambda f=getattr(mesh, _name): f(MESH))
_add("point_distance[cpu]", lambda: mesh.point_distance(PTS, MESH))
_add("mesh_surface_metrics[cpu]", lambda: metrics.mesh_surface_metrics(MESH, MESH))

# ---- metrics
_SPACINGS = dict(TRIPLES, two_triples=[(1, 2, 3), (4, 5, 6)], three_triples=[(1, 2, 3)] * 3, two_bad_triple=[(1, 2, 3), (4, 0, 6)],
                 two_bool_triple=[(1, 2, 3), (4, True, 6)], two_str_triple=[(1, 2, 3), "abc"], tensor_two=torch.ones(2, 3),
                 scalar_tensor=torch.tensor(2.0), a_range=range(1, 4))
_each("parse_spacing", _SPACINGS, lambda v: metrics.parse_spacing(v, 2) and None)
_each("compute_hausdorff_distance.spacing", _SPACINGS, lambda v: metrics.compute_hausdorff_distance(ONEHOT, ONEHOT, spacing=v))
_each("compute_average_surface_distance.spacing", TRIPLES,
      lambda v: metrics.compute_average_surface_distance(ONEHOT, ONEHOT, spacing=v))
_each("compute_surface_dice.spacing", TRIPLES, lambda v: metrics.compute_surface_dice(ONEHOT, ONEHOT, [1.0, 1.0], spacing=v))
_each("surface_metrics.spacing", _SPACINGS, lambda v: metrics.surface_metrics(U8B, U8B, 3, spacing=v))
_add("compute_hausdorff_distance[two_bad:percentile,spacing]",
     lambda: metrics.compute_hausdorff_distance(ONEHOT, ONEHOT, percentile=101, spacing=-1))
_add("compute_hausdorff_distance[two_bad:dtype,spacing]",
     lambda: metrics.compute_hausdorff_distance(ONEHOT.double(), ONEHOT, spacing=-1))
_add("compute_average_surface_distance[two_bad:shape,spacing]",
     lambda: metrics.compute_average_surface_distance(ONEHOT, ONEHOT[:1], spacing=-1))
_add("compute_surface_dice[two_bad:thresholds,spacing]", lambda: metrics.compute_surface_dice(ONEHOT, ONEHOT, [1.0], spacing=-1))
_add("surface_metrics[two_bad:tolerance,spacing]", lambda: metrics.surface_metrics(U8B, U8B, 3, tolerance=-1, spacing=-1))
_add("surface_metrics[two_bad:dtype,spacing]", lambda: metrics.surface_metrics(U8B.float(), U8B, 3, spacing=-1))

# ---- postprocess
for _name in ("distance_transform_edt", "signed_distance"):
    _each(f"{_name}.sampling", _SPACINGS, lambda v, f=getattr(postprocess, _name): f(U8B, sampling=v))
    _add(f"{_name}[two_bad:sampling,label]", lambda f=getattr(postprocess, _name): f(U8B, sampling=-1, label=1.5))
for _name in ("ball_erosion", "ball_dilation", "ball_opening", "ball_closing"):
    _each(f"{_name}.sampling", TRIPLES, lambda v, f=getattr(postprocess, _name): f(U8, 2.0, sampling=v))
    _add(f"{_name}[two_bad:radius,sampling]", lambda f=getattr(postprocess, _name): f(U8, -1.0, sampling=-1))
_each("extract_implant.sampling", TRIPLES, lambda v: postprocess.extract_implant(U8, U8, opening_radius=2.0, sampling=v))
_add("extract_implant[two_bad:opening_radius,sampling]",
     lambda: postprocess.extract_implant(U8, U8, opening_radius=-1, sampling=-1))
_add("extract_implant[cpu]", lambda: postprocess.extract_implant(U8, U8))
_add("label[cpu]", lambda: postprocess.label(U8))
_add("keep_largest_connected_component[cpu]", lambda: postprocess.keep_largest_connected_component(U8))
_add("remove_small_objects[cpu]", lambda: postprocess.remove_small_objects(U8, 4))
for _name in ("binary_erosion", "binary_dilation", "binary_opening", "binary_closing", "binary_fill_holes"):
    _add(f"{_name}[cpu]", lambda f=getattr(postprocess, _name): f(U8))
_add("distance_transform_edt[sampling_one_is_unit]", lambda: postprocess.distance_transform_edt(U8, sampling=(1, 1, 1)))

# ---- transforms
for _arg in ("degrees", "translation", "max_displacement", "spacing"):
    _each(f"RandomSpatial.{_arg}", TRIPLES, lambda v, a=_arg: _spatial(**{a: v}) and None)
_add("RandomSpatial[two_bad:scales,degrees]", lambda: _spatial(scales=(0, 1), degrees=-1))
_add("RandomSpatial[two_bad:degrees,translation]", lambda: _spatial(degrees=-1, translation="abc"))
_add("RandomSpatial[two_bad:max_displacement,spacing]", lambda: _spatial(max_displacement=NAN, spacing=0))
_add("RandomSpatial[two_bad:locked_borders,spacing]", lambda: _spatial(locked_borders=3, spacing=0))
_each("RandomSpatial.apply.out", _outs((2, 1, 4, 5, 6), torch.float32), lambda v: _spatial().apply(X5, out=v))
_add("RandomSpatial.apply[two_bad:dtype,out]", lambda: _spatial().apply(X5.double(), out=[0.0]))
_add("SaltAndPepper.apply[cpu]", lambda: transforms.SaltAndPepper(seed=1).apply(X5, out=[0.0]))
_add("SkullRandomHole.apply[cpu]", lambda: transforms.SkullRandomHole(seed=1).apply(X5, x=[0.0]))
_add("FlapRecTransform.apply[cpu]",
     lambda: transforms.FlapRecTransform(transforms.SkullRandomHole(seed=1), transforms.SaltAndPepper(seed=1)).apply(X5))


def outcome(call):
    """``[class name, message]`` of what the call raises; a call that returns is recorded as such."""
    try:
        call()
    except Exception as e:                                  # noqa: BLE001 -- the class is what is being recorded
        return [type(e).__name__, str(e)]
    return ["", "returned"]


@functools.lru_cache(maxsize=None)
def _expected():
    with open(FIXTURE) as fh:
        return json.load(fh)


def test_table_and_fixture_hold_the_same_rows():
    assert sorted(_expected()) == sorted(ROWS)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_refusal_is_unchanged(name):
    assert outcome(ROWS[name]) == _expected()[name]


if __name__ == "__main__":
    with open(FIXTURE, "w") as fh:
        json.dump({name: outcome(ROWS[name]) for name in sorted(ROWS)}, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"recorded {len(ROWS)} rows in {FIXTURE}")
