"""What a spacing, origin, grid or ``out=`` argument of a volume wrapper may be: one walk each, shared by ``resample``,
``preprocess``, ``registration``, ``mesh`` and ``transforms``.

The wrappers agree on the rule and differ in wording, in ``TypeError`` versus ``ValueError`` and in a few admissions (a
tensor, ``None``, the float32 test).  A module states those as data, a ``Triple`` or ``Grid`` next to its other constants,
and the walk reads them; nothing here knows which module calls.  Messages are ``str.format`` templates; ``{v!r}`` is the
argument as given (a tensor as its list, where tensors are admitted) and every other name is the caller's keyword.
"""
from __future__ import annotations

import ctypes as C
import math
from numbers import Integral, Real
from typing import NamedTuple, Optional, Tuple

import torch

ANY, NOT_NEGATIVE, POSITIVE = 0, 1, 2


class Triple(NamedTuple):
    """How a module takes "a number or a (z, y, x) triple": ``shape`` is raised (as ``shape_error``) for anything that is
    not one real number or three, ``value`` (as ``ValueError``) for an element that is not finite or misses ``sign``."""
    shape: str
    value: str
    sign: int = ANY
    shape_error: type = ValueError
    optional: bool = True        # None stays None: the entry point's default
    tensors: bool = True         # a tensor is read as its list
    float32: bool = False        # finiteness and sign are tested on the value rounded to float32


def triple(v, rule: Triple, **names) -> Optional[Tuple[float, float, float]]:
    """Three floats from a number or a triple, or the refusal ``rule`` words."""
    if v is None and rule.optional:
        return None
    if rule.tensors and isinstance(v, torch.Tensor):
        v = v.tolist()
    if isinstance(v, Real) and not isinstance(v, bool):
        vals = (v, v, v)
    else:
        try:
            vals = tuple(v)
        except TypeError:
            raise rule.shape_error(rule.shape.format(v=v, **names)) from None
        if len(vals) != 3 or any(isinstance(s, bool) or not isinstance(s, Real) for s in vals):
            raise rule.shape_error(rule.shape.format(v=v, **names))
    for s in vals:
        t = C.c_float(float(s)).value if rule.float32 else s
        if not math.isfinite(t) or (t < 0 and rule.sign != ANY) or (t == 0 and rule.sign == POSITIVE):
            raise ValueError(rule.value.format(v=v, **names))
    return tuple(float(s) for s in vals)


class Grid(NamedTuple):
    """How a module takes a (D, H, W) grid: ``shape`` / ``integers`` are raised (as ``shape_error``) for what is not
    iterable / not three integers, ``side`` for a side below 1 or above ``max_side``, ``voxels`` for ``max_voxels`` or more."""
    side: str
    voxels: str = ""
    shape: str = ""
    integers: str = ""
    max_side: Optional[int] = None
    max_voxels: Optional[int] = 1 << 31
    shape_error: type = ValueError


def grid(v, rule: Grid, **names) -> Tuple[int, int, int]:
    """Three ints from a (D, H, W) triple of integers, or the refusal ``rule`` words (``{vals}``: the triple as a tuple)."""
    try:
        vals = tuple(v)
    except TypeError:
        raise rule.shape_error(rule.shape.format(v=v, **names)) from None
    if len(vals) != 3 or any(isinstance(s, bool) or not isinstance(s, Integral) for s in vals):
        raise rule.shape_error(rule.integers.format(v=v, **names))
    if any(s < 1 or (rule.max_side is not None and s > rule.max_side) for s in vals):
        raise ValueError(rule.side.format(v=v, vals=vals, **names))
    if rule.max_voxels is not None and vals[0] * vals[1] * vals[2] >= rule.max_voxels:
        raise ValueError(rule.voxels.format(v=v, vals=vals, **names))
    return tuple(int(s) for s in vals)


def check_out(out, shape, dtype, device, who: str, type_error: type = ValueError) -> None:
    """Refuse an ``out=`` that is not a contiguous ``dtype`` tensor of ``shape`` on ``device``; None passes."""
    if out is None:
        return
    if not isinstance(out, torch.Tensor):
        raise type_error(f"{who}: out must be a tensor, got {type(out).__name__}")
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}, got "
                         f"{out.dtype} {tuple(out.shape)} on {out.device}{'' if out.is_contiguous() else ', not contiguous'}")
