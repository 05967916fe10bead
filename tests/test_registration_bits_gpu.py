"""The registration kernels reproduce, bit for bit, what tests/golden/registration_bits.npz holds: matrix, inverse and history
of the rigid and similarity optimisers on the analytic fixtures, and the sums of single accumulations at sizes that put the
forward/backward boundary inside a wave and across a block edge.

The file was recorded on an MI355X by tests/golden/record_registration_bits.py from the library built at commit a488337,
the last one with separate rigid (reg_*) and similarity (sim_*) kernels -- never from the code under test.  Every array is
the int64 view of the float64 (or the int64) the wrappers return, compared with torch.equal.  A toolchain change that moves
the device's sin, cos, exp or cbrt moves these bits too: re-record then from a build known to be good (one that passes the
restatement tests of test_registration_gpu.py and test_similarity_gpu.py), with the script above."""
import os

import numpy as np
import pytest
import torch

import registration_ref as G
import similarity_ref as S
import test_registration_gpu as RG
import test_similarity_gpu as SG
from test_registration_cpu import CASES, FIXED_ORIGIN, FIXED_SPACING, fixed_side, fixture_case
from test_similarity_cpu import MOVING_ORIGIN, MOVING_SPACING, SCENES, scene

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "registration_bits.npz")
FIXED_KW = dict(spacing=FIXED_SPACING, origin=FIXED_ORIGIN)
BOUNDS = (None, 3.0)


def _bits(v):
    """The int64 view of a device or host float64 array or number; integers as int64."""
    if isinstance(v, torch.Tensor):
        v = v.cpu().numpy()
    a = np.ascontiguousarray(v)
    return a.astype(np.int64) if a.dtype.kind in "iu" else a.astype(np.float64).view(np.int64)


def _result(name, r):
    return {f"{name}.{key}": _bits(getattr(r, key)) for key in ("matrix", "inverse", "history")}


def _sums(name, got, keys):
    return {f"{name}.{key}": _bits(got[key]) for key in keys}


def rigid():
    """register_points on cases 1-5: the restatement's 30 iterations from the centroid start, each case's own bound."""
    from ctunet_amd import registration as reg
    fd = RG._dev(fixed_side()[1])
    out = {}
    for case in sorted(CASES):
        c = fixture_case(case)
        out.update(_result(f"case{case}", reg.register_points(RG._dev(c["points"]), fd, init=RG._dev(c["init"]), iterations=30,
                                                               max_distance=c["bound"], **FIXED_KW)))
    return out


def similarity():
    """register(model="similarity") on scenes 1-5, scene 1 with the directed cost, and scene 1 rigid with the symmetric one."""
    out = {}
    for k in sorted(SCENES):
        out.update(_result(f"scene{k}", SG._register(k)))
    out.update(_result("scene1_directed", SG._register(1, symmetric=False)))
    out.update(_result("scene1_rigid_symmetric", SG._register(1, model="rigid", symmetric=True)))
    return out


def accumulate():
    """One rigid accumulation at P = 1, 65, 257 at both matrices of test_registration_gpu, without and with a bound."""
    from ctunet_amd import registration as reg
    fd = RG._dev(fixed_side()[1])
    general = G.rigid((0.05, -0.03, 0.04), (1.3, -0.7, 0.9), (30.0, 34.0, 36.0)) @ fixture_case(2)["init"]
    out = {}
    for P in (1, 65, 257):
        pd = RG._dev(RG._points(P))
        for name, M in (("dyadic", RG.DYADIC), ("general", general)):
            for bound in BOUNDS:
                got = reg.accumulate(pd, fd, RG._dev(M), max_distance=bound, **FIXED_KW)
                out.update(_sums(f"P{P}.{name}.{bound}", got, ("H", "b", "cost", "count", "pivot")))
    return out


def accumulate_similarity():
    """One similarity accumulation at (P, Q) = (1, 0), (65, 191), (257, 255), both dof, both matrices of test_similarity_gpu,
    without and with a bound."""
    from ctunet_amd import registration as reg
    c = scene(1)
    fd, gd = SG._dev(fixed_side()[1]), SG._dev(c["field"])
    general = G.rigid((0.05, -0.03, 0.04), (1.3, -0.7, 0.9), (30.0, 34.0, 36.0)) @ S.scale_about((30.0, 34.0, 36.0), 1.05) @ c["init"]
    out = {}
    for P, Q in ((1, 0), (65, 191), (257, 255)):
        pts, fpts = SG._sets(P, Q)
        half = dict(fixed_points=SG._dev(fpts), moving_field=gd, moving_spacing=MOVING_SPACING, moving_origin=MOVING_ORIGIN) if Q else {}
        for name, M in (("dyadic", SG.DYADIC), ("general", general)):
            for model in ("rigid", "similarity"):
                for bound in BOUNDS:
                    got = reg.accumulate_similarity(SG._dev(pts), fd, SG._dev(M), model=model, max_distance=bound, **FIXED_KW, **half)
                    out.update(_sums(f"P{P}.Q{Q}.{name}.{model}.{bound}", got,
                                     ("H", "b", "cost", "count", "count_backward", "pivot")))
    return out


GROUPS = (rigid, similarity, accumulate, accumulate_similarity)


@pytest.mark.parametrize("group", GROUPS, ids=[g.__name__ for g in GROUPS])
def test_the_library_reproduces_the_recorded_bits(group):
    got = {f"{group.__name__}/{k}": v for k, v in group().items()}
    with np.load(GOLDEN) as golden:
        recorded = {k: golden[k] for k in golden.files if k.startswith(group.__name__ + "/")}
    assert sorted(recorded) == sorted(got)
    differ = [k for k in sorted(got) if recorded[k].dtype != np.int64 or
              not torch.equal(torch.from_numpy(got[k]), torch.from_numpy(recorded[k]))]
    assert not differ, differ
