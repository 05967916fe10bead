"""Flap-reconstruction augmentation, host side (no GPU): the NumPy Philox against its known answers, the reference's hole
masks (tests/golden/shape3d.npz, from utilities.shape_3d) against the restated integer rules, the hole-size range against
np.random.randint's, argument validation, the exports and the two refusing datasets."""
import os

import numpy as np
import pytest
import torch

import augment_ref as R
from util import GOLDEN


def test_philox_known_answers():
    assert [int(v) for v in R.philox(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    r = R.philox(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)
    assert [int(v) for v in r] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # vectorised form == scalar form
    c = np.arange(5, dtype=np.uint32)
    v = R.philox(c, 1, 2, 3, 7, 9)
    for i in range(5):
        assert [int(x[i]) for x in v] == [int(x) for x in R.philox(i, 1, 2, 3, 7, 9)]


def test_uniform_and_integer_draws():
    assert R.unif(0) == 0.0 and R.unif(0xFFFFFFFF) == np.float32(1 - 2.0 ** -24)
    assert R.draw_int(0, 5, 10) == 5 and R.draw_int(0xFFFFFFFF, 5, 10) == 14


def test_golden_masks_match_the_integer_rules():
    z = np.load(os.path.join(GOLDEN, "shape3d.npz"))
    n = len([k for k in z.files if k.endswith("_dims")])
    assert n >= 90
    for i in range(n):
        dims = tuple(int(v) for v in z[f"c{i}_dims"])
        ref = np.unpackbits(z[f"c{i}_inside"])[:int(np.prod(dims))].reshape(dims).astype(bool)
        got = R.shape_mask(dims, tuple(int(v) for v in z[f"c{i}_centre"]), int(z[f"c{i}_size"]), str(z[f"c{i}_shape"]))
        assert np.array_equal(got, ref), (i, dims, str(z[f"c{i}_shape"]))


@pytest.mark.parametrize("dims", [(224, 304, 304), (64, 128, 128), (37, 45, 53), (5, 5, 5), (3, 9, 4), (1, 1, 1), (2, 50, 7)])
def test_size_range_matches_numpy(dims):
    from ctunet_amd.transforms import size_range
    lo, hi = size_range(dims)
    min_r = np.min(dims) // 5 - 1
    max_r = np.max([min_r, np.max(dims) // 3.5])
    draws = np.random.RandomState(0).randint(min_r, max_r, size=4000)
    assert draws.min() == lo and draws.max() == hi - 1


def test_empty_size_range_raises_like_numpy():
    from ctunet_amd.transforms import randint_bounds
    for lo, hi in ((3, 3), (4, 2.0), (0, 0.0)):
        with pytest.raises(ValueError):
            np.random.randint(lo, hi)
        with pytest.raises(ValueError):
            randint_bounds(lo, hi)
    assert randint_bounds(-1, 0.0) == (-1, 0)


def test_argument_validation():
    from ctunet_amd.transforms import FlapRecTransform, SaltAndPepper, SkullRandomHole
    for bad in (-0.1, 1.5, "1", True):
        with pytest.raises(ValueError):
            SkullRandomHole(p=bad)
        with pytest.raises(ValueError):
            SaltAndPepper(p=bad)
    with pytest.raises(ValueError):
        SaltAndPepper(noise_density=2.0)
    with pytest.raises(ValueError):
        SaltAndPepper(salt_ratio=-1)
    with pytest.raises(ValueError):
        SaltAndPepper(keyws=("image",), apply_to=(True, False))
    with pytest.raises(ValueError):
        SkullRandomHole(shapes=())
    with pytest.raises(ValueError):
        SkullRandomHole(shapes=("sphere", "cone"))
    with pytest.raises(ValueError):
        SkullRandomHole(seed=-1)
    with pytest.raises(ValueError):
        SkullRandomHole(seed=2 ** 64)
    with pytest.raises(TypeError):
        FlapRecTransform(SaltAndPepper(), SaltAndPepper())
    with pytest.raises(ValueError):
        FlapRecTransform(SkullRandomHole(), SaltAndPepper(apply_to=(True, True)))
    with pytest.raises(TypeError):
        SkullRandomHole()({"image": np.zeros((4, 4, 4))})
    # the batch form refuses host tensors (no CPU fallback) and wrong layouts
    h = SkullRandomHole(seed=1)
    with pytest.raises(RuntimeError):
        h.apply(torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(ValueError):
        h.apply(torch.zeros(4, 4, 4))
    with pytest.raises(RuntimeError):
        h.last_params


def test_state_dict_without_a_device():
    from ctunet_amd.transforms import SaltAndPepper, SkullRandomHole
    h = SkullRandomHole(seed=11)
    assert h.state_dict() == {"seed": 11, "counter": 0}
    h.load_state_dict({"seed": 12, "counter": 40})
    assert h.state_dict() == {"seed": 12, "counter": 40}
    s = SaltAndPepper(noise_density=0.05, seed=3)
    assert s.state_dict() == {"seed": 3, "counter": 0, "noise_density": float(np.float32(0.05))}
    s.noise_density = 0.25
    assert s.noise_density == 0.25
    assert SkullRandomHole().seed != SkullRandomHole().seed          # fresh entropy per unseeded instance


def test_seedless_instances_leave_global_generators_alone():
    from ctunet_amd.transforms import SkullRandomHole
    torch.manual_seed(5)
    a = torch.rand(3)
    torch.manual_seed(5)
    SkullRandomHole()
    assert torch.equal(torch.rand(3), a)


def test_exports():
    import ctunet_amd
    from ctunet_amd import transforms
    for name in ("SkullRandomHole", "SaltAndPepper", "FlapRecTransform", "flap_rec_transform",
                 "FlapRecWShapePrior2OTrainDataset", "FlapRec2OTrainDataset"):
        assert hasattr(ctunet_amd, name) and name in ctunet_amd.__all__, name
    t = ctunet_amd.flap_rec_transform
    assert isinstance(t, transforms.FlapRecTransform)
    assert t.hole.double_output and t.hole.p == 1.0
    assert t.noise.p == 0.5 and t.noise.salt_ratio == 0.1 and t.noise.decay
    assert t.noise.noise_density == float(np.float32(0.05))


def test_refusing_datasets():
    from ctunet_amd import datasets
    with pytest.raises(NotImplementedError, match=r"\.long\(\)"):
        datasets.FlapRecTrainDataset()
    with pytest.raises(NotImplementedError, match="torchio"):
        datasets.FlapRecWShapePriorTrainDataset()


def test_dataset_validation():
    from ctunet_amd import datasets
    from ctunet_amd.transforms import FlapRecTransform, SkullRandomHole
    with pytest.raises(ValueError):
        datasets.FlapRecWShapePrior2OTrainDataset([torch.zeros(4, 4, 4)], None)
    with pytest.raises(ValueError):
        datasets.FlapRec2OTrainDataset([torch.zeros(4, 4)])
    with pytest.raises(ValueError):
        datasets.FlapRec2OTrainDataset([torch.zeros(4, 4, 4)], transform=FlapRecTransform(SkullRandomHole()))
