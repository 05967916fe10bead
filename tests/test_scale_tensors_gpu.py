"""ops.scale_tensors / ops.unscale_tensors (ctu_scale_tensors, ctu_unscale_tensors; csrc/optim.hip) on their own: bit-equal
to torch's multiply over a list that needs a second 64-tensor launch and a tensor past the 2048-block grid cap, and every
way the non-finite flag is set or left alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 63, 257, 4099]
N_SMALL = 65                                    # tensor 64 opens the second chunk of 64
BIG = 2 * 1024 * 1024 + 1029                    # ceil(BIG / 1024) = 2050 blocks > the cap of 2048: the stride loop takes > 1 trip
BIG_AT = N_SMALL                                # index of the large tensor among the tensors that are not None
NONE_AT = 7                                     # where the list carries a None, which ops drops


@pytest.fixture(scope="module")
def base():
    """The unscaled tensors, made once and never written: every test scales clones."""
    g = torch.Generator().manual_seed(11)
    ts = [torch.randn(SIZES[i % len(SIZES)], generator=g) * 10.0 ** (i % 7 - 3) for i in range(N_SMALL)]
    ts.append(torch.randn(BIG, generator=g) * 37.0)
    return [t.cuda() for t in ts]


def _clones(base):
    return [t.clone() for t in base]


def _with_none(ts):
    return ts[:NONE_AT] + [None] + ts[NONE_AT:]


def _flag(v=0.0):
    return torch.full((1,), v, dtype=torch.float32, device="cuda")


def _bit_equal(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (i, a.numel(), (a - b).abs().max().item())


@pytest.mark.parametrize("s", [0.5, 1.0 / 3.0, 1e-4])
def test_scale_is_torchs_float32_multiply(base, s):
    from ctunet_amd import ops
    ts, flag = _clones(base), _flag()
    ops.scale_tensors(_with_none(ts), s, flag)
    _bit_equal(ts, [t * torch.tensor(s, dtype=torch.float32) for t in base])
    assert flag.item() == 0.0                                            # finite data leaves the flag alone


@pytest.mark.parametrize("scale", [65536.0, 3.0, 1000.0])
def test_unscale_multiplies_by_grad_scalers_reciprocal(base, scale):
    from ctunet_amd import ops
    ts, flag = _clones(base), _flag()
    sc = torch.full((1,), scale, dtype=torch.float32, device="cuda")
    ops.unscale_tensors(_with_none(ts), sc, flag)
    _bit_equal(ts, [t * sc.double().reciprocal().float() for t in base])
    assert flag.item() == 0.0 and sc.item() == scale


def test_a_set_flag_is_never_cleared(base):
    from ctunet_amd import ops
    ts, flag = _clones(base), _flag(1.0)
    ops.scale_tensors(_with_none(ts), 0.5, flag)
    assert flag.item() == 1.0
    ops.unscale_tensors(_with_none(ts), torch.full((1,), 2.0, device="cuda"), flag)
    assert flag.item() == 1.0
    _bit_equal(ts, [t * 0.5 * 0.5 for t in base])


def _poisoned(base, which, index, value):
    ts = _clones(base)
    ts[which][index] = value
    return ts


@pytest.mark.parametrize("which,index,value,s", [
    (64, 2000, float("inf"), 0.5),               # one inf in the first tensor of the second chunk
    (BIG_AT, BIG - 1, float("nan"), 0.5),        # one NaN in the last element of the large tensor (its last trip)
    (BIG_AT, 12345, 3e38, 2.0),                  # finite before, overflows in the multiply itself
], ids=["inf-second-chunk", "nan-last-element", "overflow-in-multiply"])
def test_non_finite_values_set_the_flag(base, which, index, value, s):
    from ctunet_amd import ops
    ts, flag = _poisoned(base, which, index, value), _flag()
    ops.scale_tensors(_with_none(ts), s, flag)
    assert flag.item() == 1.0
    _bit_equal(ts[:64], [t * torch.tensor(s, dtype=torch.float32) for t in base[:64]])   # and everything is still scaled
    ts, flag = _poisoned(base, which, index, value), _flag()
    ops.unscale_tensors(_with_none(ts), torch.full((1,), 1.0 / s, device="cuda"), flag)
    assert flag.item() == 1.0
    assert not torch.isfinite(ts[which][index])


def test_without_a_flag_the_values_are_still_scaled(base):
    from ctunet_amd import ops
    ts = _poisoned(base, 64, 0, float("inf"))
    ops.scale_tensors(_with_none(ts), 1.0 / 3.0, None)
    want = [t * torch.tensor(1.0 / 3.0, dtype=torch.float32) for t in base]
    _bit_equal(ts[:64] + ts[65:], want[:64] + want[65:])
    assert torch.isinf(ts[64][0]) and torch.equal(ts[64][1:], want[64][1:])
