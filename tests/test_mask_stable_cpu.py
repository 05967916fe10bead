"""The cases of tests/mask_stable.py stay mask-stable in the oracle ALONE (no GPU): conditions on the inputs of
tests/test_mask_stable_gpu.py, not measurements of the HIP path.  A case that misses one is unfit -- pick another
multiplier or seed for it in mask_stable.CASES -- and says nothing about a kernel.  Figures: profiles/mask_stable_gates.md."""
import pytest
import torch

import mask_stable as MS


@pytest.mark.parametrize("cid", MS.IDS)
def test_case_is_mask_stable_in_the_oracle_alone(cid):
    name, kw, shape, mult, seed = MS.BY_ID[cid]
    assert mult <= 16                                  # pre-activations within a few tens: a bf16 ulp of one stays below 1
    r64, r32 = MS.reference(cid, "fp64"), MS.reference(cid, "fp32")
    m64, m32 = r64["margin"][0], r32["margin"][0]
    err, where = MS.worst_error(r32["grads"], r32["dx"], r64)
    print(f"{cid} mult {mult:g} seed {seed}: fp64 margin {m64:.3f} at {r64['margin'][1]} (needs {MS.min_margin(cid)}), ATen fp32 "
          f"margin {m32:.3f}, worst ATen fp32 gradient error {err:.2e} of the largest entry ({where})")
    # the smallest sign(beta) * (BatchNorm output) of the train-mode forward: no ReLU mask can flip, with room for 16-bit
    # rounding where the case runs in 16 bits
    assert m64 >= MS.min_margin(cid)
    assert m32 > 0
    # ... and ATen in fp32 agrees with fp64 as two smooth evaluations do (3e-6 .. 1.2e-4 measured).  More means the case is
    # not stable after all: a max-pool window whose two largest entries lie within fp32 rounding routes its gradient
    # elsewhere (recAE_v2_fixed, batch 2, at mult 8 / seed 8: margin 1.56, ATen fp32 dx 1.2e-3 off -- hence mult 10 there)
    assert err < 1e-3
    # the rule itself, on the state the tests load: |beta| = mult |gamma|, 0.5 <= |gamma| <= 1.5, and in every BatchNorm
    # wider than one channel at least one channel off and one on
    sd = MS.state(cid)
    bns = [k[:-len("running_mean")] for k in sd if k.endswith(".running_mean")]
    assert len(bns) >= 18
    for p in bns:
        gam, beta = sd[p + "weight"], sd[p + "bias"]
        assert bool((gam.abs() >= 0.5).all()) and bool((gam.abs() <= 1.5).all()), p
        assert torch.allclose(beta.abs(), mult * gam.abs(), rtol=1e-6, atol=0), p
        if gam.numel() > 1:
            assert bool((beta < 0).any()) and bool((beta > 0).any()), p
        assert bool((sd[p + "running_var"] >= 0.5).all()) and float(sd[p + "running_mean"].abs().max()) > 0, p
    # the outputs leave the 0.5 +- 0.02 band of default initialisation: the head and loss kernels see a real range
    assert max(float(o.max() - o.min()) for o in r64["outs"]) > 0.15


def test_states_differ_between_layers_of_equal_width():
    """What the default initialisation hides: two BatchNorms of one width carry different gamma, beta and statistics, so a
    layer that is handed its sibling's vector computes something else."""
    sd = MS.state(MS.IDS[0])
    by_width = {}
    for k, v in sd.items():
        if k.endswith(".running_mean"):
            by_width.setdefault(v.numel(), []).append(k[:-len("running_mean")])
    assert any(len(v) > 1 for v in by_width.values())
    for ps in by_width.values():
        for a in ps:
            for b in ps:
                if a < b:
                    for f in ("weight", "bias", "running_mean", "running_var"):
                        assert not torch.allclose(sd[a + f], sd[b + f], atol=1e-3), (a, b, f)


def test_oracle_run_leaves_the_state_alone_and_is_cached():
    cid = MS.IDS[0]
    before = {k: v.clone() for k, v in MS.state(cid).items()}
    r = MS.reference(cid, "fp32")
    assert r is MS.reference(cid, "fp32")
    for k, v in MS.state(cid).items():
        assert torch.equal(v, before[k]), k
    moved = [k for k, v in r["buffers"].items() if "running" in k and not torch.equal(v, before[k])]
    assert len(moved) == sum("running" in k for k in before)          # every BatchNorm of the train-mode forward moved
    assert all(int(v) == 1 for k, v in r["buffers"].items() if "num_batches" in k)
