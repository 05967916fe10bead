"""SkullRandomDefect and RandomDilate without a GPU: the restated rule (tests/defect_ref.py) keeps every defect inside its
box and every lattice read inside the lattice, reduces to the plain float64 ball, draws what the rule says, and its L1-ball
dilation is scipy's iterated cross; the classes resolve the same geometry and refuse what the rule refuses."""
import numpy as np
import pytest

import defect_ref as R

CASES = [((37, 45, 53), (1.0, 1.0, 1.0), 150), ((40, 48, 56), (1.6, 0.9, 0.9), 120), ((64, 128, 128), (0.8, 0.45, 0.45), 30)]


@pytest.mark.parametrize("dims,spacing,draws", CASES)
def test_mask_inside_box_and_lattice_in_bounds(dims, spacing, draws):
    bone = R.shell(dims)
    geo = R.geometry(dims, spacing)
    for (w, i, f), g in zip(R.lattice_cells(dims, geo, spacing), geo["G"]):
        assert i.min() >= 0 and i.max() + 1 <= g - 1 and f.min() >= 0.0 and f.max() < 1.0 and g <= 64
    total = int(bone.sum())
    for seq in range(draws):
        d = R.draw(4711, seq, bone, geo, spacing)
        assert d["cut"] and bone[d["centre"]] and 3 <= d["n_balls"] <= 8 and len(d["balls"]) == d["n_balls"]
        ins = R.inside_mask(dims, d["balls"], d["lattice"], geo, spacing)
        (lz, ly, lx), (hz, hy, hx) = d["box"]
        boxed = np.zeros(dims, bool)
        boxed[lz:hz + 1, ly:hy + 1, lx:hx + 1] = True
        assert not (ins & ~boxed).any(), (seq, d["box"])
        assert 0 < (ins & bone).sum() < total, seq
        assert min(lz, ly, lx) >= 0 and hz < dims[0] and hy < dims[1] and hx < dims[2]


def test_plain_ball():
    dims, spacing = (30, 36, 41), (1.5, 0.8, 1.1)
    bone = R.shell(dims)
    geo = R.geometry(dims, spacing, radius=(7.0, 9.0), roughness=0.0)
    for seq in range(5):
        d = R.draw(3, seq, bone, geo, spacing, balls=(1, 1))
        assert d["n_balls"] == 1 and d["parents"] == []
        (cz, cy, cx, r), = d["balls"]
        assert (cz, cy, cx) == tuple(np.float64(c) * s for c, s in zip(d["centre"], spacing)) and 7.0 <= r < 9.0
        z, y, x = np.indices(dims).astype(np.float64)
        dz, dy, dx = z * spacing[0] - cz, y * spacing[1] - cy, x * spacing[2] - cx
        ball = ((dz * dz + dy * dy) + dx * dx) <= r * r
        assert np.array_equal(R.inside_mask(dims, d["balls"], d["lattice"], geo, spacing), ball)


def test_draw_statistics():
    dims = (20, 24, 30)
    bone = R.shell(dims)
    geo = R.geometry(dims)
    ks, first_parent = set(), set()
    for seq in range(400):
        d = R.draw(99, seq, bone, geo, balls=(2, 12), spread=1.3, shrink=(0.4, 1.0))
        ks.add(d["n_balls"])
        assert len(d["parents"]) == d["n_balls"] - 1 and all(0 <= i < j for j, i in enumerate(d["parents"], 1))
        if d["n_balls"] >= 4:
            first_parent.add(d["parents"][2])
        for (cz, cy, cx, r), i in zip(d["balls"][1:], d["parents"]):
            pr = d["balls"][i][3]
            assert 0.4 * pr <= r <= pr
            assert all(abs(c - q) <= 1.3 * pr for c, q in zip((cz, cy, cx), d["balls"][i][:3]))
        assert geo["radius"][0] <= d["balls"][0][3] < geo["radius"][1]
    assert ks == set(range(2, 13)) and first_parent == {0, 1, 2}
    lat = np.concatenate([R.draw(99, s, bone, geo)["lattice"].ravel() for s in range(50)])
    assert -1.0 <= lat.min() < -0.99 and 0.99 < lat.max() < 1.0 and abs(lat.mean()) < 0.02
    assert not any(R.draw(5, s, bone, geo, p=0.0)["cut"] for s in range(20))
    assert abs(sum(R.draw(5, s, bone, geo, p=0.5)["apply"] for s in range(400)) - 200) < 50      # 5 sigma


def test_empty_sample_has_no_chain():
    geo = R.geometry((12, 14, 18))
    d = R.draw(1, 0, np.zeros((12, 14, 18), bool), geo)
    assert d["apply"] and not d["cut"] and d["centre"] == (-1, -1, -1) and d["balls"] == []
    assert d["box"] == ((0, 0, 0), (-1, -1, -1)) and not d["record"][16:].any()


@pytest.mark.parametrize("k", [1, 2, 3])
def test_l1_ball_is_scipys_iterated_cross(k):
    from scipy import ndimage
    g = np.random.RandomState(k)
    for dims, density in (((9, 10, 11), 0.02), ((17, 5, 33), 0.05), ((4, 4, 4), 0.1)):
        bone = g.rand(*dims) < density
        bone[0, 0, 0] = bone[-1, -1, -1] = True               # the borders
        ref = ndimage.binary_dilation(bone, ndimage.generate_binary_structure(3, 1), iterations=k, border_value=0)
        assert np.array_equal(R.dilate_l1(bone, k), ref)


def test_classes_resolve_the_same_geometry():
    from ctunet_amd.transforms import SkullRandomDefect
    for dims, spacing, _ in CASES:
        got = SkullRandomDefect(spacing=spacing).geometry(dims)
        geo = R.geometry(dims, spacing)
        assert (got["radius"], got["roughness"], got["roughness_scale"], got["lattice"]) == \
               (geo["radius"], geo["amp"], geo["scale"], geo["G"])
    got = SkullRandomDefect(radius=(5, 9), roughness=0, roughness_scale=4.5).geometry((37, 45, 53))
    geo = R.geometry((37, 45, 53), radius=(5, 9), roughness=0, roughness_scale=4.5)
    assert (got["radius"], got["roughness"], got["roughness_scale"], got["lattice"]) == ((5.0, 9.0), 0.0, 4.5, geo["G"])


def test_constructor_errors():
    from ctunet_amd.transforms import RandomDilate, SkullRandomDefect
    SkullRandomDefect(balls=(1, 12), spread=0, shrink=(1, 1), roughness=0)                     # the edges are allowed
    for kw in (dict(balls=(0, 3)), dict(balls=(4, 3)), dict(balls=(3, 13)), dict(spread=-0.1), dict(shrink=(0, 0.5)),
               dict(shrink=(0.9, 0.5)), dict(shrink=(0.5, 1.1)), dict(roughness=-1.0), dict(radius=(0, 5)),
               dict(radius=(-2, 5)), dict(radius=(6, 5)), dict(roughness_scale=0), dict(p=1.5), dict(seed=-1)):
        with pytest.raises(ValueError):
            SkullRandomDefect(**kw)
    with pytest.raises(ValueError):                           # G_x = floor(53 / 0.8) + 2 = 68 > 64
        SkullRandomDefect(roughness_scale=0.8).geometry((37, 45, 53))
    SkullRandomDefect(roughness_scale=0.86).geometry((37, 45, 53))                             # 63
    with pytest.raises(ValueError):                           # min(dims) // 5 - 1 = 0: no radius
        SkullRandomDefect().geometry((9, 10, 11))
    for kw in (dict(iterations=0), dict(iterations=4), dict(iterations=1.0), dict(p=-0.1)):
        with pytest.raises(ValueError):
            RandomDilate(**kw)
    assert RandomDilate().iterations == 1 and RandomDilate().p == 0.3
