"""ctunet_amd.resample.affine_resample on the GPU: every comparison with the restated rule (tests/affine_ref.py) is bit-equal."""
import numpy as np
import pytest
import torch

import affine_ref as A
import registration_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the input grid and its world frame
IN_SHAPE, SPACING, ORIGIN = (10, 12, 50), (1.5, 1.25, 1.0), (-1.0, 2.0, -3.0)
# output grids where the store path changes: a tile is 4 planes x 4 rows x 16 chunks of 16 bytes (64 float32 / 128 int16 / 256
# uint8 voxels along x); odd rows shift every row's chunk grid, 64 / 65 sit on a float32 tile edge, 260 past a uint8 one
OUT_SHAPES = ((3, 5, 130), (9, 7, 64), (9, 7, 65), (1, 1, 1), (2, 3, 260))
OUT_ORIGIN = (-0.7, 2.3, -2.6)
CENTRE = (5.75, 8.9, 21.5)


def _out_spacing(shape):
    """The output grid spans about the input's world box whatever its voxel count."""
    return tuple(round(e / n, 3) for e, n in zip((13.0, 13.0, 48.0), shape))


def _matrices():
    swap = np.array([[1.0, 0, 0, 0], [0, 0, 1.0, -14.0], [0, -1.0, 0, 31.0], [0, 0, 0, 1.0]])     # y_in = x_out - 14, x_in = 31 - y_out
    far = np.eye(4)
    far[:3, 3] = (9.3, 8.1, 30.7)
    nan = np.eye(4)
    nan[1, 2] = np.nan
    return {"identity": np.eye(4), "axis_swap": swap,
            "rot17": G.rigid((np.deg2rad(17.0), 0.0, 0.0), (0.37, -1.21, 2.63), CENTRE),
            "oblique": G.rigid((0.21, -0.13, 0.3), (0.37, -1.21, 2.63), CENTRE), "mostly_outside": far, "nan": nan}


MATRICES = _matrices()
# (mode, dtype, fill)
KINDS = (("nearest", torch.uint8, 200), ("nearest", torch.int16, -1000), ("nearest", torch.float32, -2.5),
         ("linear", torch.float32, 0.75), ("linear", torch.int16, -1000.0), ("linear", torch.uint8, 3.0),
         ("label_linear", torch.uint8, 1))
NUM_CLASSES = 3


def _values(shape, mode, dtype, seed):
    rng = np.random.default_rng(seed)
    if mode == "label_linear":
        x = rng.integers(0, NUM_CLASSES, shape)
        x[rng.random(shape) < 0.1] = NUM_CLASSES + 2                    # strays: a label of no class
        return x.astype(np.uint8)
    if dtype == torch.float32:
        return (rng.standard_normal(shape) * 1000).astype(np.float32)
    lo, hi = (0, 256) if dtype == torch.uint8 else (-1024, 3072)
    return rng.integers(lo, hi, shape).astype(np.uint8 if dtype == torch.uint8 else np.int16)


def _same_bits(got: torch.Tensor, want: np.ndarray, what=""):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), \
        f"{what}: {np.count_nonzero(got != want)} of {want.size} voxels differ"


def _kw(out_shape):
    return dict(spacing=SPACING, origin=ORIGIN, out_spacing=_out_spacing(out_shape), out_origin=OUT_ORIGIN)


@pytest.mark.parametrize("name", MATRICES)
def test_every_mode_and_dtype_is_the_rule(name):
    from ctunet_amd import resample as rs
    M = MATRICES[name]
    m_dev = torch.from_numpy(M).to(DEV)
    inside = 0
    for ki, (mode, dtype, fill) in enumerate(KINDS):
        kc = dict(num_classes=NUM_CLASSES) if mode == "label_linear" else {}
        x = _values(IN_SHAPE, mode, dtype, ki)
        xd = torch.from_numpy(x).to(DEV)
        for out_shape in OUT_SHAPES:
            want = A.affine_resample(x, M, out_shape, mode=mode, fill=fill, **kc, **_kw(out_shape))
            got = rs.affine_resample(xd, m_dev if ki % 2 else m_dev[:3], out_shape, mode=mode, fill=fill, **kc, **_kw(out_shape))
            _same_bits(got, want, (name, mode, dtype, out_shape))
            inside += int(np.count_nonzero(want != np.asarray(fill, dtype=want.dtype)))
        # a batch [2, 3, ...]
        out_shape = OUT_SHAPES[2]
        xb = _values((2, 3) + IN_SHAPE, mode, dtype, 10 + ki)
        want = A.affine_resample(xb, M, out_shape, mode=mode, fill=fill, **kc, **_kw(out_shape))
        got = rs.affine_resample(torch.from_numpy(xb).to(DEV), m_dev, out_shape, mode=mode, fill=fill, **kc, **_kw(out_shape))
        assert tuple(got.shape) == (2, 3) + out_shape
        _same_bits(got, want, (name, mode, dtype, "batch"))
        # out= views that start 1, 4 and 12 bytes off a 16-byte boundary (as far as the dtype's own alignment allows)
        out_shape = OUT_SHAPES[0]
        want = A.affine_resample(x, M, out_shape, mode=mode, fill=fill, **kc, **_kw(out_shape))
        item = want.dtype.itemsize
        for off in (1, 4, 12):
            if off % item:
                continue
            nbytes = want.size * item
            buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
            base = (-buf.data_ptr()) % 16 + off
            view = buf[base:base + nbytes].view(got.dtype).view(out_shape)
            assert view.data_ptr() % 16 == off
            res = rs.affine_resample(xd, m_dev, out_shape, mode=mode, fill=fill, out=view, **kc, **_kw(out_shape))
            assert res is view
            _same_bits(view, want, (name, mode, dtype, "offset", off))
            rest = torch.cat((buf[:base], buf[base + nbytes:])).cpu().numpy()
            assert (rest == 0xA5).all(), (name, mode, dtype, off)      # nothing stored outside the view
    if name in ("nan", "mostly_outside"):
        print(f"{name}: {inside} voxels off the fill over all kinds")
    if name == "nan":
        assert inside == 0
    elif name != "mostly_outside":
        assert inside > 1000


def test_matrix_is_read_on_the_device_at_replay():
    from ctunet_amd import resample as rs
    out_shape = OUT_SHAPES[2]
    x = _values(IN_SHAPE, "linear", torch.int16, 3)
    xd = torch.from_numpy(x).to(DEV)
    m = torch.from_numpy(MATRICES["rot17"]).to(DEV)
    out = torch.empty(out_shape, dtype=torch.float32, device=DEV)

    def run():
        rs.affine_resample(xd, m, out_shape, mode="linear", fill=-1000.0, out=out, **_kw(out_shape))

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()                                                     # warm-up: library loaded, kernel resident
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    m.copy_(torch.from_numpy(MATRICES["oblique"]))                # in place: the captured launch holds the pointer
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    eager = rs.affine_resample(xd, torch.from_numpy(MATRICES["oblique"]).to(DEV), out_shape, mode="linear", fill=-1000.0,
                               **_kw(out_shape))
    assert torch.equal(replayed.view(torch.int32), eager.view(torch.int32))
    _same_bits(replayed, A.affine_resample(x, MATRICES["oblique"], out_shape, mode="linear", fill=-1000.0, **_kw(out_shape)))
    old = A.affine_resample(x, MATRICES["rot17"], out_shape, mode="linear", fill=-1000.0, **_kw(out_shape))
    assert not np.array_equal(old, replayed.cpu().numpy())


def test_round_trip_on_a_smooth_field():
    """Warp with M, then with its inverse, both between the same two grids: a check on the conventions (pull matrices, world
    frames, (z, y, x) order).  The device round trip is the restatement's bit for bit; the restatement's own error against the
    original in the interior is printed and bounded by the second differences of the field: two linear interpolations of
    f = sin-products with wavelengths of 20 voxels and more lose at most 2 * (h^2 / 8) * 3 * max|f''| = 0.75 * (2 pi / 20)^2 = 0.074."""
    from ctunet_amd import resample as rs
    shape, sp, org = (24, 28, 40), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    f = (np.sin(2 * np.pi * z / 24) * np.cos(2 * np.pi * y / 28) + np.sin(2 * np.pi * x / 20)).astype(np.float32)
    M = G.rigid((0.12, -0.08, 0.1), (0.8, -0.6, 1.1), (12.0, 14.0, 20.0))
    Minv = G.inverse(M)
    kw = dict(spacing=sp, origin=org, out_spacing=sp, out_origin=org)
    fd = torch.from_numpy(f).to(DEV)
    there = rs.affine_resample(fd, torch.from_numpy(M).to(DEV), shape, fill=0.0, **kw)
    back = rs.affine_resample(there, torch.from_numpy(Minv).to(DEV), shape, fill=0.0, **kw)
    want_there = A.affine_resample(f, M, shape, fill=0.0, **kw)
    want_back = A.affine_resample(want_there, Minv, shape, fill=0.0, **kw)
    _same_bits(there, want_there, "there")
    _same_bits(back, want_back, "back")
    interior = (slice(7, -7), slice(7, -7), slice(8, -8))
    err = np.abs(want_back[interior] - f[interior]).max()
    print(f"round trip: interior error {err:.4f} (second-difference bound 0.074)")
    assert err <= 0.074
    # the conventions matter: the same matrix twice, instead of its inverse, is far off
    wrong = A.affine_resample(want_there, M, shape, fill=0.0, **kw)
    assert np.abs(wrong[interior] - f[interior]).max() > 4 * err
