"""scipy / numpy restatements of the distance transform and ball morphology of ctunet_amd.postprocess (host only), shared
by test_distance_cpu.py and test_distance_gpu.py."""
import numpy as np
from scipy import ndimage as ndi


def triple(sampling):
    """None / scalar / triple -> float64 (z, y, x)."""
    if sampling is None:
        return np.ones(3)
    s = np.asarray(sampling, dtype=np.float64)
    return np.full(3, float(s)) if s.ndim == 0 else s


def edt(m, sampling=None, return_indices=False):
    """Distance of every voxel to the nearest zero voxel of m (float64), optionally scipy's indices."""
    return ndi.distance_transform_edt(np.asarray(m) != 0, sampling=None if sampling is None else tuple(triple(sampling)),
                                      return_indices=return_indices)


def signed(m, sampling=None):
    """edt(sites = foreground) - edt(sites = background): > 0 outside, < 0 inside.  m needs both kinds of voxel."""
    m = np.asarray(m) != 0
    return edt(~m, sampling) - edt(m, sampling)


def ball(radius, sampling=None):
    """The structure {o : ||o * s|| <= radius} in float64, an odd-sided bool array centred on o = 0."""
    s = triple(sampling)
    ext = [int(np.floor(radius / si)) for si in s]
    ax = [np.arange(-e, e + 1, dtype=np.float64) * si for e, si in zip(ext, s)]
    zz, yy, xx = np.meshgrid(*ax, indexing="ij")
    return np.sqrt(zz * zz + yy * yy + xx * xx) <= radius


def ball_margin(radius, sampling, extent):
    """Smallest relative gap |‖o * s‖ - radius| / radius over the offsets o with |o_i| <= extent_i (extent: an int or a
    triple).  A gap of 1e-4 or more means float32 and float64 agree on which offsets the ball holds."""
    s = triple(sampling)
    ext = [int(extent)] * 3 if np.ndim(extent) == 0 else [int(e) for e in extent]
    ax = [np.arange(0, e + 1, dtype=np.float64) * si for e, si in zip(ext, s)]      # the norm is even in every o_i
    zz, yy, xx = np.meshgrid(*ax, indexing="ij")
    norms = np.sqrt(zz * zz + yy * yy + xx * xx)
    return float(np.abs(norms - radius).min() / radius)


def ball_decidable(radius, sampling, extent):
    """What every ball test asserts before it compares bit for bit: ball_margin >= 1e-4.  One case passes with a margin of
    0: unit sampling and a radius whose square is an integer (1.0: the 6-neighbourhood).  Both sides then compare integers
    exactly (the kernel's int32 squared distance with float32(r^2) = r^2; scipy's sqrt of a perfect square is exact)."""
    if np.array_equal(triple(sampling), np.ones(3)) and float(radius) ** 2 == round(float(radius) ** 2) < 2 ** 24 \
            and float(radius) == round(float(radius)):
        return True
    return ball_margin(radius, sampling, extent) >= 1e-4


def _pad(radius, sampling):
    return [int(np.floor(radius / si)) + 1 for si in triple(sampling)]


def ball_dilation(m, radius, sampling=None):
    """{v : d(v, foreground) <= radius}."""
    m = np.asarray(m) != 0
    if not m.any():
        return np.zeros_like(m)
    return edt(~m, sampling) <= radius


def ball_erosion(m, radius, sampling=None):
    """{v : d(v, background or outside) > radius}: the virtual border is a zero padding wider than the ball."""
    m = np.asarray(m) != 0
    p = _pad(radius, sampling)
    padded = np.pad(m, [(k, k) for k in p], constant_values=False)
    d = edt(padded, sampling)
    return (d > radius)[p[0]:p[0] + m.shape[0], p[1]:p[1] + m.shape[1], p[2]:p[2] + m.shape[2]]


def ball_opening(m, radius, sampling=None):
    return ball_dilation(ball_erosion(m, radius, sampling), radius, sampling)


def ball_closing(m, radius, sampling=None):
    return ball_erosion(ball_dilation(m, radius, sampling), radius, sampling)


def blob(shape, seed, sigma=2.0):
    """A smooth random mask, about half foreground."""
    g = ndi.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), sigma, mode="nearest")
    return g > np.median(g)


def random_mask(shape, density, seed):
    """Foreground with probability `density`, with at least one background voxel (scipy's EDT needs a site)."""
    m = np.random.default_rng(seed).random(shape) < density
    if m.all():
        m.flat[0] = False
    return m

