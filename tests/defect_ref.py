"""NumPy restatement of SkullRandomDefect and RandomDilate (ctunet_amd/transforms.py pins the rules): the host geometry,
the per-sample draws (ball chain, box, roughness lattice), the voxel rule tested on EVERY voxel, the outputs with the fused
noise, and the L1-ball dilation.  All float64, one rounding per operation, as the kernels compute."""
import math

import numpy as np

from augment_ref import noise_fields, philox_seq, value_of

MAX_BALLS = 12
RECORD = 64


def unif64(r):
    return (np.asarray(r, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def draw_int(r, lo, span):
    return lo + ((int(r) * int(span)) >> 32)


def size_range(dims):
    """SkullRandomHole's [lo, hi) of the hole size (transforms.size_range)."""
    lo = min(dims) // 5 - 1
    return int(lo), int(max(lo, max(dims) // 3.5))


def geometry(dims, spacing=(1.0, 1.0, 1.0), radius=None, roughness=None, roughness_scale=None):
    """radius (lo, hi), amp and scale in mm and the lattice size G of a volume of ``dims``."""
    lo, hi = size_range(dims)
    s = min(float(v) for v in spacing)
    radius = (float(radius[0]), float(radius[1])) if radius is not None else ((0.75 * lo) * s, (0.75 * hi) * s)
    amp = float(roughness) if roughness is not None else 0.15 * radius[0]
    scale = float(roughness_scale) if roughness_scale is not None else 1.5 * radius[0]
    G = tuple(math.floor((n * float(sp)) / scale) + 2 for n, sp in zip(dims, spacing))
    return dict(radius=radius, amp=amp, scale=scale, G=G)


def shell(dims, semi=0.45, thickness=0.12):
    """bool [D,H,W]: an ellipsoidal shell about the grid's middle, semi-axes ``semi`` n, ``thickness`` of them thick."""
    o = np.indices(dims, dtype=np.float64)
    q = sum(((o[a] - (dims[a] - 1) / 2) / (semi * dims[a])) ** 2 for a in range(3))
    return (q <= 1.0) & (q > (1.0 - thickness) ** 2)


def draw(seed, seq, bone, geo, spacing=(1.0, 1.0, 1.0), p=1.0, balls=(3, 8), spread=0.9, shrink=(0.5, 0.9)):
    """The draws of sample number ``seq`` on the bool volume ``bone``: dict with the float64 [64] ``record`` the kernel
    writes, the ``lattice`` [Gz, Gy, Gx], the ``parents`` of balls 1 .. K - 1 and the decoded fields."""
    dims = bone.shape
    sp = [float(v) for v in spacing]
    G = geo["G"]
    idx = np.arange(G[0] * G[1] * G[2], dtype=np.uint32)
    lattice = (2.0 * unif64(philox_seq(idx, 1, seq, seed)[0]) - 1.0).reshape(G)
    r = [int(v) for v in philox_seq(0, 0, seq, seed)]
    count = int(bone.sum())
    apply = bool(unif64(r[0]) < np.float64(p))
    k = draw_int(r[1], 0, count) if count else 0
    K = balls[0] + draw_int(r[3], 0, balls[1] - balls[0] + 1)
    rec = np.zeros(RECORD, np.float64)
    rec[0], rec[1], rec[2], rec[6], rec[7] = apply, count, k, K, apply and count > 0
    out = dict(apply=apply, cut=apply and count > 0, count=count, k=k, n_balls=K, lattice=lattice, parents=[], balls=[])
    if not count:
        rec[3:6] = rec[11:14] = -1.0
        out.update(record=rec, centre=(-1, -1, -1), box=((0, 0, 0), (-1, -1, -1)))
        return out
    centre = tuple(int(v) for v in np.argwhere(bone)[k])
    lo, hi = geo["radius"]
    chain = [[np.float64(centre[a]) * sp[a] for a in range(3)] + [lo + unif64(r[2]) * (hi - lo)]]
    for j in range(1, K):
        q = [int(v) for v in philox_seq(16 + 2 * j, 0, seq, seed)]
        s = [int(v) for v in philox_seq(17 + 2 * j, 0, seq, seed)]
        i = draw_int(q[0], 0, j)
        par = chain[i]
        rj = (shrink[0] + unif64(q[1]) * (shrink[1] - shrink[0])) * par[3]
        chain.append([par[a] + ((2.0 * unif64(s[a]) - 1.0) * spread) * par[3] for a in range(3)] + [rj])
        out["parents"].append(i)
    chain = np.array(chain, np.float64)
    rec[3:6] = centre
    rec[16:16 + 4 * K] = chain.reshape(-1)
    e = chain[:, 3] + geo["amp"]
    for a in range(3):
        rec[8 + a] = max(0.0, np.floor((chain[:, a] - e) / sp[a]).min() - 1.0)
        rec[11 + a] = min(float(dims[a] - 1), np.ceil((chain[:, a] + e) / sp[a]).max() + 1.0)
    out.update(record=rec, centre=centre, balls=[tuple(float(v) for v in b) for b in chain],
               box=(tuple(int(v) for v in rec[8:11]), tuple(int(v) for v in rec[11:14])))
    return out


def lattice_cells(dims, geo, spacing=(1.0, 1.0, 1.0)):
    """Per axis (w, i, f): the world coordinate, lattice cell and fraction of every voxel index."""
    out = []
    for a in range(3):
        w = np.arange(dims[a], dtype=np.float64) * float(spacing[a])
        g = w / geo["scale"]
        i = np.floor(g)
        out.append((w, i.astype(np.int64), g - i))
    return out


def inside_mask(dims, balls, lattice, geo, spacing=(1.0, 1.0, 1.0)):
    """bool [D,H,W]: the voxel rule on every voxel (no box)."""
    (wz, iz, fz), (wy, iy, fy), (wx, ix, fx) = lattice_cells(dims, geo, spacing)
    Z, Y, X = np.ix_(iz, iy, ix)
    FZ, FY, FX = fz[:, None, None], fy[None, :, None], fx[None, None, :]
    L = lattice

    def lerp(a, b, f):
        return a + f * (b - a)

    c0 = lerp(lerp(L[Z, Y, X], L[Z, Y, X + 1], FX), lerp(L[Z, Y + 1, X], L[Z, Y + 1, X + 1], FX), FY)
    c1 = lerp(lerp(L[Z + 1, Y, X], L[Z + 1, Y, X + 1], FX), lerp(L[Z + 1, Y + 1, X], L[Z + 1, Y + 1, X + 1], FX), FY)
    rough = geo["amp"] * lerp(c0, c1, FZ)
    WZ, WY, WX = wz[:, None, None], wy[None, :, None], wx[None, None, :]
    ins = np.zeros(dims, bool)
    for cz, cy, cx, r in balls:
        rho = r + rough
        dz, dy, dx = WZ - cz, WY - cy, WX - cx
        ins |= (rho > 0.0) & (((dz * dz + dy * dy) + dx * dx) <= rho * rho)
    return ins


def expected(skull, rec, lattice, geo, spacing=(1.0, 1.0, 1.0), noise_seed=None, salt_ratio=0.1):
    """(image, bone, flap) float32 [D,H,W] of one sample from its record (a ``last_params`` entry, or ``draw``'s dict with
    the noise fields added) and its lattice."""
    val = value_of(skull)
    bone = val >= 1
    img = val.copy()
    flap = np.zeros(skull.shape, bool)
    if rec["cut"]:
        ins = inside_mask(skull.shape, rec["balls"], np.asarray(lattice), geo, spacing)
        img = (bone & ~ins).astype(np.float32)
        flap = bone & ins
    if noise_seed is not None and rec["noise_applied"]:
        f = np.float32
        nd = f(rec["nd"])
        t0, t1 = f(nd * f(f(1) - f(salt_ratio))), f(nd * f(salt_ratio))
        u1, u2 = noise_fields(noise_seed, rec["noise_seq"], skull.shape)
        img = (((img != 0) & ~(u1 <= t0)) | (u2 <= t1)).astype(np.float32)
    return img, bone.astype(np.float32), flap.astype(np.float32)


def dilate_applied(seed, seq, p):
    """RandomDilate's choice for sample number ``seq``."""
    return bool(unif64(philox_seq(0, 0, seq, seed)[0]) < np.float64(p))


def dilate_l1(bone, k):
    """bool: some bone voxel within L1 distance k, nothing outside the volume (the gather kernel's rule)."""
    d, h, w = bone.shape
    pad = np.zeros((d + 2 * k, h + 2 * k, w + 2 * k), bool)
    pad[k:k + d, k:k + h, k:k + w] = bone
    out = np.zeros(bone.shape, bool)
    for dz in range(-k, k + 1):
        for dy in range(-(k - abs(dz)), k - abs(dz) + 1):
            r = k - abs(dz) - abs(dy)
            for dx in range(-r, r + 1):
                out |= pad[k + dz:k + dz + d, k + dy:k + dy + h, k + dx:k + dx + w]
    return out


def random_dilate(x, seed, seq0, p, iterations):
    """uint8 [N,1,D,H,W]: RandomDilate.apply on a batch whose first sample has number ``seq0``."""
    bone = value_of(x) >= 1
    out = bone.copy()
    for n in range(x.shape[0]):
        if dilate_applied(seed, seq0 + n, p):
            out[n, 0] = dilate_l1(bone[n, 0], iterations)
    return out.astype(np.uint8)
