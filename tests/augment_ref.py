"""NumPy restatement of the flap-reconstruction augmentation (ctunet_amd/transforms.py pins the rules): Philox4x32-10,
the per-sample draws, the shape masks, the noise fields and the outputs, driven by the kernels' per-sample records."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
SHAPES = ("sphere", "box", "flap")
_MASK = np.uint64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over broadcast uint32 counters -> four uint32 arrays."""
    c = [x.astype(np.uint64) for x in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint32) for v in (c0, c1, c2, c3)])]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
    return [x.astype(np.uint32) for x in c]


def philox_seq(c0, stream, seq, seed):
    return philox(c0, stream, seq & 0xFFFFFFFF, seq >> 32, seed & 0xFFFFFFFF, seed >> 32)


def unif(r):
    return (np.asarray(r, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def draw_int(r, lo, span):
    return lo + ((int(r) * int(span)) >> 32)


def hole_scalars(seed, seq, count, size_lo, size_hi, shapes=SHAPES, p=1.0):
    """The hole's stream-0 draws of sample number seq."""
    r = [int(v) for v in philox_seq(0, 0, seq, seed)]
    r2 = [int(v) for v in philox_seq(1, 0, seq, seed)]
    size = draw_int(r[2], size_lo, size_hi - size_lo)
    f = np.float32
    cd = f(f(f(0.25) + f(f(0.75) * unif(r2[0]))) * f(size)) * f(0.25)
    return dict(apply=bool(unif(r[0]) < f(p)), k=draw_int(r[1], 0, count) if count else 0, size=size,
                shape=shapes[draw_int(r[3], 0, len(shapes))], c_diam=float(np.float32(cd)))


def noise_scalars(seed, seq0, n, nd0, decay=True, p=1.0, salt_ratio=0.1):
    """Per-sample (applied, nd') of samples seq0 .. seq0+n-1 of one noise instance starting at density nd0 (float32)."""
    f = np.float32
    nd, out = f(nd0), []
    for j in range(n):
        r = philox_seq(0, 0, seq0 + j, seed)
        u = unif(r[1])
        cur = f(u * nd) if decay else f(u * f(nd0))
        if decay:
            nd = cur
        out.append((bool(unif(r[0]) < f(p)), float(cur)))
    return out


def shape_mask(dims, centre, size, shape, c_diam=0.0):
    """bool [D,H,W]: inside the hole shape (integer rules; the flap restatement is the port's own, unpinned)."""
    d, h, w = dims
    z, y, x = np.indices(dims, dtype=np.int64)
    dz, dy, dx = z - centre[0], y - centre[1], x - centre[2]
    s = int(size)
    if shape == "sphere":
        return (dz * dz + dy * dy + dx * dx <= s * s) & (s >= 0)
    if shape == "box":
        return np.maximum(np.maximum(np.abs(dz), np.abs(dy)), np.abs(dx)) <= s
    zin = 2 * np.abs(dz) <= s
    cube = zin & (2 * np.abs(dy) <= s) & (2 * np.abs(dx) <= s)
    cd2 = np.float64(np.float32(np.float32(2 * c_diam) * np.float32(2 * c_diam)))
    ey = 2 * y - (2 * centre[1] - s)
    e1, e2 = 2 * x - (2 * centre[2] - s), 2 * x - (2 * centre[2] + s)
    cyl = zin & (((ey * ey + e1 * e1).astype(np.float64) <= cd2) | ((ey * ey + e2 * e2).astype(np.float64) <= cd2))
    return cube | cyl


def noise_fields(seed, seq, dims):
    """(u1, u2) float32 [D,H,W]: streams 1 and 2 of noise sample seq."""
    d, h, w = dims
    wq = (w + 3) // 4
    z, y, x = np.indices(dims, dtype=np.int64)
    c0 = ((z * h + y) * wq + x // 4).astype(np.uint32)
    lane = (x % 4)
    out = []
    for stream in (1, 2):
        r = philox_seq(c0, stream, seq, seed)
        out.append(unif(np.choose(lane, r)))
    return out


def value_of(skull):
    """The uint8 cast of a float / uint8 skull, as float32 values."""
    return np.trunc(skull.astype(np.float32)) if skull.dtype != np.uint8 else skull.astype(np.float32)


def expected(skull, rec, hole=True, noise_seed=None, salt_ratio=0.1):
    """(image, bone, flap) float32 [D,H,W] of one sample from its record (transforms.last_params entry)."""
    val = value_of(skull)
    bone = val >= 1
    img = val.copy()
    flap = np.zeros(skull.shape, bool)
    if hole and rec["cut"]:
        ins = shape_mask(skull.shape, rec["centre"], rec["size"], rec["shape"], rec["c_diam"])
        img = (bone & ~ins).astype(np.float32)
        flap = bone & ins
    if noise_seed is not None and rec["noise_applied"]:
        f = np.float32
        nd = f(rec["nd"])
        t0, t1 = f(nd * f(f(1) - f(salt_ratio))), f(nd * f(salt_ratio))
        u1, u2 = noise_fields(noise_seed, rec["noise_seq"], skull.shape)
        img = (((img != 0) & ~(u1 <= t0)) | (u2 <= t1)).astype(np.float32)
    return img, bone.astype(np.float32), flap.astype(np.float32)


def one_hot(m):
    m = np.asarray(m, np.float32)
    return np.stack([1 - m, m])
