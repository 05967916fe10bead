"""Numpy float64 restatement of the mirrored / ensemble / uncertainty blend rule pinned in ctunet_amd/inference.py (test
infrastructure, not product code).

A contribution is (model, flip mask, tile); contributions are ordered by model, then mask (identity first), then tile in
z-major order.  Masks: x = 1, y = 2, z = 4."""
import numpy as np

WEIGHT_FLOOR = 1e-3
AXIS_OF_BIT = {1: -1, 2: -2, 4: -3}


def mirror(a, mask):
    """a[..., i, j, k] -> a[..., i^, j^, k^]: the last three axes reversed where the mask's bit is set (an involution)."""
    axes = tuple(ax for bit, ax in AXIS_OF_BIT.items() if mask & bit)
    return np.flip(a, axes) if axes else a


def extract(vol, tile, patch):
    """The zero-padded patch [C,pd,ph,pw] of the tile at origin (z0,y0,x0) of vol [C,D,H,W]."""
    z0, y0, x0 = (int(t) for t in tile)
    out = np.zeros((vol.shape[0],) + tuple(patch), vol.dtype)
    src = vol[:, z0:z0 + patch[0], y0:y0 + patch[1], x0:x0 + patch[2]]
    out[:, :src.shape[1], :src.shape[2], :src.shape[3]] = src
    return out


def tables(patch, blend="gaussian", sigma_scale=0.125):
    out = []
    for p in patch:
        i = np.arange(p, dtype=np.float64)
        out.append(np.ones(p) if blend == "constant" else np.exp(-(i - (p - 1) / 2) ** 2 / (2 * (sigma_scale * p) ** 2)))
    return out


def weight(patch, blend="gaussian", sigma_scale=0.125):
    gz, gy, gx = tables(patch, blend, sigma_scale)
    return np.maximum((gz[:, None, None] * gy[None, :, None]) * gx[None, None, :], WEIGHT_FLOOR)


def entropy(y):
    """h(y) over axis 0 of y [K,...]: -sum q ln q / ln K, q = max(y,0) / sum max(y,0); 0 for a zero sum, 0 ln 0 = 0."""
    k = y.shape[0]
    m = np.maximum(np.asarray(y, np.float64), 0.0)
    s = m.sum(0)
    q = np.divide(m, s, out=np.zeros_like(m), where=s > 0)
    t = np.where(q > 0, q * np.log(np.where(q > 0, q, 1.0)), 0.0)
    return -t.sum(0) / np.log(k) if k > 1 else np.zeros(y.shape[1:])


def accumulate(ys, masks, tiles, shape, patch, blend="gaussian", sigma_scale=0.125):
    """ys [M, F, T, K, pd, ph, pw]: the net's raw outputs y~ of every contribution (model, pass, tile), pass f run on
    patches mirrored by masks[f].  Returns the float64 accumulators S0 [D,H,W], S1 [K,D,H,W], S2 [K,D,H,W], SH [D,H,W] and
    n [D,H,W], the number of contributions per voxel."""
    ys = np.asarray(ys, np.float64)
    nm, nf, nt, k = ys.shape[:4]
    assert nf == len(masks) and nt == len(tiles)
    w = weight(patch, blend, sigma_scale)
    shape = tuple(shape)
    s0, sh, n = np.zeros(shape), np.zeros(shape), np.zeros(shape, np.int64)
    s1, s2 = np.zeros((k,) + shape), np.zeros((k,) + shape)
    for m in range(nm):
        for f, mask in enumerate(masks):
            for t, (z0, y0, x0) in enumerate(tiles):
                y = mirror(ys[m, f, t], mask)
                dz, dy, dx = (min(p, s - a) for p, s, a in zip(patch, shape, (z0, y0, x0)))
                box = (slice(z0, z0 + dz), slice(y0, y0 + dy), slice(x0, x0 + dx))
                ww, yy = w[:dz, :dy, :dx], y[:, :dz, :dy, :dx]
                s0[box] += ww
                s1[(slice(None),) + box] += ww * yy
                s2[(slice(None),) + box] += ww * (yy * yy)
                if k > 1:
                    sh[box] += ww * entropy(yy)
                n[box] += 1
    return dict(S0=s0, S1=s1, S2=s2, SH=sh, n=n)


def finalize(acc):
    """probs, labels (first argmax), variance, entropy, mutual_information from the accumulators; 0 where S0 == 0."""
    s0 = acc["S0"]
    cov = s0 > 0
    div = lambda a: np.divide(a, s0, out=np.zeros_like(a), where=np.broadcast_to(cov, a.shape))
    probs = div(acc["S1"])
    ent = entropy(probs)
    return dict(probs=probs, labels=np.argmax(probs, 0).astype(np.uint8),
                variance=np.where(cov, np.maximum(div(acc["S2"]) - probs * probs, 0.0), 0.0),
                entropy=ent, mutual_information=np.where(cov, np.maximum(ent - div(acc["SH"]), 0.0), 0.0))


def predict(fn, vol, tiles, patch, masks, blend="gaussian", sigma_scale=0.125, models=1):
    """The whole rule with ``fn(model index, x [C,pd,ph,pw]) -> [K,pd,ph,pw]`` as the net: extract, mirror, apply, blend."""
    ys = [[[fn(m, mirror(extract(vol, t, patch), mask)) for t in tiles] for mask in masks] for m in range(models)]
    return finalize(accumulate(np.array(ys), masks, tiles, vol.shape[1:], patch, blend, sigma_scale))
