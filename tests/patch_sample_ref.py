"""NumPy restatement of the random patch sampling (ctunet_amd/sampling.py pins the rule): the class predicates, the chunk
index, the per-patch draw and the window crop, written from the module docstring line by line."""
import numpy as np

from augment_ref import draw_int, philox_seq

CHUNK = 8192


def predicates(labels, classes):
    """bool [K, ...]: classes=None is the one class "nonzero", otherwise class i is labels == classes[i]."""
    if classes is None:
        return (labels != 0)[None]
    return np.stack([labels == c for c in classes])


def index(labels, classes):
    """int32 [M, K, nchunks]: voxels of each class per run of CHUNK flat C-order indices of each item [M, D, H, W]."""
    m = labels.shape[0]
    pred = predicates(labels, classes).reshape(-1, m, labels[0].size)          # [K, M, V]
    starts = np.arange(0, pred.shape[2], CHUNK)
    return np.add.reduceat(pred.astype(np.int64), starts, axis=2).transpose(1, 0, 2).astype(np.int32)


def cumulative(class_p):
    cum, run = [], 0.0
    for p in class_p:
        run = run + float(p)
        cum.append(run)
    return cum


def words(seed, seq):
    """(r_class, r_k, r_z, r_y, r_x) of sample number seq."""
    a = [int(v) for v in philox_seq(0, 0, seq, seed)]
    b = [int(v) for v in philox_seq(1, 0, seq, seed)]
    return a[0], a[1], b[0], b[1], b[2]


def choose_class(r_class, cum):
    u = float(r_class >> 8) * 2.0 ** -24
    for i, c in enumerate(cum):
        if (cum[i - 1] if i else 0.0) <= u < c:
            return i
    return -1


def start_of(n, p, r, centre=None, jitter=0):
    """One axis: the uniform start, or the start of a patch about ``centre``."""
    hi = max(0, n - p)
    if centre is None:
        return draw_int(r, 0, hi + 1)
    return clamp_start(n, p, centre, draw_int(r, -jitter, 2 * jitter + 1))


def clamp_start(n, p, c, j):
    """s = min(max(c - p // 2 + j, 0), hi) of one axis (NumPy arrays broadcast)."""
    return np.minimum(np.maximum(c - p // 2 + j, 0), np.maximum(0, n - p))


def draw_one(seed, seq, item, dims, patch, jitter, cum, count_of, centre_of):
    """The record of one patch as a dict.  count_of(i) -> voxels of class i in the item; centre_of(i, k) -> (z, y, x)."""
    r_class, r_k, *r_axis = words(seed, seq)
    cls = choose_class(r_class, cum)
    count = k = 0
    centre = None
    if cls >= 0:
        count = count_of(cls)
        if count:
            k = draw_int(r_k, 0, count)
            centre = tuple(int(v) for v in centre_of(cls, k))
    start = tuple(int(start_of(dims[a], patch[a], r_axis[a], None if centre is None else centre[a], jitter[a]))
                  for a in range(3))
    return {"item": item, "start": start, "class_index": cls, "fallback": cls >= 0 and count == 0, "count": count, "k": k,
            "centre": centre if centre is not None else (-1, -1, -1)}


INVALID = {"item": -1, "start": (0, 0, 0), "class_index": -1, "fallback": False, "count": 0, "k": 0, "centre": (-1, -1, -1)}


def draw(labels, classes, items, seed, counter, patch, jitter, class_p):
    """Records of a call that draws patch j from volume items[j] at sample numbers counter, counter + 1, ..."""
    m = labels.shape[0]
    dims = labels.shape[1:]
    cum = cumulative(class_p)
    where = {}

    def voxels(item, i):
        if (item, i) not in where:
            where[(item, i)] = np.argwhere(predicates(labels[item], classes)[i])
        return where[(item, i)]
    out = []
    for j, item in enumerate(items):
        if not 0 <= item < m:
            out.append(dict(INVALID))
            continue
        out.append(draw_one(seed, counter + j, int(item), dims, patch, jitter, cum,
                            lambda i: len(voxels(item, i)), lambda i, k: voxels(item, i)[k]))
    return out


def coords_of(records):
    return np.array([[r["item"], *r["start"]] for r in records], np.int32).reshape(-1, 4)


def crop(src, coords, patch, fill=0, dtype=None):
    """src [Ms, C, D, H, W] -> [P, C, pd, ph, pw]: NumPy slicing of the part inside the volume, ``fill`` elsewhere."""
    ms, c = src.shape[:2]
    dims = src.shape[2:]
    out = np.full((len(coords), c) + tuple(patch), fill, dtype=dtype or src.dtype)
    for p, (item, *s0) in enumerate(np.asarray(coords).tolist()):
        if item < 0 or (ms > 1 and item >= ms):
            continue
        lo = [min(max(s, 0), n) for s, n in zip(s0, dims)]
        hi = [min(max(s + q, 0), n) for s, q, n in zip(s0, patch, dims)]
        if any(h <= l for l, h in zip(lo, hi)):
            continue
        dst = tuple(slice(l - s, h - s) for l, h, s in zip(lo, hi, s0))
        win = tuple(slice(l, h) for l, h in zip(lo, hi))
        out[(p, slice(None)) + dst] = src[(0 if ms == 1 else item, slice(None)) + win]
    return out
