"""NumPy restatement of the region-properties rule that ctunet_amd/postprocess.py pins ("Region properties"): the exact
integer moments, boxes and overflow count of a label map, the float64 fields derived from the moments in the order the
kernel evaluates them (numpy never fuses), the box arithmetic of ``bounding_box`` and the five starts and the selection
rule of ``registration.register(init="moments")``."""
import numpy as np

SWEEPS = 8
MAX_SIDE = 1024
PAIRS = ((0, 1, 2), (0, 2, 1), (1, 2, 0))                      # (p, q, the third index)
SIGNS = ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))     # the proper sign choices of two principal frames


def integer_tables(labels, R):
    """(moments int64 [N,R,10], boxes int32 [N,R,6], overflow int64 [N]) of a label map [N,D,H,W] or [D,H,W] of any integer
    or bool dtype; int64 sums, which are exact (every sum is below 2^51)."""
    lab = np.asarray(labels)
    if lab.ndim == 3:
        lab = lab[None]
    lab = lab.astype(np.int64)
    N, D, H, W = lab.shape
    assert max(D, H, W) <= MAX_SIDE
    moments = np.zeros((N, R, 10), dtype=np.int64)
    boxes = np.zeros((N, R, 6), dtype=np.int32)
    overflow = np.zeros(N, dtype=np.int64)
    z, y, x = np.meshgrid(np.arange(D, dtype=np.int64), np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    terms = (np.ones_like(z), z, y, x, z * z, z * y, z * x, y * y, y * x, x * x)
    for n in range(N):
        v = lab[n]
        overflow[n] = int(((v < 0) | (v > R)).sum())
        inside = (v >= 1) & (v <= R)
        r = v[inside] - 1
        for k, t in enumerate(terms):
            np.add.at(moments[n, :, k], r, t[inside])
        lo = np.full((R, 3), MAX_SIDE, dtype=np.int64)
        hi = np.full((R, 3), -1, dtype=np.int64)
        for a, c in enumerate((z, y, x)):
            np.minimum.at(lo[:, a], r, c[inside])
            np.maximum.at(hi[:, a], r, c[inside])
        some = moments[n, :, 0] > 0
        boxes[n, some, :3] = lo[some]
        boxes[n, some, 3:] = hi[some] + 1
    return moments, boxes, overflow


def _frames(v, n, default):
    if v is None:
        return np.full((n, 3), default, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    if v.ndim == 0:
        return np.full((n, 3), float(v))
    if v.shape == (3,):
        return np.tile(v, (n, 1))
    assert v.shape == (n, 3)
    return v


def _rotate(a, e, p, q, r):
    """One Jacobi rotation on the arrays a[i][j], e[i][j] (each of shape [M]), skipped where a[p][q] == 0."""
    apq = a[p][q]
    on = apq != 0.0
    safe = np.where(on, apq, 1.0)
    theta = (a[q][q] - a[p][p]) / (2.0 * safe)
    at = np.where(theta < 0.0, -theta, theta)
    t = 1.0 / (at + np.sqrt(theta * theta + 1.0))
    t = np.where(theta < 0.0, -t, t)
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    app = a[p][p] - t * apq
    aqq = a[q][q] + t * apq
    arp, arq = a[r][p], a[r][q]
    nrp = c * arp - s * arq
    nrq = s * arp + c * arq
    a[p][p] = np.where(on, app, a[p][p])
    a[q][q] = np.where(on, aqq, a[q][q])
    a[p][q] = a[q][p] = np.where(on, 0.0, apq)
    a[r][p] = a[p][r] = np.where(on, nrp, arp)
    a[r][q] = a[q][r] = np.where(on, nrq, arq)
    for k in range(3):
        ekp, ekq = e[k][p], e[k][q]
        e[k][p] = np.where(on, c * ekp - s * ekq, ekp)
        e[k][q] = np.where(on, s * ekp + c * ekq, ekq)


def derive(moments, sampling=None, origin=None):
    """(centroid [N,R,3], covariance [N,R,3,3], extent [N,R,3], axes [N,R,3,3]) of moments [N,R,10], float64."""
    mom = np.asarray(moments, dtype=np.int64)
    N, R, _ = mom.shape
    sp = _frames(sampling, N, 1.0)[:, None, :]                  # [N,1,3]
    org = _frames(origin, N, 0.0)[:, None, :]
    cnt = mom[..., 0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n = cnt.astype(np.float64)
        S = mom.astype(np.float64)                               # exact: every sum is below 2^53
        mean = [S[..., 1 + a] / n for a in range(3)]
        centroid = np.stack([org[..., a] + sp[..., a] * mean[a] for a in range(3)], axis=-1)
        second = {(0, 0): 4, (0, 1): 5, (0, 2): 6, (1, 1): 7, (1, 2): 8, (2, 2): 9}
        a = [[None] * 3 for _ in range(3)]
        for p in range(3):
            for q in range(3):
                lo, hi = min(p, q), max(p, q)
                c = S[..., second[(lo, hi)]] / n - mean[lo] * mean[hi]
                a[p][q] = (c * sp[..., lo]) * sp[..., hi]
        covariance = np.stack([np.stack([a[p][q] for q in range(3)], axis=-1) for p in range(3)], axis=-2)
        one, zero = np.ones_like(n), np.zeros_like(n)
        e = [[one.copy() if p == q else zero.copy() for q in range(3)] for p in range(3)]
        for _ in range(SWEEPS):
            for p, q, r in PAIRS:
                _rotate(a, e, p, q, r)
        w = [a[0][0], a[1][1], a[2][2]]
        ev = [np.zeros_like(n) for _ in range(3)]
        ax = [[np.zeros_like(n) for _ in range(3)] for _ in range(3)]       # ax[j][k]: component k of the j-th axis
        for k in range(3):
            rank = sum(((w[j] > w[k]) | ((w[j] == w[k]) & (j < k))).astype(np.int64) for j in range(3))
            for j in range(3):
                m = rank == j
                ev[j] = np.where(m, w[k], ev[j])
                for i in range(3):
                    ax[j][i] = np.where(m, e[i][k], ax[j][i])
        for j in range(2):
            big = np.zeros(n.shape, dtype=np.int64)
            mag = np.abs(ax[j][0])
            for k in (1, 2):
                ak = np.abs(ax[j][k])
                up = ak > mag
                mag = np.where(up, ak, mag)
                big = np.where(up, k, big)
            lead = np.where(big == 0, ax[j][0], np.where(big == 1, ax[j][1], ax[j][2]))
            neg = lead < 0.0
            for k in range(3):
                ax[j][k] = np.where(neg, -ax[j][k], ax[j][k])
        ax[2][0] = ax[0][1] * ax[1][2] - ax[0][2] * ax[1][1]
        ax[2][1] = ax[0][2] * ax[1][0] - ax[0][0] * ax[1][2]
        ax[2][2] = ax[0][0] * ax[1][1] - ax[0][1] * ax[1][0]
    extent = np.stack(ev, axis=-1)
    axes = np.stack([np.stack([ax[j][k] for j in range(3)], axis=-1) for k in range(3)], axis=-2)    # axes[..., k, j]
    empty = cnt == 0
    centroid[empty] = np.nan
    covariance[empty] = np.nan
    extent[empty] = np.nan
    axes[cnt < 2] = np.nan
    return centroid, covariance, extent, axes


def region_properties(labels, R, sampling=None, origin=None):
    moments, boxes, overflow = integer_tables(labels, R)
    return (moments, boxes, overflow) + derive(moments, sampling, origin)


def bounding_box(boxes, counts, shape, margin=0, multiple_of=1):
    """int32 [N,6] from one region's boxes [N,6] and voxel counts [N]: the arithmetic of postprocess.bounding_box."""
    boxes = np.asarray(boxes, dtype=np.int64)
    mg = (margin,) * 3 if np.isscalar(margin) else tuple(margin)
    out = np.zeros_like(boxes)
    for i in range(boxes.shape[0]):
        for a in range(3):
            S = int(shape[a])
            if counts[i] == 0:
                out[i, a], out[i, 3 + a] = 0, S
                continue
            lo, hi = int(boxes[i, a]) - mg[a], int(boxes[i, 3 + a]) + mg[a]
            side = -(-(hi - lo) // multiple_of) * multiple_of
            lo -= (side - (hi - lo)) // 2
            if side <= S:
                lo = max(min(lo, S - side), 0)
                out[i, a], out[i, 3 + a] = lo, lo + side
            else:
                out[i, a], out[i, 3 + a] = 0, S
    return out.astype(np.int32)


def moment_starts(cm, Am, cf, Af):
    """The five [4,4] starts of register(init="moments"): A_f diag(s) A_m^T for the four proper sign choices, each with the
    translation that takes the moving centroid cm onto the fixed centroid cf, then the identity rotation with that
    translation."""
    starts = []
    for s in SIGNS + (None,):
        Rm = np.eye(3) if s is None else (np.asarray(Af) * np.asarray(s, dtype=np.float64)) @ np.asarray(Am).T
        M = np.eye(4)
        M[:3, :3] = Rm
        M[:3, 3] = np.asarray(cf) - Rm @ np.asarray(cm)
        starts.append(M)
    return starts


def select_start(last_rows):
    """Index of the chosen start from the stacked last history rows [K, >= 2] (cost / P, inliers, ...): among the starts whose
    inlier count is at least half the largest, the lowest cost; the lowest index wins a tie."""
    rows = np.asarray(last_rows, dtype=np.float64)
    cost, inl = rows[:, 0], rows[:, 1]
    ok = inl >= 0.5 * inl.max()
    key = np.where(ok & ~np.isnan(cost), cost, np.inf)
    return int(np.argmin(key))


# ---- the turned-skull fixture of the registration tests ---------------------------------------------------------------------
FIXTURE_SHAPE = (48, 64, 56)
FIXTURE_CENTRE = (24.0, 32.0, 28.0)


def fixture_shape(p):
    """The analytic shape at points p [..., 3] (z, y, x): the shell 0.82 < r < 1 of the ellipsoid with semi-axes (14, 22, 17)
    about (24, 32, 28), cut away where z - 24 <= -7 (an open base), joined with the ellipsoid of semi-axes (5, 5, 6) about
    (20, 53, 28) (a "face" lump that breaks the symmetry)."""
    z, y, x = p[..., 0], p[..., 1], p[..., 2]
    r = np.sqrt(((z - 24.0) / 14.0) ** 2 + ((y - 32.0) / 22.0) ** 2 + ((x - 28.0) / 17.0) ** 2)
    shell = (r > 0.82) & (r < 1.0) & ~(z - 24.0 <= -7.0)
    lump = ((z - 20.0) / 5.0) ** 2 + ((y - 53.0) / 5.0) ** 2 + ((x - 28.0) / 6.0) ** 2 < 1.0
    return shell | lump


def turned_fixture():
    """(fixed bool [48,64,56], moving bool, to_fixed [4,4]): the shape, the same shape turned 150 degrees about z and 15
    degrees about x (about the ellipsoid's centre) and shifted by (2, -3, 1.5), sampled on the same grid, and the true
    matrix moving -> fixed."""
    import registration_ref as G
    grid = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in FIXTURE_SHAPE], indexing="ij"), axis=-1)
    motion = (G.rigid((0.0, 0.0, 0.0), (2.0, -3.0, 1.5)) @ G.rigid((np.deg2rad(150.0), 0.0, 0.0), (0.0, 0.0, 0.0), FIXTURE_CENTRE)
              @ G.rigid((0.0, 0.0, np.deg2rad(15.0)), (0.0, 0.0, 0.0), FIXTURE_CENTRE))
    to_fixed = np.linalg.inv(motion)
    moving = fixture_shape(G.apply(to_fixed, grid.reshape(-1, 3)).reshape(grid.shape))
    return fixture_shape(grid), moving, to_fixed


def surface_voxels(mask):
    """float32 [P,3] indices of mask & ~binary_erosion(mask), in C order (registration.surface_points at unit spacing)."""
    from scipy import ndimage as ndi
    return np.argwhere(mask & ~ndi.binary_erosion(mask)).astype(np.float32)


def largest_point_error(M, points, truth):
    import registration_ref as G
    return float(np.sqrt(((G.apply(M, points) - G.apply(truth, points)) ** 2).sum(1)).max())
