"""NumPy float64 restatement of the rigid registration rule that ctunet_amd/registration.py pins: the trilinear sample of
the distance field with its analytic gradient, the per-point residual and Jacobian, the sums of one accumulation and the
Levenberg-Marquardt iteration.  Every per-point expression is written in the order the kernel evaluates it (numpy never
fuses), so one accumulation differs from the device's only in the order of its sums."""
import numpy as np

TRIU = [(i, j) for i in range(6) for j in range(i, 6)]          # the 21 entries of upper H, row by row
MIN_INLIERS = 6                                                 # fewer inliers than unknowns: the step is refused


def _triple(v, default):
    if v is None:
        return np.full(3, default, dtype=np.float64)
    return np.full(3, float(v)) if np.isscalar(v) else np.asarray(v, dtype=np.float64)


def apply(M, p):
    """q_a = ((m_a0 p_0 + m_a1 p_1) + m_a2 p_2) + m_a3 for float64 points [P,3]."""
    M = np.asarray(M, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((M[a, 0] * p[:, 0] + M[a, 1] * p[:, 1]) + M[a, 2] * p[:, 2]) + M[a, 3] for a in range(3)], axis=1)


def lerp(p, q, w):
    return p + w * (q - p)


def sample(field, u):
    """(v, dv/du [P,3], inside) of the trilinear interpolant of float32 `field` [D,H,W] at voxel coordinates u [P,3].
    inside iff u is finite and 0 <= u_a <= n_a - 1; i0_a = min(floor(u_a), n_a - 2); lerp x, then y, then z.  Points that
    are not inside get v = 0 and a zero gradient."""
    field = np.asarray(field)
    assert field.dtype == np.float32 and field.ndim == 3 and min(field.shape) >= 2
    n = np.array(field.shape, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = np.all(np.isfinite(u) & (u >= 0.0) & (u <= n - 1.0), axis=1)
    us = np.where(inside[:, None], u, 0.0)
    i0 = np.minimum(np.floor(us), n - 2.0)
    f = us - i0
    i0 = i0.astype(np.int64)
    z, y, x = i0[:, 0], i0[:, 1], i0[:, 2]
    c = [[[field[z + dz, y + dy, x + dx].astype(np.float64) for dx in (0, 1)] for dy in (0, 1)] for dz in (0, 1)]
    fz, fy, fx = f[:, 0], f[:, 1], f[:, 2]
    c00, c01 = lerp(c[0][0][0], c[0][0][1], fx), lerp(c[0][1][0], c[0][1][1], fx)
    c10, c11 = lerp(c[1][0][0], c[1][0][1], fx), lerp(c[1][1][0], c[1][1][1], fx)
    c0, c1 = lerp(c00, c01, fy), lerp(c10, c11, fy)
    v = lerp(c0, c1, fz)
    gz = c1 - c0
    gy = lerp(c01 - c00, c11 - c10, fz)
    gx = lerp(lerp(c[0][0][1] - c[0][0][0], c[0][1][1] - c[0][1][0], fy),
              lerp(c[1][0][1] - c[1][0][0], c[1][1][1] - c[1][1][0], fy), fz)
    g = np.stack([gz, gy, gx], axis=1)
    return np.where(inside, v, 0.0), np.where(inside[:, None], g, 0.0), inside


def finite_mean(points):
    """float64 mean of the points whose three coordinates are finite (0 without one)."""
    p = np.asarray(points, dtype=np.float64)
    ok = np.all(np.isfinite(p), axis=1)
    return p[ok].mean(axis=0) if ok.any() else np.zeros(3)


def pivot_of(M, mean):
    return apply(M, np.asarray(mean, dtype=np.float64)[None])[0]


def accumulate(points, field, M, pivot, spacing=None, origin=None, max_distance=None):
    """The sums of one accumulation at the matrix M about `pivot`: dict with H [21] (upper triangle, row by row), b [6],
    cost, count, and absH / absb / abscost = the same sums over the terms' absolute values."""
    sp, org = _triple(spacing, 1.0), _triple(origin, 0.0)
    bound = np.inf if max_distance is None else float(max_distance)
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    q = apply(M, p)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (q - org) / sp
    v, gu, inside = sample(field, u)
    g = gu / sp
    inl = inside & (v <= bound)
    with np.errstate(invalid="ignore", over="ignore"):
        d = q - np.asarray(pivot, dtype=np.float64)
        J = np.stack([d[:, 1] * g[:, 2] - d[:, 2] * g[:, 1], d[:, 2] * g[:, 0] - d[:, 0] * g[:, 2],
                      d[:, 0] * g[:, 1] - d[:, 1] * g[:, 0], g[:, 0], g[:, 1], g[:, 2]], axis=1)
    J = np.where(inl[:, None], J, 0.0)
    v = np.where(inl, v, 0.0)
    r = np.where(inl, v, bound if np.isfinite(bound) else 0.0)
    hterms = np.stack([J[:, i] * J[:, j] for i, j in TRIU], axis=1)
    bterms = J * v[:, None]
    cterms = r * r
    return dict(H=hterms.sum(0), b=bterms.sum(0), cost=cterms.sum(), count=int(inl.sum()),
                absH=np.abs(hterms).sum(0), absb=np.abs(bterms).sum(0), abscost=np.abs(cterms).sum())


def full(H21):
    H = np.zeros((6, 6))
    for k, (i, j) in enumerate(TRIU):
        H[i, j] = H[j, i] = H21[k]
    return H


def solve(H21, b, lam, count):
    """delta of (H + lam diag(H) + 1e-12 I) delta = -b by Cholesky, or None: fewer than MIN_INLIERS inliers, a pivot that
    is not positive, or a result that is not finite."""
    if count < MIN_INLIERS:
        return None
    A = full(H21)
    A = A + lam * np.diag(np.diag(A)) + 1e-12 * np.eye(6)
    L = np.zeros((6, 6))
    for j in range(6):
        s = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not (s > 0.0 and np.isfinite(s)):
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (-b[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    x = np.zeros(6)
    for i in reversed(range(6)):
        x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x if np.all(np.isfinite(x)) else None


def rodrigues(w):
    """exp of the skew matrix of w in the index order of the vectors: I + a K + b K K, a = sin t / t, b = (1 - cos t) / t^2
    (their series below t = 1e-4)."""
    w = np.asarray(w, dtype=np.float64)
    t2 = float(np.dot(w, w))
    t = np.sqrt(t2)
    if t < 1e-4:
        a, b = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0
    else:
        a, b = np.sin(t) / t, (1.0 - np.cos(t)) / t2
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + a * K + b * (K @ K)


def rigid(w, t, centre=(0.0, 0.0, 0.0)):
    """[4,4] of p -> Rod(w) (p - centre) + centre + t."""
    R = rodrigues(w)
    c = np.asarray(centre, dtype=np.float64)
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = c - R @ c + np.asarray(t, dtype=np.float64)
    return M


def inverse(M):
    """The closed form (R^T, -R^T t)."""
    inv = np.eye(4)
    inv[:3, :3] = M[:3, :3].T
    inv[:3, 3] = -(M[:3, :3].T @ M[:3, 3])
    return inv


def register(points, field, spacing=None, origin=None, init=None, iterations=30, max_distance=None):
    """(matrix [4,4], inverse [4,4], history [iterations + 1, 4] = (cost / P, inliers, lambda, accepted or -1))."""
    points = np.asarray(points, dtype=np.float32)
    P = points.shape[0]
    mean = finite_mean(points)
    Mc = np.eye(4) if init is None else np.array(init, dtype=np.float64).reshape(4, 4)
    M = Mc.copy()
    cost, lam = np.inf, 1e-3
    H, b, count, pivot = np.zeros(21), np.zeros(6), 0, pivot_of(M, mean)
    history = np.zeros((iterations + 1, 4))
    for it in range(iterations + 1):
        pc = pivot_of(Mc, mean)
        acc = accumulate(points, field, Mc, pc, spacing, origin, max_distance)
        accepted = bool(acc["cost"] < cost)
        if accepted:
            M, cost, H, b, count, pivot = Mc.copy(), acc["cost"], acc["H"], acc["b"], acc["count"], pc
            lam = max(lam / 3.0, 1e-9)
        else:
            lam = min(lam * 10.0, 1e9)
        flag = 1.0 if accepted else 0.0
        delta = solve(H, b, lam, count)
        cand = None
        if delta is not None:
            R = rodrigues(delta[:3])
            E = np.eye(4)
            E[:3, :3] = R
            E[:3, 3] = (pivot - R @ pivot) + delta[3:]
            cand = E @ M
            cand[3] = (0.0, 0.0, 0.0, 1.0)
            if not np.all(np.isfinite(cand)):
                cand = None
        if cand is None:
            flag = -1.0
        else:
            Mc = cand
        history[it] = (cost / P if np.isfinite(cost) else cost, count, lam, flag)
    return M, inverse(M), history
