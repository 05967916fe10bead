"""NumPy float64 restatement of the similarity registration rule with the symmetric chamfer cost that
ctunet_amd/registration.py pins: the forward term (moving points against the fixed field), the backward term (fixed points,
pulled back through the inverse, against the moving field), the adjugate inverse, the sums of one accumulation and the
Levenberg-Marquardt iteration with 6 or 7 unknowns.  The sample, `apply`, `lerp`, the Rodrigues formula and the mean of the
finite points are tests/registration_ref.py's; every per-point expression is written in the order the kernel evaluates it
(numpy never fuses), so one accumulation differs from the device's only in the order of its sums."""
import numpy as np

import registration_ref as G


def triu(dof):
    """The entries of upper H, row by row."""
    return [(i, j) for i in range(dof) for j in range(i, dof)]


def scale_about(centre, s):
    """[4,4] of p -> s (p - centre) + centre."""
    c = np.asarray(centre, dtype=np.float64)
    M = np.eye(4)
    M[:3, :3] *= float(s)
    M[:3, 3] = c - float(s) * c
    return M


def inverse_adj(M):
    """(inverse [4,4], det) of the affine M by the adjugate: cofactors as differences of products,
    det = (a00 c00 + a01 c01) + a02 c02, entries adj / det, translation -((inv_a0 t_0 + inv_a1 t_1) + inv_a2 t_2)."""
    M = np.asarray(M, dtype=np.float64)
    a = M[:3, :3]
    c = np.empty((3, 3))
    inv = np.eye(4)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
                c[i, j] = a[i1, j1] * a[i2, j2] - a[i1, j2] * a[i2, j1]
        det = (a[0, 0] * c[0, 0] + a[0, 1] * c[0, 1]) + a[0, 2] * c[0, 2]
        for i in range(3):
            for j in range(3):
                inv[i, j] = c[j, i] / det
            inv[i, 3] = -((inv[i, 0] * M[0, 3] + inv[i, 1] * M[1, 3]) + inv[i, 2] * M[2, 3])
    return inv, float(det)


def invertible(inv, det):
    """The candidate's test: a finite positive determinant and a finite inverse."""
    return bool(np.isfinite(det) and det > 0.0 and np.all(np.isfinite(inv)))


def _rows(d, g, dof):
    with np.errstate(invalid="ignore", over="ignore"):
        cols = [d[:, 1] * g[:, 2] - d[:, 2] * g[:, 1], d[:, 2] * g[:, 0] - d[:, 0] * g[:, 2],
                d[:, 0] * g[:, 1] - d[:, 1] * g[:, 0], g[:, 0], g[:, 1], g[:, 2]]
        if dof == 7:
            cols.append((d[:, 0] * g[:, 0] + d[:, 1] * g[:, 1]) + d[:, 2] * g[:, 2])
    return np.stack(cols, axis=1)


def forward_terms(points, field, M, pivot, spacing, origin, bound, dof):
    """(J [P,dof], v [P], inlier [P]) of the moving points against the fixed field at M."""
    sp, org = G._triple(spacing, 1.0), G._triple(origin, 0.0)
    p = np.asarray(points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    q = G.apply(M, p)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (q - org) / sp
    v, gu, inside = G.sample(field, u)
    g = gu / sp
    inl = inside & (v <= bound)
    with np.errstate(invalid="ignore", over="ignore"):
        d = q - np.asarray(pivot, dtype=np.float64)
    return _rows(d, g, dof), v, inl


def backward_residual(fixed_points, moving_field, Minv, spacing, origin):
    """(w, gradient of G over the spacing, inside) at x = Minv y."""
    sp, org = G._triple(spacing, 1.0), G._triple(origin, 0.0)
    y = np.asarray(fixed_points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    x = G.apply(Minv, y)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x - org) / sp
    w, gu, inside = G.sample(moving_field, u)
    return w, gu / sp, inside


def backward_terms(fixed_points, moving_field, Minv, pivot, spacing, origin, bound, dof):
    """(J [Q,dof], w [Q], inlier [Q]) of the fixed points against the moving field at the inverse Minv."""
    y = np.asarray(fixed_points, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    w, g, inside = backward_residual(y, moving_field, Minv, spacing, origin)
    A = np.asarray(Minv, dtype=np.float64)[:3, :3]
    h = np.stack([-((g[:, 0] * A[0, a] + g[:, 1] * A[1, a]) + g[:, 2] * A[2, a]) for a in range(3)], axis=1)
    inl = inside & (w <= bound)
    with np.errstate(invalid="ignore", over="ignore"):
        d = y - np.asarray(pivot, dtype=np.float64)
    return _rows(d, h, dof), w, inl


def accumulate(points, field, M, Minv, pivot, fixed_points=None, moving_field=None, spacing=None, origin=None,
               moving_spacing=None, moving_origin=None, max_distance=None, dof=7):
    """The sums of one accumulation at M (inverse Minv; None: every backward point is a non-inlier) about `pivot`, forward
    points first, then backward points: dict with H [dof (dof + 1) / 2], b [dof], cost, count (both terms), count_backward and
    absH / absb / abscost = the same sums over the terms' absolute values."""
    bound = np.inf if max_distance is None else float(max_distance)
    J, v, inl = forward_terms(points, field, M, pivot, spacing, origin, bound, dof)
    nb = 0
    if fixed_points is not None and len(fixed_points):
        if Minv is None:
            Q = len(fixed_points)
            Jb, vb, ib = np.zeros((Q, dof)), np.zeros(Q), np.zeros(Q, dtype=bool)
        else:
            Jb, vb, ib = backward_terms(fixed_points, moving_field, Minv, pivot, moving_spacing, moving_origin, bound, dof)
        J, v, inl = np.concatenate([J, Jb]), np.concatenate([v, vb]), np.concatenate([inl, ib])
        nb = int(ib.sum())
    J = np.where(inl[:, None], J, 0.0)
    v = np.where(inl, v, 0.0)
    r = np.where(inl, v, bound if np.isfinite(bound) else 0.0)
    hterms = np.stack([J[:, i] * J[:, j] for i, j in triu(dof)], axis=1)
    bterms = J * v[:, None]
    cterms = r * r
    return dict(H=hterms.sum(0), b=bterms.sum(0), cost=cterms.sum(), count=int(inl.sum()), count_backward=nb,
                absH=np.abs(hterms).sum(0), absb=np.abs(bterms).sum(0), abscost=np.abs(cterms).sum())


def solve(Hu, b, lam, count, dof):
    """delta of (H + lam diag(H) + 1e-12 I) delta = -b by Cholesky, or None: fewer than `dof` inliers, a pivot that is not
    positive, or a result that is not finite."""
    if count < dof:
        return None
    A = np.zeros((dof, dof))
    for k, (i, j) in enumerate(triu(dof)):
        A[i, j] = A[j, i] = Hu[k]
    A = A + lam * np.diag(np.diag(A)) + 1e-12 * np.eye(dof)
    L = np.zeros((dof, dof))
    for j in range(dof):
        s = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not (s > 0.0 and np.isfinite(s)):
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, dof):
            L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    y = np.zeros(dof)
    for i in range(dof):
        y[i] = (-b[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    x = np.zeros(dof)
    for i in reversed(range(dof)):
        x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x if np.all(np.isfinite(x)) else None


def increment(delta, pivot, dof):
    """E = [L, pivot - L pivot + delta_t], L = exp(delta_s) Rod(delta_w) for 7 unknowns and Rod(delta_w) for 6."""
    L = G.rodrigues(delta[:3])
    if dof == 7:
        L = np.exp(delta[6]) * L
    E = np.eye(4)
    E[:3, :3] = L
    E[:3, 3] = (pivot - L @ pivot) + delta[3:6]
    return E


def register(points, field, fixed_points=None, moving_field=None, spacing=None, origin=None, moving_spacing=None,
             moving_origin=None, init=None, iterations=30, max_distance=None, dof=7):
    """(matrix [4,4], inverse [4,4], history [iterations + 1, 6] = (cost / (P + Q), inliers, lambda, accepted or -1, backward
    inliers, scale = cbrt(det)))."""
    points = np.asarray(points, dtype=np.float32)
    Q = 0 if fixed_points is None else len(fixed_points)
    n = points.shape[0] + Q
    mean = G.finite_mean(points)
    Mc = np.eye(4) if init is None else np.array(init, dtype=np.float64).reshape(4, 4)
    Mc[3] = (0.0, 0.0, 0.0, 1.0)
    Ic, dc = inverse_adj(Mc)
    alive = invertible(Ic, dc)                        # an init without an inverse: nothing ever moves
    if not alive:
        Ic, dc = None, 0.0                            # inverse = identity and scale = 0 in what is written
    M, Minv, det = Mc.copy(), (np.eye(4) if Ic is None else Ic.copy()), dc
    cost, lam = np.inf, 1e-3
    nu = dof * (dof + 1) // 2
    H, b, count, count_b, pivot = np.zeros(nu), np.zeros(dof), 0, 0, G.pivot_of(M, mean)
    history = np.zeros((iterations + 1, 6))
    for it in range(iterations + 1):
        pc = G.pivot_of(Mc, mean)
        acc = accumulate(points, field, Mc, Ic, pc, fixed_points, moving_field, spacing, origin, moving_spacing, moving_origin,
                         max_distance, dof)
        accepted = bool(acc["cost"] < cost)
        if accepted:
            M, cost, H, b, count, count_b, pivot = Mc.copy(), acc["cost"], acc["H"], acc["b"], acc["count"], \
                acc["count_backward"], pc
            if Ic is not None:
                Minv, det = Ic.copy(), dc
            lam = max(lam / 3.0, 1e-9)
        else:
            lam = min(lam * 10.0, 1e9)
        flag = 1.0 if accepted else 0.0
        delta = solve(H, b, lam, count, dof) if alive else None
        cand = None
        if delta is not None:
            cand = increment(delta, pivot, dof) @ M
            cand[3] = (0.0, 0.0, 0.0, 1.0)
            ci, cd = inverse_adj(cand)
            if not np.all(np.isfinite(cand)) or not invertible(ci, cd):
                cand = None
        if cand is None:
            flag = -1.0
        else:
            Mc, Ic, dc = cand, ci, cd
        history[it] = (cost / n if np.isfinite(cost) else cost, count, lam, flag, count_b, np.cbrt(det))
    return M, Minv, history
