"""numpy restatement of include/jaicov_surfaces.h (csrc/forms.hip, csrc/surfstart.h): cylinders and cones beside the four forms of
tests/form_reference.py, and start values from the caller for all six; the same formulas in the header's order with np.linalg for
the solves of the steps.

fit_surface is the restatement: for the kinds 0 .. 3 without a start it does what form_reference.fit_form does.  search is the start
search over the candidate axes, written out as the header has it (its 3 x 3 and 5 x 5 systems by a Cholesky factor of its own, so
that the pivot rule is the header's; all candidates are carried side by side in one array).  fit_surface_bordered is a second,
independent route that only tests/test_surface_reference.py uses: all seven parameters free, the constraints |t| = 1 (and t.x0 = 0
for the cylinder) written out, one bordered system."""
import numpy as np

import form_reference as F
from form_reference import (PLANE, SPHERE, LINE, CIRCLE, PARTIAL, TOO_SMALL, TOO_LARGE, DEGENERATE, SINGULAR, NOT_FINITE, NOT_CONVERGED,  # noqa: F401
                            MEMBER_UNTESTED, MAX_ROWS, COLUMNS, QPP_COLUMNS, MEMBER_COLUMNS, MAX_PARAMS, FATAL, basis, sign_of, gather_block,
                            expand_B, block_diagonal, correlated_cofactors)

CYLINDER, CONE = 4, 5
KINDS = dict(F.KINDS, cylinder=CYLINDER, cone=CONE)
CONDITIONS = F.CONDITIONS + (1, 1)
FREE = F.FREE + (5, 6)
LEAST = F.LEAST + (5, 6)
REPORTED = F.REPORTED + (7, 7)
REACH, N_CANDIDATES = 5, 301


def candidates():
    """the integer vectors of the header in its order, (301, 3)"""
    out = []
    for i in range(-REACH, REACH + 1):
        for j in range(-REACH, REACH + 1):
            for l in range(-REACH, REACH + 1):
                first = i if i != 0 else j if j != 0 else l
                if max(abs(i), abs(j), abs(l)) == REACH and first > 0:
                    out.append((i, j, l))
    return np.array(out, float)


def _solve_scaled(N, b):
    """x of N x = b for a stack of systems (c, n, n), (c, n) through V N V = U'U with V = 1 / sqrt(diag), column by column as the
    header has it; returns (x, ok), ok False where a pivot is <= 2^-40"""
    n = b.shape[1]
    d = np.einsum("cii->ci", N)
    V = np.where(d > 0.0, 1.0 / np.sqrt(np.where(d > 0.0, d, 1.0)), 1.0)
    A = N * V[:, :, None] * V[:, None, :]
    U = np.zeros_like(A)
    ok = np.ones(len(N), bool)
    for j in range(n):
        p = A[:, j, j] - (U[:, :j, j] * U[:, :j, j]).sum(1)
        ok &= p > 2.0 ** -40
        U[:, j, j] = np.sqrt(p)
        for i in range(j + 1, n):
            U[:, j, i] = (A[:, j, i] - (U[:, :j, i] * U[:, :j, j]).sum(1)) / U[:, j, j]
    y = np.zeros_like(b)
    for i in range(n):
        y[:, i] = (V[:, i] * b[:, i] - (U[:, :i, i] * y[:, :i]).sum(1)) / U[:, i, i]
    for i in range(n - 1, -1, -1):
        y[:, i] = (y[:, i] - (U[:, i, i + 1:] * y[:, i + 1:]).sum(1)) / U[:, i, i]
    return V * y, ok


def search(kind, x, G, ext):
    """the start row (7,) of a cylinder or a cone in the engine's frame from the centred members x, or None (no candidate left);
    every candidate at once, one row of the arrays each"""
    with np.errstate(all="ignore"):
        y = x / ext
        D = candidates()
        D = D / np.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])[:, None]
        E = np.array([basis(d) for d in D])                              # (c, 2, 3)
        q = np.einsum("cab,kb->cka", E, y)                               # (c, k, 2)
        s = y @ D.T                                                      # (k, c)
        s = s.T
        rhs = (q * q).sum(2)
        one = np.ones_like(s)
        A = np.stack([2.0 * q[:, :, 0], 2.0 * q[:, :, 1], one] + ([s * s, 2.0 * s] if kind == CONE else []), axis=2)
        th, ok = _solve_scaled(np.einsum("cka,ckb->cab", A, A), np.einsum("cka,ck->ca", A, rhs))
        rho = np.sqrt(((q - th[:, None, 0:2]) ** 2).sum(2))
        if kind == CYLINDER:
            r2 = th[:, 2] + (th[:, 0:2] * th[:, 0:2]).sum(1)
            ok &= r2 > 0.0
            r = np.sqrt(r2)
            cost = ((rho - r[:, None]) ** 2).sum(1)
        else:
            ok &= th[:, 3] > 0.0
            kappa = np.sqrt(th[:, 3]); r0 = th[:, 4] / kappa; sa = -(r0 / kappa)
            sg = np.where((s - sa[:, None]).sum(1) < 0.0, -1.0, 1.0)
            cost = ((rho - (sg * kappa)[:, None] * (s - sa[:, None])) ** 2).sum(1) / (1.0 + th[:, 3])
        cost = np.where(ok & np.isfinite(cost), cost, np.inf)
        w = int(np.argmin(cost))                                         # the first among equals
        if not cost[w] < np.inf:
            return None
        d, (e1, e2) = D[w], E[w]
        if kind == CYLINDER:
            return np.r_[ext * (th[w, 0] * e1 + th[w, 1] * e2) + G, d, ext * r[w]]
        return np.r_[ext * ((th[w, 0] * e1 + th[w, 1] * e2) + sa[w] * d) + G, sg[w] * d, np.arctan(kappa[w])]


def working_form(kind, row, G):
    """(n, c, r) of a start row given in the engine's frame, or DEGENERATE"""
    n = np.zeros(3); c = np.zeros(3); r = 0.0
    with np.errstate(all="ignore"):
        if kind == PLANE:
            n = np.array(row[0:3], float); r = float(row[3])
        else:
            c = np.array(row[0:3], float) - G
            if kind == SPHERE:
                r = float(row[3])
            else:
                n = np.array(row[3:6], float)
            if kind in (CIRCLE, CYLINDER, CONE):
                r = float(row[6])
        if kind != SPHERE:
            l = np.sqrt(n @ n)
            if not l > 0.0:
                return DEGENERATE
            n = n / l
        if kind == PLANE:
            r = r - n @ G
        if kind in (LINE, CYLINDER):
            c = c - (n @ c) * n
        if kind in (SPHERE, CIRCLE, CYLINDER) and not r > 0.0:
            return DEGENERATE
        if kind == CONE and not 0.0 < r < np.pi:
            return DEGENERATE
    return n, c, r


def rows_of(kind, xh, n, c, r):
    """B (m, 3), A (m, u), f (m) at the corrected centred members xh; n: n or t, c: c, x0 or apex, r: r, d_c or alpha"""
    if kind < CYLINDER:
        return F.rows_of(kind, xh, n, c, r)
    k = xh.shape[0]
    B = np.zeros((k, 3)); A = np.zeros((k, FREE[kind])); f = np.zeros(k)
    e1, e2 = basis(n)
    ca, sa = np.cos(r), np.sin(r)
    with np.errstate(all="ignore"):
        for i in range(k):
            dx = xh[i] - c
            s = n @ dx
            p = dx - s * n
            rho = np.sqrt(p @ p)
            g = p / rho
            if kind == CYLINDER:
                B[i] = g; A[i] = [-(g @ e1), -(g @ e2), -s * (g @ e1), -s * (g @ e2), -1.0]; f[i] = rho - r
            else:
                h = g * ca - n * sa
                q = s * ca + rho * sa
                B[i] = h; A[i] = np.r_[-h, -q * (g @ e1), -q * (g @ e2), -q]; f[i] = rho * ca - s * sa
    return B, A, f


def distances(kind, x, n, c, r):
    if kind < CYLINDER:
        return F.distances(kind, x, n, c, r)
    dx = x - c
    s = dx @ n
    perp = np.linalg.norm(dx - np.outer(s, n), axis=1)
    return perp - r if kind == CYLINDER else perp * np.cos(r) - s * np.sin(r)


def jacobian(kind, n, c, e1, e2, G):
    if kind < CYLINDER:
        return F.jacobian(kind, n, c, e1, e2, G)
    J = np.zeros((7, FREE[kind]))
    if kind == CYLINDER:
        J[0:6, 0:4] = F.jacobian(LINE, n, c, e1, e2, G)
        J[6, 4] = 1.0
    else:
        J[0:3, 0:3] = np.eye(3); J[3:6, 3] = e1; J[3:6, 4] = e2; J[6, 5] = 1.0
    return J


def fit_surface(kind, X, Qll, sigma2, start=None, max_iterations=20, tol=0.0, partial=False):
    """One form of the kinds 0 .. 5.  X (k, 3) in the engine's frame, Qll (3k, 3k); start: None, or the reported parameters in the
    engine's frame (a first entry NaN: none).  Returns what form_reference.fit_form returns."""
    X = np.asarray(X, float).reshape(-1, 3)
    k = X.shape[0]
    cc, u, npar = CONDITIONS[kind], FREE[kind], REPORTED[kind]
    m = cc * k
    tol = 1e-12 if tol == 0.0 else tol
    res = dict(out=np.full(COLUMNS, np.nan), qpp=np.full(QPP_COLUMNS, np.nan), member=np.full((k, MEMBER_COLUMNS), np.nan),
               status=PARTIAL if partial else 0, member_status=np.zeros(k, np.int32))

    def fail(bit, it=0):
        res["status"] |= bit
        res["out"][19] = it
        return res

    if k < LEAST[kind]:
        return fail(TOO_SMALL)
    if m > MAX_ROWS:
        return fail(TOO_LARGE)
    G = np.zeros(3)
    for i in range(k):
        G = G + X[i]
    G = G / k
    x = X - G
    ext = np.sqrt((x * x).sum(1)).max()
    if not np.isfinite(x).all():
        return fail(NOT_FINITE)
    if start is not None and np.isnan(np.asarray(start, float).ravel()[0]):
        start = None
    if start is None and kind >= CYLINDER:
        start = search(kind, x, G, ext)
        if start is None:
            return fail(DEGENERATE)
    sv = F.start_values(kind, x) if start is None else working_form(kind, np.asarray(start, float).ravel(), G)
    if isinstance(sv, int):
        return fail(sv)
    n, c, r = sv
    v = np.zeros((k, 3))
    it = 0
    converged = False
    while it < max_iterations:
        it += 1
        B, A, f = rows_of(kind, x + v, n, c, r)
        e1, e2 = basis(n) if kind != SPHERE else (None, None)
        c_lin = c.copy()
        Bf = expand_B(B, k, cc)
        w = f - Bf @ v.ravel()
        M = Bf @ Qll @ Bf.T
        if not (np.isfinite(M).all() and np.isfinite(w).all() and np.isfinite(A).all()):
            return fail(NOT_FINITE, it)
        d = np.diag(M)
        if not (d > 0.0).all():
            return fail(SINGULAR, it)
        s = 1.0 / np.sqrt(d)
        Ms = M * np.outer(s, s)
        try:
            L = np.linalg.cholesky(Ms)
        except np.linalg.LinAlgError:
            return fail(SINGULAR, it)
        if (np.diag(L) ** 2 <= 2.0 ** -26.5).any():
            return fail(SINGULAR, it)
        Mi = np.linalg.inv(Ms) * np.outer(s, s)
        N = A.T @ Mi @ A
        with np.errstate(all="ignore"):
            sn = 1.0 / np.sqrt(np.diag(N))
        if not np.isfinite(sn).all() or np.linalg.eigvalsh(N * np.outer(sn, sn))[0] <= 2.0 ** -26.5:
            return fail(SINGULAR, it)
        Ni = np.linalg.inv(N)
        delta = -Ni @ (A.T @ Mi @ w)
        lam = -Mi @ (A @ delta + w)
        omega = lam @ M @ lam
        v = (Qll @ Bf.T @ lam).reshape(k, 3)
        if kind == PLANE:
            n = n + delta[0] * e1 + delta[1] * e2; n = n / np.linalg.norm(n)
            r = r + delta[2]
            big = max(abs(delta[0]), abs(delta[1]), abs(delta[2]) / ext)
        elif kind == SPHERE:
            c = c + delta[0:3]; r = r + delta[3]
            big = np.abs(delta).max() / ext
        elif kind in (LINE, CYLINDER):
            c = c + delta[0] * e1 + delta[1] * e2
            n = n + delta[2] * e1 + delta[3] * e2; n = n / np.linalg.norm(n)
            c = c - (n @ c) * n
            big = max(abs(delta[0]) / ext, abs(delta[1]) / ext, abs(delta[2]), abs(delta[3]))
            if kind == CYLINDER:
                r = r + delta[4]
                big = max(big, abs(delta[4]) / ext)
        elif kind == CIRCLE:
            c = c + delta[0:3]
            n = n + delta[3] * e1 + delta[4] * e2; n = n / np.linalg.norm(n)
            r = r + delta[5]
            big = max(np.abs(delta[0:3]).max() / ext, abs(delta[5]) / ext, abs(delta[3]), abs(delta[4]))
        else:
            c = c + delta[0:3]
            n = n + delta[3] * e1 + delta[4] * e2; n = n / np.linalg.norm(n)
            r = r + delta[5]
            big = max(np.abs(delta[0:3]).max() / ext, abs(delta[3]), abs(delta[4]), abs(delta[5]))
        if not np.isfinite(big):
            return fail(NOT_FINITE, it)
        if (kind == CYLINDER and not r > 0.0) or (kind == CONE and not 0.0 < r < np.pi):
            return fail(DEGENERATE, it)
        if big <= tol:
            converged = True
            break
    if not converged:
        res["status"] |= NOT_CONVERGED
    # the sign rule and the reported parameters
    if kind == CONE:
        sg = -1.0 if r > 0.5 * np.pi else 1.0
    else:
        sg = sign_of(n) if kind != SPHERE else 1.0
    J = jacobian(kind, n, c_lin, e1, e2, G)
    sgn = np.ones(npar)
    if kind == PLANE:
        sgn[:] = sg
    elif kind in (LINE, CIRCLE, CYLINDER):
        sgn[3:6] = sg
    elif kind == CONE:
        sgn[3:7] = sg
    n = sg * n
    if kind == PLANE:
        r = sg * r
    if kind == CONE and sg < 0.0:
        r = np.pi - r
    J = J * sgn[:, None]
    Qpp = J @ Ni @ J.T
    par = {PLANE: np.r_[n, r + n @ G], SPHERE: np.r_[c + G, r], LINE: np.r_[c + G, n]}.get(kind, np.r_[c + G, n, r])
    out = res["out"]
    out[0:npar] = par
    out[7:7 + npar] = np.sqrt(sigma2 * np.maximum(np.diag(Qpp), 0.0))
    fdof = m - u
    out[14] = omega; out[15] = fdof; out[16] = omega / (fdof * sigma2) if fdof > 0 else np.nan
    dist = distances(kind, x, n, c, r)
    out[17] = np.abs(dist).max(); out[18] = np.sqrt((dist * dist).sum() / k); out[19] = it
    q7 = np.zeros((MAX_PARAMS, MAX_PARAMS)); q7[:npar, :npar] = Qpp
    res["qpp"] = q7[np.triu_indices(MAX_PARAMS)]
    # the members
    Qlam = Mi - Mi @ A @ Ni @ A.T @ Mi
    mem = res["member"]
    mem[:, 0:3] = v
    mem[:, 3] = dist
    for i in range(k):
        sl = slice(cc * i, cc * i + cc)
        Qi = Qlam[sl, sl]; li = lam[sl].copy()
        ok = fdof > 0
        if ok and cc == 1:
            ok = Qi[0, 0] > 1e-12 * Mi[sl, sl][0, 0]
        elif ok:
            Mii = Mi[sl, sl]
            p1 = Qi[0, 0]
            p2 = Qi[1, 1] - Qi[0, 1] * Qi[0, 1] / Qi[0, 0] if p1 > 0 else -1.0
            ok = p1 > 1e-12 * Mii[0, 0] and p2 > 1e-12 * Mii[1, 1]
        if not ok:
            res["member_status"][i] |= MEMBER_UNTESTED
            continue
        nab = -np.linalg.solve(Qi, li)
        Ti = -(li @ nab) / (cc * sigma2)
        if kind in (PLANE, LINE, CIRCLE, CONE):
            nab[0] = sg * nab[0]
        mem[i, 4:4 + cc] = nab
        if cc == 1:
            mem[i, 5] = np.nan
        mem[i, 6] = Ti
    return res


# ---- the second route: all seven parameters free, explicit constraints, one bordered system -----------------------------------------

def fit_surface_bordered(kind, X, Qll, start, max_iterations=50, tol=1e-13):
    """A cylinder or a cone from the start row `start` (engine's frame).  Returns (par, Qpp, omega, v) as
    form_reference.fit_form_bordered does: frame and sign as fit_surface."""
    X = np.asarray(X, float).reshape(-1, 3)
    k = X.shape[0]
    G = X.mean(0)
    x = X - G
    n, c, r = working_form(kind, np.asarray(start, float), G)
    p = np.r_[c, n, r]
    v = np.zeros(3 * k)

    def model(p, xh):
        f = np.zeros(k); B = np.zeros((k, 3 * k)); A = np.zeros((k, 7))
        x0, t, r = p[0:3], p[3:6], p[6]
        tt = t @ t; lt = np.sqrt(tt)
        for i in range(k):
            dx = xh[3 * i:3 * i + 3] - x0
            td = t @ dx
            pv = dx - t * td / tt
            rho = np.linalg.norm(pv); g = pv / rho
            if kind == CYLINDER:
                f[i] = rho - r; B[i, 3 * i:3 * i + 3] = g; A[i] = np.r_[-g, -(td / tt) * g, -1.0]
            else:
                ca, sa = np.cos(r), np.sin(r)
                s = td / lt
                h = g * ca - (t / lt) * sa
                f[i] = rho * ca - s * sa; B[i, 3 * i:3 * i + 3] = h
                A[i] = np.r_[-h, -((td / tt) * ca + rho * sa / lt) * g, -(rho * sa + s * ca)]
        if kind == CYLINDER:
            h = np.array([0.5 * (tt - 1.0), t @ x0]); H = np.vstack([np.r_[0.0, 0.0, 0.0, t, 0.0], np.r_[t, x0, 0.0]])
        else:
            h = np.array([0.5 * (tt - 1.0)]); H = np.r_[0.0, 0.0, 0.0, t, 0.0][None, :]
        return f, B, A, h, H

    def system(p, v):
        f, B, A, h, H = model(p, x.ravel() + v)
        M = B @ Qll @ B.T
        m, q = k, H.shape[0]
        K = np.zeros((m + 7 + q, m + 7 + q))
        K[:m, :m] = M; K[:m, m:m + 7] = A; K[m:m + 7, :m] = A.T
        K[m:m + 7, m + 7:] = H.T; K[m + 7:, m:m + 7] = H
        sm = np.sqrt(np.diag(M).mean()); sc = np.r_[1.0 / np.sqrt(np.diag(M)), sm * np.ones(7), np.ones(q) / sm]
        return f, B, M, K, sc, h

    for _ in range(max_iterations):
        f, B, M, K, sc, h = system(p, v)
        rhs = np.r_[-(f - B @ v), np.zeros(7), -h]
        sol = sc * np.linalg.solve(K * np.outer(sc, sc), sc * rhs)
        lam, dp = sol[:k], sol[k:k + 7]
        v = Qll @ B.T @ lam
        p = p + dp
        if np.abs(dp).max() <= tol * max(1.0, np.abs(x).max()):
            break
    f, B, M, K, sc, h = system(p, v)
    Ki = np.linalg.inv(K * np.outer(sc, sc)) * np.outer(sc, sc)
    Qpp = -Ki[k:k + 7, k:k + 7]
    omega = lam @ M @ lam
    par = p.copy()
    par[0:3] += G
    sgn = np.ones(7)
    if kind == CYLINDER:
        sgn[3:6] = sign_of(p[3:6])
    elif p[6] > 0.5 * np.pi:
        sgn[3:7] = -1.0
        par[6] = par[6] - np.pi                 # times -1 below: pi - alpha
    return par * sgn, Qpp * np.outer(sgn, sgn), omega, v.reshape(k, 3)


# ---- test scenes shared by the CPU and the GPU tests ------------------------------------------------------------------------------------

def surface_points(kind, k, rng, size=1.0, centre=(0.0, 0.0, 0.0), arc=None):
    """k points exactly on a random cylinder or cone, spread over an arc of 120 to 360 degrees (or `arc`, radians) and along the axis,
    all of them within `size` of `centre` (0.7 size across the axis and along it); returns (points, the parameters x0 | apex, t,
    r | alpha)"""
    centre = np.asarray(centre, float)
    A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    arc = rng.uniform(2.0 * np.pi / 3.0, 2.0 * np.pi) if arc is None else arc
    a = rng.uniform(0.0, 2.0 * np.pi) + np.linspace(0.0, arc, k, endpoint=False) + rng.uniform(-0.4, 0.4, k) * arc / k
    t = A[:, 2]
    if kind == CYLINDER:
        r = size * rng.uniform(0.3, 0.7)
        s = 0.7 * size * rng.permutation(np.linspace(-1.0, 1.0, k) + rng.uniform(-0.4, 0.4, k) / k)
        pts = centre + np.outer(r * np.cos(a), A[:, 0]) + np.outer(r * np.sin(a), A[:, 1]) + np.outer(s, t)
        return pts, np.r_[centre, t, r]
    alpha = rng.uniform(np.radians(15.0), np.radians(65.0))
    scale = size * min(1.0, 0.35 / np.tan(alpha))
    s = scale * rng.permutation(np.linspace(0.6, 2.0, k) + rng.uniform(-0.4, 0.4, k) / k)     # distances from the apex along the axis
    rad = s * np.tan(alpha)
    apex = centre - 1.3 * scale * t
    pts = apex + np.outer(rad * np.cos(a), A[:, 0]) + np.outer(rad * np.sin(a), A[:, 1]) + np.outer(s, t)
    return pts, np.r_[apex, t, alpha]


def same_surface(kind, par, truth, ext, tol=1e-2):
    """do the reported parameters `par` describe the surface `truth` (up to the sign of a cylinder's axis), to tol of the extent?"""
    if not np.isfinite(par[:7]).all():
        return False
    t, t0 = par[3:6], truth[3:6]
    if kind == CYLINDER:
        if t @ t0 < 0.0:
            t = -t
        d = par[0:3] - truth[0:3]
        off = np.linalg.norm(d - (d @ t0) * t0)
        return bool(np.linalg.norm(t - t0) <= tol and off <= tol * ext and abs(par[6] - truth[6]) <= tol * ext)
    return bool(np.linalg.norm(t - t0) <= tol and np.linalg.norm(par[0:3] - truth[0:3]) <= 10.0 * tol * ext and abs(par[6] - truth[6]) <= tol)
