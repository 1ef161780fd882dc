"""numpy restatement of include/jaicov_forms.h (csrc/forms.hip): planes, spheres, lines and circles through adjusted points as a
Gauss-Helmert model with the members' whole cofactor block, the same formulas in the header's order with np.linalg for the solves.

fit_form is the restatement.  fit_form_bordered is a second, independent route that only tests/test_form_reference.py uses: all
parameters free, the constraints (|n| = 1 and so on) written out, the bordered system solved with np.linalg.solve."""
import numpy as np

PLANE, SPHERE, LINE, CIRCLE = range(4)
KINDS = {"plane": PLANE, "sphere": SPHERE, "line": LINE, "circle": CIRCLE}
PARTIAL, TOO_SMALL, TOO_LARGE, DEGENERATE, SINGULAR, NOT_FINITE, NOT_CONVERGED = 1, 2, 4, 8, 16, 32, 64
MEMBER_UNTESTED = 1
MAX_ROWS, COLUMNS, QPP_COLUMNS, MEMBER_COLUMNS, MAX_PARAMS = 64, 20, 28, 7, 7
CONDITIONS = (1, 1, 2, 2)        # c
FREE = (3, 4, 4, 6)              # u
LEAST = (3, 4, 2, 3)             # least k
REPORTED = (4, 4, 6, 7)          # parameters reported
FATAL = TOO_SMALL | TOO_LARGE | DEGENERATE | SINGULAR | NOT_FINITE


def basis(n):
    """e1, e2 of the tangent plane of the unit vector n"""
    k = int(np.argmin(np.abs(n)))                      # the first among equals
    e = np.zeros(3); e[k] = 1.0
    e1 = np.cross(e, n); e1 = e1 / np.linalg.norm(e1)
    return e1, np.cross(n, e1)


def sign_of(n):
    return -1.0 if n[int(np.argmax(np.abs(n)))] < 0.0 else 1.0


def gather_block(Q, cols):
    """the members' block of the symmetric Q; cols (3 k,), a fixed coordinate (< 0) is a zero row and column"""
    cols = np.asarray(cols).ravel()
    out = np.zeros((cols.size, cols.size))
    ok = cols >= 0
    out[np.ix_(ok, ok)] = Q[np.ix_(cols[ok], cols[ok])]
    return out


def rows_of(kind, xh, n, c, r):
    """B (m, 3), A (m, u), f (m) at the corrected centred members xh and the parameters (n: n or t; c: c or x0; r: r or d_c)"""
    k = xh.shape[0]
    cc, u = CONDITIONS[kind], FREE[kind]
    B = np.zeros((cc * k, 3)); A = np.zeros((cc * k, u)); f = np.zeros(cc * k)
    if kind in (PLANE, LINE, CIRCLE):
        e1, e2 = basis(n)
    for i in range(k):
        x = xh[i]
        if kind == PLANE:
            B[i] = n; A[i] = [e1 @ x, e2 @ x, -1.0]; f[i] = n @ x - r
        elif kind == SPHERE:
            dx = x - c; rho = np.linalg.norm(dx); g = dx / rho
            B[i] = g; A[i] = [-g[0], -g[1], -g[2], -1.0]; f[i] = rho - r
        elif kind == LINE:
            dx = x - c; s = n @ dx
            B[2 * i] = e1; A[2 * i] = [-1.0, 0.0, -s, 0.0]; f[2 * i] = e1 @ dx
            B[2 * i + 1] = e2; A[2 * i + 1] = [0.0, -1.0, 0.0, -s]; f[2 * i + 1] = e2 @ dx
        else:
            dx = x - c; rho = np.linalg.norm(dx); g = dx / rho
            B[2 * i] = n; A[2 * i] = [-n[0], -n[1], -n[2], e1 @ dx, e2 @ dx, 0.0]; f[2 * i] = n @ dx
            B[2 * i + 1] = g; A[2 * i + 1] = [-g[0], -g[1], -g[2], 0.0, 0.0, -1.0]; f[2 * i + 1] = rho - r
    return B, A, f


def expand_B(B, k, cc):
    """the m x 3k matrix of the rows B"""
    Bf = np.zeros((cc * k, 3 * k))
    for r in range(cc * k):
        Bf[r, 3 * (r // cc):3 * (r // cc) + 3] = B[r]
    return Bf


def start_values(kind, x):
    """(n, c, r) or a status: the header's start values from the centred members x"""
    S = x.T @ x
    lam, E = np.linalg.eigh(S)
    lam, E = lam[::-1], E[:, ::-1].T                   # falling, rows
    n = np.zeros(3); c = np.zeros(3); r = 0.0
    if kind in (PLANE, CIRCLE):
        if lam[1] <= 1e-12 * lam[0]:
            return DEGENERATE
        n = E[2].copy()
    if kind == LINE:
        if not lam[0] > 0.0:
            return DEGENERATE
        n = E[0].copy()
    if kind == SPHERE:
        Am = np.c_[-2.0 * x, np.ones(len(x))]
        b = -(x * x).sum(1)
    elif kind == CIRCLE:
        e1, e2 = basis(n)
        p = np.c_[x @ e1, x @ e2]
        Am = np.c_[-2.0 * p, np.ones(len(x))]
        b = -(p * p).sum(1)
    if kind in (SPHERE, CIRCLE):
        Nm = Am.T @ Am
        s = 1.0 / np.sqrt(np.diag(Nm))
        Ns = Nm * np.outer(s, s)
        if np.linalg.eigvalsh(Ns)[0] <= 2.0 ** -26.5:         # the solve's pivot rule, as an eigenvalue
            return DEGENERATE
        th = np.linalg.solve(Nm, Am.T @ b)
        r2 = th[:-1] @ th[:-1] - th[-1]
        if not r2 > 0.0:
            return DEGENERATE
        r = np.sqrt(r2)
        c = th[:3].copy() if kind == SPHERE else th[0] * e1 + th[1] * e2
    return n, c, r


def distances(kind, x, n, c, r):
    if kind == PLANE:
        return x @ n - r
    if kind == SPHERE:
        return np.linalg.norm(x - c, axis=1) - r
    dx = x - c
    s = dx @ n
    perp = np.linalg.norm(dx - np.outer(s, n), axis=1)
    if kind == LINE:
        return perp
    return np.sqrt(s * s + (perp - r) ** 2)


def jacobian(kind, n, c, e1, e2, G):
    """J: tangent coordinates -> reported parameters (the header's table)"""
    J = np.zeros((REPORTED[kind], FREE[kind]))
    if kind == PLANE:
        J[0:3, 0] = e1; J[0:3, 1] = e2; J[3] = [e1 @ G, e2 @ G, 1.0]
    elif kind == SPHERE:
        J = np.eye(4)
    elif kind == LINE:
        J[0:3, 0] = e1; J[0:3, 1] = e2; J[0:3, 2] = -(e1 @ c) * n; J[0:3, 3] = -(e2 @ c) * n
        J[3:6, 2] = e1; J[3:6, 3] = e2
    else:
        J[0:3, 0:3] = np.eye(3); J[3:6, 3] = e1; J[3:6, 4] = e2; J[6, 5] = 1.0
    return J


def fit_form(kind, X, Qll, sigma2, max_iterations=20, tol=0.0, partial=False):
    """One form.  X (k, 3) in the engine's frame, Qll (3k, 3k).  Returns a dict: out (20,), qpp (28,), member (k, 7), status,
    member_status (k,)."""
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
    sv = start_values(kind, x)
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
        elif kind == LINE:
            c = c + delta[0] * e1 + delta[1] * e2
            n = n + delta[2] * e1 + delta[3] * e2; n = n / np.linalg.norm(n)
            c = c - (n @ c) * n
            big = max(abs(delta[0]) / ext, abs(delta[1]) / ext, abs(delta[2]), abs(delta[3]))
        else:
            c = c + delta[0:3]
            n = n + delta[3] * e1 + delta[4] * e2; n = n / np.linalg.norm(n)
            r = r + delta[5]
            big = max(np.abs(delta[0:3]).max() / ext, abs(delta[5]) / ext, abs(delta[3]), abs(delta[4]))
        if not np.isfinite(big):
            return fail(NOT_FINITE, it)
        if big <= tol:
            converged = True
            break
    if not converged:
        res["status"] |= NOT_CONVERGED
    # the sign rule and the reported parameters
    sg = sign_of(n) if kind != SPHERE else 1.0
    J = jacobian(kind, n, c_lin, e1, e2, G)
    sgn = np.ones(npar)
    if kind == PLANE:
        sgn[:] = sg
    elif kind == LINE:
        sgn[3:6] = sg
    elif kind == CIRCLE:
        sgn[3:6] = sg
    n = sg * n
    if kind == PLANE:
        r = sg * r
    J = J * sgn[:, None]
    Qpp = J @ Ni @ J.T
    par = {PLANE: np.r_[n, r + n @ G], SPHERE: np.r_[c + G, r], LINE: np.r_[c + G, n], CIRCLE: np.r_[c + G, n, r]}[kind]
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
        if kind in (PLANE, LINE, CIRCLE):
            nab[0] = sg * nab[0]
        mem[i, 4:4 + cc] = nab
        if cc == 1:
            mem[i, 5] = np.nan
        mem[i, 6] = Ti
    return res


# ---- the second route: all parameters free, explicit constraints, one bordered system -------------------------------------------------

def fit_form_bordered(kind, X, Qll, max_iterations=50, tol=1e-13):
    """Returns (par, Qpp, omega, v): the reported parameters (frame and sign as fit_form), their cofactors, Omega and v (k, 3)."""
    X = np.asarray(X, float).reshape(-1, 3)
    k = X.shape[0]
    cc = CONDITIONS[kind]
    G = X.mean(0)
    x = X - G
    sv = start_values(kind, x)
    n, c, r = sv
    if kind == PLANE:
        p = np.r_[n, r]
    elif kind == SPHERE:
        p = np.r_[c, r]
    elif kind == LINE:
        p = np.r_[c, n]
    else:
        p = np.r_[c, n, r]
    npar = p.size
    v = np.zeros(3 * k)

    def model(p, xh):
        """f (m), B (m, 3k), A (m, npar); constraints h (q), H (q, npar)"""
        m = cc * k
        f = np.zeros(m); B = np.zeros((m, 3 * k)); A = np.zeros((m, npar))
        for i in range(k):
            xi = xh[3 * i:3 * i + 3]
            if kind == PLANE:
                nn, d = p[0:3], p[3]
                f[i] = nn @ xi - d; B[i, 3 * i:3 * i + 3] = nn; A[i] = np.r_[xi, -1.0]
            elif kind == SPHERE:
                dx = xi - p[0:3]; rho = np.linalg.norm(dx)
                f[i] = rho - p[3]; B[i, 3 * i:3 * i + 3] = dx / rho; A[i] = np.r_[-dx / rho, -1.0]
            elif kind == LINE:
                x0, t = p[0:3], p[3:6]
                e1, e2 = basis(t / np.linalg.norm(t))
                dx = xi - x0
                # the two components of the part of dx across t, in a basis held fixed during the step: f = E (dx - t (t.dx) / (t.t))
                E = np.vstack([e1, e2])
                tt = t @ t
                f[2 * i:2 * i + 2] = E @ (dx - t * (t @ dx) / tt)
                P = np.eye(3) - np.outer(t, t) / tt
                B[2 * i:2 * i + 2, 3 * i:3 * i + 3] = E @ P
                A[2 * i:2 * i + 2, 0:3] = -E @ P
                A[2 * i:2 * i + 2, 3:6] = -E * ((t @ dx) / tt)          # E t = 0 removes the other terms of d(P dx)/dt
            else:
                cen, nn, rad = p[0:3], p[3:6], p[6]
                dx = xi - cen; rho = np.linalg.norm(dx)
                f[2 * i] = nn @ dx; B[2 * i, 3 * i:3 * i + 3] = nn; A[2 * i] = np.r_[-nn, dx, 0.0]
                f[2 * i + 1] = rho - rad; B[2 * i + 1, 3 * i:3 * i + 3] = dx / rho; A[2 * i + 1] = np.r_[-dx / rho, 0.0, 0.0, 0.0, -1.0]
        if kind == PLANE:
            h = np.array([0.5 * (p[0:3] @ p[0:3] - 1.0)]); H = np.r_[p[0:3], 0.0][None, :]
        elif kind == SPHERE:
            h = np.zeros(0); H = np.zeros((0, npar))
        elif kind == LINE:
            h = np.array([0.5 * (p[3:6] @ p[3:6] - 1.0), p[3:6] @ p[0:3]])
            H = np.vstack([np.r_[0.0, 0.0, 0.0, p[3:6]], np.r_[p[3:6], p[0:3]]])
        else:
            h = np.array([0.5 * (p[3:6] @ p[3:6] - 1.0)]); H = np.r_[0.0, 0.0, 0.0, p[3:6], 0.0][None, :]
        return f, B, A, h, H

    xf = x.ravel()
    for _ in range(max_iterations):
        f, B, A, h, H = model(p, xf + v)
        w = f - B @ v
        M = B @ Qll @ B.T
        m, q = M.shape[0], H.shape[0]
        K = np.zeros((m + npar + q, m + npar + q))
        K[:m, :m] = M; K[:m, m:m + npar] = A; K[m:m + npar, :m] = A.T
        K[m:m + npar, m + npar:] = H.T; K[m + npar:, m:m + npar] = H
        rhs = np.r_[-w, np.zeros(npar), -h]
        # scale the rows and columns: the blocks differ by many orders of magnitude
        sm = np.sqrt(np.diag(M).mean()); sc = np.r_[1.0 / np.sqrt(np.diag(M)), sm * np.ones(npar), np.ones(q) / sm]
        sol = sc * np.linalg.solve(K * np.outer(sc, sc), sc * rhs)
        lam, dp = sol[:m], sol[m:m + npar]              # M lambda + A dp = -w
        v = Qll @ B.T @ lam
        p = p + dp
        if np.abs(dp).max() <= tol * max(1.0, np.abs(x).max()):
            break
    f, B, A, h, H = model(p, xf + v)
    M = B @ Qll @ B.T
    m, q = M.shape[0], H.shape[0]
    K = np.zeros((m + npar + q, m + npar + q))
    K[:m, :m] = M; K[:m, m:m + npar] = A; K[m:m + npar, :m] = A.T
    K[m:m + npar, m + npar:] = H.T; K[m + npar:, m:m + npar] = H
    sm = np.sqrt(np.diag(M).mean()); sc = np.r_[1.0 / np.sqrt(np.diag(M)), sm * np.ones(npar), np.ones(q) / sm]
    Ki = np.linalg.inv(K * np.outer(sc, sc)) * np.outer(sc, sc)
    Qpp = -Ki[m:m + npar, m:m + npar]
    omega = lam @ M @ lam
    # to the engine's frame and the sign rule
    T = np.eye(npar)
    if kind == PLANE:
        T[3, 0:3] = G
    par = p.copy()
    if kind == PLANE:
        par[3] = p[3] + p[0:3] @ G
    elif kind == SPHERE:
        par[0:3] += G
    else:
        par[0:3] += G
    Qpp = T @ Qpp @ T.T
    sgn = np.ones(npar)
    if kind == PLANE:
        sgn[:] = sign_of(p[0:3])
    elif kind in (LINE, CIRCLE):
        sgn[3:6] = sign_of(p[3:6])
    return par * sgn, Qpp * np.outer(sgn, sgn), omega, v.reshape(k, 3)


# ---- test scenes shared by the CPU and the GPU tests -----------------------------------------------------------------------------------

def points_on(kind, k, rng, size=1.0, centre=(0.0, 0.0, 0.0)):
    """k points exactly on a form of the kind, of extent about `size` around `centre`"""
    centre = np.asarray(centre, float)
    A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    if kind == PLANE:
        p = np.c_[rng.uniform(-1, 1, (k, 2)), np.zeros(k)]
    elif kind == SPHERE:
        p = rng.normal(size=(k, 3)); p /= np.linalg.norm(p, axis=1)[:, None]
    elif kind == LINE:
        p = np.c_[np.linspace(-1, 1, k) + rng.uniform(-0.3, 0.3, k) / k, np.zeros(k), np.zeros(k)]
    else:
        a = np.linspace(0.0, 2.0 * np.pi, k, endpoint=False) + rng.uniform(-0.5, 0.5, k) / k
        p = np.c_[np.cos(a), np.sin(a), np.zeros(k)]
    return centre + size * (p @ A.T)


def correlated_cofactors(k, rng, scale=1e-10, rho=0.0):
    """an SPD 3k x 3k matrix of magnitude `scale`; rho: the share of a part common to all points (strong inter-point correlation)"""
    R = rng.normal(size=(3 * k, 3 * k + 5))
    Q = R @ R.T / (3 * k + 5)
    if rho > 0.0:
        C = rng.normal(size=(3, 3)); C = C @ C.T / 3.0 + np.eye(3)
        Q = (1.0 - rho) * Q + rho * np.kron(np.ones((k, k)), C)
    return scale * Q


def block_diagonal(Q):
    out = np.zeros_like(Q)
    for i in range(0, Q.shape[0], 3):
        out[i:i + 3, i:i + 3] = Q[i:i + 3, i:i + 3]
    return out
