"""numpy restatement of include/jaicov_precision.h: the 3 x 3 cyclic Jacobi with its rotation order, stopping rule, sorting and sign
rule; the figures of a point and of a length; the start block of the component iteration and the subspace iteration with
Rayleigh-Ritz and CholeskyQR2.  Written from the header, in its order of operations; host side only."""
import math

import numpy as np

EPS = 2.0 ** -52
SWEEPS = 30
PARTIAL, NEGATIVE, NOT_FINITE, DEGENERATE = 1, 2, 4, 8
MASK = (1 << 64) - 1


def gather(Q, cols):
    """Q[cols, cols] of a full symmetric matrix; a column < 0 (fixed coordinate) is a zero row and column."""
    cols = np.asarray(cols)
    ok = cols >= 0
    B = np.zeros((cols.size, cols.size))
    B[np.ix_(ok, ok)] = Q[np.ix_(cols[ok], cols[ok])]
    return B


def _rotate(a, v, p, q, r):
    apq = a[p][q]
    if abs(apq) <= EPS * math.sqrt(abs(a[p][p] * a[q][q])):
        return False
    th = (a[q][q] - a[p][p]) / (2.0 * apq)
    t = (1.0 if th >= 0.0 else -1.0) / (abs(th) + math.sqrt(th * th + 1.0))
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    a[p][p] -= t * apq
    a[q][q] += t * apq
    a[p][q] = a[q][p] = 0.0
    arp, arq = a[r][p], a[r][q]
    a[r][p] = a[p][r] = c * arp - s * arq
    a[r][q] = a[q][r] = s * arp + c * arq
    for k in range(3):
        vp, vq = v[k][p], v[k][q]
        v[k][p] = c * vp - s * vq
        v[k][q] = s * vp + c * vq
    return True


def sign_rule(x):
    """The component of largest magnitude positive (the first among equals)."""
    x = np.asarray(x, float)
    i = int(np.argmax(np.abs(x)))
    return -x if x[i] < 0 else x


def jacobi3(C):
    """(eigenvalues descending, V with the eigenvectors as columns, sweeps) of the symmetric 3 x 3 block C."""
    C = np.asarray(C, float)
    m = max(C[0, 0], C[1, 1], C[2, 2])
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    l = [0.0, 0.0, 0.0]
    sweeps = 0
    if m != 0.0:
        a = [[float(C[i, j]) / m for j in range(3)] for i in range(3)]
        for sweeps in range(1, SWEEPS + 1):
            any_ = _rotate(a, v, 0, 1, 2)
            any_ = _rotate(a, v, 0, 2, 1) or any_
            any_ = _rotate(a, v, 1, 2, 0) or any_
            if not any_:
                break
        l = [m * a[k][k] for k in range(3)]
    V = np.array(v)
    l = np.array(l)
    for i, j in ((0, 1), (1, 2), (0, 1)):
        if l[j] > l[i]:
            l[[i, j]] = l[[j, i]]
            V[:, [i, j]] = V[:, [j, i]]
    for c in range(3):
        V[:, c] = sign_rule(V[:, c])
    return l, V, sweeps


def point_figures(Q3, sigma2, k3=1.0, k2=1.0, fixed=(False, False, False)):
    """One row of jaicov_prec_points (22 entries) and its status, from the gathered cofactor block."""
    Q3 = np.asarray(Q3, float)
    st = PARTIAL if any(fixed) else 0
    if not (np.isfinite(Q3).all() and math.isfinite(sigma2 + k3 + k2)):
        return np.full(22, np.nan), st | NOT_FINITE
    tr = (Q3[0, 0] + Q3[1, 1]) + Q3[2, 2]
    l, V, _ = jacobi3(Q3)
    if l[2] < -1e-12 * tr:
        st |= NEGATIVE
    out = np.zeros(22)
    out[0:3] = np.sqrt(sigma2 * np.maximum(np.diag(Q3), 0.0))
    out[3] = math.sqrt(sigma2 * max(tr, 0.0))
    out[4:7] = k3 * np.sqrt(sigma2 * np.maximum(l, 0.0))
    out[7:16] = V.T.ravel()
    hm, hd = 0.5 * (Q3[0, 0] + Q3[1, 1]), 0.5 * (Q3[0, 0] - Q3[1, 1])
    hw = math.hypot(hd, Q3[0, 1])
    out[16] = k2 * math.sqrt(sigma2 * max(hm + hw, 0.0))
    out[17] = k2 * math.sqrt(sigma2 * max(hm - hw, 0.0))
    d = 0.5 * math.atan2(2.0 * Q3[0, 1], Q3[0, 0] - Q3[1, 1])
    if d < 0.0:
        d += math.pi
    if d >= math.pi:
        d = 0.0
    out[18] = d
    out[19:22] = l
    return out, st


def length_figures(XA, XB, Q6, sigma2, fixed=False):
    """One row of jaicov_prec_lengths (L, sigma_L, sigma of the three coordinate differences) and its status."""
    XA, XB, Q6 = np.asarray(XA, float), np.asarray(XB, float), np.asarray(Q6, float)
    st = PARTIAL if fixed else 0
    D = XB - XA
    L = math.sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2])
    if not (np.isfinite(Q6).all() and math.isfinite(sigma2 + L)):
        return np.full(5, np.nan), st | NOT_FINITE
    out = np.zeros(5)
    out[0] = L
    if L == 0.0:
        st |= DEGENERATE
        out[1] = np.nan
    else:
        u = D / L
        g = np.concatenate([-u, u])
        var = 0.0
        for r in range(6):
            s = 0.0
            for c in range(6):
                s += Q6[r, c] * g[c]
            var += g[r] * s
        if var < 0.0:
            st |= NEGATIVE
        out[1] = math.sqrt(sigma2 * max(var, 0.0))
    for k in range(3):
        dv = (Q6[k, k] + Q6[3 + k, 3 + k]) - 2.0 * Q6[3 + k, k]
        if dv < 0.0:
            st |= NEGATIVE
        out[2 + k] = math.sqrt(sigma2 * max(dv, 0.0))
    return out, st


def splitmix64(c):
    z = ((c + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def start_block(n):
    """X0 [n][8] of the header's counter-based generator."""
    return np.array([[(splitmix64(8 * i + a) >> 11) * 2.0 ** -53 - 0.5 for a in range(8)] for i in range(n)])


def _orth(W):
    """CholeskyQR2; None when a Gram matrix has no Cholesky factor."""
    for _ in range(2):
        G = W.T @ W
        try:
            R = np.linalg.cholesky(0.5 * (G + G.T)).T
        except np.linalg.LinAlgError:
            return None
        W = np.linalg.solve(R.T, W.T).T
    return W


def subspace_iteration(S, k, tol=0.0, max_iterations=200):
    """(values [k], vectors [k][n], trace, residuals [k], iterations, converged) of the header's iteration on the full symmetric S."""
    S = np.asarray(S, float)
    n = S.shape[0]
    tol = 1e-10 if tol == 0.0 else tol
    X = _orth(start_block(n))
    assert X is not None
    it = 0
    while True:
        Y = S @ X
        it += 1
        H = X.T @ Y
        th, Z = np.linalg.eigh(0.5 * (H + H.T))
        order = np.argsort(-th, kind="stable")
        th, Z = th[order], Z[:, order]
        R = Y @ Z - (X @ Z) * th
        res = np.sqrt((R * R).sum(0))
        converged = bool(np.all(res[:k] <= tol * th[0]))
        if converged or it >= max_iterations:
            break
        X = _orth(Y)
        if X is None:
            raise np.linalg.LinAlgError("the Gram matrix of S X has no Cholesky factor")
    V = (X @ Z)[:, :k].T
    V = np.array([sign_rule(x / np.linalg.norm(x)) for x in V])
    return th[:k], V, float(np.trace(S)), res[:k], it, converged
