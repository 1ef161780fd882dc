"""numpy restatement of include/jaicov_parameters.h (csrc/parameters.hip): the same formulas in the same order.

Every coefficient is rho_ij = (Q[i][j] * s_i) * s_j for i > j with s_j = 1.0 / sqrt(q_jj): two products and no sum, so numpy's
element-wise products round exactly as the device does.  Only the lower part of Q is read.  The group solve is the Jacobi-scaled
Cholesky of csrc/wavealg.h (wave_solve_lds), restated as tests/resection_reference.py restates wave_solve, on a block whose
diagonal group_test has brought into [1, 4) by powers of two first (the header says why)."""
import math

import numpy as np

NONPOSITIVE, NOT_FINITE, PARTIAL, EMPTY, TOO_LARGE, SINGULAR = 1, 2, 4, 8, 16, 32
SKIP_SAME_POINT, SKIP_SAME_IMAGE = 1, 2
POINT, INTERIOR, DISTORTION, EXTERIOR = range(4)
ALL = 0xFFFF
MAX_GROUP = 64
EPS = 2.0 ** -53
SQRT_EPS = math.sqrt(EPS)
ULP4 = 4 * 2.0 ** -52                  # 4 ulp of 1: 8.9e-16


def mask_of(*pairs):
    """pair_mask of (class a considers partners of class b) pairs."""
    m = 0
    for a, b in pairs:
        m |= 1 << (4 * a + b)
    return m


def column_tables(slot_col, n_points, n_cameras, n_dist, n_images, order, flags=0):
    """(class, item) of every column < order from the slot layout [3 P | 3 C | n_dist | 6 I].  Two columns with equal items are no
    pair: the point's number under SKIP_SAME_POINT, P + the image's number under SKIP_SAME_IMAGE, otherwise -1 - column."""
    slot_col = np.asarray(slot_col).ravel()
    assert slot_col.size == 3 * n_points + 3 * n_cameras + n_dist + 6 * n_images
    cls = np.zeros(order, np.int32)
    item = -1 - np.arange(order, dtype=np.int32)
    io0 = 3 * n_points; di0 = io0 + 3 * n_cameras; eo0 = di0 + n_dist
    for sl, c in enumerate(slot_col):
        if c < 0 or c >= order:
            continue
        if sl < io0:
            if flags & SKIP_SAME_POINT:
                item[c] = sl // 3
        elif sl < di0:
            cls[c] = INTERIOR
        elif sl < eo0:
            cls[c] = DISTORTION
        else:
            cls[c] = EXTERIOR
            if flags & SKIP_SAME_IMAGE:
                item[c] = n_points + (sl - eo0) // 6
    return cls, item


def tables_of(fp, order, flags=0):
    return column_tables(fp.slot_columns(), fp.n_points, fp.n_cameras, fp.n_dist, fp.n_images, order, flags)


def scales(Q, d):
    """s (0 for a column that takes no part), status of the diagonal."""
    n = Q.shape[0]
    q = np.diag(Q).astype(np.float64)
    fin = np.isfinite(q)
    st = np.zeros(n, np.int32)
    st[~fin] = NOT_FINITE
    st[fin & ~(q > 0.0)] = NONPOSITIVE
    st[:d] = 0
    good = fin & (q > 0.0)
    good[:d] = False
    s = np.zeros(n)
    s[good] = 1.0 / np.sqrt(q[good])
    return s, st


def coefficients(Q, d, item=None):
    """(R, bad): R[i, j] = R[j, i] = rho_ij, NaN where (i, j) is no pair (diagonal, border, bad column, entry not finite, equal
    items); bad[i, j]: an entry of the strict lower part inside [d, n) that is not finite."""
    n = Q.shape[0]
    s, _ = scales(Q, d)
    low = np.tril(np.ones((n, n), bool), -1)
    low[:d, :] = False; low[:, :d] = False
    Ql = np.where(low, Q, 0.0)
    bad = low & ~np.isfinite(Ql)
    ok = low & ~bad & (s[:, None] > 0.0) & (s[None, :] > 0.0)
    if item is not None:
        ok &= item[:, None] != item[None, :]
    with np.errstate(all="ignore"):
        Rl = (np.where(ok, Ql, 0.0) * s[:, None]) * s[None, :]
    Rl = np.where(ok, Rl, np.nan)
    R = np.where(low, Rl, Rl.T)
    return R, bad


def admitted(cls, mask):
    """A[j, k]: a column of class(j) considers partners of class(k)."""
    return ((mask >> (4 * cls[:, None] + cls[None, :])) & 1).astype(bool)


def maxima(Q, d, cls, item, mask):
    """jaicov_par_maxima: (rho, partner, status)."""
    n = Q.shape[0]
    R, bad = coefficients(Q, d, item)
    _, st = scales(Q, d)
    A = np.where(admitted(cls, mask) & ~np.isnan(R), np.abs(R), -1.0)
    partner = np.argmax(A, axis=1).astype(np.int32)           # the first of equal values: the lowest k
    best = A[np.arange(n), partner]
    rho = R[np.arange(n), partner]
    none = best < 0.0
    rho[none] = np.nan
    partner[none] = -1
    st = st | np.where(bad.any(axis=1) | bad.any(axis=0), NOT_FINITE, 0).astype(np.int32)
    st[:d] = 0
    return rho, partner, st


def second_best_gap(Q, d, cls, item, mask):
    """For every column the difference between its two largest admissible |rho| (inf with fewer than two candidates)."""
    R, _ = coefficients(Q, d, item)
    A = np.where(admitted(cls, mask) & ~np.isnan(R), np.abs(R), -1.0)
    if A.shape[1] < 2:
        return np.full(A.shape[0], np.inf)
    top = -np.partition(-A, 1, axis=1)[:, :2]
    return np.where(top[:, 1] >= 0.0, top[:, 0] - top[:, 1], np.inf)


def near_ties(Q, d, cls, item, mask, tol=ULP4):
    """Columns whose best two candidates lie within tol of each other."""
    return second_best_gap(Q, d, cls, item, mask) <= tol


def pairs(Q, d, cls, item, mask, threshold):
    """jaicov_par_pairs: (cols (m, 2) with i > j, rho (m,)), sorted by |rho| descending, then i, then j."""
    R, _ = coefficients(Q, d, item)
    n = Q.shape[0]
    A = admitted(cls, mask)
    sel = np.tril(np.ones((n, n), bool), -1) & (A | A.T) & ~np.isnan(R)
    with np.errstate(invalid="ignore"):
        sel &= np.abs(R) >= threshold
    i, j = np.nonzero(sel)
    r = R[i, j]
    o = np.lexsort((j, i, -np.abs(r)))
    return np.stack([i[o], j[o]], 1).astype(np.int32), r[o]


def block(Q, rows, cols):
    """jaicov_par_block."""
    q = np.diag(Q)
    out = np.full((len(rows), len(cols)), np.nan)
    for a, ca in enumerate(rows):
        for b, cb in enumerate(cols):
            i, j = max(ca, cb), min(ca, cb)
            if not (np.isfinite(q[i]) and q[i] > 0.0 and np.isfinite(q[j]) and q[j] > 0.0):
                continue
            with np.errstate(all="ignore"):
                out[a, b] = 1.0 if i == j else (Q[i, j] * (1.0 / np.sqrt(q[i]))) * (1.0 / np.sqrt(q[j]))
    return out


def solve(N, n):
    """N (k, k) symmetric (upper part read), n (k,): wave_solve_lds.  Returns (status, x): 0, SINGULAR or NOT_FINITE."""
    k = len(n)
    if not (np.all(np.isfinite(np.triu(N))) and np.all(np.isfinite(n))):
        return NOT_FINITE, None
    V = [1.0 / math.sqrt(N[i][i]) if N[i][i] > EPS else 1.0 for i in range(k)]
    U = [[float(N[i][j]) * (V[i] * V[j]) if j >= i else 0.0 for j in range(k)] for i in range(k)]
    for j in range(k):
        s = 0.0
        for r in range(j):
            s += U[r][j] * U[r][j]
        p = U[j][j] - s
        if not p > SQRT_EPS:
            return SINGULAR, None
        dj = math.sqrt(p)
        U[j][j] = dj
        for i in range(j + 1, k):
            acc = 0.0
            for r in range(j):
                acc += U[r][i] * U[r][j]
            U[j][i] = (U[j][i] - acc) / dj
    y = [0.0] * k
    for i in range(k):
        acc = 0.0
        for r in range(i):
            acc += U[r][i] * y[r]
        y[i] = (V[i] * float(n[i]) - acc) / U[i][i]
    for i in range(k - 1, -1, -1):
        acc = 0.0
        for r in range(i + 1, k):
            acc += U[i][r] * y[r]
        y[i] = (y[i] - acc) / U[i][i]
    return 0, np.array([V[i] * y[i] for i in range(k)])


def gather(Q, cols):
    """Q_gg from the lower part."""
    c = np.asarray(cols, np.int64)
    return Q[np.maximum(c[:, None], c[None, :]), np.minimum(c[:, None], c[None, :])]


def group_test(Qgg, delta, sigma2, st=0):
    """One group from its block and differences: ([q, T, k, t], status)."""
    k = len(delta)
    out = [np.nan, np.nan, float(k), np.nan]
    if k == 0:
        return out, st | EMPTY
    if k > MAX_GROUP:
        return out, st | TOO_LARGE
    # powers of two bring the diagonal into [1, 4) first: frexp's exponent is ilogb + 1, // is the floor
    W = np.array([2.0 ** -((math.frexp(Qgg[i][i])[1] - 1) // 2) if Qgg[i][i] > 0.0 and np.isfinite(Qgg[i][i]) else 1.0 for i in range(k)])
    with np.errstate(all="ignore"):
        ws, y = solve(np.asarray(Qgg, np.float64) * (W[:, None] * W[None, :]), W * delta)
    if ws:
        return out, st | ws
    q = 0.0
    for i in range(k):
        q += float(delta[i]) * (float(W[i]) * float(y[i]))
    with np.errstate(all="ignore"):
        T = q / (float(k) * sigma2)
        t = float(delta[0] / np.sqrt(sigma2 * Qgg[0][0])) if k == 1 else np.nan
    if not (np.isfinite(q) and np.isfinite(T) and (k != 1 or np.isfinite(t))):
        return out, st | NOT_FINITE
    return [q, T, float(k), t], st


def tests(Q, slot_col, values, sigma2, groups, x0=None):
    """jaicov_par_tests: groups = a list of slot lists, x0 = None or lists parallel to them.  (out (n, 4), status (n,))."""
    slot_col = np.asarray(slot_col).ravel()
    out = np.zeros((len(groups), 4)); status = np.zeros(len(groups), np.int32)
    for g, slots in enumerate(groups):
        st = 0
        cols, delta = [], []
        for m, sl in enumerate(slots):
            c = int(slot_col[sl])
            assert c < Q.shape[0], "BAD_STATE: the member's column is not in the matrix"
            if c < 0:
                st |= PARTIAL
                continue
            cols.append(c)
            delta.append(float(values[sl]) - (0.0 if x0 is None else float(x0[g][m])))
        Qgg = gather(Q, cols) if cols else np.zeros((0, 0))
        out[g], status[g] = group_test(Qgg, np.array(delta), sigma2, st)
    return out, status
