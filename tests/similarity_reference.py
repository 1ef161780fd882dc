"""Independent restatement of the absolute orientation of include/jaicov_simil.h for its tests.  TEST INFRASTRUCTURE ONLY.

One model at a time, in numpy: the rotation is PartialDerivativeFactory.java:125-135 (= PDF), the preconditioning NES:82-91
(resection_reference.solve).  Every term of a point is rounded as the kernel rounds it (one rounding per product, sum and quotient, no
contraction).  The sums over a model's points run in plain point order by default; with order="lanes" they run in the kernel's order
(resection_reference.sums).  The small algebra after the sums (Jacobi sweeps of order 3, the Kabsch rotation, Cholesky of order 7, J Q J')
is written with the kernel's order of operations.  Outputs and status follow the ABI (NaN after a failure), so they compare one to
one with the device.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import resection_reference as X  # noqa: E402
from bundle_adjustment_amd import scene  # noqa: E402

OK, NOT_CONVERGED, TOO_FEW_POINTS, SINGULAR, NOT_FINITE = range(5)
START_GIVEN, START_CLOSED = range(2)
EPS = 2.0 ** -53
SQRT_EPS = math.sqrt(EPS)
NOUT = 36
SWEEPS3 = 6
CHUNK = 128                       # SIMIL_CHUNK of csrc/simil.h: the points the kernel stages in LDS at a time
sums, solve = X.sums, X.solve


def tri(n, i, j):
    """index of (i, j >= i) in an upper triangle of order n packed row by row"""
    return i * n - i * (i - 1) // 2 + (j - i)


def rotation(ang):
    """R(omega, phi, kappa) of PDF:125-135, and the sine and cosine of omega"""
    return X.rotation([0.0, 0.0, 0.0, ang[0], ang[1], ang[2]])[0], math.sin(ang[0]), math.cos(ang[0])


def angles_of(R):
    return [math.atan2(-R[1][2], R[2][2]), math.asin(min(1.0, max(-1.0, R[0][2]))), math.atan2(-R[0][1], R[0][0])]


def angle_columns(R, so, co, m, x0, x1, r):
    """the columns of d(m R x)/d(omega, phi, kappa) at r = R x"""
    ao = [np.zeros_like(np.asarray(r[0], np.float64)) if np.ndim(r[0]) else 0.0, -(m * r[2]), m * r[1]]
    ap = [m * (co * r[2] - so * r[1]), m * (so * r[0]), -(m * (co * r[0]))]
    ak = [m * (R[i][1] * x0 - R[i][0] * x1) for i in range(3)]
    return ao, ap, ak


def condition(tc, m, ang, sb, pts):
    """per point of pts = (s (n, 3), d (n, 3), qs (6 arrays) or None, qd (6 arrays)): e (3), P (6), the four columns of A after the unit
    matrix, q, and whether C is positive"""
    s, d, qs, qd = pts
    R, so, co = rotation(ang)
    R = [[float(R[i, j]) for j in range(3)] for i in range(3)]
    with np.errstate(all="ignore"):
        x0, x1, x2 = s[:, 0] - sb[0], s[:, 1] - sb[1], s[:, 2] - sb[2]
        r = [R[i][0] * x0 + R[i][1] * x1 + R[i][2] * x2 for i in range(3)]
        e = [(d[:, i] - tc[i]) - m * r[i] for i in range(3)]
        c = [qd[k].copy() for k in range(6)]
        if qs is not None:
            m2 = m * m
            Q = [[qs[0], qs[1], qs[2]], [qs[1], qs[3], qs[4]], [qs[2], qs[4], qs[5]]]
            B = [[R[i][0] * Q[0][j] + R[i][1] * Q[1][j] + R[i][2] * Q[2][j] for j in range(3)] for i in range(3)]
            for i in range(3):
                for j in range(i, 3):
                    c[tri(3, i, j)] = c[tri(3, i, j)] + m2 * (B[i][0] * R[j][0] + B[i][1] * R[j][1] + B[i][2] * R[j][2])
        p = [c[3] * c[5] - c[4] * c[4], c[2] * c[4] - c[1] * c[5], c[1] * c[4] - c[2] * c[3],
             c[0] * c[5] - c[2] * c[2], c[1] * c[2] - c[0] * c[4], c[0] * c[3] - c[1] * c[1]]
        det = c[0] * p[0] + c[1] * p[1] + c[2] * p[2]
        positive = (c[0] > 0.0) & (p[5] > 0.0) & (det > 0.0)
        idet = 1.0 / det
        p = [v * idet for v in p]
        pe = [p[0] * e[0] + p[1] * e[1] + p[2] * e[2], p[1] * e[0] + p[3] * e[1] + p[4] * e[2], p[2] * e[0] + p[4] * e[1] + p[5] * e[2]]
        q = e[0] * pe[0] + e[1] * pe[1] + e[2] * pe[2]
        a = [r] + list(angle_columns(R, so, co, m, x0, x1, r))
    return e, p, pe, a, q, positive


def normal(tc, m, ang, sb, pts, sel, order):
    """N (7, 7), n (7,) of the step (N dx = n), Omega over sel, q of every point, and whether a point of sel has a C that is not positive"""
    e, p, pe, a, q, positive = condition(tc, m, ang, sb, pts)
    with np.errstate(all="ignore"):
        pa = [[p[0] * a[k][0] + p[1] * a[k][1] + p[2] * a[k][2], p[1] * a[k][0] + p[3] * a[k][1] + p[4] * a[k][2],
               p[2] * a[k][0] + p[4] * a[k][1] + p[5] * a[k][2]] for k in range(4)]
        T = [None] * NOUT
        for i in range(3):
            for j in range(i, 3):
                T[tri(7, i, j)] = p[tri(3, i, j)]
            for k in range(4):
                T[tri(7, i, 3 + k)] = pa[k][i]
            T[28 + i] = pe[i]
        for k in range(4):
            for l in range(k, 4):
                T[tri(7, 3 + k, 3 + l)] = a[k][0] * pa[l][0] + a[k][1] * pa[l][1] + a[k][2] * pa[l][2]
            T[31 + k] = a[k][0] * pe[0] + a[k][1] * pe[1] + a[k][2] * pe[2]
        T[35] = q
        S = sums(np.array([np.broadcast_to(t, q.shape) for t in T]), sel, order)
    N = np.zeros((7, 7))
    N[np.triu_indices(7)] = S[:28]
    N = N + np.triu(N, 1).T
    return N, S[28:35], S[35], q, bool((~positive[sel]).any())


def closed_start(s, d, sb, db, sel, order):
    """(status, m, angles) of the closed start with unit weights: the Kabsch rotation from M = sum (d - dbar)(s - sbar)'"""
    with np.errstate(all="ignore"):
        x = [s[:, j] - sb[j] for j in range(3)]
        y = [d[:, i] - db[i] for i in range(3)]
        S = sums(np.array([y[i] * x[j] for i in range(3) for j in range(3)] + [x[0] * x[0] + x[1] * x[1] + x[2] * x[2]]), sel, order)
    if not np.all(np.isfinite(S)):
        return NOT_FINITE, None, None
    M = [[float(S[3 * i + j]) for j in range(3)] for i in range(3)]
    s2 = float(S[9])
    S3 = [[M[0][j] * M[0][k] + M[1][j] * M[1][k] + M[2][j] * M[2][k] for k in range(3)] for j in range(3)]
    lam, V = X.eigen3(S3, SWEEPS3)
    if not lam[1] > SQRT_EPS * lam[0]:
        return SINGULAR, None, None
    v1, v2, v3 = V
    u1 = [M[i][0] * v1[0] + M[i][1] * v1[1] + M[i][2] * v1[2] for i in range(3)]
    w = [M[i][0] * v2[0] + M[i][1] * v2[1] + M[i][2] * v2[2] for i in range(3)]
    l1 = math.sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2])
    u1 = [v / l1 for v in u1]
    h = u1[0] * w[0] + u1[1] * w[1] + u1[2] * w[2]
    u2 = [w[i] - h * u1[i] for i in range(3)]
    l2 = math.sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2])
    u2 = [v / l2 for v in u2]
    u3 = [u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]]
    R = [[u1[i] * v1[j] + u2[i] * v2[j] + u3[i] * v3[j] for j in range(3)] for i in range(3)]
    tr = 0.0
    for i in range(3):
        for j in range(3):
            tr += R[i][j] * M[i][j]
    m = tr / s2
    if not m > 0.0:
        return SINGULAR, None, None
    return OK, m, angles_of(R)


def similarity_model(src, dst, cof_src=None, cof_dst=None, start=None, max_iterations=50, reject_threshold=0.0, min_points=3,
                     order="plain"):
    """One model from its points: (out[36], status, iterations, start_kind, used (n,), q (n,))"""
    s = np.asarray(src, np.float64).reshape(-1, 3)
    n_all = s.shape[0]
    d = np.asarray(dst, np.float64).reshape(n_all, 3)
    qs = None if cof_src is None else [np.asarray(cof_src, np.float64).reshape(n_all, 6)[:, k] for k in range(6)]
    qd = [np.asarray(cof_dst, np.float64).reshape(n_all, 6)[:, k] for k in range(6)] if cof_dst is not None else \
        [np.full(n_all, 1.0 if k in (0, 3, 5) else 0.0) for k in range(6)]
    pts = (s, d, qs, qd)
    nan = np.full(NOUT, np.nan)
    iterations = 0
    fail = lambda st: (nan, st, iterations, START_GIVEN, np.zeros(n_all, np.uint8), np.full(n_all, np.nan))      # noqa: E731
    given = start is not None and bool(np.all(np.isfinite(start)))
    used = np.ones(n_all, bool)
    while True:
        sel = np.flatnonzero(used)
        if sel.size < 3:
            return fail(TOO_FEW_POINTS)
        with np.errstate(all="ignore"):
            S = sums(np.array([s[:, 0], s[:, 1], s[:, 2], d[:, 0], d[:, 1], d[:, 2]]), sel, order)
            n = float(sel.size)
            sb = [float(S[i] / n) for i in range(3)]
            db = [float(S[3 + i] / n) for i in range(3)]
        if not np.all(np.isfinite(sb + db)):
            return fail(NOT_FINITE)
        if given:
            kind = START_GIVEN
            st7 = [float(v) for v in start]
            m, ang = st7[3], st7[4:7]
            if not m > 0.0:
                return fail(SINGULAR)
            R = rotation(ang)[0]
            tc = [st7[i] + m * float(R[i, 0] * sb[0] + R[i, 1] * sb[1] + R[i, 2] * sb[2]) for i in range(3)]
        else:
            kind = START_CLOSED
            st, m, ang = closed_start(s, d, sb, db, sel, order)
            if st != OK:
                return fail(st)
            tc = list(db)
        status = NOT_CONVERGED
        for _ in range(max_iterations):
            N, nv, _om, _q, bad = normal(tc, m, ang, sb, pts, sel, order)
            if bad:
                return fail(SINGULAR)
            iterations += 1
            st, dx = solve(N, nv)
            if st == OK and not np.all(np.isfinite(dx)):
                st = NOT_FINITE
            if st != OK:
                return fail(st)
            dx = [float(v) for v in dx]
            tc = [tc[i] + dx[i] for i in range(3)]
            m = m + dx[3]
            ang = [ang[i] + dx[4 + i] for i in range(3)]
            if not m > 0.0:
                return fail(SINGULAR)
            if max(abs(v) for v in dx) <= SQRT_EPS:
                status = OK
                break
        N, nv, omega, q, bad = normal(tc, m, ang, sb, pts, sel, order)
        if bad:
            return fail(SINGULAR)
        with np.errstate(all="ignore"):
            if reject_threshold > 0 and sel.size > min_points and np.nanmax(q[sel]) > reject_threshold * reject_threshold:
                used[sel[int(np.nanargmax(q[sel]))]] = False
                continue
        break
    st, Q = solve(N, nv, inverse=True)
    if st != OK:
        return fail(st)
    R, so, co = rotation(ang)
    R = [[float(R[i, j]) for j in range(3)] for i in range(3)]
    rb = [R[i][0] * sb[0] + R[i][1] * sb[1] + R[i][2] * sb[2] for i in range(3)]
    col = [rb] + list(angle_columns(R, so, co, m, sb[0], sb[1], rb))
    G = [[-col[k][i] for k in range(4)] for i in range(3)]
    H = [[0.0] * 4 for _ in range(3)]
    for i in range(3):
        for k in range(4):
            t = 0.0
            for l in range(4):
                t += G[i][l] * Q[3 + l, 3 + k]
            H[i][k] = Q[i, 3 + k] + t
    Q7 = np.zeros((7, 7))
    for i in range(7):
        for j in range(i, 7):
            if j < 3:
                t, u = 0.0, 0.0
                for l in range(4):
                    t += G[i][l] * Q[j, 3 + l]
                for l in range(4):
                    u += H[i][l] * G[j][l]
                Q7[i, j] = (Q[i, j] + t) + u
            elif i < 3:
                Q7[i, j] = H[i][j - 3]
            else:
                Q7[i, j] = Q[i, j]
    out = np.zeros(NOUT)
    out[:3] = [tc[i] - m * rb[i] for i in range(3)]
    out[3] = m
    out[4:7] = ang
    out[7:35] = Q7[np.triu_indices(7)]
    out[35] = omega
    if not np.all(np.isfinite(out)):
        return fail(NOT_FINITE)
    return out, status, iterations, kind, used.astype(np.uint8), q


def similarity(pt_begin, src, dst, cof_src=None, cof_dst=None, start=None, **kw):
    """Every model of a CSR batch, as engine.similarity_models takes it: (out (n, 36), status, iterations, start_kind, used, q)."""
    pb = np.asarray(pt_begin, np.int64)
    n = pb.size - 1
    src = np.asarray(src, np.float64).reshape(-1, 3); dst = np.asarray(dst, np.float64).reshape(-1, 3)
    cs = None if cof_src is None else np.asarray(cof_src, np.float64).reshape(-1, 6)
    cd = None if cof_dst is None else np.asarray(cof_dst, np.float64).reshape(-1, 6)
    s7 = None if start is None else np.asarray(start, np.float64).reshape(-1, 7)
    out = np.zeros((n, NOUT)); st = np.zeros(n, np.int32); it = np.zeros(n, np.int32); kind = np.zeros(n, np.int32)
    used = np.zeros(src.shape[0], np.uint8); q = np.zeros(src.shape[0])
    for g in range(n):
        sl = slice(pb[g], pb[g + 1])
        out[g], st[g], it[g], kind[g], used[sl], q[sl] = similarity_model(
            src[sl], dst[sl], None if cs is None else cs[sl], None if cd is None else cd[sl], None if s7 is None else s7[g], **kw)
    return out, st, it, kind, used, q


def cofactor(out):
    """the 7 x 7 cofactor matrix of one model's output"""
    Q = np.zeros((7, 7))
    Q[np.triu_indices(7)] = out[7:35]
    return Q + np.triu(Q, 1).T


def apply(par, pt_begin, xyz, cof=None, img_begin=None, eo=None):
    """jaicov_simil_apply in numpy, written from the header: (xyz, cof, eo) in the target frame"""
    par = np.asarray(par, np.float64)[:, :7]
    xo = qo = eo_out = None
    if pt_begin is not None:
        xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
        xo = np.full_like(xyz, np.nan)
        qo = None if cof is None else np.full((xyz.shape[0], 6), np.nan)
        for g, p in enumerate(par):
            sl = slice(pt_begin[g], pt_begin[g + 1])
            if not np.all(np.isfinite(p)):
                continue
            R = scene.rotation(*p[4:7])
            xo[sl] = p[:3] + p[3] * xyz[sl] @ R.T
            if cof is not None:
                for k in range(sl.start, sl.stop):
                    Q = np.zeros((3, 3)); Q[np.triu_indices(3)] = np.asarray(cof, np.float64).reshape(-1, 6)[k]
                    Q = Q + np.triu(Q, 1).T
                    qo[k] = (p[3] ** 2 * R @ Q @ R.T)[np.triu_indices(3)]
    if img_begin is not None:
        eo = np.asarray(eo, np.float64).reshape(-1, 6)
        eo_out = np.full_like(eo, np.nan)
        for g, p in enumerate(par):
            if not np.all(np.isfinite(p)):
                continue
            R = scene.rotation(*p[4:7])
            for k in range(img_begin[g], img_begin[g + 1]):
                eo_out[k, :3] = p[:3] + p[3] * R @ eo[k, :3]
                eo_out[k, 3:] = angles_of(R @ scene.rotation(*eo[k, 3:]))
    return xo, qo, eo_out


# ---- truth and batches -------------------------------------------------------------------------------------------------------------
def pose_error(out, truth, magnitude):
    """(largest difference of T over `magnitude`, of m relative, of the rotation matrix's entries) between out[:, :7] and truth (n, 7)"""
    dt = float(np.abs(out[:, :3] - truth[:, :3]).max() / magnitude)
    dm = float(np.abs(out[:, 3] / truth[:, 3] - 1.0).max())
    dr = max(float(np.abs(scene.rotation(*o[4:7]) - scene.rotation(*t[4:7])).max()) for o, t in zip(out, truth))
    return dt, dm, dr


def random_cofactors(rng, n, scale):
    """n different, fully populated SPD 3 x 3 matrices of size about scale^2: (n, 6) and their Cholesky factors (n, 3, 3)"""
    A = rng.normal(0.0, 1.0, (n, 3, 3))
    Q = scale ** 2 * (A @ A.transpose(0, 2, 1) / 3.0 + 0.2 * np.eye(3))
    iu = np.triu_indices(3)
    return Q[:, iu[0], iu[1]], np.linalg.cholesky(Q)


def cat(parts):
    """one batch of several: parts of (pt_begin, src, dst, cof_src, cof_dst, start)"""
    begin = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(p[0]) for p in parts]))]).astype(np.int32)
    return (begin,) + tuple(np.concatenate([p[k] for p in parts]) for k in range(1, 6))


def models(counts, seed=1, extent=1000.0, offset=0.0, sigma=0.0, plane=False, angles=None):
    """Models of counts[g] points within `extent`, the source coordinates moved by `offset` on every axis, each with a random
    transformation (T within 2 extents of the offset, m in 0.5 .. 2, omega and kappa anywhere, |phi| < 1.2; angles: (n, 3) overrides
    them).  plane: the points lie on a tilted plane.  Every point has its own fully populated cofactor matrices of size sigma^2 (source)
    and (1.5 sigma)^2 (target); with sigma > 0 both coordinates carry noise drawn from them.  Returns (batch = (pt_begin, src, dst,
    cof_src, cof_dst, start (n, 7) of NaN), truth (n, 7))."""
    rng = np.random.default_rng(seed)
    S, D, QS, QD, T = [], [], [], [], []
    for g, n in enumerate(counts):
        loc = rng.uniform(-0.5 * extent, 0.5 * extent, (n, 3))
        if plane:
            loc[:, 2] = 0.0
            loc = loc @ scene.rotation(*rng.uniform(-1.0, 1.0, 3)).T
        s = loc + offset
        ang = np.array([rng.uniform(-3.1, 3.1), rng.uniform(-1.2, 1.2), rng.uniform(-3.1, 3.1)]) if angles is None else np.asarray(angles[g])
        m = rng.uniform(0.5, 2.0)
        t = offset + rng.uniform(-2.0 * extent, 2.0 * extent, 3)
        d = t + m * s @ scene.rotation(*ang).T
        unit = sigma if sigma > 0 else 0.01
        qs, ls = random_cofactors(rng, n, unit)
        qd, ld = random_cofactors(rng, n, 1.5 * unit)
        if sigma > 0:
            s = s + np.einsum("nij,nj->ni", ls, rng.normal(0, 1, (n, 3)))
            d = d + np.einsum("nij,nj->ni", ld, rng.normal(0, 1, (n, 3)))
        S.append(s); D.append(d); QS.append(qs); QD.append(qd); T.append(np.concatenate([t, [m], ang]))
    begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return (begin, np.concatenate(S), np.concatenate(D), np.concatenate(QS), np.concatenate(QD), np.full((len(counts), 7), np.nan)), np.array(T)


SIGMA = 0.02                      # noise of the parity inputs in the units of an extent of 1000
COUNTS = [3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 200]     # both sides of the lane width (64) and of the LDS chunk
NEAR_PI = [[3.1, 0.3, -3.1], [-3.12, -0.7, 3.13], [3.14, 1.1, 0.2], [0.1, -1.2, -3.14]]


def lane_batch(sigma=SIGMA):
    """10 models in shuffled order with COUNTS points; the model of 4 points has start values (the truth moved a little), every other
    NaN there.  Returns (batch, counts, truth)."""
    counts = np.array(COUNTS)[np.random.default_rng(3).permutation(len(COUNTS))]
    batch, truth = models(counts, seed=21, sigma=sigma)
    batch[5][counts == 4] = truth[counts == 4] + [1.0, -1.0, 1.0, 0.001, 0.01, -0.01, 0.01]
    return batch, counts, truth


def lane_batch_with_gross_errors():
    """lane_batch with one gross error of 1 000 sigma on one coordinate of the source or the target of every model of at least 63
    points, on its first point or on point 70 mod count: (batch, counts, planted points)"""
    batch, counts, _ = lane_batch()
    pb = batch[0]
    big = np.flatnonzero(counts >= 63)
    bad = pb[big] + np.where(np.arange(big.size) % 2 == 0, 0, 70 % counts[big])
    batch[1][bad[0::2], 1] += 1000.0 * SIGMA
    batch[2][bad[1::2], 2] -= 1000.0 * SIGMA
    return batch, counts, bad


def gross_error_batch(sigmas=100.0, seed=7):
    """four noisy models, one gross error of `sigmas` sigma on all three target coordinates of one random point each: (batch, planted)"""
    batch, _ = models([12, 25, 40, 9], seed=seed, sigma=SIGMA)
    rng = np.random.default_rng(seed)
    pb = batch[0]
    planted = np.array([rng.integers(pb[g], pb[g + 1]) for g in range(pb.size - 1)])
    batch[2][planted] += rng.choice([-1.0, 1.0], (planted.size, 3)) * sigmas * SIGMA
    return batch, planted


def mixed_start_batch():
    """four noisy models with start values (the truth moved a little) for every second one, NaN in one value of every other"""
    batch, truth = models([12, 25, 40, 9], seed=8, sigma=SIGMA)
    start = truth + np.array([2.0, -2.0, 2.0, 0.002, 0.02, -0.02, 0.02])
    start[1::2, 5] = np.nan
    return batch[:5] + (start,)


def degenerate_batch():
    """A good model, 7 exactly collinear points, a model with a NaN coordinate, 2 points, the good model again: (batch, expected status)"""
    good, _ = models([12], seed=9, sigma=SIGMA)
    other, _ = models([7, 12, 2], seed=10, sigma=SIGMA)
    pb = other[0]
    line = np.outer(np.arange(7.0), [3.0, -2.0, 5.0]) + [10.0, 20.0, 30.0]
    other[1][pb[0]:pb[1]] = line
    other[2][pb[0]:pb[1]] = line
    other[2][pb[1] + 3, 1] = np.nan
    return cat([good, other, good]), [OK, SINGULAR, NOT_FINITE, TOO_FEW_POINTS, OK]


def parity_inputs():
    """Every input on which tests/test_gpu_similarity.py holds the device against this restatement: (name, batch, keywords).  Every
    point of every input has its own fully populated cofactor matrices on both sides (with equal isotropic ones the closed start is the
    solution already, Gauss-Newton ends after one step and the cofactors between m and the angles are zero but for rounding, which no
    column-wise comparison can hold); two more inputs drop one side to run the NULL paths, and the exact-recovery tests drop both.
    tests/test_similarity_abi.py runs the restatement on each of them in both summation orders."""
    inputs = []
    full = models([12, 40, 7, 25], seed=5, sigma=SIGMA)[0]
    inputs.append(("weights", full, {}))
    inputs.append(("weights, angles near pi", models([12, 40, 7, 25], seed=6, sigma=SIGMA, angles=NEAR_PI)[0], {}))
    inputs.append(("plane fields", models([4, 40, 9], seed=11, sigma=SIGMA, plane=True)[0], {}))
    # coordinates of 1e6 are rounded to 1.2e-10, and so is every e; q = e'Pe then carries 2 x 1.2e-10 / sigma of itself whatever the
    # order of the sums: sigma = 5 keeps that at 5e-11, below what both parity tests ask (with SIGMA it is 1e-8)
    inputs.append(("offset 1e6", models([12, 40, 200], seed=12, sigma=5.0, offset=1.0e6)[0], {}))
    inputs.append(("lane boundaries", lane_batch()[0], {}))
    inputs.append(("lane boundaries with rejection", lane_batch_with_gross_errors()[0], dict(reject_threshold=8.0, min_points=4)))
    inputs.append(("mixed starts", mixed_start_batch(), {}))
    inputs.append(("gross errors", gross_error_batch()[0], dict(reject_threshold=6.0, min_points=5)))
    inputs.append(("degenerate", degenerate_batch()[0], {}))
    inputs.append(("one iteration", full, dict(max_iterations=1)))
    inputs.append(("error-free source (NULL)", full[:3] + (None,) + full[4:], {}))
    inputs.append(("unit target (NULL)", full[:4] + (None,) + full[5:], {}))
    return inputs
