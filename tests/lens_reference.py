"""numpy restatement of include/jaicov_lens.h: the distortion terms and their chain-rule factors in the operation order of
bundle-adjustment_amd/csrc/lens.hip (every product and sum rounded on its own, left to right as the kernel writes them), both
directions, the statuses and the iteration count.  Vectorised over the points of one camera; cameras are worked one after the other.
Also the inputs that tests/test_lens_abi.py and tests/test_gpu_lens.py share."""
import math

import numpy as np

from bundle_adjustment_amd import scene

OK, NOT_CONVERGED, SINGULAR, NOT_FINITE = range(4)
CX, CY, BX, BY, BI, AI, DI, ZX, ZY, ZZ = range(10)
EPS = 2.0 ** -53
SQRT_EPS = math.sqrt(EPS)
MAX_DIST = 20
MAX_ZERNIKE_ORDER = 702       # the last single index of radial order 36

# the Zernike set: the orders of host/example_distortion_model for X, Y and Gradient (even radial order 2 .. 10, m = 0)
ZERNIKE_ORDERS = (4, 12, 24, 40, 60)
DIST_ZERNIKE = [(ZX, 4, 2.0e-5), (ZX, 12, -1.5e-5), (ZX, 24, 4.0e-6), (ZX, 40, -6.0e-7), (ZX, 60, 5.0e-8),
                (ZY, 4, -3.0e-5), (ZY, 12, 1.0e-5), (ZY, 24, -3.0e-6), (ZY, 40, 5.0e-7), (ZY, 60, -4.0e-8),
                (ZZ, 4, 4.0e-4), (ZZ, 12, -2.0e-4), (ZZ, 24, 5.0e-5), (ZZ, 40, -8.0e-6), (ZZ, 60, 6.0e-7)]
DIST_NO_DI = [t for t in scene.DIST_FULL if t[0] != DI]


def ipow(b, e):
    r = np.ones_like(b) if isinstance(b, np.ndarray) else 1.0
    for _ in range(e):
        r = r * b
    return r


def binomial(n, k):
    """MathExtension.binomial (MathExtension.java:53-64)"""
    if k < 0 or k > n:
        return 0
    if k > n - k:
        k = n - k
    result = 1
    for i in range(1, k + 1):
        result = result * (n - k + i) // i
    return result


def zernike_terms(order):
    """n, m and the (p, c) of every term: what the host tabulates per coefficient (ZernikeCoefficient.java:43-44, ZDF)"""
    n = int(math.ceil((-3.0 + math.sqrt(9.0 + 8.0 * order)) / 2.0))
    mi = 2 * order - n * (n + 2)
    half = (n - abs(mi)) // 2
    length = math.sqrt((1 + (1 if mi != 0 else 0)) * (n + 1) / 3.14159265358979323846)
    terms = [(n - 2 * k, length * float((1 if k % 2 == 0 else -1) * binomial(n - k, k) * binomial(n - 2 * k, half - k))) for k in range(half + 1)]
    return n, mi, terms


def delta(xs, ys, N, r0, dist):
    """sum of the terms of one camera at (xs, ys, N) and of their chain-rule factors: (sx, sy, [dXxs, dXys, dYxs, dYys]).
    dist: [(kind, order, value)] in table order."""
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    N = np.broadcast_to(np.asarray(N, np.float64), xs.shape)
    acc = [np.zeros_like(xs) for _ in range(6)]

    def add(*terms):
        for a, t in enumerate(terms):
            acc[a] = acc[a] + t
    zero = np.zeros_like(xs)
    last = {}
    for j, (k, _, _) in enumerate(dist):
        if k in (CX, CY, BX, BY):
            last[k] = j
    r2 = xs * xs + ys * ys
    r02 = r0 * r0
    xxs2, yys2, xys2 = 2.0 * xs * xs, 2.0 * ys * ys, 2.0 * xs * ys
    with np.errstate(all="ignore"):
        if CX in last and CY in last:
            cx, cy = dist[last[CX]][2], dist[last[CY]][2]
            add(cx * xs + cy * ys, zero, cx + zero, cy + zero, zero, zero)
        if BX in last and BY in last:
            bx, by = dist[last[BX]][2], dist[last[BY]][2]
            dX = bx * (r2 + xxs2) + by * xys2
            dY = by * (r2 + yys2) + bx * xys2
            dXxs = 2.0 * (3.0 * bx * xs + by * ys)
            dXys = 2.0 * (by * xs + bx * ys)
            dYxs = 2.0 * (by * xs + bx * ys)
            dYys = 2.0 * (bx * xs + 3.0 * by * ys)
            add(dX, dY, dXxs, dXys, dYxs, dYys)
            for k, e, bi in dist:
                if k != BI:
                    continue
                rim1 = ipow(r2, e - 1)
                ri = rim1 * r2
                dT = bi * ri
                cT = 2.0 * bi * e * rim1
                cX, cY = dX * cT, dY * cT
                add(dX * dT, dY * dT, dT * dXxs + xs * cX, dT * dXys + ys * cX, dT * dYxs + xs * cY, dT * dYys + ys * cY)
        for k, e, ai in dist:
            if k != AI:
                continue
            rim1 = ipow(r2, e - 1)
            dRi = rim1 * r2 - ipow(r02, e)
            dR = ai * dRi
            cR = ai * e * rim1
            add(xs * dR, ys * dR, xxs2 * cR + dR, xys2 * cR, xys2 * cR, yys2 * cR + dR)
        for k, e, di in dist:
            if k != DI:
                continue
            rim1 = ipow(r2, e - 1)
            dRi = rim1 * r2 - ipow(r02, e)
            dD = (di * dRi) / N
            cR = (di * e * rim1) / N
            add(xs * dD, ys * dD, xxs2 * cR + dD, xys2 * cR, xys2 * cR, yys2 * cR + dD)
        if any(k >= ZX for k, _, _ in dist):
            xxs, yys, xys = xs * xs, ys * ys, xs * ys
            phi = np.arctan2(ys, xs)
            rn2 = r2 / r02
            c2 = 2.0 / rn2 / r02
            for kind in (ZX, ZY, ZZ):
                for k, order, zi in dist:
                    if k != kind:
                        continue
                    n, mi, terms = zernike_terms(order)
                    m = float(mi)
                    s, c = np.sin(m * phi), np.cos(m * phi)
                    for pj, cj in terms:
                        ce = pj // 2 - 1
                        pw_lo = np.power(rn2, float(ce))
                        pw_hi = pw_lo * rn2
                        if mi < 0:
                            cX = -pj * xs * s + m * ys * c
                            cY = -pj * ys * s - m * xs * c
                        else:
                            cX = pj * xs * c + m * ys * s
                            cY = pj * ys * c - m * xs * s
                        if kind != ZZ:
                            constC = cj * pw_hi
                            constZ = zi * cj / r02 * pw_lo
                            az = -constC * s if mi < 0 else constC * c
                            d = zi * az
                            if kind == ZX:
                                add(d, zero, constZ * cX, constZ * cY, zero, zero)
                            else:
                                add(zero, d, zero, zero, constZ * cX, constZ * cY)
                        else:
                            constC = cj / r02 * pw_lo
                            if mi < 0:
                                dXxs = ce * xs * c2 * cX - pj * s + m / r2 * (pj * xys * c + m * yys * s)
                                dXys = ce * ys * c2 * cX + m * c - m / r2 * (pj * xxs * c + m * xys * s)
                                dYxs = ce * xs * c2 * cY - m * c + m / r2 * (pj * yys * c - m * xys * s)
                                dYys = ce * ys * c2 * cY - pj * s - m / r2 * (pj * xys * c - m * xxs * s)
                            else:
                                dXxs = ce * xs * c2 * cX + pj * c + m / r2 * (pj * xys * s - m * yys * c)
                                dXys = ce * ys * c2 * cX + m * s - m / r2 * (pj * xxs * s - m * xys * c)
                                dYxs = ce * xs * c2 * cY - m * s + m / r2 * (pj * yys * s + m * xys * c)
                                dYys = ce * ys * c2 * cY + pj * c - m / r2 * (pj * xys * s + m * xxs * c)
                            zc = zi * constC
                            add(zc * cX, zc * cY, zc * dXxs, zc * dXys, zc * dYxs, zc * dYys)
    return acc[0], acc[1], acc[2:]


def _camera(correct, x, y, N, x0, y0, r0, dist, max_iterations, tol):
    """the points of one camera: (ox, oy, J (4 arrays), det, status, iterations)"""
    n = x.size
    mx, my = x - x0, y - y0
    xs, ys = mx.copy(), my.copy()
    st = np.full(n, NOT_CONVERGED if correct else OK, np.int32)
    it = np.zeros(n, np.int32)
    ox, oy, det_out = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    J = [np.full(n, np.nan) for _ in range(4)]
    converged = np.zeros(n, bool)
    todo = np.arange(n)
    with np.errstate(all="ignore"):
        while todo.size:
            a = todo
            sx, sy, d = delta(xs[a], ys[a], N[a], r0, dist)
            d[0] = 1.0 + d[0]; d[3] = 1.0 + d[3]
            z = (xs[a] + ys[a] + sx + sy + d[0] + d[1] + d[2] + d[3]) * 0.0
            nf = z != 0.0
            det = d[0] * d[3] - d[1] * d[2]
            sing = ~nf & ~(det > SQRT_EPS)
            good = ~nf & ~sing
            stop = good & (converged[a] | (it[a] >= max_iterations)) if correct else good
            st[a[nf]] = NOT_FINITE
            st[a[sing]] = SINGULAR
            e = a[stop]
            ox[e] = (x0 + xs[e]) if correct else (x0 + xs[e]) + sx[stop]
            oy[e] = (y0 + ys[e]) if correct else (y0 + ys[e]) + sy[stop]
            det_out[e] = det[stop]
            for k in range(4):
                J[k][e] = d[k][stop]
            go = good & ~stop
            g = a[go]
            f0, f1 = (mx[g] - xs[g]) - sx[go], (my[g] - ys[g]) - sy[go]
            dx = (d[3][go] * f0 - d[1][go] * f1) / det[go]
            dy = (d[0][go] * f1 - d[2][go] * f0) / det[go]
            it[g] += 1
            xs[g] = xs[g] + dx; ys[g] = ys[g] + dy
            c = np.fmax(np.abs(dx), np.abs(dy)) <= tol * np.fmax(1.0, np.fmax(np.abs(xs[g]), np.abs(ys[g])))
            converged[g[c]] = True
            st[g[c]] = OK
            todo = g
    return ox, oy, J, det_out, st, it


def run(correct, xy, camera, cam_io, cam_r0, cam_dist_begin, dist_kind, dist_order, dist_value, var=None, depth=None, max_iterations=20,
        tolerance=0.0):
    """jaicov_lens_correct (correct) or jaicov_lens_distort: (xy (n, 2), var (n, 3), status, iterations, J (n, 2, 2))"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    camera = np.asarray(camera, np.int64)
    cam_io = np.asarray(cam_io, np.float64).reshape(-1, 3)
    n = camera.size
    tol = tolerance if tolerance > 0.0 else SQRT_EPS
    xo = np.full((n, 2), np.nan); J = np.full((n, 4), np.nan); det = np.full(n, np.nan)
    st = np.zeros(n, np.int32); it = np.zeros(n, np.int32)
    for c in np.unique(camera):
        a = np.flatnonzero(camera == c)
        dist = [(int(dist_kind[j]), int(dist_order[j]), float(dist_value[j])) for j in range(cam_dist_begin[c], cam_dist_begin[c + 1])]
        N = np.ones(a.size)
        if any(k == DI for k, _, _ in dist):
            dep = np.asarray(depth, np.float64)[a]
            with np.errstate(all="ignore"):
                N = np.where((np.abs(dep) > 0.0) & (np.abs(dep) < np.inf), dep, np.nan)
        ox, oy, Jc, dc, sc, ic = _camera(correct, xy[a, 0], xy[a, 1], N, cam_io[c, 0], cam_io[c, 1], float(cam_r0[c]), dist, max_iterations, tol)
        xo[a, 0], xo[a, 1], det[a], st[a], it[a] = ox, oy, dc, sc, ic
        for k in range(4):
            J[a, k] = Jc[k]
    if var is None:
        q00, q11, q01 = np.ones(n), np.ones(n), np.zeros(n)
    else:
        var = np.asarray(var, np.float64).reshape(-1, 3)
        q00, q11, q01 = var[:, 0], var[:, 1], var[:, 2] * np.sqrt(var[:, 0] * var[:, 1])
    with np.errstate(all="ignore"):
        if correct:
            m00, m01, m10, m11 = J[:, 3] / det, -(J[:, 1] / det), -(J[:, 2] / det), J[:, 0] / det
        else:
            m00, m01, m10, m11 = J[:, 0], J[:, 1], J[:, 2], J[:, 3]
        b00, b01 = m00 * q00 + m01 * q01, m00 * q01 + m01 * q11
        b10, b11 = m10 * q00 + m11 * q01, m10 * q01 + m11 * q11
        p00, p01, p11 = b00 * m00 + b01 * m01, b00 * m10 + b01 * m11, b10 * m10 + b11 * m11
        vo = np.stack([p00, p11, p01 / np.sqrt(p00 * p11)], 1)
    bad = st >= SINGULAR
    vo[bad] = np.nan
    return xo, vo, st, it, J.reshape(-1, 2, 2)


def correct(*a, **kw):
    return run(True, *a, **kw)


def distort(*a, **kw):
    kw.pop("max_iterations", None); kw.pop("tolerance", None)
    return run(False, *a, **kw)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def tables(dists, io=None, r0=None):
    """(cam_io, cam_r0, cam_dist_begin, dist_kind, dist_order, dist_value) of cameras with the given [(kind, order, value)] lists"""
    nc = len(dists)
    io = np.tile([scene.X0_EX, scene.Y0_EX, scene.C_EX], (nc, 1)) if io is None else np.asarray(io, np.float64).reshape(nc, 3)
    r0 = np.full(nc, scene.R0_EX) if r0 is None else np.asarray(r0, np.float64)
    begin = np.concatenate([[0], np.cumsum([len(d) for d in dists])]).astype(np.int32)
    flat = [t for d in dists for t in d]
    return (io, r0, begin, np.array([t[0] for t in flat], np.int32), np.array([t[1] for t in flat], np.int32),
            np.array([t[2] for t in flat], np.float64))


def sensor_points(n, seed, half=(18.0, 12.0)):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(-half[0], half[0], n), rng.uniform(-half[1], half[1], n)])


def dispersions(n, seed, rho=True):
    rng = np.random.default_rng(seed)
    s = scene.SIGMA_IMG ** 2
    return np.column_stack([rng.uniform(0.5, 2.0, n) * s, rng.uniform(0.5, 2.0, n) * s, rng.uniform(-0.6, 0.6, n) if rho else np.zeros(n)])


def grid():
    """41 x 31 points over the bundled sensor, +-18 x +-12 mm about the principal point"""
    gx, gy = np.meshgrid(np.linspace(-18.0, 18.0, 41), np.linspace(-12.0, 12.0, 31))
    return np.column_stack([gx.ravel() + scene.X0_EX, gy.ravel() + scene.Y0_EX])


def golden_inputs(sets):
    """every set of tests/golden/jacobian_rows.json as a call: one camera per case, the point at the case's ideal coordinates"""
    out = []
    for name, s in sets.items():
        dist, cases = s["dist"], s["cases"]
        dists = [[(k, o, v) for (k, o), v in zip(dist, c["dist_values"])] for c in cases]
        t = tables(dists, io=[c["io"] for c in cases], r0=[c["r0"] for c in cases])
        xs, ys, N = ideal_of_cases(cases)
        xy = np.column_stack([xs + t[0][:, 0], ys + t[0][:, 1]])
        out.append((f"golden {name}", xy, np.arange(len(cases), dtype=np.int32), t, dict(depth=N, var=dispersions(len(cases), 5))))
    return out


def ideal_of_cases(cases):
    """xs, ys, N of every golden case from its point, io and eo (PDF:125-152)"""
    xs, ys, Ns = [], [], []
    for c in cases:
        eo, io = np.array(c["eo"]), np.array(c["io"])
        k = (np.array(c["point"]) - eo[:3]) @ scene.rotation(eo[3], eo[4], eo[5])
        xs.append(-io[2] * k[0] / k[2]); ys.append(-io[2] * k[1] / k[2]); Ns.append(k[2])
    return np.array(xs), np.array(ys), np.array(Ns)


def parity_inputs(sets):
    """(name, xy, camera, tables, kw) of every call on which the device is held against this restatement, in both directions"""
    out = golden_inputs(sets)
    n = 300
    pts = sensor_points(n, 1) + [scene.X0_EX, scene.Y0_EX]
    cam = np.zeros(n, np.int32)
    depth = np.random.default_rng(2).uniform(-3000.0, -400.0, n)
    out.append(("radial", pts, cam, tables([scene.DIST_RADIAL]), dict(var=dispersions(n, 3, rho=False))))
    out.append(("full, depth", pts, cam, tables([scene.DIST_FULL]), dict(depth=depth, var=dispersions(n, 3))))
    out.append(("full without Di", pts, cam, tables([DIST_NO_DI]), dict(var=dispersions(n, 4))))
    out.append(("zernike", pts, cam, tables([DIST_ZERNIKE]), dict(var=dispersions(n, 3))))
    out.append(("c < 0", pts, cam, tables([scene.DIST_FULL], io=[[scene.X0_EX, scene.Y0_EX, -scene.C_EX]]), dict(depth=-depth)))
    out.append(("var NULL", pts, cam, tables([scene.DIST_FULL]), dict(depth=depth)))
    out.append(("tolerance 1e-14", pts, cam, tables([scene.DIST_FULL]), dict(depth=depth, var=dispersions(n, 3), tolerance=1e-14)))
    out.append(("zernike, tolerance 1e-14", pts, cam, tables([DIST_ZERNIKE]), dict(tolerance=1e-14)))
    return out


def mixed_cameras(n, seed=7):
    """three cameras with 0, 3 and 11 coefficients, interleaved point by point"""
    t = tables([[], scene.DIST_RADIAL, scene.DIST_FULL], io=[[0.1, -0.2, 28.0], [scene.X0_EX, scene.Y0_EX, scene.C_EX], [-0.05, 0.02, -35.0]],
               r0=[10.0, scene.R0_EX, 12.0])
    cam = (np.arange(n) % 3).astype(np.int32)
    xy = sensor_points(n, seed)
    depth = np.random.default_rng(seed + 1).uniform(-2000.0, -500.0, n)
    return xy, cam, t, dict(depth=depth, var=dispersions(n, seed + 2))


def degenerate():
    """good points beside: a fold (camera 1: a radial coefficient that makes det J <= sqrt(EPS) inside the sensor), NaN coordinates,
    a depth of 0 and an infinite one on a camera with Di (camera 2)"""
    t = tables([scene.DIST_RADIAL, [(AI, 1, -4.0e-3)], scene.DIST_FULL])
    xy = sensor_points(12, 21, half=(8.0, 6.0)) + [scene.X0_EX, scene.Y0_EX]
    cam = np.array([0, 1, 0, 0, 2, 2, 2, 0, 1, 2, 0, 2], np.int32)
    depth = np.full(12, -900.0)
    xy[1] = [scene.X0_EX + 15.0, scene.Y0_EX + 9.0]            # the fold
    xy[3] = [np.nan, 1.0]
    depth[5] = 0.0
    depth[6] = np.inf
    xy[8] = [scene.X0_EX + 1.0, scene.Y0_EX - 1.0]             # the folding camera near its centre: fine
    expected = [OK, SINGULAR, OK, NOT_FINITE, OK, NOT_FINITE, NOT_FINITE, OK, OK, OK, OK, OK]
    return xy, cam, t, dict(depth=depth, var=dispersions(12, 22)), expected
