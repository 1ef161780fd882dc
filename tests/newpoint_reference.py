"""numpy restatement of include/jaicov_newpoints.h, and the scenes, new points and measurements that the tests of it share.

J and w of a ray come from the oracle's own rows on an auxiliary problem (`aux_problem`): the new points are appended to the object
points as fixed points, the rays are its image points (sorted by image, ordinary weights, the block tables cleared) and the slot
vector is extended accordingly, so oracle/ is used as it is.  The cofactor matrix is an argument everywhere: the oracle's inverse
on the CPU, the engine's exported matrix on the GPU.  `evaluate` forms every figure at a given X, `iterate` is the Gauss-Newton
loop; beside every figure `evaluate` forms the bound on what a second evaluation of the same formulas may differ by."""
import dataclasses

import numpy as np

import helpers
import predict_reference as PR
from bundle_adjustment_amd import scene

PARTIAL, NOT_CONVERGED, TOO_FEW_RAYS, TOO_MANY, SINGULAR, NOT_FINITE = 1, 2, 4, 8, 16, 32
FAILED = TOO_FEW_RAYS | TOO_MANY | SINGULAR | NOT_FINITE
PAIR_PARTIAL, PAIR_NEGATIVE, PAIR_NOT_FINITE, PAIR_DEGENERATE = 1, 2, 4, 8
COLUMNS, PAIR_COLUMNS, MAX_RAYS, MAX_COLS = 20, 7, 64, 448
KLOC = PR.KLOC
ROW_PARITY = PR.ROW_PARITY    # the project's bound on a row entry against the oracle (tests/test_gpu_parity.py)
U53 = PR.U53
EPS = 2.0 ** -53
SQRT_EPS = np.sqrt(EPS)
TRI = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # xx xy xz yy yz zz


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def block_scene():
    return scene.make_scene(40, 80, 30, dist=scene.DIST_FULL, weights="block", n_control=4)


def five_camera_scene():
    """64 images shared out between five cameras of 11 coefficients each: a point seen in all of them has 64 * 6 + 5 * 14 = 454 shared
    columns, more than MAX_COLS (two cameras of the largest size stay below it)"""
    base = scene.make_scene(64, 60, 30, dist=scene.DIST_FULL, weights="diag", n_control=4)
    P, I, nd, nc = base.n_points, base.n_images, base.dist_kind.size, 5
    v, s_io = base.values, 3 * base.n_points
    values = np.concatenate([v[:s_io]] + [v[s_io:s_io + 3]] * nc + [v[s_io + 3:s_io + 3 + nd]] * nc + [v[s_io + 3 + nd:]])
    return helpers.renumber(base, image_camera=((np.arange(I) * nc) // I).astype(np.int32), cam_dist_begin=(nd * np.arange(nc + 1)).astype(np.int32),
                            cam_r0=np.full(nc, base.cam_r0[0]), dist_kind=np.tile(base.dist_kind, nc).astype(np.int32),
                            dist_order=np.tile(base.dist_order, nc).astype(np.int32), values=values, truth=None)


SCENES = dict(PR.SCENES, block=block_scene)
_FP = {}


def scene_of(name):
    if name not in _FP:
        _FP[name] = PR.scene_of(name) if name in PR.SCENES else dict(SCENES, five_camera=five_camera_scene)[name]()
    return _FP[name]


def model_values(fp):
    """the slot vector the measurements of new points are made at: the scene's truth, or its values where it has none (two_camera)"""
    return fp.values if fp.truth is None else fp.truth


def new_points(fp, n, seed=31):
    """n points within +-300 mm of the centroid of the scene's points"""
    v = model_values(fp)
    centre = v[:3 * fp.n_points].reshape(-1, 3).mean(0)
    return centre + np.random.default_rng(seed).uniform(-300.0, 300.0, (n, 3))


def project(fp, values, X, images):
    """x, y (n, 2) of the points X (n, 3) in the images (n,) by scene.project at the slot vector `values`"""
    out = np.zeros((len(images), 2))
    for k, (im, x) in enumerate(zip(images, np.asarray(X, float).reshape(-1, 3))):
        cam = int(fp.image_camera[im])
        io = values[fp.slot_io(cam):fp.slot_io(cam) + 3]
        jb, je = int(fp.cam_dist_begin[cam]), int(fp.cam_dist_begin[cam + 1])
        dist = [(int(fp.dist_kind[j]), int(fp.dist_order[j]), float(values[fp.slot_dist(j)])) for j in range(jb, je)]
        px, py, _ = scene.project(io[2], io[0], io[1], values[fp.slot_eo(im):fp.slot_eo(im) + 6], x[None, :], fp.cam_r0[cam], dist)
        out[k] = px[0], py[0]
    return out


def measure(fp, values, X, ray_begin, ray_image, sigma=0.0, seed=37):
    """the measurements of the rays: the projection of every ray's point at `values`, plus N(0, sigma^2)"""
    pt = np.repeat(np.arange(len(ray_begin) - 1), np.diff(ray_begin))
    xy = project(fp, values, np.asarray(X, float).reshape(-1, 3)[pt], ray_image)
    return xy + sigma * np.random.default_rng(seed).normal(size=xy.shape) if sigma else xy


def rays_of(fp, counts, seed=41, images=None):
    """(ray_begin, ray_image): counts[i] rays of point i in distinct random images while the scene has them, repeated images beyond"""
    rng = np.random.default_rng(seed)
    pool = np.arange(fp.n_images) if images is None else np.asarray(images)
    im = []
    for m in counts:
        perm = rng.permutation(pool)
        im.append(np.resize(perm, m))
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), (np.concatenate(im) if im else np.zeros(0)).astype(np.int32)


def dispersions(fp, n, seed=43):
    return PR.some_dispersions(n, float(np.mean(fp.ip_var_x)), seed=seed)


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------
def shared_columns(fp, image):
    """the columns of the local row layout behind X, Y, Z: x0 y0 c | X0 Y0 Z0 omega phi kappa | coefficients; -1: fixed"""
    return PR.local_columns(fp, image, 0)[3:]


def shared_slots(fp, image):
    return PR.local_slots(fp, image, 0)[3:]


def aux_problem(fp, values, X, ray_begin, ray_image, xy):
    """(the problem whose last object points are the new points, fixed, and whose image points are the rays; its slot vector; order):
    image point s of it is ray order[s]"""
    X = np.asarray(X, float).reshape(-1, 3)
    n, P = X.shape[0], fp.n_points
    ray_image = np.asarray(ray_image, np.int32)
    R = ray_image.size
    pt = np.repeat(np.arange(n), np.diff(ray_begin)).astype(np.int32)
    order = np.argsort(ray_image, kind="stable")
    l = np.asarray(xy, float).reshape(R, 2)
    var = float(np.mean(fp.ip_var_x))
    dg = fp.dg_slot.copy()
    dg[dg >= 3 * P] += 3 * n
    aux = dataclasses.replace(fp, point_col=np.vstack([fp.point_col, np.full((n, 3), -1, np.int32)]),
                              point_datum=np.concatenate([fp.point_datum, np.zeros(n, np.uint8)]), dg_slot=dg,
                              ip_image=ray_image[order], ip_point=(P + pt[order]).astype(np.int32), ip_x=l[order, 0].copy(), ip_y=l[order, 1].copy(),
                              ip_var_x=np.full(R, var), ip_var_y=np.full(R, var), ip_rho=np.zeros(R), blk_ip_begin=np.zeros(1, np.int32),
                              blk_disp_offset=np.zeros(0, np.int64), blk_disp=np.zeros(0), n_observations=0, values=np.zeros(0), truth=None,
                              names=None)
    vals = np.concatenate([values[:3 * P], X.ravel(), values[3 * P:]])
    return aux, vals, order


def rows(oracle_mod, fp, values, X, ray_begin, ray_image, xy):
    """w (R, 2) and J (R, 2, 32) of the rays in the caller's order, by the oracle"""
    aux, vals, order = aux_problem(fp, values, X, ray_begin, ray_image, xy)
    aux.values = vals
    orc = oracle_mod.Oracle(aux)
    R = order.size
    w = np.zeros((R, 2)); J = np.zeros((R, 2, KLOC))
    for s in range(R):
        ws, A, _, _ = orc.rows(vals, s)
        w[order[s]] = ws; J[order[s]] = A
    return w, J


def weight(disp, s0):
    """P of one ray (jaicov_intersect.h)"""
    vx, vy, rho = disp
    if rho == 0.0:
        return np.diag([s0 / vx, s0 / vy])
    inv = s0 / ((1.0 - rho * rho) * vx * vy)
    c = -inv * rho * np.sqrt(vx * vy)
    return np.array([[inv * vy, c], [c, inv * vx]])


# ---- one point at a given X ---------------------------------------------------------------------------------------------------------------
def solve3(N, n):
    """(status, dx, Q_meas, cond of the Jacobi-scaled N, V): Jacobi preconditioning and Cholesky as jaicov_intersect.h states them"""
    if not (np.isfinite(N).all() and np.isfinite(n).all()):
        return NOT_FINITE, None, None, np.inf, None
    d = np.diag(N)
    V = np.where(d > EPS, 1.0 / np.sqrt(np.where(d > EPS, d, 1.0)), 1.0)
    M = N * np.outer(V, V)
    L = np.zeros((3, 3))
    for j in range(3):
        p = M[j, j] - L[j, :j] @ L[j, :j]
        if not p > SQRT_EPS:
            return SINGULAR, None, None, np.inf, V
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, 3):
            L[i, j] = (M[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    Mi = np.linalg.inv(M)
    return 0, V * (Mi @ (V * n)), Mi * np.outer(V, V), float(np.linalg.cond(M)), V


def evaluate(fp, Q, w, J, images, disp, s0):
    """Every figure of ONE point from the rows (w (m, 2), J (m, 2, 32)) of its m rays at some X, and the bounds of the figures.
    Returns a dict: status (PARTIAL, SINGULAR, NOT_FINITE), dx, Q_meas, cols, F, Q_sys, Q_XX, omega, and with the prefix E_ the
    entrywise bounds: two evaluations of these formulas whose rows agree to ROW_PARITY differ by no more."""
    m = len(images)
    A = J[:, :, 0:3]
    Pk = [weight(disp[k], s0) for k in range(m)]
    N = sum(A[k].T @ Pk[k] @ A[k] for k in range(m))
    nn = sum(A[k].T @ Pk[k] @ w[k] for k in range(m))
    S = sum(np.abs(A[k]).T @ np.abs(Pk[k]) @ np.abs(A[k]) for k in range(m))
    omega = sum(w[k] @ Pk[k] @ w[k] for k in range(m))
    cols_k = [shared_columns(fp, images[k]) for k in range(m)]
    r = dict(status=PARTIAL if any((c < 0).any() for c in cols_k) else 0, omega=omega)
    cols = np.unique(np.concatenate(cols_k)); cols = cols[cols >= 0]
    if cols.size > MAX_COLS:
        r["status"] |= TOO_MANY
        return r
    st, dx, Qm, cond, V = solve3(N, nn)
    if st:
        r["status"] |= st
        return r
    # Q_meas = V inv(M) V: with |dN| <= d_N S entrywise, |d inv(M)| <= |inv(M)|^2 |dM| <= cond trace(inv(M)) 3 d_N max(S scaled)
    d_N = 2.0 * ROW_PARITY + 4.0 * m * U53
    Ss = S * np.outer(V, V)
    E_Qm = 3.0 * d_N * Ss.max() * cond * np.trace(Qm / np.outer(V, V)) * np.outer(V, V)
    M = cols.size
    T = np.zeros((3, M)); Tabs = np.zeros((3, M))
    for k in range(m):
        ok = cols_k[k] >= 0
        pos = np.searchsorted(cols, cols_k[k][ok])
        B = J[k][:, 3:3 + cols_k[k].size][:, ok]
        np.add.at(T, (slice(None), pos), A[k].T @ Pk[k] @ B)
        np.add.at(Tabs, (slice(None), pos), np.abs(A[k]).T @ np.abs(Pk[k]) @ np.abs(B))
    F = -Qm @ T
    Fabs = np.abs(Qm) @ Tabs
    E_F = E_Qm @ Tabs + (2.0 * ROW_PARITY + (6.0 * m + 6.0) * U53) * Fabs
    Qc = Q[np.ix_(cols, cols)]
    Qsys = F @ Qc @ F.T
    Qabs = np.abs(Qc)
    E_sys = E_F @ Qabs @ Fabs.T + Fabs @ Qabs @ E_F.T + (M * M + 2.0) * U53 * (Fabs @ Qabs @ Fabs.T)
    r.update(dx=dx, Q_meas=Qm, cond=cond, cols=cols, F=F, Fabs=Fabs, Q_sys=Qsys, Q_XX=Qm + Qsys, E_meas=E_Qm, E_F=E_F, E_sys=E_sys,
             E_XX=E_Qm + E_sys, P=Pk)
    return r


def bound_w(w, xy):
    """a misclosure is l - f: two evaluations of f agree to ROW_PARITY of its size"""
    return ROW_PARITY * (np.abs(xy) + np.abs(w)) + 4.0 * U53 * np.abs(xy)


def bound_omega(w, Ew, Pk):
    return sum(2.0 * np.abs(w[k]) @ np.abs(Pk[k]) @ Ew[k] + 4.0 * len(Pk) * U53 * (np.abs(w[k]) @ np.abs(Pk[k]) @ np.abs(w[k])) for k in range(len(Pk)))


def sym6(M):
    return np.array([M[i, j] for i, j in TRI])


def iterate(oracle_mod, fp, values, ray_begin, ray_image, xy, disp, s0, start, max_iterations=20):
    """(X (n, 3), status (n,), iterations (n,)): the Gauss-Newton loop of every point with 2 .. MAX_RAYS rays"""
    X = np.array(start, float).reshape(-1, 3)
    n = X.shape[0]
    status = np.zeros(n, np.int32); iters = np.zeros(n, np.int32)
    m = np.diff(ray_begin)
    status[m < 2] = TOO_FEW_RAYS; status[m > MAX_RAYS] = TOO_MANY
    moving = status == 0
    for _ in range(max_iterations):
        if not moving.any():
            break
        w, J = rows(oracle_mod, fp, values, X, ray_begin, ray_image, xy)
        for i in np.flatnonzero(moving):
            k = slice(ray_begin[i], ray_begin[i + 1])
            A = J[k, :, 0:3]
            Pk = [weight(d, s0) for d in disp[k]]
            N = sum(a.T @ p @ a for a, p in zip(A, Pk)); nn = sum(a.T @ p @ ww for a, p, ww in zip(A, Pk, w[k]))
            st, dx, _, _, _ = solve3(N, nn)
            iters[i] += 1
            if st or not np.isfinite(dx).all():
                status[i] = st or NOT_FINITE; moving[i] = False
                continue
            X[i] += dx
            X0 = values[fp.slot_eo(ray_image[ray_begin[i]]):][:3]
            if np.abs(dx).max() <= SQRT_EPS * max(1.0, np.abs(X[i] - X0).max()):
                moving[i] = False
    status[moving] = NOT_CONVERGED
    return X, status, iters


def refine(oracle_mod, fp, values, ray_begin, ray_image, xy, disp, s0, X, steps=2):
    """`steps` more Gauss-Newton steps of every point, whatever their size: for the differences of converged solutions"""
    X = np.array(X, float).reshape(-1, 3)
    for _ in range(steps):
        w, J = rows(oracle_mod, fp, values, X, ray_begin, ray_image, xy)
        for i in range(X.shape[0]):
            k = slice(ray_begin[i], ray_begin[i + 1])
            Pk = [weight(d, s0) for d in disp[k]]
            N = sum(a.T @ p @ a for a, p in zip(J[k, :, 0:3], Pk)); nn = sum(a.T @ p @ ww for a, p, ww in zip(J[k, :, 0:3], Pk, w[k]))
            X[i] += solve3(N, nn)[1]
    return X


def threshold(fp, values, X, first_image):
    """the convergence threshold of a point at X"""
    X0 = values[fp.slot_eo(first_image):][:3]
    return SQRT_EPS * max(1.0, np.abs(X - X0).max())


# ---- pairs ----------------------------------------------------------------------------------------------------------------------------------
def new_member(X, ev):
    """a new point as a member of a pair, from its position and its `evaluate`"""
    return dict(X=np.asarray(X, float), cols=ev["cols"], F=ev["F"], Fabs=ev["Fabs"], E_F=ev["E_F"], Q_XX=ev["Q_XX"], E_XX=ev["E_XX"],
                partial=bool(ev["status"] & PARTIAL))


def block_member(fp, values, Q, P):
    """object point P of the problem: columns point_col[P], F = I, Q_meas = 0, X from the slot vector"""
    cols = fp.point_col[P].astype(np.int64)
    return dict(X=values[3 * P:3 * P + 3].copy(), cols=cols, F=np.eye(3), Fabs=np.eye(3), E_F=np.zeros((3, 3)), Q_XX=PR.gather(Q, cols, cols),
                E_XX=np.zeros((3, 3)), partial=bool((cols < 0).any()))


def pair_figures(Q, a, b, sigma2):
    """(row of 7, status, bound of columns 5 and 6, bound of the variances of D_X, D_Y, D_Z) of the pair of members (a, b)"""
    G = PR.gather(Q, a["cols"], b["cols"])
    C = a["F"] @ G @ b["F"].T
    Gabs = np.abs(G)
    E_C = a["E_F"] @ Gabs @ b["Fabs"].T + a["Fabs"] @ Gabs @ b["E_F"].T + (G.size + 2.0) * U53 * (a["Fabs"] @ Gabs @ b["Fabs"].T)
    st = PAIR_PARTIAL if a["partial"] or b["partial"] else 0
    Q6 = np.block([[a["Q_XX"], C], [C.T, b["Q_XX"]]])
    Q60 = np.block([[a["Q_XX"], np.zeros((3, 3))], [np.zeros((3, 3)), b["Q_XX"]]])
    E6 = np.block([[a["E_XX"], E_C], [E_C.T, b["E_XX"]]])
    D = b["X"] - a["X"]
    L = np.sqrt(D @ D)
    out = np.full(PAIR_COLUMNS, np.nan)
    out[0] = L
    dv = np.diag(a["Q_XX"]) + np.diag(b["Q_XX"]) - 2.0 * np.diag(C)
    E_dv = np.diag(a["E_XX"]) + np.diag(b["E_XX"]) + 2.0 * np.diag(E_C) + 6.0 * U53 * (np.abs(np.diag(a["Q_XX"])) + np.abs(np.diag(b["Q_XX"])) + 2.0 * np.abs(np.diag(C)))
    if (dv < 0.0).any():
        st |= PAIR_NEGATIVE
    out[2:5] = np.sqrt(sigma2 * np.maximum(dv, 0.0))
    if L == 0.0:
        return out, st | PAIR_DEGENERATE, np.zeros(2), E_dv
    g = np.concatenate([-D / L, D / L])
    qL, qL0 = g @ Q6 @ g, g @ Q60 @ g
    if qL < 0.0:
        st |= PAIR_NEGATIVE
    out[1] = np.sqrt(sigma2 * max(qL, 0.0)); out[5] = qL; out[6] = qL0
    ag = np.abs(g)
    E60 = np.block([[a["E_XX"], np.zeros((3, 3))], [np.zeros((3, 3)), b["E_XX"]]])
    bound = np.array([ag @ E6 @ ag + 38.0 * U53 * (ag @ np.abs(Q6) @ ag), ag @ E60 @ ag + 38.0 * U53 * (ag @ np.abs(Q60) @ ag)])
    return out, st, bound, E_dv
