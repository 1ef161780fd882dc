"""numpy restatement of include/jaicov_vce.h: variance components of groups of weight blocks, every sum in np.longdouble.

The weight blocks follow the construction of tests/test_gpu_reliability.py (design / blocks): the dense 2m x 2m of an image block,
the 2 x 2 of an ordinary image point, the scalar of a scale bar, the diagonal or dense block of a directly observed group.  Beside
the table the reference returns, per group, S_g = |v|' |P| |v| and R_g = sum |r_i|: the scales of the rounding bounds."""
import dataclasses
from collections import namedtuple

import numpy as np

from bundle_adjustment_amd.problem import packed_to_full, scale_dispersions

EMPTY, UNCONTROLLED, NOT_FINITE = 1, 2, 4
COLUMNS = 6
UNCONTROLLED_TOL = 1e-10
LD = np.longdouble

Groups = namedtuple("Groups", ["ip", "sb", "dg", "n_groups", "names"])
Block = namedtuple("Block", ["rows", "D", "kind", "index"])       # kind: "blk" | "ip" | "sb" | "dg"; index in the caller's order
Components = namedtuple("Components", ["table", "status", "S", "R", "omega_total", "r_total", "S_total", "R_total"])


def weight_blocks(fp):
    """Every weight block of the problem with its rows and its dispersion D (P = sigma0^2 inv(D)), in ascending row order."""
    n_ip = fp.n_image_points
    out = []
    in_blk = np.zeros(n_ip, bool)
    for g in range(fp.n_image_blocks):
        b, e = int(fp.blk_ip_begin[g]), int(fp.blk_ip_begin[g + 1])
        if e <= b:
            continue
        m = 2 * (e - b)
        off = int(fp.blk_disp_offset[g])
        out.append(Block(np.arange(2 * b, 2 * e), fp.blk_disp[off:off + m * m].reshape(m, m), "blk", g))
        in_blk[b:e] = True
    for k in np.flatnonzero(~in_blk):
        vx, vy, rho = fp.ip_var_x[k], fp.ip_var_y[k], fp.ip_rho[k]
        c = rho * np.sqrt(vx * vy)
        out.append(Block(np.array([2 * k, 2 * k + 1]), np.array([[vx, c], [c, vy]]), "ip", int(k)))
    for s in range(fp.n_scale_bars):
        out.append(Block(np.array([2 * n_ip + s]), np.array([[fp.sb_var[s]]]), "sb", s))
    for g in range(fp.n_direct_groups):
        b, e = int(fp.dg_row_begin[g]), int(fp.dg_row_begin[g + 1])
        if e <= b:
            continue
        rows = 2 * n_ip + fp.n_scale_bars + np.arange(b, e)
        off = int(fp.dg_disp_offset[g]) if len(fp.dg_disp_offset) > g else -1
        D = fp.dg_disp[off:off + (e - b) ** 2].reshape(e - b, e - b) if off >= 0 else np.diag(fp.dg_var[b:e])
        out.append(Block(rows, D, "dg", g))
    out.sort(key=lambda blk: int(blk.rows[0]))
    return out


def block_weights(blocks, s0, eng=None):
    """P of every block: sigma0^2 inv(D); with an engine, the dense image blocks take the inverse the device holds."""
    out = []
    for blk in blocks:
        if blk.kind == "blk" and eng is not None:
            out.append(s0 * eng.get_block_weight(blk.index))
        elif blk.D.shape[0] == 2 and blk.D[0, 1] != 0:
            vx, vy, c = blk.D[0, 0], blk.D[1, 1], blk.D[0, 1]
            det = vx * vy - c * c
            out.append(s0 * np.array([[vy, -c], [-c, vx]]) / det)
        elif np.count_nonzero(blk.D - np.diag(np.diag(blk.D))) == 0:
            out.append(np.diag(s0 / np.diag(blk.D)))
        else:
            out.append(s0 * np.linalg.inv(blk.D))
    return out


def block_group(fp, groups, blk):
    """The group of a weight block (-1: none); a dense image block must be in one group."""
    if blk.kind == "blk":
        if groups.ip is None:
            return -1
        b, e = int(fp.blk_ip_begin[blk.index]), int(fp.blk_ip_begin[blk.index + 1])
        ids = np.asarray(groups.ip)[b:e]
        assert np.all(ids == ids[0]), "a group is a union of weight blocks"
        return int(ids[0])
    ids = {"ip": groups.ip, "sb": groups.sb, "dg": groups.dg}[blk.kind]
    return -1 if ids is None else int(np.asarray(ids)[blk.index])


def derived(n, omega, r, s0):
    """status, s2, k, sd of a group in float64, as the header defines them"""
    if n == 0:
        st = EMPTY
    elif not (np.isfinite(omega) and np.isfinite(r)):
        st = NOT_FINITE
    elif r <= UNCONTROLLED_TOL * n:
        st = UNCONTROLLED
    else:
        st = 0
    if st:
        return st, np.nan, np.nan, np.nan
    s2 = np.float64(omega) / np.float64(r)
    k = s2 / np.float64(s0)
    return st, s2, k, k * np.sqrt(np.float64(2.0) / np.float64(r))


def components(fp, groups, v, r, blocks, weights, s0):
    """The table of the header from v, r of every row and the blocks' P, every sum in longdouble."""
    G = int(groups.n_groups)
    n = np.zeros(G); om = np.zeros(G, LD); rs = np.zeros(G, LD); S = np.zeros(G, LD); R = np.zeros(G, LD)
    tot = np.zeros(4, LD)
    for blk, P in zip(blocks, weights):
        vb = v[blk.rows].astype(LD); Pb = P.astype(LD)
        o = vb @ (Pb @ vb); s = np.abs(vb) @ (np.abs(Pb) @ np.abs(vb))
        rb = r[blk.rows].astype(LD).sum(); ra = np.abs(r[blk.rows]).astype(LD).sum()
        tot += np.array([o, rb, s, ra], LD)
        g = block_group(fp, groups, blk)
        if g < 0:
            continue
        n[g] += blk.rows.size; om[g] += o; rs[g] += rb; S[g] += s; R[g] += ra
    table = np.zeros((COLUMNS, G)); status = np.zeros(G, np.int32)
    table[0] = n; table[1] = om.astype(np.float64); table[2] = rs.astype(np.float64)
    for g in range(G):
        status[g], table[3, g], table[4, g], table[5, g] = derived(n[g], table[1, g], table[2, g], s0)
    return Components(table, status, S.astype(np.float64), R.astype(np.float64), float(tot[0]), float(tot[1]), float(tot[2]), float(tot[3]))


def redundancy(A, Q, blocks, weights):
    """r = diag(Q_vv P) = 1 - diag(A Q A' P), block by block"""
    r = np.zeros(A.shape[0])
    AQ = A @ Q
    for blk, P in zip(blocks, weights):
        H = AQ[blk.rows] @ A[blk.rows].T
        r[blk.rows] = 1.0 - np.einsum("ij,ji->i", H, P)
    return r


# ---- the adjustment on the CPU (the oracle's rows and its estimate) ---------------------------------------------------------------
def oracle_design(orc, fp, vals):
    """Dense A (n_rows x U) and w (observed - computed) at `vals`, the image rows from the oracle's row routine."""
    n_ip, U = fp.n_image_points, fp.n_unknowns
    A = np.zeros((fp.n_observations, U)); w = np.zeros(fp.n_observations)
    for k in range(n_ip):
        wr, Ar, _, _ = orc.rows(vals, k)
        img, pt = int(fp.ip_image[k]), int(fp.ip_point[k])
        cam = int(fp.image_camera[img])
        jb, je = int(fp.cam_dist_begin[cam]), int(fp.cam_dist_begin[cam + 1])
        cols = np.array(list(fp.point_col[pt]) + list(fp.io_col[cam]) + list(fp.eo_col[img]) + list(fp.dist_col[jb:je]))
        ok = cols >= 0
        for c in range(2):
            w[2 * k + c] = wr[c]
            np.add.at(A[2 * k + c], cols[ok], Ar[c, :cols.size][ok])
    row = 2 * n_ip
    for s in range(fp.n_scale_bars):
        a, b = int(fp.sb_point_a[s]), int(fp.sb_point_b[s])
        d = vals[3 * b:3 * b + 3] - vals[3 * a:3 * a + 3]
        ln = np.linalg.norm(d)
        for t, c in enumerate(list(fp.point_col[a]) + list(fp.point_col[b])):
            if c >= 0:
                A[row + s, c] += (-d if t < 3 else d)[t % 3] / ln
        w[row + s] = fp.sb_length[s] - ln
    row += fp.n_scale_bars
    slot_col = fp.slot_columns()
    for i in range(fp.n_direct_rows):
        c = slot_col[fp.dg_slot[i]]
        if c >= 0:
            A[row + i, c] = 1.0
        w[row + i] = fp.dg_obs[i] - vals[fp.dg_slot[i]]
    return A, w


def gauss_newton(orc, fp, blocks, P, values, max_iter=30):
    """Dense undamped Gauss-Newton in numpy for a problem without datum defect: (values, Q = inv(A' P A), A, w) at the solution."""
    assert fp.rank_defect == 0
    vals = np.array(fp.values if values is None else values, np.float64)
    for _ in range(max_iter):
        A, w = oracle_design(orc, fp, vals)
        PA = np.zeros_like(A); Pw = np.zeros_like(w)
        for blk, Pb in zip(blocks, P):
            PA[blk.rows] = Pb @ A[blk.rows]
            Pw[blk.rows] = Pb @ w[blk.rows]
        Q = np.linalg.inv(A.T @ PA)
        dx = Q @ (A.T @ Pw)
        if np.max(np.abs(dx)) <= 1e-7:                     # (mm, rad) far below the noise: A, w, Q are the solution's
            return vals, Q, A, w
        vals, _ = orc.update(vals, dx)
    raise ArithmeticError("the Gauss-Newton iteration did not converge")


def cpu_components(orc_mod, fp, groups, values=None):
    """Adjusts fp on the CPU and returns (Components, adjusted values): dense Gauss-Newton in numpy on the oracle's rows, or, for a
    free network (whose bordered system the oracle knows how to build), the oracle's own estimate."""
    orc = orc_mod.Oracle(fp)
    blocks = weight_blocks(fp)
    P = block_weights(blocks, fp.sigma2apriori)
    if fp.rank_defect == 0:
        vals, Q, A, w = gauss_newton(orc, fp, blocks, P, values)
    else:
        vals, Qp, res = orc.estimate(values=values, invert=True)
        Q = packed_to_full(Qp, fp.n_unknowns)
        A, w = oracle_design(orc, fp, vals)
    return components(fp, groups, -w, redundancy(A, Q, blocks, P), blocks, P, fp.sigma2apriori), vals


def cpu_estimate(orc_mod, fp, groups, tol=0.05, max_iter=10):
    """The iteration of engine.estimate_variance_components with the oracle in the engine's place: (factors, tables, converged)."""
    factors = np.ones(groups.n_groups)
    tables, vals = [], None
    for _ in range(max_iter):
        comp, vals = cpu_components(orc_mod, fp, groups, vals)
        tables.append(comp)
        k = np.where(np.isfinite(comp.table[4]), comp.table[4], 1.0)
        factors = factors * k
        if np.max(np.abs(k - 1.0)) <= tol:
            return factors, tables, True
        fp = scale_dispersions(fp, groups, k)
    return factors, tables, False


# ---- scenes whose declared dispersions are misstated by known factors -------------------------------------------------------------
MISSTATED = (0.25, 2.25, 1.0)       # first half of the images, second half, the control group


def halves(fp):
    """Three groups: the image points of the first and of the second half of the images, the directly observed groups."""
    ip = (np.asarray(fp.ip_image) >= fp.n_images // 2).astype(np.int32)
    return Groups(ip, None, np.full(fp.n_direct_groups, 2, np.int32), 3, ["first half", "second half", "control"])


def misstated(fp):
    """(problem with the declared dispersions of the groups multiplied by MISSTATED -- the noise stays what it was --, groups)"""
    g = halves(fp)
    return dataclasses.replace(scale_dispersions(fp, g, np.array(MISSTATED)), truth=fp.truth), g
