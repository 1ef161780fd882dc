"""Plain numpy restatement of the leave-one-out table of every image point (include/jaicov_reliability_points.h): the dense
P A Q A' P of every weight block, numpy.linalg for inv(M) and the eigenvalues.  Held to truth by
tests/test_point_reliability_reference.py (row deletion and a second solve), used by tests/test_gpu_point_reliability.py."""
import numpy as np

UNCONTROLLED = 1e-10
COLUMNS = ["q", "T_prio", "T_post", "nabla_x", "nabla_y", "Mxx", "Mxy", "Myy", "mdb_major", "mdb_minor", "delta_ext", "dX", "dY", "dZ"]


def point_reliability(A, w, blocks, Q, s0, s2t, lambda0, omega, dof, dx=None, point_cols=None, n_image_points=None, points=None,
                      full_shift=False):
    """blocks: [(rows, D)] as design() of tests/test_gpu_reliability.py gives them.  A block holds image points when its rows are
    consecutive pairs (2k, 2k+1) below 2 n_image_points (default: len(point_cols), or every such block).  points: the image points
    k to form (default: all).  point_cols: (n_points, 3) columns of every image point's own object point (-1: fixed) for dX, dY, dZ; None leaves
    them NaN.  Returns (table (14, n), cond2(M) (n,)) and, with full_shift, also the whole vectors -Q A' P[:, S] nabla^ (n, U)."""
    dxv = np.zeros(A.shape[1]) if dx is None else np.asarray(dx, float)
    v = A @ dxv - w
    img = [(np.asarray(rows), D) for rows, D in blocks if len(rows) >= 2 and len(rows) % 2 == 0 and rows[0] % 2 == 0
           and np.array_equal(rows, np.arange(rows[0], rows[0] + len(rows)))]
    if n_image_points is None and point_cols is not None:
        n_image_points = len(point_cols)
    if n_image_points is not None:                         # rows past the image coordinates are never image points
        img = [(rows, D) for rows, D in img if rows[-1] < 2 * n_image_points]
    n = n_image_points if n_image_points is not None else (max(int(rows[-1]) for rows, _ in img) // 2 + 1 if img else 0)
    want = np.ones(n, bool) if points is None else np.isin(np.arange(n), points)
    tab = np.full((14, n), np.nan)
    cond = np.full(n, np.nan)
    shifts = np.full((n, A.shape[1]), np.nan) if full_shift else None
    for rows, D in img:
        if not want[rows[::2] // 2].any():
            continue
        Ab = A[rows]
        P = s0 * np.linalg.inv(D)
        PA = P @ Ab
        N = PA @ Q @ PA.T                                  # P A Q A' P of the block
        g = P @ v[rows]
        QAtP = Q @ PA.T                                    # Q A' P[:, rows] (U x m)
        for i in range(0, len(rows), 2):
            k = int(rows[i]) // 2
            if not want[k]:
                continue
            S = [i, i + 1]
            PS = P[np.ix_(S, S)]
            M = PS - N[np.ix_(S, S)]
            M = 0.5 * (M + M.T)
            tab[5, k], tab[6, k], tab[7, k] = M[0, 0], M[0, 1], M[1, 1]
            mu = np.linalg.eigvalsh(M)
            cond[k] = abs(mu[1]) / max(abs(mu[0]), np.finfo(float).tiny)
            if not mu[0] > UNCONTROLLED * max(PS[0, 0], PS[1, 1]):
                continue
            nab = -np.linalg.solve(M, g[S])
            q = float(-g[S] @ nab)
            tab[0, k] = q
            tab[1, k] = q / (2.0 * s2t)
            if dof > 2 and omega > 0 and omega - q > 0:
                tab[2, k] = (q / 2.0) / ((omega - q) / (dof - 2))
            tab[3, k], tab[4, k] = nab
            tab[8, k] = np.sqrt(lambda0 * s2t / mu[0])
            tab[9, k] = np.sqrt(lambda0 * s2t / mu[1])
            lam = np.max(np.linalg.eigvals(np.linalg.solve(M, PS)).real)
            tab[10, k] = np.sqrt(lambda0 * max(lam - 1.0, 0.0))
            sh = -QAtP[:, S] @ nab
            if full_shift:
                shifts[k] = sh
            if point_cols is not None:
                for a in range(3):
                    c = int(point_cols[k][a])
                    tab[11 + a, k] = sh[c] if c >= 0 else 0.0
    return (tab, cond, shifts) if full_shift else (tab, cond)
