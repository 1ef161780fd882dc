"""CPU: tests/point_reliability_reference.py, the numpy restatement of include/jaicov_reliability_points.h, held to truth without any
engine.  The two identities it rests on are checked the long way: delete the two rows of an image point and the matching rows and
columns of the dispersion, solve again, compare the step and Omega."""
import numpy as np
import pytest

from point_reliability_reference import point_reliability

SIZES = [2, 2, 2, 8, 6, 2, 1]       # weight blocks: three 2 x 2, two dense image blocks, one more 2 x 2, one single row (23 rows, 9 unknowns)
U = 9
S0 = 0.7
LAMBDA0 = 17.075


def spd(rng, m):
    R = rng.standard_normal((m, m))
    return (R @ R.T + m * np.eye(m)) * 0.05


def model(seed, border):
    rng = np.random.default_rng(seed)
    n = sum(SIZES)
    A = rng.standard_normal((n, U))
    B = None
    if border:                                           # a datum defect of 2 spanned by the border rows, as inner constraints leave it
        B = rng.standard_normal((2, U))
        A = A @ (np.eye(U) - np.linalg.pinv(B) @ B)
    w = rng.standard_normal(n)
    blocks, r = [], 0
    for m in SIZES:
        blocks.append((np.arange(r, r + m), spd(rng, m)))
        r += m
    return A, w, blocks, B


def solve(A, w, blocks, B):
    """dx, Q, Omega of v = A dx - w with P = S0 inv(D), the bordered system where there is a border"""
    n = A.shape[0]
    P = np.zeros((n, n))
    for rows, D in blocks:
        P[np.ix_(rows, rows)] = S0 * np.linalg.inv(D)
    N = A.T @ P @ A
    rhs = A.T @ P @ w
    if B is not None:
        d = B.shape[0]
        K = np.block([[N, B.T], [B, np.zeros((d, d))]])
        Q = np.linalg.inv(K)[:U, :U]
    else:
        Q = np.linalg.inv(N)
    dx = Q @ rhs
    v = A @ dx - w
    return dx, Q, float(v @ P @ v)


def delete(A, w, blocks, k):
    """the model without the rows 2k, 2k+1 and without the matching rows and columns of their dispersion block"""
    S = np.array([2 * k, 2 * k + 1])
    keep = np.setdiff1d(np.arange(A.shape[0]), S)
    new = -np.ones(A.shape[0], int)
    new[keep] = np.arange(keep.size)
    out = []
    for rows, D in blocks:
        sel = ~np.isin(rows, S)
        if sel.any():
            out.append((new[rows[sel]], D[np.ix_(sel, sel)]))
    return A[keep], w[keep], out


@pytest.mark.parametrize("border", [False, True])
def test_deleting_an_image_point_gives_the_shift_and_the_drop_of_omega(border):
    A, w, blocks, B = model(11 + border, border)
    dx, Q, omega = solve(A, w, blocks, B)
    n_pts = (sum(SIZES) - 1) // 2
    dof = A.shape[0] - U + (2 if border else 0)
    tab, cond, shifts = point_reliability(A, w, blocks, Q, S0, S0, LAMBDA0, omega, dof, dx=dx, n_image_points=n_pts, full_shift=True)
    assert tab.shape == (14, n_pts) and np.all(np.isfinite(tab[:11]))
    worst = [0.0, 0.0]
    for k in (0, 1, 2, 3, 6, 7, 9, 10):                   # every 2-row block, two points inside each dense block
        A2, w2, blocks2 = delete(A, w, blocks, k)
        dx2, _, omega2 = solve(A2, w2, blocks2, B)
        d = dx2 - dx
        e_dx = np.max(np.abs(d - shifts[k])) / np.max(np.abs(d))
        e_om = abs(omega2 - (omega - tab[0, k])) / omega
        worst = [max(worst[0], e_dx), max(worst[1], e_om)]
        assert e_dx <= 1e-12 and e_om <= 1e-12, (k, e_dx, e_om)
        # the 2-D test of the deleted point against the variance of the rest: T_post by its definition
        assert tab[2, k] == pytest.approx((tab[0, k] / 2) / (omega2 / (dof - 2)), rel=1e-10)
    print("deletion identities, border=%s: step %.1e, omega %.1e" % (border, *worst))


def one_dimensional(A, w, blocks, Q, dx):
    """g, (P Q_vv P)_ii and r_i of every row, as the one-dimensional test forms them"""
    n = A.shape[0]
    v = A @ dx - w
    g = np.zeros(n); ppp = np.zeros(n); r = np.zeros(n)
    for rows, D in blocks:
        P = S0 * np.linalg.inv(D)
        H = A[rows] @ Q @ A[rows].T
        g[rows] = P @ v[rows]
        ppp[rows] = np.diag(P - P @ H @ P)
        r[rows] = 1.0 - np.diag(H @ P)
    return g, ppp, r


def test_the_joint_test_is_never_below_half_the_larger_one_dimensional_one():
    A, w, blocks, B = model(5, False)
    dx, Q, omega = solve(A, w, blocks, B)
    s2t = 1.3
    n_pts = (sum(SIZES) - 1) // 2
    tab, _ = point_reliability(A, w, blocks, Q, S0, s2t, LAMBDA0, omega, A.shape[0] - U, dx=dx, n_image_points=n_pts)
    g, ppp, _ = one_dimensional(A, w, blocks, Q, dx)
    for k in range(n_pts):
        assert np.allclose([tab[5, k], tab[7, k]], ppp[2 * k:2 * k + 2], rtol=1e-12)
        for c in range(2):
            t2 = g[2 * k + c] ** 2 / (s2t * ppp[2 * k + c])
            assert tab[0, k] >= g[2 * k + c] ** 2 / ppp[2 * k + c] * (1 - 1e-12)
            assert tab[1, k] >= t2 / 2 * (1 - 1e-12)
        assert tab[8, k] >= tab[9, k] > 0 and tab[10, k] >= 0


def test_uncorrelated_coordinates_with_a_diagonal_m():
    """x rows and y rows over separate unknowns with diagonal weights: M is diagonal, q = s2t (t_x^2 + t_y^2), nabla^ = -v / r and
    delta_ext^2 = lambda0 (1 - r) / r of the weaker coordinate."""
    rng = np.random.default_rng(3)
    n_pts, ux, uy = 7, 3, 2
    A = np.zeros((2 * n_pts, ux + uy))
    A[0::2, :ux] = rng.standard_normal((n_pts, ux))
    A[1::2, ux:] = rng.standard_normal((n_pts, uy))
    w = rng.standard_normal(2 * n_pts)
    blocks = [(np.array([2 * k, 2 * k + 1]), np.diag(rng.uniform(0.5, 2.0, 2))) for k in range(n_pts)]
    dx, Q, omega = solve(A, w, blocks, None)
    s2t = 0.9
    tab, cond = point_reliability(A, w, blocks, Q, S0, s2t, LAMBDA0, omega, 2 * n_pts - ux - uy, dx=dx)
    g, ppp, r = one_dimensional(A, w, blocks, Q, dx)
    v = A @ dx - w
    t2 = g ** 2 / (s2t * ppp)
    assert np.max(np.abs(tab[6])) <= 1e-14 * np.max(tab[5])
    np.testing.assert_allclose(tab[0], s2t * (t2[0::2] + t2[1::2]), rtol=1e-11)
    np.testing.assert_allclose(tab[3], -v[0::2] / r[0::2], rtol=1e-11)
    np.testing.assert_allclose(tab[4], -v[1::2] / r[1::2], rtol=1e-11)
    rmin = np.minimum(r[0::2], r[1::2])
    np.testing.assert_allclose(tab[10] ** 2, LAMBDA0 * (1 - rmin) / rmin, rtol=1e-10)


def test_a_point_seen_twice_is_not_controlled():
    """Four rows of two image points over three private unknowns: each M has rank 1.  Columns 0-4 and 8-13 are NaN, M is written."""
    rng = np.random.default_rng(8)
    n_pts, u = 8, 7
    A = np.zeros((2 * n_pts, u))
    A[:4, :3] = rng.standard_normal((4, 3))              # image points 0 and 1 see the private point (unknowns 0-2) and nothing else
    A[4:, 3:] = rng.standard_normal((2 * n_pts - 4, u - 3))
    w = rng.standard_normal(2 * n_pts)
    blocks = [(np.array([2 * k, 2 * k + 1]), spd(rng, 2)) for k in range(n_pts)]
    dx, Q, omega = solve(A, w, blocks, None)
    cols = np.array([[0, 1, 2]] * 2 + [[3, 4, -1]] * (n_pts - 2))
    tab, cond = point_reliability(A, w, blocks, Q, S0, S0, LAMBDA0, omega, 2 * n_pts - u, dx=dx, point_cols=cols)
    bad = [0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 13]
    assert np.all(np.isnan(tab[bad][:, :2])) and np.all(np.isfinite(tab[5:8]))
    assert np.all(cond[:2] > 1e10)
    assert np.all(np.isfinite(tab[:, 2:]))
    assert np.all(tab[13, 2:] == 0.0)                      # a fixed coordinate does not move
