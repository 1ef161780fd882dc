"""numpy restatement of the datum transformation of include/jaicov_datum.h (Baarda's S-transformation), for the tests.

Q is the complete bordered inverse of order U (border rows / columns 0 .. d-1 first, the layout of jaicov_neq_get_cofactor and of
the oracle); B_new holds the d datum rows of the new datum over all U columns (zeros in the border columns), as the engine's and
the oracle's finalize write them into the border of N."""
import numpy as np


def border_rows(oracle, values):
    """The d datum rows (d x U) that the oracle's finalize writes for its problem's point_datum at `values`."""
    fp = oracle.fp
    U, d = fp.n_unknowns, fp.rank_defect
    N = np.zeros(fp.packed_length); n = np.zeros(U)
    oracle.finalize(values, N, n)
    B = np.zeros((d, U))
    for r in range(d):
        for c in range(d, U):
            B[r, c] = N[r + c * (c + 1) // 2]
    return B


def s_parts(Q, B_new, d):
    """(Z, Y~) of the transformation: G^ = Q[d:, :d], C = (B' G^)^-1, Z = G^ C, Y = Q B'', W = B' Y, Y~ = Y - Z W / 2 (over the
    unknowns, rows d .. n-1 of an order-n cofactor matrix)."""
    n = Q.shape[0]
    Bp = B_new[:, d:n]
    G = Q[d:, :d]
    C = np.linalg.inv(Bp @ G)
    Z = G @ C
    Y = Q[d:, d:] @ Bp.T
    W = Bp @ Y
    W = 0.5 * (W + W.T)
    return Z, Y - 0.5 * Z @ W


def transform(Q, B_new, d):
    """The bordered inverse in the new datum: Q' = Q - Z Y~' - Y~ Z' on the unknowns, Z in the border block, 0 in the border x
    border block.  Works for the reduced cofactor matrix too (B_new touches point columns only)."""
    n = Q.shape[0]
    Z, Yt = s_parts(Q, B_new, d)
    out = np.zeros((n, n))
    out[d:, d:] = Q[d:, d:] - Z @ Yt.T - Yt @ Z.T
    out[d:, :d] = Z
    out[:d, d:] = Z.T
    return out


def apply(Q_old, B_new, d, v):
    """S v = v - Z (B' v) with the S of the transformation of Q_old to the datum of B_new; border entries 0."""
    n = Q_old.shape[0]
    Z, _ = s_parts(Q_old, B_new, d)
    out = np.zeros(n)
    out[d:] = v[d:] - Z @ (B_new[:, d:n] @ v[d:])
    return out
