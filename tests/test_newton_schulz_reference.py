"""The plain reference of the exact-residual Newton-Schulz step (tests/newton_schulz_reference.py) against certified truth, no device.

tests/test_gpu_weight_refinement.py and tests/test_gpu_inverse_refinement.py give the device a multiple of what `step` itself
reaches and ask for fixed ratios besides (refined against unrefined: 100; after against before a step: 1e-3).  Here the reference
alone is shown to have that room: its error is at the rounding of the inverse's entries, and both ratios hold with orders to spare."""
import numpy as np
import pytest

import newton_schulz_reference as ns


def test_slices_are_exact_and_short():
    rng = np.random.Generator(np.random.Philox(3))
    A = rng.normal(size=(37, 300)) * 10.0 ** rng.uniform(-6, 6, (37, 1))
    A[5] = 0.0                                                 # a zero row gives zero slices
    A[7, 3] = 0.0
    hi, lo = ns.slice_rows(A)
    assert np.array_equal(hi + lo, A) and np.array_equal(A - hi, lo)
    assert not hi[5].any() and not lo[5].any()
    _, ex = np.frexp(np.abs(A).max(axis=1))
    unit = np.ldexp(1.0, ex - 20)[:, None]
    k = hi / unit
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max() <= 2 ** 20        # integers of at most 21 bits, in the row's unit
    assert (np.abs(lo) <= 0.5 * unit).all()


def test_the_leading_product_is_exact_in_any_order():
    """Integers below 2^20 times a power of two per row are their own leading slice: R is then I - M Q to the bit, which int64 knows."""
    n = 256
    Mi, Qi = ns.signed_integers(n, 1), ns.signed_integers(n, 2, symmetric=True)
    e = np.random.Generator(np.random.Philox(4)).integers(-12, 1, n)               # (<= 0: 1 - P 2^e keeps its last bit)
    M = np.ldexp(Mi.astype(np.float64), e[:, None])
    Q = Qi.astype(np.float64)
    assert not ns.slice_rows(M)[1].any() and not ns.slice_rows(Q)[1].any()
    _, R = ns.step(M, Q)
    want = np.eye(n) - np.ldexp((Mi @ Qi).astype(np.float64), e[:, None])
    assert np.abs(Mi @ Qi).max() < 2 ** 53
    assert np.array_equal(R, want)


# (order, decades of the spectrum, rows scaled over three decades, bound on the step's error, reason)
#   uniform scale: the step ends at the rounding of X's entries and of the update, a few 2^-53 (measured 2.2e-16 ... 2.7e-16);
#   scaled rows (cond 1e11): the two small products of R are rounded relative to |D1| |X2| + |D2| |X|, which the scaling lifts
#   over D X = I by the spread of the scales -- measured 2.0e-14, five times that allowed.
CASES = [(42, 7, False, 1e-15), (130, 7, False, 1e-15), (42, 7, True, 1e-13), (130, 7, True, 1e-13)]


@pytest.mark.parametrize("m,decades,scaled,bound", CASES)
def test_one_step_from_the_fp64_inverse_reaches_certified_truth(oracle_mod, m, decades, scaled, bound):
    D = ns.spectrum_matrix(m, decades, 100 + m, scaled)
    assert np.array_equal(D, D.T)
    fp = ns.with_dispersions(ns.carrier(m), [D] * 3)
    o = oracle_mod.Oracle(fp)
    s2 = fp.sigma2apriori
    P, _ = o.exact_block_weight(s2, 0)
    W0 = o.block_weight(s2, 0)                                 # dpptrf + dpptri in fp64
    W1 = ns.step(D, W0 / s2)[0] * s2
    e0, e1 = ns.corr_err(W0, P), ns.corr_err(W1, P)
    assert e1 <= bound, (e0, e1)
    assert e0 >= (1e2 if scaled else 1e3) * e1, (e0, e1)       # the GPU test asks 100 of the device, at uniform scale
    assert np.array_equal(W1, W1.T)


def test_the_step_is_quadratic_with_the_right_sign():
    """From truth with every entry off by a relative 1e-6: R = -M (T o 1e-6 E) must stay far below 1 for the step to be in its quadratic
    region, so the matrix is well conditioned (spectrum 1 ... 0.1).  The step lands below 1e-3 of the start's distance (measured: 5e-6 of
    it); one with the wrong sign doubles the distance instead."""
    n = 384
    M = ns.spectrum_matrix(n, 1, 12)
    T = ns.newton_ld(M, np.linalg.inv(M)).astype(np.float64)
    E = np.random.Generator(np.random.Philox(5)).normal(size=(n, n))
    E = np.tril(E) + np.tril(E, -1).T
    X0 = T * (1.0 + 1e-6 * E)
    X1, R = ns.step(M, X0)
    before, after = ns.corr_err(X0, T), ns.corr_err(X1, T)
    assert 1e-6 < before < 1e-5 and after < 1e-3 * before, (before, after)
    Y = X0 @ R
    wrong = X0 - 0.5 * (Y + Y.T)
    assert ns.corr_err(wrong, T) > 1.5 * before


def test_permuted_blocks_carry_the_small_blocks_truth(oracle_mod):
    """Order 640 from one block of order 128: the arranged exact inverse of the block is the exact inverse of the whole, and the step
    reaches it from the arranged fp64 inverse as it does at order 128."""
    B = ns.spectrum_matrix(128, 7, 21)
    fp = ns.with_dispersions(ns.carrier(128), [B] * 3)
    o = oracle_mod.Oracle(fp)
    Ph, Pl = o.exact_block_weight(1.0, 0)
    M, arrange = ns.permuted_blocks(B, 640, 22)
    assert np.array_equal(M, M.T) and np.count_nonzero(M) == 5 * 128 * 128
    T = arrange(Ph)
    res = np.eye(640, dtype=np.longdouble) - M.astype(np.longdouble) @ (T.astype(np.longdouble) + arrange(Pl))
    assert np.abs(res).max() < 1e-9                           # (fp80 residual of a cond 1e7 matrix: only that the arrangement is the inverse's)
    rows = np.abs(M).max(axis=1)
    assert np.unique(np.frexp(rows)[1]).size > 3              # rows of different binary scale
    X0 = arrange(o.block_weight(1.0, 0))
    X1, _ = ns.step(M, X0)
    e0, e1 = ns.corr_err(X0, T), ns.corr_err(X1, T)
    assert e1 <= 1e-15 and e0 >= 1e3 * e1, (e0, e1)


def test_dispersions_are_written_with_their_variances():
    fp0 = ns.carrier(20, n_images=4)
    mats = [ns.spectrum_matrix(20, 2, 30 + i) for i in range(3)] + [ns.spectrum_matrix(12, 2, 40)]     # the last image keeps 6 of its 10 points
    fp = ns.with_dispersions(fp0, mats)
    assert list(np.diff(fp.blk_ip_begin)) == [10, 10, 10, 6] and fp.n_image_points == 36
    for b, D in enumerate(mats):
        m, off, ip = D.shape[0], int(fp.blk_disp_offset[b]), int(fp.blk_ip_begin[b])
        assert np.array_equal(fp.blk_disp[off:off + m * m].reshape(m, m), D)
        assert np.array_equal(fp.ip_var_x[ip:ip + m // 2], np.diag(D)[0::2]) and np.array_equal(fp.ip_var_y[ip:ip + m // 2], np.diag(D)[1::2])
