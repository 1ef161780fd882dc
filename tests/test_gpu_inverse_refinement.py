"""newton_schulz_exact (csrc/batchinv.hip), the step that refines the solver's inverse for orders up to 8192, through the debug hook
jaicov_debug_newton_schulz: host matrices in, the refined inverse and the residual square out, the device leading dimension the
solver's (n + 128).

Two kinds of assert.  Accuracy: the device's result and newton_schulz_reference.step from the same start are two evaluations of one
formula; their difference, scaled by truth's diagonal, is held to MARGIN times the reference's own distance from truth.  Exactness:
with integer operands that are their own leading slices the residual is known to the bit, at an ordinary order and at the one where
the 53 bits of the exactness argument are all used.  Only these tell an exact product from a merely accurate one."""
import ctypes as C

import numpy as np
import pytest

import newton_schulz_reference as ns
from bundle_adjustment_amd import engine

pytestmark = pytest.mark.gpu

MARGIN = 8.0


def device_step(M, Q0, want_residual=True):
    lib = engine.load_library()
    lib.jaicov_debug_newton_schulz.argtypes = [C.c_int] + [C.c_void_p] * 4
    lib.jaicov_debug_newton_schulz.restype = C.c_int
    n = M.shape[0]
    M, Q0 = np.ascontiguousarray(M, np.float64), np.ascontiguousarray(Q0, np.float64)
    Q = np.empty((n, n)); R = np.empty((n, n)) if want_residual else None
    rc = lib.jaicov_debug_newton_schulz(n, M.ctypes.data, Q0.ctypes.data, Q.ctypes.data, R.ctypes.data if want_residual else None)
    assert rc == 0, rc
    return Q, R


def certified_inverse(oracle_mod, M):
    """inv(M) by the oracle's extended-precision inverse + compensated step (exact_block_weight with sigma0^2 = 1 on a carrier problem whose
    dispersions are M): what tests/test_oracle.py certifies in binary128."""
    m = M.shape[0]
    return oracle_mod.Oracle(ns.with_dispersions(ns.carrier(m), [M] * 3)).exact_block_weight(1.0, 0)[0]


def scaled_diff(A, B, T):
    s = np.sqrt(np.diag(T))
    return float((np.abs(A - B) / np.outer(s, s)).max())


@pytest.mark.parametrize("n", [128, 384, 2048, 2176])
def test_the_device_and_the_reference_step_agree_from_the_same_start(oracle_mod, n):
    """Spectrum 1 ... 1e-8, Q0 = numpy's inverse, symmetrised (7e-10 from truth).  2176 is the first order whose rows slice_rows_kernel reads
    twice instead of keeping them in registers.  Truth: extended-precision Newton steps to convergence for n <= 384, and for the two
    large orders the permuted block-diagonal arrangement of the truth of one block of order 128.

    Extended precision converges to cond * 2^-64 = 5e-13 at this spectrum (measured), so that is the reference's distance from THAT truth
    and the first assert allows 4e-12 -- still 200 times below what a missing or wrong step leaves.  The second assert takes the
    oracle's certified inverse as truth instead, from which the reference step is 2e-15 ... 4e-15 away: two evaluations of one formula
    from one start differ by the rounding of three small products, and are held to that.  So the first truth shows little more than that a
    step happened, and the second is the assert that binds."""
    if n <= 384:
        M = ns.spectrum_matrix(n, 8, 300 + n)
        Q0 = np.linalg.inv(M)
        T = ns.newton_ld(M, Q0, tol=2e-12).astype(np.float64)
        Tc = certified_inverse(oracle_mod, M)
    else:
        B = ns.spectrum_matrix(128, 8, 300)
        M, arrange = ns.permuted_blocks(B, n, 300 + n)
        Q0 = np.linalg.inv(M)
        T = arrange(ns.newton_ld(B, np.linalg.inv(B), tol=2e-12).astype(np.float64))
        Tc = arrange(certified_inverse(oracle_mod, B))
    Q0 = 0.5 * (Q0 + Q0.T)
    ref, Rref = ns.step(M, Q0)
    Q, R = device_step(M, Q0)
    assert np.array_equal(Q, Q.T)
    for name, truth in (("extended-precision Newton", T), ("certified", Tc)):
        own, diff, start = ns.corr_err(ref, truth), scaled_diff(Q, ref, truth), ns.corr_err(Q0, truth)
        print(f"n {n}, truth {name}: start {start:.2e}, reference step {own:.2e}, device {ns.corr_err(Q, truth):.2e}, device - reference {diff:.2e}")
        assert start > 10 * MARGIN * own                        # a step that does nothing is far outside
        assert diff <= MARGIN * own, (name, diff, own)
    # The residual square is the one the reference formed, to the rounding of the two inexact products: each evaluation is within
    # (n + 2) 2^-53 (|D1| |X2| + |D2| |X|) of their exact value entry by entry in ANY summation order (the classical bound of a dot
    # product), the leading product is exact in both, and adding the three costs each side two more roundings of a partial sum.
    D1, D2 = ns.slice_rows(M)
    X1r, X2r = ns.slice_rows(Q0)
    u = 2.0 ** -53
    bound = 2 * (n + 2) * u * (np.abs(D1) @ np.abs(X2r).T + np.abs(D2) @ np.abs(Q0)) + 4 * u * (np.abs(np.eye(n) - D1 @ X1r.T) + np.abs(Rref))
    share = np.divide(np.abs(R - Rref), bound, out=np.zeros_like(bound), where=bound > 0)      # (bound = 0: outside the blocks, where both are 0)
    print(f"n {n}: max |R| {np.abs(Rref).max():.2e}, max |R - R_ref| {np.abs(R - Rref).max():.2e}, worst share of the rounding bound {share.max():.2e}")
    assert (np.abs(R - Rref) <= bound).all()


def test_the_step_is_quadratic_with_the_right_sign():
    """Start: truth with every entry off by a relative 1e-6 (E symmetric standard normal), n = 384.  R = -M (T o 1e-6 E) has to stay far
    below 1 for the quadratic region, so the matrix is well conditioned (spectrum 1 ... 0.1; extended-precision truth is then good to
    1e-16).  The result agrees with the reference step and is closer to truth than 1e-3 of the start's distance (the reference: 5e-6 of
    it); a step with the wrong sign, or slices that are not transposed, ends no closer than it began."""
    n = 384
    M = ns.spectrum_matrix(n, 1, 12)
    T = ns.newton_ld(M, np.linalg.inv(M)).astype(np.float64)
    E = np.random.Generator(np.random.Philox(5)).normal(size=(n, n))
    E = np.tril(E) + np.tril(E, -1).T
    X0 = T * (1.0 + 1e-6 * E)
    ref, _ = ns.step(M, X0)
    before, own = ns.corr_err(X0, T), ns.corr_err(ref, T)
    assert own < 1e-3 * before                                  # the reference alone (also tests/test_newton_schulz_reference.py)
    Q, _ = device_step(M, X0, want_residual=False)
    after, diff = ns.corr_err(Q, T), scaled_diff(Q, ref, T)
    print(f"quadratic: start {before:.2e}, reference {own:.2e}, device {after:.2e}, device - reference {diff:.2e}")
    assert diff <= MARGIN * own, (diff, own)
    assert after < 1e-3 * before, (after, before)


def int64_product(A, B):
    import torch                                               # (numpy's int64 product is unblocked: 6 s at this order)
    return (torch.from_numpy(A) @ torch.from_numpy(B)).numpy()


def test_the_leading_product_is_exact():
    """n = 1024; M and Q0 random signed integers below 2^20 in magnitude, every row of M times its own power of two, Q0 symmetric: both
    low slices are zero and R = I - M Q0 to the bit, which int64 arithmetic on the host knows."""
    n = 1024
    Mi, Qi = ns.signed_integers(n, 1), ns.signed_integers(n, 2, symmetric=True)
    e = np.random.Generator(np.random.Philox(4)).integers(-12, 1, n)               # (<= 0: 1 - P 2^e keeps its last bit)
    M = np.ldexp(Mi.astype(np.float64), e[:, None])
    assert not ns.slice_rows(M)[1].any() and not ns.slice_rows(Qi.astype(np.float64))[1].any()
    P = int64_product(Mi, Qi)
    assert np.abs(P).max() < 2 ** 52                            # 1 - P 2^e is an fp64 number: P 2^e has its last bit at e <= 0 and its first below e + 52
    want = np.eye(n) - np.ldexp(P.astype(np.float64), e[:, None])
    assert np.array_equal(np.ldexp((np.eye(n) - want), -e[:, None]).astype(np.int64), P)       # nothing was rounded on the way
    _, R = device_step(M, Qi.astype(np.float64))
    assert np.array_equal(R, want), int(np.count_nonzero(R != want))


def test_the_bound_of_the_exactness_argument_met_with_equality():
    """n = 8192, every entry of M and Q0 2^20 - 1: every product is maximal, a row sum is 8192 (2^20 - 1)^2 = 2^53 - 2^34 + 2^13 and the
    diagonal of R one less in magnitude, a 53-bit odd integer.  Four GEMMs of the order (0.1 s) and the transfers: the one large shape
    here, because no smaller one reaches 53 bits."""
    n, v = 8192, 2 ** 20 - 1
    off = -(n * v * v)
    assert float(off) == off and float(1 + off) == 1 + off and (1 + off) % 2 != 0 and abs(1 + off).bit_length() == 53
    A = np.full((n, n), float(v))
    _, R = device_step(A, A)
    assert np.array_equal(np.diag(R), np.full(n, float(1 + off)))
    assert int(np.count_nonzero(R != float(off))) == n         # (the diagonal)


def test_the_hook_refuses_orders_it_does_not_serve():
    lib = engine.load_library()
    lib.jaicov_debug_newton_schulz.argtypes = [C.c_int] + [C.c_void_p] * 4
    lib.jaicov_debug_newton_schulz.restype = C.c_int
    a = np.eye(4)
    for n in (0, 100, 8192 + 128):
        rc = lib.jaicov_debug_newton_schulz(n, a.ctypes.data, a.ctypes.data, a.ctypes.data, None)
        assert engine.STATUS[rc] == "BAD_ARGUMENT", rc          # before any access
