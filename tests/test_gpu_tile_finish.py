"""Off-diagonal tiles finished from the accumulators (csrc/cholflow.hip, chol_tile_kernel with REG_FINISH): the factor itself, every
entry against LAPACK, at the orders where the finish can go wrong on its own -- one off-diagonal tile, a ragged last block, several
tiles per column with the chain workgroups' own tiles beside them, and a tile that is finished after a partial sum was added.
tests/test_tile_finish_model.py holds the index work on the host."""
import ctypes as C

import numpy as np
import pytest

from bundle_adjustment_amd import engine

pytestmark = pytest.mark.gpu


def _factor(S):
    """The factor of S from jaicov_debug_potrf_factor.  The solver works on whole 128-blocks: an order in between is padded with the
    identity, as the engine pads its own matrices (the last block row's tiles are then ragged: zeros right of and below the data), and
    the padding must come back as the identity."""
    lib = engine.load_library()
    lib.jaicov_debug_potrf_factor.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    n = S.shape[0]
    npad = -(-n // 128) * 128
    P = np.eye(npad)
    P[:n, :n] = S
    out = np.zeros((npad, npad))
    assert lib.jaicov_debug_potrf_factor(npad, P.ctypes.data, out.ctypes.data) == 0
    out = np.tril(out)
    assert np.array_equal(out[n:, :n], np.zeros((npad - n, n))) and np.array_equal(out[n:, n:], np.eye(npad - n))
    return np.ascontiguousarray(out[:n, :n])


def _matrix(n, seed):
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(n, n + 20))
    return np.ascontiguousarray(G @ G.T / n + np.eye(n))


def _set_form(monkeypatch, form):
    monkeypatch.setenv("JAICOV_FLOW_MIN_BLOCKS", "1")
    if form != "chain":
        monkeypatch.setenv("JAICOV_FACTOR_FORM", form)


@pytest.mark.parametrize("form", ["chain", "chain3", "two_step"])
@pytest.mark.parametrize("n", [256, 300, 640])
def test_finished_tiles_against_lapack(n, form, monkeypatch):
    """atol 1e-12, rtol 0: the bound of the tile-by-tile tests of test_gpu_parity.py, on the same kind of matrix.  Two runs, same bits."""
    _set_form(monkeypatch, form)
    S = _matrix(n, n)
    L = _factor(S)
    err = float(np.abs(L - np.linalg.cholesky(S)).max())
    print(f"n = {n}, {form}: max |L - LAPACK| = {err:.2e}")
    assert err <= 1e-12
    assert _factor(S).tobytes() == L.tobytes()


@pytest.mark.parametrize("form", ["chain", "two_step"])
def test_finish_after_a_partial_sum(form, monkeypatch):
    """18 block columns, update ranges in two pieces from block column 16 on: the tiles of the last columns are finished after the
    partial sum of the other piece was added to the accumulators."""
    _set_form(monkeypatch, form)
    monkeypatch.setenv("JAICOV_FLOW_SPLIT", "2:0")
    n = 2304
    S = _matrix(n, n + len(form))
    L = _factor(S)
    err = float(np.abs(L - np.linalg.cholesky(S)).max())
    print(f"n = {n}, {form}, split 2:0: max |L - LAPACK| = {err:.2e}")
    assert err <= 1e-12
    assert _factor(S).tobytes() == L.tobytes()


@pytest.mark.parametrize("form", ["chain", "two_step"])
def test_finished_tiles_of_a_badly_scaled_matrix(form, monkeypatch):
    """D S D with D = diag(10^e), e uniform in [-3, 3]: still SPD, entries of L over six decades.  Held to 1e-12 max|L| against LAPACK.
    (LAPACK itself stays at 1.3e-16 max|L| from a factor computed in extended precision on this very matrix, measured on the host;
    the bound needs no widening.)"""
    _set_form(monkeypatch, form)
    n = 640
    rng = np.random.default_rng(77)
    d = 10.0 ** rng.uniform(-3, 3, size=n)
    S = np.ascontiguousarray(_matrix(n, 78) * d[:, None] * d[None, :])
    ref = np.linalg.cholesky(S)
    L = _factor(S)
    err = float(np.abs(L - ref).max() / np.abs(ref).max())
    print(f"n = {n}, {form}, scaled: max |L - LAPACK| = {err:.2e} of max|L|")
    assert err <= 1e-12
    assert _factor(S).tobytes() == L.tobytes()


@pytest.mark.parametrize("n", [640, 2304])
def test_the_finish_keeps_the_sums_of_the_pipelined_loop(n, monkeypatch):
    """The one-kernel form still finishes its tiles through a scratch tile and the pipelined loop; the two-step form has the same diagonal
    blocks and finishes from the accumulators.  The finish feeds the MFMA the same values in the same lane groups in the same order and
    skips only products with zeros at the end of a sum (cholflow.hip, transpose_acc), so both forms give the same bits."""
    S = _matrix(n, n)
    _set_form(monkeypatch, "two_step")
    L = _factor(S)
    _set_form(monkeypatch, "one_kernel")
    assert _factor(S).tobytes() == L.tobytes()
