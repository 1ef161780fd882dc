"""CPU: the C ABI of include/jaicov_precision.h is exported, declared and bound (Python: engine.PREC_EXPORTS, C++ mirror), and the
numpy restatement of tests/precision_reference.py does what the header says: the 3 x 3 Jacobi against numpy's eigvalsh, the length
sigma against a finite-difference propagation, the subspace iteration from the header's start block on the oracle's Qxx."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import precision_reference as R
from bundle_adjustment_amd import engine, scene
from bundle_adjustment_amd.problem import packed_to_full

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jaicov_precision.h")


def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(jaicov_prec_[a-z_0-9]+)\s*\(", src)))


def _lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def test_header_declarations_are_exported_and_bound():
    names = declared()
    assert names == sorted(engine.PREC_EXPORTS) == ["jaicov_prec_components", "jaicov_prec_lengths", "jaicov_prec_points", "jaicov_prec_stations"]
    for other in (engine.EXPORTS, engine.XFORM_EXPORTS, engine.DLT_EXPORTS, engine.REL_EXPORTS, engine.REL_POINT_EXPORTS, engine.DATUM_EXPORTS,
                  engine.ISECT_EXPORTS, engine.RESECT_EXPORTS, engine.RELOR_EXPORTS, engine.SIMIL_EXPORTS, engine.LENS_EXPORTS):
        assert not set(names) & set(other)
    L = _lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    for n in names:
        assert hasattr(L, n), n
        assert re.search(r"\bT %s\b" % n, syms), f"{n} is declared but not exported"
    for m in ("precision_points", "precision_stations", "precision_lengths", "principal_components", "point_column_range"):
        assert callable(getattr(engine.Engine, m)), m
    from bundle_adjustment_amd import host_api
    for m in ("pointPrecision", "stationPrecision", "lengthPrecision", "principalComponents"):
        assert hasattr(host_api.BundleAdjustment, m), m
    # the header's constants are the binding's
    text = open(HEADER).read()
    consts = dict(re.findall(r"#define JAICOV_PREC_(\w+) (\d+)", text))
    assert {k: int(v) for k, v in consts.items()} == {
        "PARTIAL": engine.PREC_PARTIAL, "NEGATIVE": engine.PREC_NEGATIVE, "NOT_FINITE": engine.PREC_NOT_FINITE,
        "DEGENERATE": engine.PREC_DEGENERATE, "POINT_COLUMNS": engine.PREC_POINT_COLUMNS, "STATION_COLUMNS": engine.PREC_STATION_COLUMNS,
        "LENGTH_COLUMNS": engine.PREC_LENGTH_COLUMNS}
    assert (R.PARTIAL, R.NEGATIVE, R.NOT_FINITE, R.DEGENERATE) == (engine.PREC_PARTIAL, engine.PREC_NEGATIVE, engine.PREC_NOT_FINITE,
                                                                    engine.PREC_DEGENERATE)


def test_null_engine_is_refused_and_outputs_stay():
    L = _lib()
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    out = np.full(25, 3.0); st = np.full(1, 7, np.int32); idx = np.zeros(2, np.int32); it = C.c_int32(5)
    assert L.jaicov_prec_points(None, 1.0, 1.0, 1.0, idx.ctypes.data_as(pi), 1, out.ctypes.data_as(pd), st.ctypes.data_as(pi)) == -1
    assert L.jaicov_prec_stations(None, 1.0, 1.0, 1.0, idx.ctypes.data_as(pi), 1, out.ctypes.data_as(pd), st.ctypes.data_as(pi)) == -1
    assert L.jaicov_prec_lengths(None, 1.0, idx.ctypes.data_as(pi), 1, out.ctypes.data_as(pd), st.ctypes.data_as(pi)) == -1
    assert L.jaicov_prec_components(None, 0, 8, 1, 0.0, 10, out.ctypes.data_as(pd), out.ctypes.data_as(pd), out.ctypes.data_as(pd),
                                    out.ctypes.data_as(pd), C.byref(it)) == -1
    assert np.all(out == 3.0) and st[0] == 7 and it.value == 5


# ---- the 3 x 3 Jacobi ---------------------------------------------------------------------------------------------------------------
def _spd_blocks():
    rng = np.random.default_rng(11)
    blocks = []
    for _ in range(40):                                   # random SPD blocks, condition up to 1e8
        A = rng.normal(size=(3, 3))
        U, _ = np.linalg.qr(A)
        blocks.append(("random", (U * 10.0 ** rng.uniform(-4, 4, 3)) @ U.T))
    for _ in range(20):                                   # two equal eigenvalues
        U, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        a, b = rng.uniform(0.1, 5.0, 2)
        blocks.append(("double", (U * np.array([a, a, b])) @ U.T))
    blocks.append(("double", 2.5 * np.eye(3)))
    for k in range(3):                                    # a zero row and column (fixed coordinate)
        for _ in range(5):
            A = rng.normal(size=(3, 3)); S = A @ A.T
            S[k, :] = 0.0; S[:, k] = 0.0
            blocks.append(("zero row %d" % k, S))
    blocks.append(("zero", np.zeros((3, 3))))
    out = []
    for name, S in blocks:
        S = 0.5 * (S + S.T)
        for scale in (1.0, 1e-12, 1e12):
            out.append((f"{name} x {scale:g}", S * scale))
    return out


def test_restated_jacobi_agrees_with_eigvalsh_and_has_small_residuals():
    worst_l = worst_r = 0.0
    most = 0
    for name, S in _spd_blocks():
        l, V, sweeps = R.jacobi3(S)
        most = max(most, sweeps)
        tr = np.trace(S)
        ref = np.linalg.eigvalsh(S)[::-1]
        if tr == 0.0:
            assert np.all(l == 0.0) and np.array_equal(V, np.eye(3)), name
            continue
        el = np.abs(l - ref).max() / tr
        er = max(np.linalg.norm(S @ V[:, c] - l[c] * V[:, c]) for c in range(3)) / tr
        worst_l, worst_r = max(worst_l, el), max(worst_r, er)
        assert el <= 1e-14 and er <= 1e-14, (name, el, er)
        assert l[0] >= l[1] >= l[2], name
        assert np.abs(V.T @ V - np.eye(3)).max() <= 1e-14, name
        for c in range(3):                                # the sign rule: the first component of largest magnitude is positive
            assert V[int(np.argmax(np.abs(V[:, c]))), c] > 0.0, name
    print(f"3 x 3 Jacobi: eigenvalues {worst_l:.2e} of the trace, residuals {worst_r:.2e} of the trace, at most {most} sweeps")
    assert most < R.SWEEPS


def test_restated_point_figures():
    rng = np.random.default_rng(5)
    A = rng.normal(size=(3, 3)); Q3 = A @ A.T
    out, st = R.point_figures(Q3, 0.7, 2.0, 3.0)
    assert st == 0
    l = np.linalg.eigvalsh(Q3)[::-1]
    np.testing.assert_allclose(out[0:3], np.sqrt(0.7 * np.diag(Q3)), rtol=1e-15)
    np.testing.assert_allclose(out[3], np.sqrt(0.7 * np.trace(Q3)), rtol=1e-15)
    np.testing.assert_allclose(out[4:7], 2.0 * np.sqrt(0.7 * l), rtol=1e-13)
    l2 = np.linalg.eigvalsh(Q3[:2, :2])[::-1]
    np.testing.assert_allclose(out[16:18], 3.0 * np.sqrt(0.7 * l2), rtol=1e-13)
    d = np.array([np.cos(out[18]), np.sin(out[18])])
    assert 0.0 <= out[18] < np.pi and np.linalg.norm(Q3[:2, :2] @ d - l2[0] * d) <= 1e-13 * l2[0]
    # a fixed Y: PARTIAL, a zero semi-axis along Y
    Qf = Q3.copy(); Qf[1, :] = 0.0; Qf[:, 1] = 0.0
    out, st = R.point_figures(Qf, 1.0, fixed=(False, True, False))
    assert st == R.PARTIAL and out[6] == 0.0 and np.array_equal(out[13:16], [0.0, 1.0, 0.0]) and out[1] == 0.0
    # rounding noise below zero
    U, _ = np.linalg.qr(A)
    out, st = R.point_figures((U * np.array([1.0, 0.5, -1e-9])) @ U.T, 1.0)
    assert st == R.NEGATIVE and out[6] == 0.0 and out[21] < 0.0
    out, st = R.point_figures(np.full((3, 3), np.nan), 1.0)
    assert st == R.NOT_FINITE and np.isnan(out).all()


# ---- the length ------------------------------------------------------------------------------------------------------------------------
def test_restated_length_sigma_agrees_with_a_finite_difference_propagation():
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(20):
        XA, XB = rng.normal(size=3) * 100.0, rng.normal(size=3) * 100.0
        A = rng.normal(size=(6, 6)); Q6 = A @ A.T * 1e-4
        out, st = R.length_figures(XA, XB, Q6, 0.9)
        assert st == 0
        x = np.concatenate([XA, XB])
        f = lambda v: np.linalg.norm(v[3:] - v[:3])      # noqa: E731
        h = 1e-4
        g = np.array([(f(x + h * e) - f(x - h * e)) / (2 * h) for e in np.eye(6)])
        ref = np.sqrt(0.9 * g @ Q6 @ g)
        worst = max(worst, abs(out[1] - ref) / ref)
        assert out[0] == f(x) or abs(out[0] - f(x)) <= 4e-16 * f(x)
        np.testing.assert_allclose(out[2:5], np.sqrt(0.9 * np.array([Q6[k, k] + Q6[3 + k, 3 + k] - 2 * Q6[k, 3 + k] for k in range(3)])), rtol=1e-12)
    print(f"length sigma against central differences (h = 1e-4 on lengths of some 100): worst {worst:.2e} relative")
    # central differences of a norm: truncation h^2 / L^2 ~ 1e-12, rounding eps L / h ~ 2e-10 of a gradient of order 1
    assert worst <= 1e-8
    out, st = R.length_figures(XA, XA, Q6, 1.0)
    assert st == R.DEGENERATE and out[0] == 0.0 and np.isnan(out[1]) and np.isfinite(out[2:]).all()
    # without the cross block the sigma is another one: the correlations matter
    Q0 = Q6.copy(); Q0[:3, 3:] = 0.0; Q0[3:, :3] = 0.0
    assert abs(R.length_figures(XA, XB, Q0, 0.9)[0][1] - R.length_figures(XA, XB, Q6, 0.9)[0][1]) > 0.0


# ---- the start block and the subspace iteration ---------------------------------------------------------------------------------------
def test_start_block_is_the_headers_generator():
    X = R.start_block(3)
    assert X.shape == (3, 8) and np.all(np.abs(X) <= 0.5)
    # splitmix64 of the state 0x9E3779B97F4A7C15 (counter 0) is the first output of the published generator seeded with 0
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF
    assert X[0, 0] == (0xE220A8397B1DCDAF >> 11) * 2.0 ** -53 - 0.5
    big = R.start_block(600)
    assert abs(big.mean()) < 0.02 and abs(big.std() - np.sqrt(1 / 12)) < 0.01
    assert np.linalg.cond(big) < 2.0


SCENES = {"tiny_free": lambda: scene.config("tiny_free"), "cfg2": lambda: scene.config("cfg2"),
          "block_free": lambda: scene.make_scene(8, 60, 40, weights="block", n_control=0, scale_bar=True)}
ORDERS = {"tiny_free": 96, "cfg2": 600, "block_free": 171}


@pytest.mark.parametrize("name", list(SCENES))
def test_restated_subspace_iteration_converges_on_the_oracles_cofactor_matrix(oracle_mod, name):
    fp = SCENES[name]()
    _, Qp, _, _ = oracle_mod.Oracle(fp).step(fp.values, fp.sigma2apriori, 0.0, True)
    Q = packed_to_full(Qp, fp.n_unknowns)
    first, n = engine.point_column_range(fp)
    assert first == fp.rank_defect and n == ORDERS[name]
    S = Q[first:first + n, first:first + n]
    ref = np.linalg.eigvalsh(S)[::-1]
    for k in (1, 3, 4):
        th, V, tr, res, it, ok = R.subspace_iteration(S, k, 0.0, 200)
        err = np.abs(th - ref[:k]).max() / ref[0]
        rr = max(np.linalg.norm(S @ V[a] - th[a] * V[a]) for a in range(k)) / ref[0]
        print(f"{name} order {n} k {k}: {it} products, eigenvalues {err:.2e} of lambda_1, residuals {rr:.2e} of lambda_1, "
              f"first share {th[0] / tr:.4f}")
        assert ok and it <= 200
        assert err <= 1e-12 and rr <= 2e-10
        assert abs(tr - np.trace(S)) <= 1e-13 * tr
        for a in range(k):
            assert abs(np.linalg.norm(V[a]) - 1.0) <= 1e-14 and V[a][int(np.argmax(np.abs(V[a])))] > 0.0
    th, V, tr, res, it, ok = R.subspace_iteration(S, 3, 0.0, 1)
    assert not ok and it == 1 and np.isfinite(th).all() and np.isfinite(V).all()
