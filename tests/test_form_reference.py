"""CPU: the numpy restatement of include/jaicov_forms.h (tests/form_reference.py) against its second route (all parameters free, explicit
constraints, one bordered system), against closed solutions where the model has one, and against the properties the model promises."""
import numpy as np
import pytest

import form_reference as R

KINDS = [R.PLANE, R.SPHERE, R.LINE, R.CIRCLE]
NAMES = {R.PLANE: "plane", R.SPHERE: "sphere", R.LINE: "line", R.CIRCLE: "circle"}
S2 = 1.3


def noisy_case(kind, k, seed, rho=0.0, scale=1e-10, sigmas=1.0):
    rng = np.random.default_rng(seed)
    X = R.points_on(kind, k, rng, size=0.4, centre=(3.0, -2.0, 1.5))
    Q = R.correlated_cofactors(k, rng, scale=scale, rho=rho)
    X = X + sigmas * (np.linalg.cholesky(Q) @ rng.normal(size=3 * k)).reshape(k, 3)
    return X, Q


@pytest.mark.parametrize("k", [5, 9, 21])
@pytest.mark.parametrize("kind", KINDS)
def test_both_routes_agree(kind, k):
    X, Q = noisy_case(kind, k, 100 * kind + k, rho=0.5)
    a = R.fit_form(kind, X, Q, S2)
    par, Qpp, omega, v = R.fit_form_bordered(kind, X, Q)
    npar = R.REPORTED[kind]
    assert a["status"] == 0 and a["out"][19] <= 6
    scale = np.abs(par).max()
    assert np.abs(a["out"][:npar] - par).max() <= 1e-10 * scale, (a["out"][:npar], par)
    q7 = np.zeros((7, 7)); q7[np.triu_indices(7)] = a["qpp"]; q7 = q7 + np.triu(q7, 1).T
    assert np.abs(q7[:npar, :npar] - Qpp).max() <= 1e-6 * np.abs(Qpp).max()
    assert abs(a["out"][14] - omega) <= 1e-7 * omega
    assert np.abs(a["member"][:, 0:3] - v).max() <= 1e-7 * np.abs(v).max()
    f = R.CONDITIONS[kind] * k - R.FREE[kind]
    assert a["out"][15] == f and abs(a["out"][16] - omega / (f * S2)) <= 1e-7 * a["out"][16]
    assert 0.1 * f < a["out"][14] < 4.0 * f + 10                  # Omega ~ f: the noise was drawn from Q


@pytest.mark.parametrize("kind", KINDS)
def test_points_on_the_form_need_no_corrections(kind):
    rng = np.random.default_rng(7 + kind)
    X = R.points_on(kind, 12, rng, size=0.4, centre=(1.0, 2.0, 3.0))
    Q = R.correlated_cofactors(12, rng)
    a = R.fit_form(kind, X, Q, S2)
    assert a["status"] == 0
    assert a["out"][14] <= 1e-18 * 12 and np.abs(a["member"][:, 0:3]).max() <= 1e-14 and a["out"][17] <= 1e-14


@pytest.mark.parametrize("kind", [R.PLANE, R.LINE])
def test_unit_cofactors_give_the_eigenvector_solution(kind):
    rng = np.random.default_rng(21 + kind)
    k = 15
    X = R.points_on(kind, k, rng, size=0.4, centre=(1.0, 2.0, 3.0)) + 1e-3 * rng.normal(size=(k, 3))
    a = R.fit_form(kind, X, np.eye(3 * k), S2)
    x = X - X.mean(0)
    lam, E = np.linalg.eigh(x.T @ x)
    e = E[:, 0] if kind == R.PLANE else E[:, 2]
    e = e * R.sign_of(e)
    got = a["out"][0:3] if kind == R.PLANE else a["out"][3:6]
    assert np.abs(got - e).max() <= 1e-10
    d2 = (x @ e) ** 2 if kind == R.PLANE else (x * x).sum(1) - (x @ e) ** 2
    assert abs(a["out"][14] - d2.sum()) <= 1e-10 * d2.sum()
    assert abs(a["out"][18] - np.sqrt(d2.sum() / k)) <= 1e-10 * a["out"][18]
    if kind == R.PLANE:
        assert abs(a["out"][3] - e @ X.mean(0)) <= 1e-12
    else:                                                                    # the point of the line nearest the centroid
        assert np.abs(a["out"][0:3] - X.mean(0)).max() <= 1e-12


@pytest.mark.parametrize("kind", KINDS)
def test_invariants_of_the_solution(kind):
    k = 11
    X, Q = noisy_case(kind, k, 300 + kind, rho=0.4)
    a = R.fit_form(kind, X, Q, S2)
    out, v = a["out"], a["member"][:, 0:3]
    G = X.mean(0)
    ext = np.linalg.norm(X - G, axis=1).max()
    npar = R.REPORTED[kind]
    if kind == R.PLANE:
        n, c, r = out[0:3], np.zeros(3), out[3]
    elif kind == R.SPHERE:
        n, c, r = np.zeros(3), out[0:3], out[3]
    elif kind == R.LINE:
        n, c, r = out[3:6], out[0:3], 0.0
    else:
        n, c, r = out[3:6], out[0:3], out[6]
    d = R.distances(kind, X + v, n, c, r)                                    # X + v meets the conditions
    assert np.abs(d).max() <= 1e-12 * ext
    q7 = np.zeros((7, 7)); q7[np.triu_indices(7)] = a["qpp"]; q7 = q7 + np.triu(q7, 1).T
    if kind != R.SPHERE:
        assert abs(np.linalg.norm(n) - 1.0) <= 4e-16
        assert n[np.argmax(np.abs(n))] > 0.0
        full = np.zeros(7)
        full[{R.PLANE: 0, R.LINE: 3, R.CIRCLE: 3}[kind]:][:3] = n
        assert np.abs(q7 @ full).max() <= 1e-11 * np.abs(q7).max()         # no variance along the redundant direction
    assert abs(out[14] - v.ravel() @ np.linalg.solve(Q, v.ravel())) <= 1e-7 * out[14]     # Omega = v' inv(Q_ll) v
    assert np.all(out[7:7 + npar] >= 0.0) and np.isnan(out[7 + npar:14]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_a_member_off_the_form_has_the_largest_test_and_its_offset_is_recovered(kind):
    k = 12
    rng = np.random.default_rng(500 + kind)
    X0 = R.points_on(kind, k, rng, size=0.4, centre=(3.0, -2.0, 1.5))
    Q = R.correlated_cofactors(k, rng, rho=0.3)
    X = X0 + (np.linalg.cholesky(Q) @ rng.normal(size=3 * k)).reshape(k, 3)
    clean = R.fit_form(kind, X, Q, 1.0)
    j = 4
    # the direction off the form at member j, and its sigma from the member's own block
    out = clean["out"]
    if kind == R.PLANE:
        u = out[0:3]
    elif kind == R.SPHERE:
        u = (X[j] - out[0:3]) / np.linalg.norm(X[j] - out[0:3])
    elif kind == R.LINE:
        u = R.basis(out[3:6])[0]
    else:
        u = out[3:6]
    sig = np.sqrt(u @ Q[3 * j:3 * j + 3, 3 * j:3 * j + 3] @ u)
    X2 = X.copy(); X2[j] += 10.0 * sig * u
    a = R.fit_form(kind, X2, Q, 1.0)
    T = a["member"][:, 6]
    assert int(np.argmax(T)) == j and T[j] > clean["member"][:, 6].max()
    nab = a["member"][j, 4]                               # the first condition is the one along u for every kind
    base = clean["member"][j, 4]
    cc = R.CONDITIONS[kind]
    # its sigma: sqrt(1 / Q_lambda_lambda,jj) >= sig; the recovered offset is the given one plus the member's own noise share
    assert abs((nab - base) - 10.0 * sig) <= 0.05 * 10.0 * sig, (nab, base, 10.0 * sig)
    assert cc == 1 or np.isfinite(a["member"][j, 5])


def test_the_correlations_between_the_points_matter():
    """the case the GPU test reuses: sigma of the plane's d from the whole block against the one from the block diagonal"""
    X, Q = noisy_case(R.PLANE, 10, 77, rho=0.9)
    full = R.fit_form(R.PLANE, X, Q, S2)
    diag = R.fit_form(R.PLANE, X, R.block_diagonal(Q), S2)
    assert full["status"] == 0 and diag["status"] == 0
    assert abs(full["out"][10] - diag["out"][10]) > 0.10 * full["out"][10], (full["out"][10], diag["out"][10])
    assert abs(full["out"][16] - diag["out"][16]) > 0.10 * full["out"][16]


def test_status_paths():
    rng = np.random.default_rng(3)
    Q = R.correlated_cofactors(70, rng)
    X = R.points_on(R.PLANE, 70, rng)
    assert R.fit_form(R.PLANE, X[:2], Q[:6, :6], S2)["status"] == R.TOO_SMALL
    assert R.fit_form(R.SPHERE, X[:3], Q[:9, :9], S2)["status"] == R.TOO_SMALL
    assert R.fit_form(R.PLANE, X[:65], Q[:195, :195], S2)["status"] == R.TOO_LARGE
    assert R.fit_form(R.LINE, X[:33], Q[:99, :99], S2)["status"] == R.TOO_LARGE
    assert R.fit_form(R.PLANE, X[:64], Q[:192, :192], S2)["status"] == 0
    line = R.points_on(R.LINE, 3, rng)
    assert R.fit_form(R.PLANE, line, Q[:9, :9], S2)["status"] == R.DEGENERATE
    assert R.fit_form(R.SPHERE, X[:4], Q[:12, :12], S2)["status"] == R.DEGENERATE           # four coplanar points
    assert R.fit_form(R.PLANE, X[:5], np.zeros((15, 15)), S2)["status"] == R.SINGULAR       # all members fixed
    noisy = X[:8] + 0.05 * rng.normal(size=(8, 3))
    r1 = R.fit_form(R.SPHERE, R.points_on(R.SPHERE, 8, rng) + 0.05 * rng.normal(size=(8, 3)), Q[:24, :24], S2, max_iterations=1)
    assert r1["status"] == R.NOT_CONVERGED and r1["out"][19] == 1 and np.isfinite(r1["out"][:4]).all()
    assert R.fit_form(R.PLANE, noisy, Q[:24, :24], S2, partial=True)["status"] == R.PARTIAL
    least = R.fit_form(R.CIRCLE, R.points_on(R.CIRCLE, 3, rng), Q[:9, :9], S2)              # f = 0: no test
    assert least["status"] == 0 and least["out"][15] == 0 and np.isnan(least["out"][16])
    assert (least["member_status"] == R.MEMBER_UNTESTED).all() and np.isnan(least["member"][:, 4:7]).all()
