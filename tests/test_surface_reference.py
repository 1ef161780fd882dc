"""CPU: the numpy restatement of include/jaicov_surfaces.h (tests/surface_reference.py) is sound before the device is held to it: its
two routes agree, a given exact start converges at once, the kinds 0 .. 3 are form_reference.fit_form bit for bit, and the start
search finds planted cylinders and cones."""
import numpy as np
import pytest

import form_reference as F
import surface_reference as R

S2 = 1.3


def planted(kind, k, seed, noise=1e-4, size=0.4, centre=(3.0, -2.0, 7.0)):
    rng = np.random.default_rng(seed)
    pts, truth = R.surface_points(kind, k, rng, size=size, centre=centre)
    ext = np.linalg.norm(pts - pts.mean(0), axis=1).max()
    Q = R.correlated_cofactors(k, rng, scale=(noise * ext) ** 2, rho=0.3)
    X = pts + (np.linalg.cholesky(Q) @ rng.normal(size=3 * k)).reshape(k, 3)
    return X, Q, truth, ext


@pytest.mark.parametrize("kind", [R.CYLINDER, R.CONE])
@pytest.mark.parametrize("k", [9, 24])
def test_the_two_routes_agree(kind, k):
    X, Q, truth, ext = planted(kind, k, 100 + 7 * k + kind)
    a = R.fit_surface(kind, X, Q, S2, max_iterations=30)
    assert a["status"] == 0 and R.same_surface(kind, a["out"], truth, ext)
    par, Qpp, omega, v = R.fit_surface_bordered(kind, X, Q, truth)
    q7 = np.zeros((7, 7)); q7[np.triu_indices(7)] = a["qpp"]; q7 = q7 + np.triu(q7, 1).T
    dpar = np.abs(a["out"][:7] - par).max() / max(np.abs(par).max(), 1.0)
    dq = np.abs(q7 - Qpp).max() / np.abs(Qpp).max()
    dv = np.abs(a["member"][:, 0:3] - v).max() / np.abs(v).max()
    print(f"kind {kind} k {k}: parameters {dpar:.2e}, Q_pp {dq:.2e}, Omega {abs(a['out'][14] - omega) / omega:.2e}, v {dv:.2e}")
    assert dpar <= 1e-10 and dq <= 1e-6 and abs(a["out"][14] - omega) <= 1e-6 * omega and dv <= 1e-6
    # the conditions hold at X + v, t is a unit vector and Q_pp knows it
    G = X.mean(0)
    n, c, r = R.working_form(kind, a["out"][:7], G)
    assert np.abs(R.distances(kind, X - G + a["member"][:, 0:3], n, c, r)).max() <= 1e-12 * ext
    assert abs(np.linalg.norm(a["out"][3:6]) - 1.0) <= 1e-15 and np.abs(q7[:, 3:6] @ a["out"][3:6]).max() <= 1e-11 * np.abs(q7).max()
    assert (a["member"][:, 3] > 0).any() and (a["member"][:, 3] < 0).any()


@pytest.mark.parametrize("kind", [R.CYLINDER, R.CONE])
def test_a_given_exact_start_converges_in_two_steps(kind):
    X, truth = R.surface_points(kind, 16, np.random.default_rng(40 + kind), size=0.4, centre=(3.0, -2.0, 7.0))
    ext = np.linalg.norm(X - X.mean(0), axis=1).max()
    a = R.fit_surface(kind, X, 1e-10 * np.eye(48), S2, start=truth, tol=1e-9)
    assert a["status"] == 0 and a["out"][19] <= 2 and R.same_surface(kind, a["out"], truth, ext, tol=1e-9)
    own = R.fit_surface(kind, X, 1e-10 * np.eye(48), S2, tol=1e-9)
    assert own["status"] == 0 and R.same_surface(kind, own["out"], truth, ext, tol=1e-9)


def test_a_cone_given_the_other_way_round_comes_back_turned():
    X, Q, truth, ext = planted(R.CONE, 14, 77)
    a = R.fit_surface(R.CONE, X, Q, S2, start=truth)
    b = R.fit_surface(R.CONE, X, Q, S2, start=np.r_[truth[0:3], -truth[3:6], np.pi - truth[6]])
    assert a["status"] == b["status"] == 0 and b["out"][6] < 0.5 * np.pi
    assert np.abs(a["out"][:14] - b["out"][:14]).max() <= 1e-9 and np.abs(a["member"][:, 3:5] - b["member"][:, 3:5]).max() <= 1e-9 * np.abs(a["member"][:, 3:5]).max()


@pytest.mark.parametrize("kind", [F.PLANE, F.SPHERE, F.LINE, F.CIRCLE])
def test_the_four_forms_are_form_reference_bit_for_bit_and_take_a_start(kind):
    rng = np.random.default_rng(kind)
    k = 9
    X = F.points_on(kind, k, rng, size=0.5, centre=(1.0, 2.0, 3.0)) + 1e-5 * rng.normal(size=(k, 3))
    Q = F.correlated_cofactors(k, rng, scale=1e-10, rho=0.2)
    a, b = F.fit_form(kind, X, Q, S2), R.fit_surface(kind, X, Q, S2)
    assert all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes() for key in a)
    c = R.fit_surface(kind, X, Q, S2, start=a["out"][:7])
    npar = R.REPORTED[kind]
    assert c["status"] == 0 and c["out"][19] <= a["out"][19] and np.abs(c["out"][:npar] - a["out"][:npar]).max() <= 1e-11
    assert np.abs(c["out"][7:7 + npar] - a["out"][7:7 + npar]).max() <= 1e-9 * np.abs(a["out"][7:7 + npar]).max()


def test_statuses_of_the_start():
    X, Q, truth, ext = planted(R.CYLINDER, 12, 5)
    assert R.fit_surface(R.CYLINDER, X[:4], Q[:12, :12], S2)["status"] == R.TOO_SMALL
    assert R.fit_surface(R.CONE, X[:5], Q[:15, :15], S2)["status"] == R.TOO_SMALL
    assert R.fit_surface(R.CYLINDER, X, Q, S2, start=np.r_[truth[:6], -1.0])["status"] == R.DEGENERATE
    assert R.fit_surface(R.CYLINDER, X, Q, S2, start=np.r_[truth[:3], 0.0, 0.0, 0.0, 1.0])["status"] == R.DEGENERATE
    assert R.fit_surface(R.CONE, X, Q, S2, start=np.r_[truth[:6], 4.0])["status"] == R.DEGENERATE
    line = np.outer(np.linspace(-1.0, 1.0, 8), [1.0, 2.0, -1.0]) + [5.0, 5.0, 5.0]
    assert R.fit_surface(R.CYLINDER, line, 1e-10 * np.eye(24), S2)["status"] & (R.DEGENERATE | R.SINGULAR | R.NOT_FINITE)
    bad = R.fit_surface(R.CYLINDER, X, Q, S2, start=np.r_[X[3], 0.0, 0.0, 1.0, 0.1])      # an axis along Z through member 3: rho = 0
    assert bad["status"] == R.NOT_FINITE and bad["out"][19] == 1
    assert len(R.candidates()) == R.N_CANDIDATES and tuple(R.candidates()[0]) == (0.0, 0.0, 5.0)


# the shares the search must reach: every planted cylinder, and 0.85 of the cones (the prototype of the search found 55 of 60 at its worst)
SHARE = {R.CYLINDER: 1.0, R.CONE: 0.85}


@pytest.mark.parametrize("kind", [R.CYLINDER, R.CONE])
def test_the_search_finds_planted_surfaces(kind):
    """200 seeded random surfaces, k in {12, 24, 64}, arcs of 120 degrees and more, noise 1e-4 of the extent: the start of the search
    alone, with unit weights behind it, must lead to the planted surface"""
    rng = np.random.default_rng(1000 + kind)
    found = 0
    lost = []
    for case in range(200):
        k = (12, 24, 64)[case % 3]
        pts, truth = R.surface_points(kind, k, rng, size=rng.uniform(0.2, 2.0), centre=rng.normal(size=3) * 5.0)
        ext = np.linalg.norm(pts - pts.mean(0), axis=1).max()
        X = pts + 1e-4 * ext * rng.normal(size=(k, 3))
        a = R.fit_surface(kind, X, (1e-4 * ext) ** 2 * np.eye(3 * k), S2, max_iterations=30)
        ok = a["status"] == 0 and R.same_surface(kind, a["out"], truth, ext)
        found += ok
        if not ok:
            lost.append((case, k, a["status"]))
    print(f"kind {kind}: {found} of 200 planted surfaces found by the search; lost {lost}")
    assert found / 200.0 >= SHARE[kind]
