"""GPU: the precision figures of include/jaicov_precision.h (csrc/precision.hip) against numpy on the cofactor matrix that the same
engine exports (get_cofactor_sub): both sides round the same fp64 formulas on the same bits, so the bound is 1e-12 (relative for
sigmas and lengths, of the trace for eigenvalues and eigenvector residuals), four orders over the unit round-off.

Scenes: tiny_free (96 point columns: one partial tile, d = 6), the block scene (171: two tiles, d = 6), cfg2 (600: five tiles, the
last of 88 columns, d = 0).  Every test prints the worst figure it saw before it asserts."""
import gc
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import helpers
import precision_reference as R
from bundle_adjustment_amd import engine, scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "example")
MODES = {"FULL": engine.INVERT_FULL, "FULL_EXPANDED": engine.INVERT_FULL_EXPANDED, "REDUCED": engine.INVERT_REDUCED}
SCENES = {"tiny_free": lambda: scene.config("tiny_free"), "cfg2": lambda: scene.config("cfg2"),
          "block_free": lambda: scene.make_scene(8, 60, 40, weights="block", n_control=0, scale_bar=True)}
ORDERS = {"tiny_free": (6, 96), "cfg2": (0, 600), "block_free": (6, 171)}
_FP = {}
S2, K3, K2 = 0.83, 2.5, 1.7
TOL = 1e-12


def scene_of(name):
    if name not in _FP:
        _FP[name] = SCENES[name]()
    return _FP[name]


def inverting_pass(fp, mode):
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(mode)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(mode)
    return eng


def exported(eng):
    """The whole cofactor matrix as the gather hands it out (full, symmetric)."""
    return eng.get_cofactor_sub(np.arange(eng.cofactor_order(), dtype=np.int32))


def same_bits(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b) if x is not None)


def check_blocks(got, Q, cols, ang_cols=None):
    """PointPrecision `got` against numpy on the blocks Q[cols[i], cols[i]] (cols: (n, 3), -1 = fixed).  Returns the worst figures."""
    worst = dict(sigma=0.0, eig=0.0, axes=0.0, orth=0.0, ell=0.0)
    n = cols.shape[0]
    assert got.sigma.shape == (n, 3) and got.axes.shape == (n, 3, 3) and got.status.shape == (n,)
    for i in range(n):
        C3 = R.gather(Q, cols[i])
        tr = np.trace(C3)
        ref, st = R.point_figures(C3, S2, K3, K2, fixed=tuple(cols[i] < 0))
        assert got.status[i] == st, (i, got.status[i], st)
        if tr == 0.0:
            assert not got.sigma[i].any() and not got.semi_axes[i].any() and np.array_equal(got.axes[i], np.eye(3))
            continue
        sig = np.sqrt(S2 * np.diag(C3))
        free = sig > 0
        worst["sigma"] = max(worst["sigma"], (np.abs(got.sigma[i] - sig)[free] / sig[free]).max(), abs(got.helmert[i] - np.sqrt(S2 * tr)) / np.sqrt(S2 * tr))
        assert not got.sigma[i][~free].any()
        lam = np.linalg.eigvalsh(C3)[::-1]
        worst["eig"] = max(worst["eig"], np.abs(got.eigenvalues[i] - lam).max() / tr,
                           np.abs(got.semi_axes[i] ** 2 - K3 * K3 * S2 * np.maximum(lam, 0.0)).max() / (K3 * K3 * S2 * tr))
        assert np.all(np.diff(got.semi_axes[i]) <= 0.0)
        V = got.axes[i]                                   # row j: the unit vector of semi-axis j
        for j in range(3):
            worst["axes"] = max(worst["axes"], np.linalg.norm(C3 @ V[j] - got.eigenvalues[i][j] * V[j]) / tr)
            assert V[j][int(np.argmax(np.abs(V[j])))] > 0.0, (i, j, V[j])
        worst["orth"] = max(worst["orth"], np.abs(V @ V.T - np.eye(3)).max())
        C2 = C3[:2, :2]
        l2 = np.linalg.eigvalsh(C2)[::-1]
        t2 = max(np.trace(C2), 1e-300)
        dvec = np.array([np.cos(got.direction[i]), np.sin(got.direction[i])])
        assert 0.0 <= got.direction[i] < np.pi
        worst["ell"] = max(worst["ell"], np.abs(got.ellipse[i] ** 2 - K2 * K2 * S2 * np.maximum(l2, 0.0)).max() / (K2 * K2 * S2 * t2),
                           np.linalg.norm(C2 @ dvec - l2[0] * dvec) / t2)
        # the restatement, figure by figure (its vectors may differ where eigenvalues meet: not compared)
        np.testing.assert_allclose(np.r_[got.sigma[i], got.helmert[i]], ref[0:4], rtol=TOL)
    if ang_cols is not None:
        for i in range(n):
            sa = np.sqrt(S2 * np.diag(R.gather(Q, ang_cols[i])))
            free = sa > 0
            worst["sigma"] = max(worst["sigma"], (np.abs(got.sigma_angles[i] - sa)[free] / sa[free]).max(initial=0.0))
            assert not got.sigma_angles[i][~free].any()
    return worst


def assert_worst(label, worst):
    print(label + ": " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= TOL, (label, k, v)


def check_lengths(got, Q, cols, X, pairs):
    worst = 0.0
    for i, (a, b) in enumerate(pairs):
        c6 = np.r_[cols[a], cols[b]]
        Q6 = R.gather(Q, c6)
        D = X[b] - X[a]
        L = np.linalg.norm(D)
        g = np.r_[-D, D] / L
        sig = np.sqrt(S2 * (g @ Q6 @ g))
        sd = np.sqrt(S2 * np.array([Q6[k, k] + Q6[3 + k, 3 + k] - 2.0 * Q6[k, 3 + k] for k in range(3)]))
        worst = max(worst, abs(got.length[i] - L) / L, abs(got.sigma[i] - sig) / sig, (np.abs(got.sigma_diff[i] - sd) / np.maximum(sd, 1e-300)).max())
        ref, st = R.length_figures(X[a], X[b], Q6, S2, fixed=bool((c6 < 0).any()))
        assert got.status[i] == st
    return worst


def some_pairs(fp):
    P = fp.n_points
    pairs = [(i, i + 1) for i in range(P - 1)] + [(P - 1, 0), (0, P // 2), (P // 3, P - 2)]
    pairs += [(int(a), int(b)) for a, b in zip(np.atleast_1d(fp.sb_point_a), np.atleast_1d(fp.sb_point_b))]
    return np.array(pairs, np.int32)


# ---- 1. points, stations, lengths against numpy ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(SCENES))
def test_points_stations_and_lengths_match_numpy_on_the_exported_blocks(name, mode):
    fp = scene_of(name)
    eng = inverting_pass(fp, MODES[mode])
    Q = exported(eng)
    pcol = np.asarray(fp.point_col).reshape(-1, 3)
    pts = eng.precision_points(S2, K3, K2)
    assert pts.sigma_angles is None and not pts.status.any()
    assert_worst(f"{name} {mode} points", check_blocks(pts, Q, pcol))
    sub = np.array([fp.n_points - 1, 0, 5, 5], np.int32)                     # a list, in the caller's order, with a repeat
    assert same_bits([x[sub] if x is not None else None for x in pts], eng.precision_points(S2, K3, K2, sub))
    X = eng.get_parameters()[:3 * fp.n_points].reshape(-1, 3)
    pairs = some_pairs(fp)
    ln = eng.precision_lengths(S2, pairs)
    w = check_lengths(ln, Q, pcol, X, pairs)
    print(f"{name} {mode} lengths: worst relative {w:.2e} over {len(pairs)} pairs")
    assert w <= TOL and not ln.status.any()
    if name == "block_free" and mode == "REDUCED":         # jointly dispersed images: the exterior orientations are pre-eliminated
        assert eng.cofactor_order() < fp.n_unknowns
    if eng.cofactor_order() < fp.n_unknowns:               # (an engine without the pre-elimination answers REDUCED with all of Qxx)
        with pytest.raises(engine.EngineError) as ei:
            eng.precision_stations(S2)
        assert ei.value.code == -2
    else:
        ecol = np.asarray(fp.eo_col).reshape(-1, 6)
        sta = eng.precision_stations(S2, K3, K2)
        assert_worst(f"{name} {mode} stations", check_blocks(sta, Q, ecol[:, :3], ecol[:, 3:]))
        sub = np.array([fp.n_images - 1, 1], np.int32)
        assert same_bits([x[sub] for x in sta], eng.precision_stations(S2, K3, K2, sub))
    np.testing.assert_array_equal(exported(eng), Q)
    eng.close()


# ---- 2. fixed coordinates ----------------------------------------------------------------------------------------------------------------
def test_fixed_coordinates_give_partial_and_zero_axes():
    fp = helpers.base_scene()
    ctrl = set(int(s) // 3 for s in fp.dg_slot)
    assert 7 not in ctrl and 3 not in ctrl
    pf = np.zeros((fp.n_points, 3), bool)
    pf[7, 1] = True                                        # Y of point 7
    pf[3, :] = True                                        # all of point 3
    ef = np.zeros((fp.n_images, 6), bool)
    ef[2, 0] = True; ef[2, 4] = True                       # X0 and phi of image 2
    fx = helpers.renumber(fp, point_fixed=pf, eo_fixed=ef)
    eng = inverting_pass(fx, engine.INVERT_FULL)
    Q = exported(eng)
    pcol, ecol = np.asarray(fx.point_col).reshape(-1, 3), np.asarray(fx.eo_col).reshape(-1, 6)
    pts = eng.precision_points(S2, K3, K2)
    assert_worst("fixed points", check_blocks(pts, Q, pcol))
    assert pts.status[7] == engine.PREC_PARTIAL and pts.status[3] == engine.PREC_PARTIAL and int((pts.status != 0).sum()) == 2
    assert pts.sigma[7, 1] == 0.0 and pts.semi_axes[7, 2] == 0.0 and np.array_equal(pts.axes[7, 2], [0.0, 1.0, 0.0])
    assert pts.semi_axes[7, 1] > 0.0 and abs(pts.axes[7, 0, 1]) == 0.0 and abs(pts.axes[7, 1, 1]) == 0.0
    assert not pts.semi_axes[3].any() and pts.helmert[3] == 0.0
    sta = eng.precision_stations(S2, K3, K2)
    assert_worst("fixed stations", check_blocks(sta, Q, ecol[:, :3], ecol[:, 3:]))
    assert sta.status[2] == engine.PREC_PARTIAL and sta.sigma[2, 0] == 0.0 and sta.sigma_angles[2, 1] == 0.0 and sta.sigma_angles[2, 0] > 0.0
    assert np.array_equal(sta.axes[2, 2], [1.0, 0.0, 0.0]) and sta.semi_axes[2, 2] == 0.0
    pairs = np.array([(7, 8), (3, 7), (3, 4), (0, 1)], np.int32)
    ln = eng.precision_lengths(S2, pairs)
    X = eng.get_parameters()[:3 * fx.n_points].reshape(-1, 3)
    w = check_lengths(ln, Q, pcol, X, pairs)
    print(f"fixed lengths: worst relative {w:.2e}")
    assert w <= TOL and list(ln.status) == [engine.PREC_PARTIAL] * 3 + [0]
    eng.close()


# ---- 3. the correlations between two points matter -----------------------------------------------------------------------------------
def test_length_sigma_needs_the_cross_covariances():
    fp = scene_of("block_free")
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    Q = exported(eng)
    pcol = np.asarray(fp.point_col).reshape(-1, 3)
    X = eng.get_parameters()[:3 * fp.n_points].reshape(-1, 3)
    pairs = some_pairs(fp)
    ln = eng.precision_lengths(S2, pairs)
    ratio = []
    for i, (a, b) in enumerate(pairs):
        Q6 = R.gather(Q, np.r_[pcol[a], pcol[b]])
        Q0 = Q6.copy(); Q0[:3, 3:] = 0.0; Q0[3:, :3] = 0.0
        full, _ = R.length_figures(X[a], X[b], Q6, S2)
        zero, _ = R.length_figures(X[a], X[b], Q0, S2)
        assert abs(ln.sigma[i] - full[1]) <= TOL * full[1]
        ratio.append(zero[1] / full[1])
    ratio = np.array(ratio)
    print(f"sigma_L without the cross block / with it: {ratio.min():.4f} .. {ratio.max():.4f} over {len(pairs)} pairs")
    assert np.abs(ratio - 1.0).max() > 0.01
    # a degenerate pair: two points at the same place
    v = eng.get_parameters()
    v[3:6] = v[0:3]
    eng.set_parameters(v)
    deg = eng.precision_lengths(S2, [(0, 1), (1, 2)])
    assert deg.status[0] == engine.PREC_DEGENERATE and deg.length[0] == 0.0 and np.isnan(deg.sigma[0]) and np.isfinite(deg.sigma_diff[0]).all()
    assert deg.status[1] == 0 and np.isfinite(deg.sigma[1])
    eng.close()


# ---- 4. principal components -----------------------------------------------------------------------------------------------------------
def check_components(pc, S, k, tol=1e-10):
    ref = np.linalg.eigvalsh(S)[::-1]
    n = S.shape[0]
    assert pc.values.shape == (k,) and pc.vectors.shape == (k, n) and pc.residuals.shape == (k,)
    err = np.abs(pc.values - ref[:k]).max() / ref[0]
    res = max(np.linalg.norm(S @ pc.vectors[a] - pc.values[a] * pc.vectors[a]) for a in range(k)) / pc.values[0]
    tr = abs(pc.trace - np.trace(S)) / np.trace(S)
    for a in range(k):
        assert abs(np.linalg.norm(pc.vectors[a]) - 1.0) <= 1e-14
        assert pc.vectors[a][int(np.argmax(np.abs(pc.vectors[a])))] > 0.0
    return err, res, tr


@pytest.mark.parametrize("mode", ["FULL_EXPANDED", "REDUCED"])
@pytest.mark.parametrize("name", list(SCENES))
def test_principal_components_of_the_point_block(name, mode):
    fp = scene_of(name)
    eng = inverting_pass(fp, MODES[mode])
    Q = exported(eng)
    first, n = eng.point_column_range()
    assert (first, n) == ORDERS[name] and first == fp.rank_defect
    S = Q[first:first + n, first:first + n]
    for k in (1, 4):
        pc = eng.principal_components(k)
        err, res, tr = check_components(pc, S, k)
        print(f"{name} {mode} order {n} k {k}: {pc.iterations} products, eigenvalues {err:.2e} of lambda_1, residuals {res:.2e} of theta_1 "
              f"(reported {pc.residuals.max() / pc.values[0]:.2e}), trace {tr:.2e}, first share {pc.values[0] / pc.trace:.4f}")
        assert pc.converged and pc.iterations <= 200
        assert err <= 1e-12 and res <= 2e-10 and tr <= 1e-13
        assert np.all(pc.residuals <= 1e-10 * pc.values[0])
    one = eng.principal_components(3, max_iterations=1)
    assert not one.converged and one.iterations == 1
    assert np.isfinite(one.values).all() and np.isfinite(one.vectors).all() and np.isfinite(one.residuals).all() and np.isfinite(one.trace)
    # a range that starts off the tile grid and ends before the last point column
    f2, n2 = first + 3, n - 5
    pc = eng.principal_components(3, first_col=f2, n_cols=n2)
    err, res, tr = check_components(pc, Q[f2:f2 + n2, f2:f2 + n2], 3)
    print(f"{name} {mode} columns {f2} .. {f2 + n2 - 1}: {pc.iterations} products, eigenvalues {err:.2e}, residuals {res:.2e}, trace {tr:.2e}")
    assert pc.converged and err <= 1e-12 and res <= 2e-10 and tr <= 1e-13
    # a looser tolerance is honoured as given
    loose = eng.principal_components(2, tol=1e-6)
    assert loose.converged and loose.iterations <= pc.iterations + 200 and np.all(loose.residuals <= 1e-6 * loose.values[0])
    assert max(np.linalg.norm(S @ loose.vectors[a] - loose.values[a] * loose.vectors[a]) for a in range(2)) <= 2e-6 * loose.values[0]
    np.testing.assert_array_equal(exported(eng), Q)
    eng.close()


# ---- 5. after a datum transformation the figures speak of the new datum ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_free", "block_free"])
def test_every_call_follows_a_datum_transformation(name):
    fp = scene_of(name)
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    Q0 = exported(eng)
    before = eng.precision_points(S2, K3, K2)
    mask = np.zeros(fp.n_points, np.uint8); mask[::2] = 1
    eng.datum_transform(mask)
    Q = exported(eng)
    assert np.abs(Q - Q0).max() > 1e-6 * np.abs(Q0).max()
    pcol, ecol = np.asarray(fp.point_col).reshape(-1, 3), np.asarray(fp.eo_col).reshape(-1, 6)
    pts = eng.precision_points(S2, K3, K2)
    assert np.abs(pts.helmert - before.helmert).max() > 1e-3 * before.helmert.max()
    assert_worst(f"{name} after the transformation, points", check_blocks(pts, Q, pcol))
    assert_worst(f"{name} after the transformation, stations", check_blocks(eng.precision_stations(S2, K3, K2), Q, ecol[:, :3], ecol[:, 3:]))
    X = eng.get_parameters()[:3 * fp.n_points].reshape(-1, 3)
    pairs = some_pairs(fp)
    w = check_lengths(eng.precision_lengths(S2, pairs), Q, pcol, X, pairs)
    first, n = eng.point_column_range()
    pc = eng.principal_components(3)
    err, res, tr = check_components(pc, Q[first:first + n, first:first + n], 3)
    print(f"{name} after the transformation: lengths {w:.2e}; components in {pc.iterations} products, eigenvalues {err:.2e}, residuals {res:.2e}")
    assert w <= TOL and pc.converged and err <= 1e-12 and res <= 2e-10 and tr <= 1e-13
    eng.close()


# ---- 6. determinism -----------------------------------------------------------------------------------------------------------------------
def test_two_runs_of_every_call_give_the_same_bits():
    fp = scene_of("block_free")
    pairs = some_pairs(fp)
    runs = []
    for _ in range(2):
        eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
        for _ in range(2):
            runs.append((eng.precision_points(S2, K3, K2), eng.precision_stations(S2, K3, K2), eng.precision_lengths(S2, pairs),
                         eng.principal_components(4), eng.principal_components(2, first_col=9, n_cols=150)))
        eng.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert same_bits(a, b)


# ---- 7. refusals leave the cofactor matrix as it is -------------------------------------------------------------------------------------
def code_of(fn, *a, **kw):
    with pytest.raises(engine.EngineError) as ei:
        fn(*a, **kw)
    return ei.value.code


def test_refusals_give_the_stated_status_and_leave_the_matrix_bit_identical():
    fp = scene_of("block_free")
    P, I, d = fp.n_points, fp.n_images, fp.rank_defect
    # no cofactor matrix
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(engine.INVERT_NONE)
    assert code_of(eng.precision_points, S2) == -2 and code_of(eng.precision_stations, S2) == -2
    assert code_of(eng.precision_lengths, S2, [(0, 1)]) == -2 and code_of(eng.principal_components, 3) == -2
    assert code_of(eng.precision_points, S2, points=[P]) == -2            # the state is looked at before the arguments
    eng.close()
    # a shard: looked at before the state
    sh = engine.Engine(fp, device=0, image_range=(0, 3))
    assert code_of(sh.precision_points, S2) == -3 and code_of(sh.precision_stations, S2) == -3
    assert code_of(sh.precision_lengths, S2, [(0, 1)]) == -3 and code_of(sh.principal_components, 3) == -3
    sh.close()
    sh = engine.Engine(fp, device=0, apply_shared=False)
    assert code_of(sh.precision_points, S2) == -3
    sh.close()
    for mode in (engine.INVERT_FULL_EXPANDED, engine.INVERT_REDUCED):
        eng = inverting_pass(fp, mode)
        Q0 = eng.get_cofactor()
        order = eng.cofactor_order()
        first, n = eng.point_column_range()
        assert first == d == 6
        for k in (0, 5, -1):
            assert code_of(eng.principal_components, k) == -1
        assert code_of(eng.principal_components, 3, first_col=d - 1, n_cols=20) == -1          # enters the border
        assert code_of(eng.principal_components, 3, first_col=first, n_cols=order - first + 1) == -1   # leaves the order
        assert code_of(eng.principal_components, 3, first_col=order - 4, n_cols=8) == -1
        assert code_of(eng.principal_components, 3, first_col=first, n_cols=7) == -1
        assert code_of(eng.principal_components, 3, max_iterations=0) == -1
        assert code_of(eng.principal_components, 3, tol=-1.0) == -1
        eng.principal_components(3, first_col=first, n_cols=order - first)                     # the largest range there is
        for bad in ([P], [-1], [0, P + 3]):
            assert code_of(eng.precision_points, S2, points=bad) == -1
        assert code_of(eng.precision_points, -1.0) == -1 and code_of(eng.precision_points, S2, k3=float("nan")) == -1
        assert code_of(eng.precision_lengths, S2, [(0, P)]) == -1 and code_of(eng.precision_lengths, S2, [(-1, 0)]) == -1
        assert code_of(eng.precision_lengths, S2, [(0, 1), (4, 4)]) == -1                      # a pair (p, p)
        if order < fp.n_unknowns:
            assert code_of(eng.precision_stations, S2) == -2
        else:
            assert code_of(eng.precision_stations, S2, images=[I]) == -1
        np.testing.assert_array_equal(eng.get_cofactor(), Q0)
        assert eng.precision_points(S2, points=np.zeros(0, np.int32)).sigma.shape == (0, 3)
        assert eng.precision_lengths(S2, np.zeros((0, 2), np.int32)).length.shape == (0,)
        np.testing.assert_array_equal(eng.get_cofactor(), Q0)
        eng.close()


def test_a_matrix_that_is_not_finite_is_flagged():
    """sigma2 = inf reaches the NOT_FINITE branch without touching the matrix."""
    fp = scene_of("tiny_free")
    eng = inverting_pass(fp, engine.INVERT_FULL)
    pts = eng.precision_points(float("inf"), points=[0, 1])
    assert np.all(pts.status == engine.PREC_NOT_FINITE) and np.isnan(pts.sigma).all() and np.isnan(pts.axes).all()
    ln = eng.precision_lengths(float("inf"), [(0, 1)])
    assert ln.status[0] == engine.PREC_NOT_FINITE and np.isnan(ln.length[0])
    eng.close()


# ---- 8. the work buffers go with the engine -----------------------------------------------------------------------------------------------
def test_work_buffers_go_with_the_engine():
    from test_gpu_ownership import census
    fp = scene_of("tiny_free")

    def scenario():
        eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
        a = census()
        eng.precision_points(S2)
        eng.precision_stations(S2)
        eng.precision_lengths(S2, [(0, 1)])
        b = census()
        assert b[0] > a[0] and b[1] == a[1] + 2, (a, b)        # PrecisionState::tab and ::out, used again by every call
        eng.principal_components(3)
        c = census()
        assert c[0] > b[0] and c[1] == b[1] + 1, (b, c)        # PrecisionState::work
        eng.principal_components(4)
        eng.precision_points(S2)
        assert census() == c
        eng.close()

    scenario()
    gc.collect()
    c0 = census()
    scenario()
    assert census() == c0


# ---- 9. the C++ mirror and the example program --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example_base(tmp_path_factory):
    d = tmp_path_factory.mktemp("example")
    for f in ("ior", "eor", "obc", "scale"):
        shutil.copy(os.path.join(GOLDEN, f"example.{f}"), d)
    with gzip.open(os.path.join(GOLDEN, "example.phc.gz")) as src, open(d / "example.phc", "wb") as dst:
        dst.write(src.read())
    return str(d / "example")


def test_cpp_mirror_returns_the_bits_of_the_python_calls(example_base):
    """The mirror's BundleAdjustment on the bundled block (FULL); the ctypes calls go to the mirror's own engine."""
    import ctypes as C
    from bundle_adjustment_amd import host_api as H
    from test_host import example_adjustment
    keep, ba = example_adjustment(H, example_base)
    assert ba.estimateModel() == H.EstimationStateType.ERROR_FREE_ESTIMATION, ba.lastError()
    fp = H.flat_problem(ba).validate()
    L = engine.load_library()
    h = C.c_void_p(ba.nativeEngineHandle())
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    P = len(ba.getObjectCoordinates())
    tab, st = ba.pointPrecision(S2, K3, K2)
    out = np.zeros((P, 22)); s = np.zeros(P, np.int32)
    assert L.jaicov_prec_points(h, S2, K3, K2, None, P, out.ctypes.data_as(pd), s.ctypes.data_as(pi)) == 0
    assert tab.shape == (P, 22) and tab.tobytes() == out.tobytes() and st.tobytes() == s.tobytes() and (tab[:, 3] > 0).all()
    tab, st = ba.pointPrecision(S2, K3, K2, [3, 1])
    assert tab.tobytes() == out[[3, 1]].tobytes()
    tab, st = ba.stationPrecision(S2, K3, K2)
    I = tab.shape[0]
    out = np.zeros((I, 25)); s = np.zeros(I, np.int32)
    assert L.jaicov_prec_stations(h, S2, K3, K2, None, I, out.ctypes.data_as(pd), s.ctypes.data_as(pi)) == 0
    assert I == fp.n_images and tab.tobytes() == out.tobytes() and st.tobytes() == s.tobytes()
    pairs = np.array([(0, P - 1), (2, 7)], np.int32)
    tab, st = ba.lengthPrecision(S2, pairs.ravel().tolist())
    out = np.zeros((2, 5)); s = np.zeros(2, np.int32)
    assert L.jaicov_prec_lengths(h, S2, pairs.ctypes.data_as(pi), 2, out.ctypes.data_as(pd), s.ctypes.data_as(pi)) == 0
    assert tab.tobytes() == out.tobytes() and st.tobytes() == s.tobytes() and (tab[:, 1] > 0).all()
    first, n = engine.point_column_range(fp)
    vals, vecs, tr, res, it, ok = ba.principalComponents(first, n, 3)
    v = np.zeros(3); x = np.zeros((3, n)); t = np.zeros(1); r = np.zeros(3); k = C.c_int32(0)
    assert L.jaicov_prec_components(h, first, n, 3, 0.0, 200, v.ctypes.data_as(pd), x.ctypes.data_as(pd), t.ctypes.data_as(pd),
                                    r.ctypes.data_as(pd), C.byref(k)) == 0
    assert ok and it == k.value and vals.tobytes() == v.tobytes() and vecs.tobytes() == x.tobytes() and tr == t[0] and res.tobytes() == r.tobytes()
    with pytest.raises(RuntimeError):
        ba.principalComponents(first, n, 5)
    del keep


def test_native_example_precision_program(example_base):
    """host/example_precision on the bundled block: status 0, three points with their ellipsoids, the scale bar's length with a
    positive sigma, and the first component's share of the trace inside (0, 1)."""
    host = os.path.join(ROOT, "bundle-adjustment_amd", "host")
    subprocess.check_call(["make", "-C", host, "example_precision"], stdout=subprocess.DEVNULL)
    a = subprocess.run([os.path.join(host, "example_precision"), example_base], capture_output=True, text=True, timeout=600)
    print(a.stdout[-3000:])
    assert a.returncode == 0, (a.stdout[-2000:], a.stderr[-2000:])
    pts = re.findall(r"^point (\S+)\s+Helmert (\S+) mm", a.stdout, flags=re.M)
    assert len(pts) == 3 and [float(h) for _, h in pts] == sorted((float(h) for _, h in pts), reverse=True)
    axes = [float(x) for x in re.findall(r"semi-axis (\S+) mm", a.stdout)]
    assert len(axes) == 9 and all(x > 0 for x in axes)
    bars = re.findall(r"^scale bar .* length (\S+) mm, sigma (\S+) mm \(observed (\S+)\), status 0", a.stdout, flags=re.M)
    assert bars and all(float(s) > 0 and abs(float(length) - float(obs)) < 1.0 for length, s, obs in bars)
    share = [float(x) for x in re.findall(r"share of the trace (\S+)", a.stdout)]
    assert len(share) == 3 and 0.0 < share[2] <= share[1] <= share[0] < 1.0
    assert "converged after" in a.stdout and "NOT converged" not in a.stdout
