"""GPU: the surfaces of include/jaicov_surfaces.h (csrc/forms.hip, csrc/surfstart.h) against the numpy restatement
(tests/surface_reference.py) on the cofactor matrix and the coordinates that the same engine exports.

Scenes and inversion modes: those of test_gpu_forms.py.  Before the inverting pass the object-point start values are overwritten as
there: one group of points lies on a cylinder, one on a cone (fresh points on a surface within 0.7 of the group's extent of its
centroid, spread over an arc of 120 degrees and more, plus noise of 3 sigma; sigma from a first pass of the unchanged scene), seven
more exactly on a line.  The seeds (SEED) were chosen on the CPU so that the restatement, with unit weights and noise of 1e-5 of the
extent in the place of the engine's, finds the planted surface from every group and subset used here; on the device that is asserted
for the whole groups (planted_found), and no case is skipped.

Tolerances.  As in test_gpu_forms.py the device and the restatement round the same formulas in another order.  Measured on the MI355X
over all cases of this file, norm-wise relative per form (|difference|_max / |figure|_max), the worst of four runs:
    parameters 4.7e-14, sigma 3.7e-13, Q_pp 7.3e-13, Omega 2.9e-11, T 2.9e-11, v 1.4e-11, distances 3.9e-11, T_i 2.9e-11, nabla 2.2e-11
(rounded up; the largest come from the block scene, whose cofactors differ most in magnitude, and from one step off a noisy start).
TOL is 10 x these (none above 1e-8).  The invariants are asserted at fixed bounds that follow from the construction, as in
test_gpu_forms.py: the conditions at X + v to 1e-12 of the extent, | |t| - 1 | <= 1e-15, |Q_pp t| <= 1e-11 |Q_pp|.  Every test prints
its worst figures before it asserts."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import helpers
import surface_reference as R
from bundle_adjustment_amd import engine
from test_gpu_forms import MODES, S2, SCENES, code_of, exported, inverting_pass, rel, same_bits
from test_gpu_forms import cases_of as form_cases_of
from test_gpu_forms import planted as forms_planted

pytestmark = pytest.mark.gpu

# members of the planted groups: cylinder, cone, collinear
QUOTA = {"tiny_free": (11, 12, 7), "cfg2": (65, 65, 7), "block_free": (20, 20, 7)}
SEED = {"tiny_free": 4, "cfg2": 1, "block_free": 3}
TOL = dict(params=4.7e-13, sigma=3.7e-12, qpp=7.3e-12, omega=2.9e-10, T=2.9e-10, v=1.4e-10, dist=3.9e-10, T_i=2.9e-10, nabla=2.2e-10)
_PLANTED = {}


def plant(fp, quota, seed, sig):
    """(values with the planted groups, groups, truth): groups[g] = the point indices of group g, scattered over the point range;
    truth[g] = the parameters of the planted cylinder and cone in the reported order"""
    P = fp.n_points
    assert sum(quota) <= P
    groups = [[] for _ in quota]
    g = 0
    for p in range(P):
        for _ in range(len(quota)):
            if len(groups[g]) < quota[g]:
                groups[g].append(p)
                g = (g + 1) % len(quota)
                break
            g = (g + 1) % len(quota)
    rng = np.random.default_rng(seed)
    vals = np.array(fp.values, float)
    X = vals[:3 * P].reshape(P, 3)
    truth = []
    for kind, idx in zip((R.CYLINDER, R.CONE), groups):
        c0 = X[idx].mean(0)
        size = max(np.linalg.norm(X[idx] - c0, axis=1).max(), 1e-3) * 0.7
        pts, par = R.surface_points(kind, len(idx), rng, size=size, centre=c0)
        X[idx] = pts + 3.0 * sig * rng.normal(size=(len(idx), 3))
        truth.append(par)
    idx = groups[2]
    c0 = X[idx].mean(0)
    X[idx] = R.F.points_on(R.LINE, len(idx), rng, size=0.7 * np.linalg.norm(X[idx] - c0, axis=1).max(), centre=c0)
    return vals, [np.array(g, np.int32) for g in groups], truth


def planted(name):
    if name in _PLANTED:
        return _PLANTED[name]
    fp = SCENES[name]()
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)                  # a first pass of the unchanged scene for the size of sigma
    pcol = np.asarray(fp.point_col).reshape(-1, 3)
    dq = np.diag(exported(eng))
    eng.close()
    sig = np.sqrt(fp.sigma2apriori * np.median(dq[pcol[pcol >= 0]]))
    vals, groups, truth = plant(fp, QUOTA[name], SEED[name], sig)
    _PLANTED[name] = (dataclasses.replace(fp, values=vals), groups, truth)
    return _PLANTED[name]


def spread(grp, k):
    """k members of the group spread over it (the arc of a planted surface ascends with the member)"""
    return grp[np.round(np.linspace(0, len(grp) - 1, k)).astype(int)]


def cases_of(name, groups):
    """the forms of one call: k at the least (f = 0) and one more, the whole group in descending order (m = 64 on cfg2), k below the
    least, m = 65 where the scene has the points, and the collinear ones"""
    cy, co, col = groups
    forms = []
    for kind, grp in ((R.CYLINDER, cy), (R.CONE, co)):
        least = R.LEAST[kind]
        forms += [(kind, spread(grp[:64], least)), (kind, spread(grp[:64], least + 1)), (kind, grp[:64][::-1]), (kind, grp[:least - 1])]
        if name == "cfg2":
            forms.append((kind, grp))
    forms += [(R.CYLINDER, col), (R.CONE, col)]
    return forms


def restate(eng, fp, forms, Q=None, start=None, max_iterations=20):
    Q = exported(eng) if Q is None else Q
    X = eng.get_parameters()[:3 * fp.n_points].reshape(-1, 3)
    pcol = np.asarray(fp.point_col).reshape(-1, 3)
    out = []
    for g, (kind, pts) in enumerate(forms):
        cols = pcol[pts].ravel()
        out.append(R.fit_surface(kind, X[pts], R.gather_block(Q, cols), S2, start=None if start is None else start[g],
                                 max_iterations=max_iterations, partial=bool((cols < 0).any())))
    return out


def compare(fits, refs, forms, label):
    """every figure of every form against the restatement; returns the worst relative difference of every class"""
    worst = {k: 0.0 for k in TOL}
    for g, ((kind, pts), ref) in enumerate(zip(forms, refs)):
        b, e = fits.begin[g], fits.begin[g + 1]
        assert fits.status[g] == ref["status"], (label, g, kind, len(pts), fits.status[g], ref["status"])
        o = ref["out"]
        if ref["status"] & R.FATAL:
            assert np.isnan(fits.params[g]).all() and np.isnan(fits.sigma[g]).all() and np.isnan(fits.qpp[g]).all() and np.isnan(fits.omega[g])
            assert np.isnan(fits.v[b:e]).all() and np.isnan(fits.T_member[b:e]).all() and not fits.member_status[b:e].any()
            assert fits.iterations[g] == o[19]
            continue
        npar = R.REPORTED[kind]
        assert abs(fits.iterations[g] - o[19]) <= 1 and fits.dof[g] == o[15], (label, g, fits.iterations[g], o[19])
        assert np.isnan(fits.params[g, npar:]).all() and np.isnan(fits.sigma[g, npar:]).all()
        q7 = np.zeros((7, 7)); q7[np.triu_indices(7)] = ref["qpp"]; q7 = q7 + np.triu(q7, 1).T
        worst["params"] = max(worst["params"], rel(fits.params[g, :npar], o[:npar]))
        worst["sigma"] = max(worst["sigma"], rel(fits.sigma[g, :npar], o[7:7 + npar]))
        worst["qpp"] = max(worst["qpp"], rel(fits.qpp[g], q7))
        ext = max(np.abs(o[:npar]).max(), 1.0)
        if o[15] > 0:
            worst["omega"] = max(worst["omega"], rel(fits.omega[g], o[14]))
            worst["T"] = max(worst["T"], rel(fits.T[g], o[16]))
            worst["v"] = max(worst["v"], rel(fits.v[b:e], ref["member"][:, 0:3]))
            worst["dist"] = max(worst["dist"], rel(fits.distance[b:e], ref["member"][:, 3]), rel(fits.max_distance[g], o[17]), rel(fits.rms_distance[g], o[18]))
            assert np.array_equal(fits.member_status[b:e], ref["member_status"]), (label, g)
            worst["T_i"] = max(worst["T_i"], rel(fits.T_member[b:e], ref["member"][:, 6]))
            worst["nabla"] = max(worst["nabla"], rel(fits.nabla[b:e], ref["member"][:, 4:6]))
            assert R.CONDITIONS[kind] == 2 or np.isnan(fits.nabla[b:e, 1]).all()
        else:                                       # f = 0: the surface goes through its members, nothing is left to test
            assert np.isnan(fits.T[g]) and (fits.member_status[b:e] == engine.FORM_MEMBER_UNTESTED).all() and np.isnan(fits.T_member[b:e]).all()
            assert np.abs(fits.v[b:e]).max() <= 1e-9 * ext and fits.max_distance[g] <= 1e-9 * ext
    print(label + ": " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    return worst


def assert_worst(label, worst):
    for k, v in worst.items():
        assert v <= TOL[k], (label, k, v)


def invariants(eng, fp, fits, forms, label):
    X = eng.get_parameters()[:3 * fp.n_points].reshape(-1, 3)
    worst = dict(conditions=0.0, unit=0.0, redundant=0.0)
    for g, (kind, pts) in enumerate(forms):
        if fits.status[g] & (R.FATAL | R.NOT_CONVERGED) or kind < R.CYLINDER:
            continue
        b, e = fits.begin[g], fits.begin[g + 1]
        p = fits.params[g]
        x = X[pts]
        ext = np.linalg.norm(x - x.mean(0), axis=1).max()
        t = p[3:6]
        worst["conditions"] = max(worst["conditions"], np.abs(R.distances(kind, x + fits.v[b:e], t, p[0:3], p[6])).max() / ext)
        worst["unit"] = max(worst["unit"], abs(np.linalg.norm(t) - 1.0))
        if kind == R.CYLINDER:
            assert t[np.argmax(np.abs(t))] > 0.0 and p[6] > 0.0
        else:
            assert 0.0 < p[6] <= 0.5 * np.pi and ((x - p[0:3]) @ t).mean() > 0.0     # t points into the nappe of the members
        full = np.zeros(7); full[3:6] = t
        worst["redundant"] = max(worst["redundant"], np.abs(fits.qpp[g] @ full).max() / np.abs(fits.qpp[g]).max())
    print(label + " invariants: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["conditions"] <= 1e-12 and worst["unit"] <= 1e-15 and worst["redundant"] <= 1e-11, (label, worst)


def planted_found(fits, forms, groups, truth, X):
    """the whole groups come back as the planted surfaces"""
    for g, (kind, pts) in enumerate(forms):
        if kind >= R.CYLINDER and set(pts) == set(groups[kind - R.CYLINDER][:64]):
            ext = np.linalg.norm(X[pts] - X[pts].mean(0), axis=1).max()
            assert fits.status[g] == 0 and R.same_surface(kind, fits.params[g], truth[kind - R.CYLINDER], ext), (g, kind, fits.params[g])


# ---- 1. both surfaces, every size class, every inversion mode against the restatement --------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(SCENES))
def test_surfaces_match_the_restatement(name, mode):
    fp, groups, truth = planted(name)
    eng = inverting_pass(fp, MODES[mode])
    Q = exported(eng)
    forms = cases_of(name, groups)
    fits = eng.fit_surfaces(S2, forms)
    refs = restate(eng, fp, forms, Q)
    st = fits.status
    assert (st == [r["status"] for r in refs]).all(), (st, [r["status"] for r in refs])
    assert (st == engine.FORM_TOO_SMALL).sum() == 2 and (st == engine.FORM_DEGENERATE).sum() == 2 and (st == 0).sum() >= 6
    if name == "cfg2":
        assert (st == engine.FORM_TOO_LARGE).sum() == 2 and [len(p) for k, p in forms].count(64) == 2
    label = f"{name} {mode}"
    worst = compare(fits, refs, forms, label)
    planted_found(fits, forms, groups, truth, eng.get_parameters()[:3 * fp.n_points].reshape(-1, 3))
    invariants(eng, fp, fits, forms, label)
    assert_worst(label, worst)
    again = eng.fit_surfaces(S2, forms)                                      # two calls give the same bits
    assert same_bits(fits, again)
    one = eng.fit_surfaces(S2, [forms[2]])                                   # a form's figures do not depend on its neighbours
    assert one.params.tobytes() == fits.params[2:3].tobytes() and one.v.tobytes() == fits.v[fits.begin[2]:fits.begin[3]].tobytes()
    np.testing.assert_array_equal(exported(eng), Q)
    eng.close()


# ---- 2. the correlations between the points matter -----------------------------------------------------------------------------------------
def test_a_kernel_without_the_cross_blocks_cannot_pass():
    """on the planted block scene sigma and T from the block diagonals of Q_ll differ from the rigorous ones by orders of magnitude
    more than the tolerance: asserted on the restatement, the device is held to the rigorous figures"""
    fp, groups, truth = planted("block_free")
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    Q = exported(eng)
    forms = [(R.CYLINDER, groups[0]), (R.CONE, groups[1])]
    fits = eng.fit_surfaces(S2, forms)
    X = eng.get_parameters()[:3 * fp.n_points].reshape(-1, 3)
    pcol = np.asarray(fp.point_col).reshape(-1, 3)
    for g, (kind, pts) in enumerate(forms):
        Qll = R.gather_block(Q, pcol[pts].ravel())
        full = R.fit_surface(kind, X[pts], Qll, S2)
        diag = R.fit_surface(kind, X[pts], R.block_diagonal(Qll), S2)
        gap = rel(diag["out"][7:14], full["out"][7:14])
        print(f"kind {kind}: sigma from the block diagonal differs by {gap:.2e}, T by {rel(diag['out'][16], full['out'][16]):.2e}; "
              f"the device by {rel(fits.sigma[g], full['out'][7:14]):.2e}")
        assert gap > 1e-3 and rel(fits.sigma[g], full["out"][7:14]) <= TOL["sigma"]
        assert rel(diag["out"][16], full["out"][16]) > 1e-3 and rel(fits.T[g], full["out"][16]) <= TOL["T"]
    eng.close()


# ---- 3. start values from the caller ---------------------------------------------------------------------------------------------------------
def noisy(truth, kind, ext, rng, amount=0.02):
    row = np.array(truth, float)
    row[0:3] += amount * ext * rng.normal(size=3)
    row[3:6] += amount * rng.normal(size=3)
    row[6] *= 1.0 + amount * rng.normal()
    return row


def test_one_step_from_a_given_noisy_start_is_the_restatements_step():
    """the check of the rows that does not lean on the search: max_iterations = 1 from a start two per cent off"""
    fp, groups, truth = planted("tiny_free")
    eng = inverting_pass(fp, engine.INVERT_FULL)
    X = eng.get_parameters()[:3 * fp.n_points].reshape(-1, 3)
    rng = np.random.default_rng(3)
    forms = [(R.CYLINDER, groups[0]), (R.CONE, groups[1])]
    start = [noisy(truth[g], kind, np.linalg.norm(X[pts] - X[pts].mean(0), axis=1).max(), rng) for g, (kind, pts) in enumerate(forms)]
    one = eng.fit_surfaces(S2, forms, start=start, max_iterations=1)
    assert (one.status == engine.FORM_NOT_CONVERGED).all() and (one.iterations == 1).all() and np.isfinite(one.params).all()
    refs = restate(eng, fp, forms, start=start, max_iterations=1)
    assert_worst("one step", compare(one, refs, forms, "one step"))
    more = eng.fit_surfaces(S2, forms, start=start)                          # NOT_CONVERGED returned the last values: more steps go on from there
    assert not more.status.any() and (more.iterations > 1).all()
    assert_worst("noisy start", compare(more, restate(eng, fp, forms, start=start), forms, "noisy start"))
    eng.close()


def test_a_given_start_and_the_search_end_at_the_same_figures():
    """both runs stop with |Delta| <= 1e-12 of the extent at the same minimum, whose neighbourhood the steps contract quadratically:
    the parameters agree to 1e-10 of the extent, sigma and Omega to 1e-8 relative.  A cone given as (-t, pi - alpha) comes back turned
    round, with positive distances outside.  The four forms take a start as well."""
    fp, groups, truth = planted("block_free")
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    X = eng.get_parameters()[:3 * fp.n_points].reshape(-1, 3)
    forms = [(R.CYLINDER, groups[0]), (R.CONE, groups[1]), (R.CONE, groups[1])]
    turned = np.r_[truth[1][0:3], -truth[1][3:6], np.pi - truth[1][6]]
    own = eng.fit_surfaces(S2, forms)
    given = eng.fit_surfaces(S2, forms, start=[truth[0], None, turned])
    assert not own.status.any() and not given.status.any()
    for g, (kind, pts) in enumerate(forms):
        ext = np.linalg.norm(X[pts] - X[pts].mean(0), axis=1).max()
        d = np.abs(given.params[g] - own.params[g]) / np.r_[ext, ext, ext, 1.0, 1.0, 1.0, ext if kind == R.CYLINDER else 1.0]
        print(f"form {g}: given against own start: parameters {d.max():.2e}, sigma {rel(given.sigma[g], own.sigma[g]):.2e}, Omega {rel(given.omega[g], own.omega[g]):.2e}")
        assert d.max() <= 1e-10 and rel(given.sigma[g], own.sigma[g]) <= 1e-8 and rel(given.omega[g], own.omega[g]) <= 1e-8
    assert given.params[1].tobytes() == own.params[1].tobytes()              # a row of None is the search
    b, e = given.begin[2], given.begin[3]
    assert given.params[2, 6] < 0.5 * np.pi and given.params[2, 3:6] @ truth[1][3:6] > 0.99
    dx = X[forms[2][1]] - given.params[2, 0:3]
    s = dx @ given.params[2, 3:6]
    rho = np.linalg.norm(dx - np.outer(s, given.params[2, 3:6]), axis=1)
    outside = rho * np.cos(given.params[2, 6]) - s * np.sin(given.params[2, 6])         # positive outside the reported cone
    assert rel(given.distance[b:e], outside) <= 1e-8 and (outside > 0.0).any() and (outside < 0.0).any() and (s > 0.0).all()
    assert rel(given.distance[b:e], own.distance[own.begin[1]:own.begin[2]]) <= 1e-6 and rel(given.nabla[b:e, 0], own.nabla[own.begin[1]:own.begin[2], 0]) <= 1e-6
    refs = restate(eng, fp, forms, start=[truth[0], None, turned])
    assert_worst("given start", compare(given, refs, forms, "given start"))
    # the four forms from the figures of fit_forms as a start: the same figures
    ffp, fgroups = forms_planted("block_free")
    feng = inverting_pass(ffp, engine.INVERT_FULL_EXPANDED)
    four = [(k, fgroups[k]) for k in range(4)]
    a = feng.fit_forms(S2, four)
    b4 = feng.fit_surfaces(S2, four, start=list(a.params))
    assert not a.status.any() and not b4.status.any()
    for g in range(4):
        npar = R.REPORTED[g]
        assert np.abs(b4.params[g, :npar] - a.params[g, :npar]).max() <= 1e-10 * max(np.abs(a.params[g, :npar]).max(), 1.0)
        assert rel(b4.sigma[g, :npar], a.sigma[g, :npar]) <= 1e-8
    refs4 = restate(feng, ffp, four, start=list(a.params))
    assert_worst("four forms from a start", compare(b4, refs4, four, "four forms from a start"))
    feng.close()
    eng.close()


# ---- 4. the old call keeps its bits, and the new one returns them ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_free", "cfg2"])
def test_the_four_forms_without_a_start_are_fit_forms_bit_for_bit(name):
    fp, groups = forms_planted(name)
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    forms = form_cases_of(name, groups)                                       # k at the least ... m = 64 and beyond on cfg2, all four kinds
    old = eng.fit_forms(S2, forms)
    new = eng.fit_surfaces(S2, forms)
    none = eng.fit_surfaces(S2, forms, start=[None] * len(forms))
    assert same_bits(old, new) and same_bits(old, none)
    assert {k for k, _ in forms} == {0, 1, 2, 3} and (old.status == 0).sum() >= 15
    if name == "cfg2":
        assert [len(p) * R.CONDITIONS[k] for k, p in forms].count(64) == 4
    eng.close()


# ---- 5. status paths ---------------------------------------------------------------------------------------------------------------------------
def test_fixed_coordinates_are_partial():
    fp = helpers.base_scene()
    pf = np.zeros((fp.n_points, 3), bool)
    ctrl = set(int(s) // 3 for s in fp.dg_slot)
    free = [p for p in range(fp.n_points) if p not in ctrl]
    pf[free[1], 1] = True                                                   # Y of one point
    fx = helpers.renumber(fp, point_fixed=pf)
    eng = inverting_pass(fx, engine.INVERT_FULL)                            # a first pass for the size of sigma
    pcol = np.asarray(fx.point_col).reshape(-1, 3)
    sig = np.sqrt(fx.sigma2apriori * np.median(np.diag(exported(eng))[pcol[pcol >= 0]]))
    eng.close()
    rng = np.random.default_rng(6)
    vals = np.array(fx.values, float)
    X = vals[:3 * fx.n_points].reshape(-1, 3)
    grp = np.array(free[:12], np.int32)
    c0 = X[grp].mean(0)
    pts, par = R.surface_points(R.CYLINDER, len(grp), rng, size=0.5 * np.linalg.norm(X[grp] - c0, axis=1).max(), centre=c0)
    X[grp] = pts + 3.0 * sig * rng.normal(size=(len(grp), 3))
    fx = dataclasses.replace(fx, values=vals)
    eng = inverting_pass(fx, engine.INVERT_FULL)
    forms = [(R.CYLINDER, grp), (R.CYLINDER, grp), (R.CYLINDER, grp[2:])]
    fits = eng.fit_surfaces(S2, forms, start=[None, par, None])
    refs = restate(eng, fx, forms, start=[None, par, None])
    assert fits.status[0] == engine.FORM_PARTIAL and fits.status[1] == engine.FORM_PARTIAL and fits.status[2] == 0
    worst = compare(fits, refs, forms, "fixed")
    i1 = fits.begin[0] + 1                                                  # the member with the fixed Y moves in X and Z only
    assert fits.v[i1, 1] == 0.0 and fits.v[i1, 0] != 0.0
    assert_worst("fixed", worst)
    eng.close()


def test_statuses_of_the_start_and_of_the_steps():
    fp, groups, truth = planted("tiny_free")
    eng = inverting_pass(fp, engine.INVERT_FULL)
    X = eng.get_parameters()[:3 * fp.n_points].reshape(-1, 3)
    cy, co, col = groups
    on_axis = np.r_[X[cy[3]], 0.0, 0.0, 1.0, 100.0]                           # an axis along Z through member 3: rho = 0 in the first step
    forms = [(R.CYLINDER, cy[:4]), (R.CONE, co[:5]), (R.CYLINDER, cy), (R.CYLINDER, cy), (R.CONE, co), (R.CONE, co), (R.CYLINDER, cy),
             (R.CONE, co), (R.CYLINDER, col), (R.SPHERE, cy)]
    start = [None, None, np.r_[truth[0][:6], 0.0], np.r_[truth[0][:3], 0.0, 0.0, 0.0, truth[0][6]], np.r_[truth[1][:6], np.pi],
             np.r_[truth[1][:6], -0.1], on_axis, np.r_[X[co[2]], 0.0, 1.0, 0.0, 0.5], None, np.r_[X[cy].mean(0), -1.0, 0.0, 0.0, 0.0]]
    fits = eng.fit_surfaces(S2, forms, start=start)
    S = engine
    assert list(fits.status) == [S.FORM_TOO_SMALL, S.FORM_TOO_SMALL, S.FORM_DEGENERATE, S.FORM_DEGENERATE, S.FORM_DEGENERATE, S.FORM_DEGENERATE,
                                 S.FORM_NOT_FINITE, S.FORM_NOT_FINITE, S.FORM_DEGENERATE, S.FORM_DEGENERATE], fits.status
    assert list(fits.iterations) == [0, 0, 0, 0, 0, 0, 1, 1, 0, 0] and np.isnan(fits.params).all() and np.isnan(fits.v).all()
    refs = restate(eng, fp, forms, start=start)
    compare(fits, refs, forms, "statuses")
    # NOT_CONVERGED returns the last values: two steps from a start five per cent off
    two = eng.fit_surfaces(S2, [(R.CONE, co)], max_iterations=2, start=[noisy(truth[1], R.CONE, 500.0, np.random.default_rng(8), amount=0.05)])
    assert two.status[0] == engine.FORM_NOT_CONVERGED and two.iterations[0] == 2 and np.isfinite(two.params[0]).all() and np.isfinite(two.v).all()
    eng.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_in_the_headers_order_and_leave_the_matrix_bit_identical():
    fp, groups, truth = planted("tiny_free")
    good = [(R.CYLINDER, groups[0])]
    bad = [(6, groups[0])]
    for kw in (dict(image_range=(0, 3)), dict(apply_shared=False)):        # a shard: looked at before the state and the arguments
        sh = engine.Engine(fp, device=0, **kw)
        assert code_of(sh.fit_surfaces, S2, good) == -3 and code_of(sh.fit_surfaces, -1.0, bad) == -3
        sh.close()
    eng = engine.Engine(fp, device=0)                                        # no cofactor matrix: before the arguments
    eng.set_parameters(fp.values)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(engine.INVERT_NONE)
    assert code_of(eng.fit_surfaces, S2, good) == -2 and code_of(eng.fit_surfaces, -1.0, bad) == -2
    eng.close()
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    Q0 = exported(eng)
    P = fp.n_points
    L = engine.load_library()
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    out = np.zeros(20); st = np.zeros(1, np.int32); ty = np.full(1, R.CYLINDER, np.int32); pts = np.ascontiguousarray(groups[0], np.int32)

    def raw(ty_=ty, begin=(0, len(pts)), pts_=pts, out_=out, st_=st, n=1, start=None):
        bg = None if begin is None else np.array(begin, np.int32)
        return L.jaicov_surf_fit(eng._h, S2, n, None if ty_ is None else ty_.ctypes.data_as(pi), None if begin is None else bg.ctypes.data_as(pi),
                                 None if pts_ is None else pts_.ctypes.data_as(pi), None if start is None else start.ctypes.data_as(pd), 20, 0.0,
                                 None if out_ is None else out_.ctypes.data_as(pd), None, None, None if st_ is None else st_.ctypes.data_as(pi), None, None)

    assert raw() == 0 and st[0] == 0 and np.isfinite(out[:7]).all()           # the optional outputs and the start may all be NULL
    assert raw(ty_=None) == -1 and raw(begin=None) == -1 and raw(pts_=None) == -1 and raw(out_=None) == -1 and raw(st_=None) == -1
    assert raw(n=-1) == -1 and raw(begin=(1, len(pts))) == -1
    assert code_of(eng.fit_surfaces, S2, bad) == -1 and code_of(eng.fit_surfaces, S2, [(-1, groups[0])]) == -1
    assert code_of(eng.fit_surfaces, S2, [(R.CONE, [0, 1, 2, 3, 4, P])]) == -1 and code_of(eng.fit_surfaces, S2, [(R.CONE, [0, 1, 2, 1, 4, 5])]) == -1
    for s2 in (0.0, -1.0, float("nan")):
        assert code_of(eng.fit_surfaces, s2, good) == -1
    for tol in (-1e-9, float("nan")):
        assert code_of(eng.fit_surfaces, S2, good, tol=tol) == -1
    assert code_of(eng.fit_surfaces, S2, good, max_iterations=0) == -1
    # a start row with a non-finite value behind its first entry; behind the form's parameters anything may stand
    for at, value in ((3, np.nan), (6, np.nan), (1, np.inf), (0, np.inf)):
        row = np.array(truth[0], float); row[at] = value
        assert code_of(eng.fit_surfaces, S2, good, start=[row]) == -1
    assert code_of(eng.fit_surfaces, S2, good, start=[truth[0]], max_iterations=0) == -1
    sphere_row = np.r_[fp.values[0:3], 100.0, np.nan, np.inf, np.nan]
    assert eng.fit_surfaces(S2, [(R.SPHERE, groups[0])], start=[sphere_row]).status.shape == (1,)
    assert eng.fit_surfaces(S2, []).params.shape == (0, 7) and eng.fit_surfaces(S2, [], start=[]).params.shape == (0, 7)
    np.testing.assert_array_equal(exported(eng), Q0)
    eng.close()


# ---- 7. after a datum transformation the figures follow the new matrix ---------------------------------------------------------------------------
def test_the_figures_follow_a_datum_transformation():
    fp, groups, truth = planted("tiny_free")
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    forms = [(R.CYLINDER, groups[0]), (R.CONE, groups[1])]
    before = eng.fit_surfaces(S2, forms)
    mask = np.zeros(fp.n_points, np.uint8); mask[::2] = 1
    eng.datum_transform(mask)
    after = eng.fit_surfaces(S2, forms)
    refs = restate(eng, fp, forms)
    assert rel(after.sigma, before.sigma) > 1e-6
    worst = compare(after, refs, forms, "new datum")
    invariants(eng, fp, after, forms, "new datum")
    assert_worst("new datum", worst)
    eng.close()


# ---- 8. the C++ mirror --------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_agrees_with_the_ctypes_route(tmp_path):
    """fitSurfaces through the pybind module returns the bits of jaicov_surf_fit on the mirror's own engine"""
    import gzip
    import os
    import shutil
    from bundle_adjustment_amd import host_api as H
    from test_host import example_adjustment
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example")
    for f in ("ior", "eor", "obc", "scale"):
        shutil.copy(os.path.join(golden, f"example.{f}"), tmp_path)
    with gzip.open(os.path.join(golden, "example.phc.gz")) as src, open(tmp_path / "example.phc", "wb") as dst:
        dst.write(src.read())
    keep, ba = example_adjustment(H, str(tmp_path / "example"))
    assert ba.estimateModel() == H.EstimationStateType.ERROR_FREE_ESTIMATION, ba.lastError()
    s2 = ba.getVarianceFactorAposteriori()
    types = [R.CYLINDER, R.CONE, R.PLANE]; begin = [0, 12, 22, 28]; points = np.arange(28, dtype=np.int32)
    start = np.full((3, 7), np.nan); start[2, :4] = [0.0, 0.0, 1.0, 0.0]
    tab, qpp, mem, st, mst = ba.fitSurfaces(s2, types, begin, points.tolist(), start.ravel().tolist(), 30)
    L = engine.load_library()
    h = C.c_void_p(ba.nativeEngineHandle())
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    o = np.zeros((3, 20)); q = np.zeros((3, 28)); m = np.zeros((28, 7)); s = np.zeros(3, np.int32); ms = np.zeros(28, np.int32)
    assert L.jaicov_surf_fit(h, s2, 3, np.array(types, np.int32).ctypes.data_as(pi), np.array(begin, np.int32).ctypes.data_as(pi),
                             points.ctypes.data_as(pi), start.ctypes.data_as(pd), 30, 0.0, o.ctypes.data_as(pd), q.ctypes.data_as(pd),
                             m.ctypes.data_as(pd), s.ctypes.data_as(pi), ms.ctypes.data_as(pi), None) == 0
    print("status", s, "iterations", o[:, 19])
    assert tab.tobytes() == o.tobytes() and qpp.tobytes() == q.tobytes() and mem.tobytes() == m.tobytes()
    assert st.tobytes() == s.tobytes() and mst.tobytes() == ms.tobytes()
    del keep
