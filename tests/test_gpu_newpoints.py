"""GPU: new object points intersected in the adjusted block with its full Qxx (include/jaicov_newpoints.h, csrc/newpoints.hip)
against the numpy restatement of tests/newpoint_reference.py, evaluated at the device's own X on the cofactor matrix that the same
engine exports (get_cofactor_sub).

Scenes: the free network with a scale bar (d = 6), two cameras with 11 and 5 coefficients, the scene with a fixed point, a fixed c
and a fixed kappa (PARTIAL) of predict_reference, and the block of 40 images.  A call of 63 points or more holds, beside points
with 2, 3 and 8 rays: one with 64 rays (images repeated), one with 65 (TOO_MANY), one with 1 ray and one with none (TOO_FEW_RAYS),
one with two near-parallel rays (SINGULAR), two that share their images, one that shares only the camera with them, and one whose
rays come from the first and the last image (both cameras of the two-camera scene).  A fifth scene with five cameras and 64
images holds a point with more than 448 shared columns (the other half of TOO_MANY) and one with exactly 448.  Every test prints
the worst figure it saw before it asserts."""
import ctypes as C
import gc
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import newpoint_reference as R
from bundle_adjustment_amd import engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "example")

NAMES = list(R.SCENES)
MODES = {"FULL": engine.INVERT_FULL, "FULL_EXPANDED": engine.INVERT_FULL_EXPANDED}
COUNTS = (1, 63, 65, 257)
S2 = 0.83
NOISE = 0.0005                       # mm: the sigma of the scenes' own image points
_pd, _pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
I_64, I_65, I_ONE, I_PARALLEL, I_A, I_FAR, I_SAME, I_ENDS, I_NONE = 1, 2, 3, 4, 5, 6, 7, 8, 9        # the special points of a call


def inverting_pass(fp, mode):
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(mode)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(mode)
    return eng


def exported(eng):
    return eng.get_cofactor_sub(np.arange(eng.cofactor_order(), dtype=np.int32))


def make_call(fp, count, seed=51):
    """the points of one call: (truth, ray_begin, ray_image, xy, disp, start); measurements at the scene's truth plus noise"""
    counts = np.resize([2, 3, 8, 3], count)
    special = count >= 63
    if special:
        counts[[I_64, I_65, I_ONE, I_PARALLEL, I_A, I_FAR, I_SAME, I_ENDS, I_NONE]] = [64, 65, 1, 2, 3, 3, 3, 3, 0]
    rb, ri = R.rays_of(fp, counts, seed=seed)
    if special:
        ri[rb[I_PARALLEL]:rb[I_PARALLEL + 1]] = ri[rb[I_PARALLEL]]
        ri[rb[I_A]:rb[I_A + 1]] = [0, 1, 2]; ri[rb[I_SAME]:rb[I_SAME + 1]] = [0, 1, 2]; ri[rb[I_FAR]:rb[I_FAR + 1]] = [3, 4, 5]
        ri[rb[I_ENDS]:rb[I_ENDS + 1]] = [0, fp.n_images - 1, 1]
    X = R.new_points(fp, count, seed=seed + 1)
    xy = R.measure(fp, R.model_values(fp), X, rb, ri, sigma=NOISE, seed=seed + 2)
    if special:
        xy[rb[I_PARALLEL] + 1] = xy[rb[I_PARALLEL]] + 1e-9
    disp = R.dispersions(fp, ri.size, seed=seed + 3)
    start = X + np.random.default_rng(seed + 4).uniform(-5.0, 5.0, X.shape)
    return X, rb, ri, xy, disp, start


def make_pairs(fp, count):
    """pairs of every kind among the points of make_call: new-new sharing images, new-new sharing only the camera, new-block point
    in both orders, a failed member, and ordinary neighbours"""
    if count < 63:
        return np.zeros((0, 2), np.int32)
    p = [(I_A, I_SAME), (I_A, I_FAR), (I_FAR, I_SAME), (I_A, -1 - 5), (-1 - 7, I_FAR), (I_64, I_ENDS), (I_ONE, I_A), (I_A, I_65), (I_PARALLEL, -1 - 0)]
    p += [(i, i + 1) for i in range(10, min(count, 40) - 1)]
    return np.array(p, np.int32)


def bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def point_bits(r, k=slice(None)):
    return bits(r.xyz[k], r.cof_meas[k], r.cof[k], r.sigma[k], r.omega[k], r.dof[k], r.status[k], r.iterations[k])


def check_against_reference(oracle_mod, fp, Q, got, call, pairs, label, min_shared=3):
    """every figure of `got` against the reference at the device's X; returns the worst ratios"""
    X, rb, ri, xy, disp, start = call
    s0 = fp.sigma2apriori
    n = len(rb) - 1
    failed = (got.status & R.FAILED) != 0
    Xd = np.where(failed[:, None], X, got.xyz)
    w, J = R.rows(oracle_mod, fp, fp.values, Xd, rb, ri, xy)
    worst = dict(step=0.0, meas=0.0, sys=0.0, xx=0.0, omega=0.0, w=0.0, sigma=0.0, pair=0.0)
    members = {}
    for i in range(n):
        k = slice(rb[i], rb[i + 1])
        m = rb[i + 1] - rb[i]
        if m < 2 or m > R.MAX_RAYS:
            assert got.status[i] == (R.TOO_FEW_RAYS if m < 2 else R.TOO_MANY), (label, i, got.status[i])
            assert np.isnan(np.r_[got.xyz[i], got.cof_meas[i], got.cof[i], got.sigma[i], got.omega[i], got.dof[i]]).all() and np.isnan(got.ray_w[k]).all()
            continue
        e = R.evaluate(fp, Q, w[k], J[k], ri[k], disp[k], s0)
        if e["status"] & R.FAILED:
            assert got.status[i] == e["status"], (label, i, got.status[i], e["status"])
            assert np.isnan(np.r_[got.xyz[i], got.cof_meas[i], got.cof[i], got.sigma[i], got.omega[i], got.dof[i]]).all() and np.isnan(got.ray_w[k]).all()
            continue
        assert got.status[i] == e["status"], (label, i, got.status[i], e["status"])       # converged, and PARTIAL where the reference says so
        assert got.dof[i] == 2 * m - 3 and 1 <= got.iterations[i] <= 20
        worst["step"] = max(worst["step"], np.abs(e["dx"]).max() / R.threshold(fp, fp.values, got.xyz[i], ri[rb[i]]))
        worst["meas"] = max(worst["meas"], (np.abs(got.cof_meas[i] - R.sym6(e["Q_meas"])) / R.sym6(e["E_meas"])).max())
        worst["xx"] = max(worst["xx"], (np.abs(got.cof[i] - R.sym6(e["Q_XX"])) / R.sym6(e["E_XX"])).max())
        sys_got = got.cof[i] - got.cof_meas[i]
        worst["sys"] = max(worst["sys"], (np.abs(sys_got - R.sym6(e["Q_sys"])) / (R.sym6(e["E_sys"]) + 4.0 * R.U53 * np.abs(got.cof[i]))).max())
        Ew = R.bound_w(w[k], xy[k])
        worst["w"] = max(worst["w"], (np.abs(got.ray_w[k] - w[k]) / Ew).max())
        worst["omega"] = max(worst["omega"], abs(got.omega[i] - e["omega"]) / R.bound_omega(w[k], Ew, e["P"]))
        sig = np.sqrt(S2 * np.maximum(got.cof[i][[0, 3, 5]], 0.0))
        worst["sigma"] = max(worst["sigma"], (np.abs(got.sigma[i] - sig) / sig).max())
        assert np.all(np.linalg.eigvalsh(e["Q_sys"]) >= -1e-9 * np.trace(e["Q_sys"]))
        assert np.all(got.cof[i][[0, 3, 5]] >= got.cof_meas[i][[0, 3, 5]])                 # the adjustment's share only adds
        members[i] = R.new_member(got.xyz[i], e)
    shared = 0
    for j, (a, b) in enumerate(pairs):
        row, st = got.lengths[j], got.length_status[j]
        if any(x >= 0 and failed[x] for x in (a, b)):
            assert st & R.PAIR_NOT_FINITE and np.isnan(row).all(), (label, j, st, row)
            continue
        ma, mb = (members[x] if x >= 0 else R.block_member(fp, fp.values, Q, -1 - x) for x in (a, b))
        ref, rst, bound, E_dv = R.pair_figures(Q, ma, mb, S2)
        assert st == rst, (label, j, st, rst)
        assert abs(row[0] - ref[0]) <= 8.0 * R.U53 * ref[0]
        worst["pair"] = max(worst["pair"], abs(row[5] - ref[5]) / bound[0], abs(row[6] - ref[6]) / bound[1])
        assert abs(row[1] - np.sqrt(S2 * max(row[5], 0.0))) <= 1e-14 * row[1]
        worst["pair"] = max(worst["pair"], (np.abs(row[2:5] ** 2 - ref[2:5] ** 2) / (S2 * E_dv + 8.0 * R.U53 * ref[2:5] ** 2)).max())
        if np.intersect1d(ma["cols"][ma["cols"] >= 0], mb["cols"][mb["cols"] >= 0]).size:
            shared += 1
            assert row[5] != row[6], (label, j, row)
    if len(pairs):
        assert shared >= min_shared
    print(f"{label}: {n} points, {len(pairs)} pairs: step {worst['step']:.2e} of the threshold; of their bounds: Q_meas {worst['meas']:.2e}, "
          f"Q_sys {worst['sys']:.2e}, Q_XX {worst['xx']:.2e}, Omega {worst['omega']:.2e}, ray_w {worst['w']:.2e}, q_L {worst['pair']:.2e}; "
          f"sigma {worst['sigma']:.2e} relative; status {sorted(set(got.status.tolist()))}, pair status {sorted(set(got.length_status.tolist()))}")
    return worst


# ---- 1. against the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_new_points_and_pairs_match_the_reference_on_the_exported_matrix(oracle_mod, name, mode):
    fp = R.scene_of(name)
    eng = inverting_pass(fp, MODES[mode])
    Q = exported(eng)
    for count in COUNTS:
        call = make_call(fp, count)
        X, rb, ri, xy, disp, start = call
        pairs = make_pairs(fp, count)
        got = eng.intersect_new_points(S2, rb, ri, xy, disp, start=start, pairs=pairs)
        assert got.xyz.shape == (count, 3) and got.cof.shape == (count, 6) and got.ray_w.shape == (ri.size, 2) and got.lengths.shape == (len(pairs), 7)
        worst = check_against_reference(oracle_mod, fp, Q, got, call, pairs, f"{name} {mode}")
        assert worst["step"] <= 1.0
        assert max(worst[k] for k in ("meas", "sys", "xx", "omega", "w", "pair")) <= 1.0
        assert worst["sigma"] <= 1e-14
        ok = (got.status & R.FAILED) == 0
        if count >= 63:
            assert got.status[I_65] == R.TOO_MANY and got.status[I_ONE] == R.TOO_FEW_RAYS == got.status[I_NONE]
            assert got.status[I_PARALLEL] & R.SINGULAR and not got.status[I_64] & R.FAILED
        if name == "partial":
            assert (got.status[ok] & R.PARTIAL).all() and (count < 63 or got.length_status[4] & R.PAIR_PARTIAL)
        else:
            assert not (got.status & R.PARTIAL).any()
    eng.close()


def test_more_than_448_shared_columns_are_too_many(oracle_mod):
    """64 images of five cameras give a point 64 * 6 + 5 * 14 = 454 shared columns: TOO_MANY, NaN, and NOT_FINITE for a pair that names
    it; 63 of them give exactly 448, the most a point may have, and every figure of that point holds against the reference"""
    fp = R.scene_of("five_camera")
    assert fp.n_cameras == 5 and fp.n_images == 64
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    Q = exported(eng)
    rb = np.array([0, 64, 127, 130], np.int32)
    ri = np.concatenate([np.arange(64), np.arange(63), [0, 30, 63]]).astype(np.int32)
    X = R.new_points(fp, 3, seed=61)
    xy = R.measure(fp, fp.values, X, rb, ri, sigma=NOISE, seed=62)
    disp = R.dispersions(fp, ri.size, seed=63)
    start = X + 3.0
    pairs = np.array([[0, 2], [1, 2], [2, 1], [1, -1 - 3], [1, 0]], np.int32)
    got = eng.intersect_new_points(S2, rb, ri, xy, disp, start=start, pairs=pairs)
    assert got.status[0] == R.TOO_MANY and np.isnan(got.xyz[0]).all() and np.isnan(got.ray_w[:64]).all()
    assert got.status[1] == 0 and got.status[2] == 0
    assert (got.length_status[[0, 4]] & R.PAIR_NOT_FINITE).all() and np.isnan(got.lengths[[0, 4]]).all() and not got.length_status[[1, 2, 3]].any()
    cols = np.unique(np.concatenate([R.shared_columns(fp, im) for im in range(63)]))
    assert cols.size == R.MAX_COLS
    worst = check_against_reference(oracle_mod, fp, Q, got, (X, rb, ri, xy, disp, start), pairs, "five_camera FULL_EXPANDED", min_shared=2)
    assert worst["step"] <= 1.0 and max(worst[k] for k in ("meas", "sys", "xx", "omega", "w", "pair")) <= 1.0
    alone = eng.intersect_new_points(S2, rb[1:3] - 64, ri[64:127], xy[64:127], disp[64:127], start=start[1:2])
    assert point_bits(got, slice(1, 2)) == point_bits(alone)
    eng.close()


def test_start_values_from_the_lens_correction_and_the_intersection():
    """start=None composes lens_correct and intersect_points; the result is the one of explicit start values to the convergence threshold"""
    fp = R.scene_of("block")
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    X, rb, ri, xy, disp, start = make_call(fp, 40)
    a = eng.intersect_new_points(S2, rb, ri, xy, disp, start=start)
    b = eng.intersect_new_points(S2, rb, ri, xy, disp)
    assert not a.status.any() and not b.status.any()
    d = np.abs(a.xyz - b.xyz).max()
    print(f"start values from the intersection: {b.iterations.max()} steps at most, against explicit ones {a.iterations.max()}; |dX| {d:.2e} mm")
    assert d <= 2.0 * R.SQRT_EPS * 3000.0
    one = eng.intersect_new_points(S2, rb, ri, xy, disp, start=start, max_iterations=1)
    assert (one.status == R.NOT_CONVERGED).all() and (one.iterations == 1).all() and np.isfinite(one.xyz).all() and np.isfinite(one.cof).all()
    sv = eng.new_point_start_values(rb, ri, xy, disp)
    assert sv.shape == (40, 3) and np.isfinite(sv).all()
    print(f"start values against the solution: {np.abs(sv - a.xyz).max():.3f} mm at most")
    # where the composition fails the start value is NaN and the point ends as NOT_FINITE: two parallel rays (the intersection is
    # SINGULAR), and a measurement that is not finite (the lens correction fails, the raw measurement goes on, the intersection fails)
    ri2, xy2 = ri.copy(), xy.copy()
    assert rb[1] - rb[0] == 2 and rb[2] - rb[1] == 3
    ri2[rb[0] + 1] = ri2[rb[0]]; xy2[rb[0] + 1] = xy2[rb[0]] + 1e-9
    xy2[rb[1], 0] = np.nan
    sv2 = eng.new_point_start_values(rb, ri2, xy2, disp)
    assert np.isnan(sv2[0:2]).all() and bits(sv2[2:]) == bits(sv[2:])
    c = eng.intersect_new_points(S2, rb, ri2, xy2, disp)
    assert c.status[0] == R.NOT_FINITE == c.status[1] and np.isnan(c.xyz[0:2]).all() and not c.status[2:].any()
    assert point_bits(b, slice(2, None)) == point_bits(c, slice(2, None))
    assert eng.new_point_start_values([0], [], np.zeros((0, 2)), np.zeros((0, 3))).shape == (0, 3)
    eng.close()


# ---- 2. bits -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_two_runs_sublists_and_permutations_give_the_same_bits(name):
    fp = R.scene_of(name)
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    X, rb, ri, xy, disp, start = make_call(fp, 65)
    pairs = make_pairs(fp, 65)

    def run(order, pr):
        """the points `order` of the call, and pairs given in the numbering of the whole call"""
        idx = np.concatenate([np.arange(rb[i], rb[i + 1]) for i in order]).astype(np.int64)
        b2 = np.concatenate([[0], np.cumsum([rb[i + 1] - rb[i] for i in order])]).astype(np.int32)
        new = {int(o): k for k, o in enumerate(order)}
        p2 = np.array([[new[int(m)] if m >= 0 else m for m in p] for p in pr], np.int32).reshape(-1, 2)
        return eng.intersect_new_points(S2, b2, ri[idx], xy[idx], disp[idx], start=start[list(order)], pairs=p2), idx

    a, _ = run(range(65), pairs)
    a2, _ = run(range(65), pairs)
    assert point_bits(a) == point_bits(a2) and bits(a.ray_w, a.lengths, a.length_status) == bits(a2.ray_w, a2.lengths, a2.length_status)
    perm = np.random.default_rng(21).permutation(65)
    pperm = np.random.default_rng(22).permutation(len(pairs))
    b, idx = run(perm, pairs[pperm])
    assert point_bits(a, perm) == point_bits(b) and bits(a.ray_w[idx]) == bits(b.ray_w)
    assert bits(a.lengths[pperm], a.length_status[pperm]) == bits(b.lengths, b.length_status)
    sub = np.sort(np.random.default_rng(23).choice(np.arange(10, 65), 20, replace=False))
    c, idx = run(np.r_[[I_A, I_FAR], sub], pairs[1:2])
    assert point_bits(a, np.r_[[I_A, I_FAR], sub]) == point_bits(c) and bits(a.ray_w[idx]) == bits(c.ray_w)
    assert bits(a.lengths[1:2], a.length_status[1:2]) == bits(c.lengths, c.length_status)
    one, _ = run([I_64], pairs[:0])
    assert point_bits(a, slice(I_64, I_64 + 1)) == point_bits(one)
    eng.close()


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------
def raw(eng, sigma2, n, rb, ri, xy, disp, start, max_it, pairs, G, out, st, it, rw, pout, pst):
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)      # noqa: E731
    return eng.L.jaicov_newpt_intersect(eng._h, sigma2, n, p(rb, _pi), p(ri, _pi), p(xy, _pd), p(disp, _pd), p(start, _pd), max_it, p(pairs, _pi), G,
                                        p(out, _pd), p(st, _pi), p(it, _pi), p(rw, _pd), p(pout, _pd), p(pst, _pi))


def test_refusals_leave_the_outputs_and_the_matrix_untouched():
    fp = R.scene_of("free")
    rb = np.array([0, 2, 5], np.int32); ri = np.array([0, 1, 2, 3, 4], np.int32)
    X = R.new_points(fp, 2)
    xy = np.ascontiguousarray(R.measure(fp, fp.values, X, rb, ri)); disp = np.tile([1e-6, 1e-6, 0.1], (5, 1)); start = X + 1.0
    pairs = np.array([[0, 1], [1, -1]], np.int32)
    out = np.full((2, 20), 3.0); st = np.full(2, 7, np.int32); it = np.full(2, 8, np.int32); rw = np.full((5, 2), 2.0)
    pout = np.full((2, 7), 5.0); pst = np.full(2, 9, np.int32)
    ok = [1.0, 2, rb, ri, xy, disp, start, 20, pairs, 2, out, st, it, rw, pout, pst]

    def untouched():
        return np.all(out == 3.0) and np.all(st == 7) and np.all(it == 8) and np.all(rw == 2.0) and np.all(pout == 5.0) and np.all(pst == 9)

    # a shard of either kind: UNSUPPORTED, before the state (these engines have no cofactor matrix either) and before any argument
    for kw in (dict(image_range=(0, 3)), dict(apply_shared=False)):
        sh = engine.Engine(fp, device=0, **kw)
        assert raw(sh, *ok) == -3 and untouched()
        assert raw(sh, -1.0, 2, None, *ok[3:]) == -3 and untouched()
        assert raw(sh, 1.0, -1, *ok[2:]) == -3 and untouched()
        assert "shard" in sh.L.jaicov_neq_last_error(sh._h).decode()
        sh.close()
    # no inverting solve, and the matrix of the EO-reduced system: BAD_STATE, before any argument is looked at
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    assert raw(eng, *ok) == -2 and untouched()
    assert raw(eng, -1.0, 2, None, *ok[3:]) == -2 and untouched()
    eng.close()
    fr = R.scene_of("two_camera")                            # dense image blocks: its REDUCED matrix has no EO columns
    eng = inverting_pass(fr, engine.INVERT_REDUCED)
    assert 0 < eng.cofactor_order() < fr.n_unknowns
    idx = np.arange(eng.cofactor_order(), dtype=np.int32)
    before = eng.get_cofactor_sub(idx).tobytes()
    assert raw(eng, *ok) == -2 and untouched()
    assert "FULL" in eng.L.jaicov_neq_last_error(eng._h).decode()
    assert eng.get_cofactor_sub(idx).tobytes() == before
    eng.close()
    # bad arguments
    eng = inverting_pass(fp, engine.INVERT_FULL)
    idx = np.arange(eng.cofactor_order(), dtype=np.int32)
    before = eng.get_cofactor_sub(idx).tobytes()

    def d(i, k, v):
        a = disp.copy(); a[i, k] = v
        return a

    bad_im = ri.copy(); bad_im[3] = fp.n_images
    neg_im = ri.copy(); neg_im[0] = -1
    cases = []
    for pos, vals in ((0, (-1.0, np.nan)), (1, (-1,)), (2, (None, np.array([1, 2, 5], np.int32), np.array([0, 3, 2], np.int32))), (3, (None, bad_im, neg_im)),
                      (4, (None,)), (5, (None, d(0, 0, 0.0), d(1, 1, -1e-6), d(2, 2, 1.0), d(3, 2, -1.0), d(0, 0, np.nan), d(4, 2, np.nan))),
                      (6, (None,)), (7, (0, -3)),
                      (8, (None, np.array([[0, 2], [1, -1]], np.int32), np.array([[0, 0], [1, -1]], np.int32), np.array([[-1, -2], [1, -1]], np.int32),
                           np.array([[0, 1], [1, -1 - fp.n_points]], np.int32), np.array([[-3, -3], [0, 1]], np.int32))),
                      (9, (-1,)), (10, (None,)), (11, (None,)), (14, (None,)), (15, (None,))):
        for v in vals:
            a = list(ok); a[pos] = v
            cases.append(a)
    for a in cases:
        assert raw(eng, *a) == -1, a
        assert untouched()
    assert eng.get_cofactor_sub(idx).tobytes() == before
    # the empty call is a call; iterations and ray_w may be NULL; a call without pairs needs no pair arguments
    assert raw(eng, 1.0, 0, None, None, None, None, None, 20, None, 0, None, None, None, None, None, None) == 0 and untouched()
    assert raw(eng, 1.0, 0, None, None, None, None, None, 20, pairs, 2, None, None, None, None, pout, pst) == -1 and untouched()     # no member to name
    assert raw(eng, 1.0, 2, rb, ri, xy, disp, start, 20, None, 0, out, st, None, None, None, None) == 0
    assert not st.any() and np.isfinite(out).all() and np.all(it == 8) and np.all(rw == 2.0) and np.all(pout == 5.0)
    e = eng.intersect_new_points(1.0, [0], [], np.zeros((0, 2)), np.zeros((0, 3)), start=np.zeros((0, 3)))
    assert e.xyz.shape == (0, 3) and e.status.size == 0 and e.lengths.shape == (0, 7)
    # a start value that is not finite is no refusal
    s2 = start.copy(); s2[1, 2] = np.nan
    g = eng.intersect_new_points(1.0, rb, ri, xy, disp, start=s2)
    assert g.status[0] == 0 and g.status[1] == R.NOT_FINITE and np.isnan(g.xyz[1]).all() and np.isfinite(g.xyz[0]).all()
    assert eng.get_cofactor_sub(idx).tobytes() == before
    eng.close()


# ---- 4. ownership ------------------------------------------------------------------------------------------------------------------------
def census():
    lib = engine.load_library()
    lib.jaicov_debug_device_census.argtypes = [C.POINTER(C.c_longlong)]
    lib.jaicov_debug_device_census.restype = None
    a = (C.c_longlong * 2)()
    lib.jaicov_debug_device_census(a)
    return int(a[0]), int(a[1])


def test_the_work_buffers_go_with_the_engine():
    fp = R.scene_of("two_camera")
    X, rb, ri, xy, disp, start = make_call(fp, 65)
    small = make_call(fp, 5)

    def scenario():
        eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
        a = census()
        eng.intersect_new_points(1.0, rb, ri, xy, disp, start=start, pairs=make_pairs(fp, 65))
        b = census()
        assert b[0] > a[0] and b[1] == a[1] + 4, (a, b)          # tab, rows, vals and out of NewPointState
        eng.intersect_new_points(1.0, small[1], small[2], small[3], small[4], start=small[5])
        assert census()[1] == b[1]                                # a smaller call fits the buffers
        eng.close()

    scenario()
    gc.collect()
    c0 = census()
    scenario()
    c1 = census()
    print(f"census after warm-up {c0}, after the scenario {c1}")
    assert c1 == c0


# ---- 5. the C++ mirror and the example program ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example_base(tmp_path_factory):
    d = tmp_path_factory.mktemp("example")
    for f in ("ior", "eor", "obc", "scale"):
        shutil.copy(os.path.join(GOLDEN, f"example.{f}"), d)
    with gzip.open(os.path.join(GOLDEN, "example.phc.gz")) as src, open(d / "example.phc", "wb") as dst:
        dst.write(src.read())
    return str(d / "example")


def test_cpp_mirror_and_example_program(example_base):
    """intersectNewPoints through the pybind module returns the bits of the C call and of Engine.intersect_new_points, all three on
    the mirror's own engine.  host/example_new_points adjusts the bundled block without every tenth point in a process of its own and
    intersects those points from (at most 64 of) their withheld measurements; it is judged by its exit status (no sigma from Q_XX
    below the one from Q_meas) and by its listing, not against a Python call: Python has no reader that withholds measurements."""
    from bundle_adjustment_amd import host_api as H
    from test_host import example_adjustment
    host = os.path.join(ROOT, "bundle-adjustment_amd", "host")
    if not os.path.exists(os.path.join(host, "example_new_points")):
        subprocess.check_call(["make", "-C", host, "example_new_points"], stdout=subprocess.DEVNULL)
    a = subprocess.run([os.path.join(host, "example_new_points"), example_base], capture_output=True, text=True, timeout=600)
    print(a.stdout[-4000:])
    assert a.returncode == 0, (a.stdout[-2000:], a.stderr[-2000:])
    m = re.search(r"^new points intersected: (\d+) of (\d+), sigma from Q_XX not below that from Q_meas: (\d+)", a.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 5 and int(m.group(2)) >= int(m.group(1)) == int(m.group(3))
    ln = re.search(r"^length \S+ - \S+: L (\S+) mm, sigma_L (\S+) mm, q_L (\S+), without the correlations (\S+) \(status (\d+)\)", a.stdout, flags=re.M)
    assert ln and float(ln.group(1)) > 0.0 and float(ln.group(2)) > 0.0 and float(ln.group(3)) != float(ln.group(4))
    assert not int(ln.group(5)) & (R.PAIR_NOT_FINITE | R.PAIR_DEGENERATE)

    keep, ba = example_adjustment(H, example_base)
    assert ba.estimateModel() == H.EstimationStateType.ERROR_FREE_ESTIMATION, ba.lastError()
    s2 = ba.getVarianceFactorAposteriori()
    L = engine.load_library()
    h = C.c_void_p(ba.nativeEngineHandle())
    # two adjusted points measured again as if new: where they appear in the images 0 .. 3, the start 2 mm beside their adjusted place
    tab0, _ = ba.predictImagePoints(s2, [0, 1, 2, 3, 0, 1, 2], [5, 5, 5, 5, 9, 9, 9], 1.0)
    rb = np.array([0, 4, 7], np.int32); ri = np.array([0, 1, 2, 3, 0, 1, 2], np.int32)
    xy = np.ascontiguousarray(tab0[:, 0:2] + 1e-4); disp = np.tile([4e-6, 9e-6, 0.2], (7, 1)); pairs = np.array([[0, 1], [0, -1 - 5]], np.int32)
    oc = ba.getObjectCoordinates()
    start = np.array([[oc[k].getX().getValue(), oc[k].getY().getValue(), oc[k].getZ().getValue()] for k in (5, 9)]) + 2.0
    o = np.zeros((2, 20)); s = np.zeros(2, np.int32); it = np.zeros(2, np.int32); rw = np.zeros((7, 2)); po = np.zeros((2, 7)); ps = np.zeros(2, np.int32)
    rc = L.jaicov_newpt_intersect(h, s2, 2, rb.ctypes.data_as(_pi), ri.ctypes.data_as(_pi), xy.ctypes.data_as(_pd), disp.ctypes.data_as(_pd),
                                  start.ctypes.data_as(_pd), 50, pairs.ctypes.data_as(_pi), 2, o.ctypes.data_as(_pd), s.ctypes.data_as(_pi),
                                  it.ctypes.data_as(_pi), rw.ctypes.data_as(_pd), po.ctypes.data_as(_pd), ps.ctypes.data_as(_pi))
    assert rc == 0
    tab, st, iters, rayw, lengths, lst = ba.intersectNewPoints(s2, rb.tolist(), ri.tolist(), xy.ravel().tolist(), disp.ravel().tolist(),
                                                               start.ravel().tolist(), pairs.ravel().tolist(), 50)
    assert tab.shape == (2, 20) and tab.tobytes() == o.tobytes() and st.tobytes() == s.tobytes() and iters.tobytes() == it.tobytes()
    assert rayw.tobytes() == rw.tobytes() and lengths.tobytes() == po.tobytes() and lst.tobytes() == ps.tobytes()
    # Engine.intersect_new_points bound to the mirror's engine (the handle stays the mirror's: it is taken back before the object goes)
    py = engine.Engine.__new__(engine.Engine)
    py.L, py._h = L, h
    try:
        g = py.intersect_new_points(s2, rb, ri, xy, disp, start=start, pairs=pairs, max_iterations=50)
    finally:
        py._h = C.c_void_p()
    assert bits(g.xyz, g.cof_meas, g.cof, g.omega, g.dof, g.sigma) == bits(tab[:, 0:3], tab[:, 3:9], tab[:, 9:15], tab[:, 15], tab[:, 16], tab[:, 17:20])
    assert bits(g.status, g.iterations, g.ray_w, g.lengths, g.length_status) == bits(st, iters, rayw, lengths, lst)
    print(f"mirror: status {s.tolist()}, iterations {it.tolist()}, X {o[:, 0:3].tolist()}, lengths {po[:, 0].tolist()}, pair status {ps.tolist()}")
    assert not (s & R.FAILED).any() and np.isfinite(o).all() and np.isfinite(po).all()
    assert po[1, 0] < 1.0                                     # the re-measured point 5 lies beside the adjusted point 5
    del keep
