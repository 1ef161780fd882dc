"""GPU: one pass, the whole loop and everything that reads the border, at every datum defect d = 0 .. 7.

The rest of the suite runs d = 0 and d = 6 only.  The scenes of tests/datum_defect_scenes.py reach every other count of border rows
on two base scenes, and with them: the SCALE condition row (d = 7, 4, 1), border rows numbered with gaps (d = 5 .. 1), d + 1 = 2 ..
8 right-hand sides through the factorisation and backsolve_chain_kernel<2 / 4 / 8> full and ragged, all seven slots of the
refinement's border and the full 7 x 14 elimination of the datum transformation.  The checkers are the ones of the tests named in
each docstring, with their bounds; tests/test_datum_defect_scenes.py holds the table and the reference on the CPU first.

Path taken (create_plan.h, asserted in test_path_taken_by_every_scene and device-free in tests/test_datum_defect_scenes.py):
  block scenes, d in {0, 3, 4, 5, 6, 7}: EO-reduced, order U - 6 I -- the border sits inside the reduced system;
  block scenes, d in {1, 2}: full order U -- a fixed angle takes the exterior orientations out of the trailing 6 I columns;
  diag scenes, every d: full order U -- ordinary image groups, and the elimination would save less than two block columns
  (test_forced_elimination_of_ordinary_images_with_a_border switches it on for d in {3, 4, 5, 7}).

The oracle needs about a second per pass on a block scene (literal stacking of the dense dispersions): every reference is computed
once per session and shared (lru_cache); nobody writes into one."""
import functools

import numpy as np
import pytest

import datum_defect_scenes as S
import datum_reference
from bundle_adjustment_amd import engine
from bundle_adjustment_amd.problem import packed_to_full
from test_gpu_refinement import bordered, exact_solution, rel

pytestmark = pytest.mark.gpu

BLOCK_147 = ["block_d1", "block_d4", "block_d7"]
DOWNSTREAM = ["block_d7", "block_d4"]


# ---- shared references ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_pass(name, lam):
    """(dx, Qxx packed, N, n) of the oracle's inverting pass at the start values: N, n as built (datum rows, damping)."""
    import oracle
    oracle.build()
    fp = S.get_scene(name)
    dx, Q, N0, n0 = oracle.Oracle(fp).step(fp.values, fp.sigma2apriori, lam, True)
    for a in (dx, Q, N0, n0):
        a.setflags(write=False)
    return dx, Q, N0, n0


def expected_order(name):
    fp = S.get_scene(name)
    reduced = name.startswith("block") and S.DEFECT[name] not in (1, 2)
    return fp.n_unknowns - (6 * fp.n_images if reduced else 0)


def correlation_scale(Qref):
    sd = np.sqrt(np.abs(np.diag(Qref))); sd[sd == 0] = 1.0
    return np.outer(sd, sd)


def one_pass(fp, invert, lam=0.0, **kw):
    eng = engine.Engine(fp, **kw)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(invert)
    eng.build(fp.sigma2apriori, lam)
    return eng


# ---- path taken ---------------------------------------------------------------------------------------------------------------------
def test_path_taken_by_every_scene():
    """reduced_order() of the default build of every scene.  The block scenes of d in {0, 3, 4, 5, 6, 7} take the EO-reduced path
    (order U - 6 I); the d = 1 and d = 2 scenes fix angles of one image, so their exterior orientations are not the trailing 6 I
    columns and create_plan keeps the full order U (eo_columns_trailing); the diag scenes keep U at every d (ordinary groups below
    the size rule of synthesize_blocks)."""
    for name in S.NAMES:
        fp = S.get_scene(name)
        eng = one_pass(fp, engine.INVERT_NONE)
        order = eng.reduced_order()
        eng.close()
        U, I = fp.n_unknowns, fp.n_images
        print(f"path {name}: d = {fp.rank_defect}, U = {U}, order {order} ({'EO-reduced' if order < U else 'full order'})")
        assert order == expected_order(name)
        if name.startswith("block") and S.DEFECT[name] in (3, 4, 5, 7):
            assert order == U - 6 * I


# ---- normal equations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_normal_equations_match_oracle_at_every_defect(name):
    """test_gpu_parity.test_normal_equations_match_oracle on the table: N (datum rows included) and n at 1e-11, lambda 0 and 0.5,
    full-order path.  The border rows alone as well: unit rows from sums of at most 60 terms, so two correct fp64 evaluations
    differ by a few 1e-15; held to 1e-13 absolute."""
    fp = S.get_scene(name)
    U, d = fp.n_unknowns, fp.rank_defect
    for lam in (0.0, 0.5):
        _, _, No, no = oracle_pass(name, lam)
        eng = one_pass(fp, True, lam)
        assert eng.reduced_order() == U
        N, n = eng.get_normal()
        eng.close()
        Nf, Nof = packed_to_full(N, U), packed_to_full(No, U)
        dg = np.sqrt(np.abs(np.diag(Nof))); dg[dg == 0] = 1.0
        err = float((np.abs(Nf - Nof) / np.outer(dg, dg)).max())
        nerr = float(np.abs(n - no).max() / np.abs(no).max())
        berr = float(np.abs(Nf[:d] - Nof[:d]).max()) if d else 0.0
        print(f"{name} lambda {lam}: N {err:.2e}, n {nerr:.2e}, border rows {berr:.2e}")
        assert err < 1e-11
        np.testing.assert_allclose(n, no, rtol=0, atol=1e-11 * np.abs(no).max())
        assert berr <= 1e-13
        assert np.array_equal(Nf[:d] != 0, Nof[:d] != 0)


# ---- step and cofactors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("name", S.NAMES)
def test_solve_matches_oracle_at_every_defect(name, invert):
    """test_gpu_parity.test_solve_matches_oracle on the table.  Without inversion the build takes the scene's default path (EO-reduced
    on the block scenes of d in {0, 3 .. 7}), with it the full order."""
    fp = S.get_scene(name)
    U, d, s2 = fp.n_unknowns, fp.rank_defect, fp.sigma2apriori
    dxo, Qo, _, _ = oracle_pass(name, 0.0)
    import oracle
    o = oracle.Oracle(fp)
    eng = one_pass(fp, invert)
    order = eng.reduced_order()
    assert order == (U if invert else expected_order(name))
    dx = eng.solve(invert)
    step = float(np.abs(dx[d:] - dxo[d:]).max() / np.abs(dxo[d:]).max())
    mult = float(np.abs(dx[:d] - dxo[:d]).max()) if d else 0.0
    print(f"{name} invert {invert}: order {order}, step vs oracle {step:.2e}, multipliers |diff| {mult:.2e} (max {np.abs(dxo[:d]).max() if d else 0.0:.2e})")
    np.testing.assert_allclose(dx[d:], dxo[d:], rtol=0, atol=1e-9 * np.abs(dxo[d:]).max())
    if d:
        np.testing.assert_allclose(dx[:d], dxo[:d], rtol=0, atol=1e-6 * np.abs(dxo[:d]).max() + 1e-12)
    om_o = o.omega(fp.values, s2, dxo)
    assert abs(eng.omega(s2, dxo) - om_o) <= 1e-10 * om_o
    if invert:
        Q = packed_to_full(eng.get_cofactor(), U); Qref = packed_to_full(Qo, U)
        qerr = float((np.abs(Q - Qref)[d:, d:] / correlation_scale(Qref)[d:, d:]).max())
        print(f"{name}: Q vs oracle {qerr:.2e} (correlation scale), {np.abs(Q - Qref).max() / np.abs(Qref).max():.2e} of max|Q| with the border")
        assert qerr < 1e-9
        np.testing.assert_allclose(np.diag(Q)[d:], np.diag(Qref)[d:], rtol=1e-9)
        assert np.abs(Q - Qref).max() <= 1e-9 * np.abs(Qref).max()
        idx = np.array([d, d + 3, U - 1, d + 1], np.int32)
        np.testing.assert_array_equal(eng.get_cofactor_sub(idx), Q[np.ix_(idx, idx)])
        np.testing.assert_array_equal(eng.get_dispersion_sub(0.37, idx), 0.37 * Q[np.ix_(idx, idx)])
    eng.close()


# ---- exact solution of the assembled system --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chains", ["default", "polling_wave_from_one_block_column"])
@pytest.mark.parametrize("name", S.NAMES)
def test_refined_step_is_the_exact_solution_at_every_defect(name, chains, monkeypatch):
    """test_gpu_refinement.test_refined_step_is_the_exact_solution_of_the_assembled_system on the table: refinement -1, 0 and 2, both
    settings of the one-right-hand-side chains, the refined step < 2e-13 from the long-double-refined solution of the device's own
    bordered system, the multipliers < 1e-13 of max|f|."""
    import oracle
    if chains != "default":
        monkeypatch.setenv("JAICOV_CHAIN8_MIN_NB", "1")
    fp = S.get_scene(name)
    s2, U, d = fp.sigma2apriori, fp.n_unknowns, fp.rank_defect
    out = {}
    for refinement in (-1, 0, 2):
        eng = engine.Engine(fp, refinement=refinement)
        eng.set_parameters(fp.values)
        eng.build(s2, 0.0)
        N, n = eng.get_normal()
        order = eng.reduced_order()
        dx = eng.solve(False)
        eng.close()
        assert order == expected_order(name)
        K, f = bordered(fp, oracle, N, n, order)
        z = exact_solution(K, f)
        out[refinement] = (rel(dx[d:order], z[d:order]), float(np.abs(dx[:d] - z[:d]).max() / np.abs(f).max()) if d else 0.0)
    print(f"{name} {chains}: U = {U}, order = {order}: unrefined {out[-1][0]:.2e}, one step {out[0][0]:.2e}, two steps {out[2][0]:.2e}"
          f"; multipliers {out[-1][1]:.2e} -> {out[0][1]:.2e} -> {out[2][1]:.2e}")
    assert out[0][0] < 2e-13 and out[2][0] < 2e-13
    assert out[0][0] <= max(out[-1][0], 2e-15)
    if d:
        assert out[0][1] < 1e-13 and out[2][1] < 1e-13


# ---- the three inversion modes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BLOCK_147)
def test_inversion_modes_at_defects_1_4_7(name):
    """test_gpu_parity.test_reduced_inverse_is_the_block_of_the_full_cofactor: REDUCED is the leading block of the oracle's full
    cofactor matrix (at d = 1 there is no pre-elimination and REDUCED is served with all of Qxx); FULL_EXPANDED equals FULL within
    1e-9 entrywise (test_gpu_refinement.test_full_cofactor_expanded_from_the_reduced_inverse)."""
    fp = S.get_scene(name)
    U, d = fp.n_unknowns, fp.rank_defect
    dxo, Qo, _, _ = oracle_pass(name, 0.0)
    Qfull = packed_to_full(Qo, U)
    eng = one_pass(fp, engine.INVERT_REDUCED)
    e0 = eng.reduced_order()
    assert e0 == expected_order(name)
    dx = eng.solve(engine.INVERT_REDUCED)
    np.testing.assert_allclose(dx[d:], dxo[d:], rtol=0, atol=1e-9 * np.abs(dxo[d:]).max())
    assert eng.cofactor_order() == e0
    Q = packed_to_full(eng.get_cofactor(), e0)
    Qref = Qfull[:e0, :e0]
    sc = correlation_scale(Qref)
    r_err = float((np.abs(Q - Qref)[d:, d:] / sc[d:, d:]).max())
    assert r_err < 1e-9
    assert np.abs(Q - Qref).max() <= 1e-9 * np.abs(Qref).max()
    idx = np.array([d, d + 3, e0 - 1, d + 1], np.int32)
    np.testing.assert_array_equal(eng.get_cofactor_sub(idx), Q[np.ix_(idx, idx)])
    # FULL
    eng.prepare_inverse(engine.INVERT_FULL); eng.build(fp.sigma2apriori, 0.0); eng.solve(engine.INVERT_FULL)
    assert eng.cofactor_order() == U and eng.reduced_order() == U
    Qf = packed_to_full(eng.get_cofactor(), U)
    scf = correlation_scale(Qfull)
    assert (np.abs(Qf[:e0, :e0] - Q)[d:, d:] / sc[d:, d:]).max() < 1e-9
    # FULL_EXPANDED: from the reduced system where there is one
    eng.prepare_inverse(engine.INVERT_FULL_EXPANDED); eng.build(fp.sigma2apriori, 0.0)
    assert eng.reduced_order() == e0
    dxe = eng.solve(engine.INVERT_FULL_EXPANDED)
    np.testing.assert_allclose(dxe[d:], dxo[d:], rtol=0, atol=1e-9 * np.abs(dxo[d:]).max())
    assert eng.cofactor_order() == U
    Qe = packed_to_full(eng.get_cofactor(), U)
    x_err = float((np.abs(Qe - Qf)[d:, d:] / scf[d:, d:]).max())
    x_oracle = float((np.abs(Qe - Qfull)[d:, d:] / scf[d:, d:]).max())
    x_border = float(np.abs(Qe - Qf).max() / np.abs(Qf).max())
    print(f"{name}: order {e0}: REDUCED vs oracle {r_err:.2e}; FULL_EXPANDED vs FULL {x_err:.2e} (with the border {x_border:.2e} of max|Q|), vs oracle {x_oracle:.2e}")
    assert x_err < 1e-9 and x_oracle < 1e-9
    assert x_border <= 1e-8                               # border rows (the multipliers' cofactors) included: the bound of the test followed
    if e0 < U:
        idx = np.array([d, e0 - 1, e0, e0 + 7, U - 1, e0 + 6], np.int32)
    np.testing.assert_array_equal(eng.get_cofactor_sub(idx), Qe[np.ix_(idx, idx)])
    eng.close()


# ---- damping with a border ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["diag_d1", "diag_d7", "block_d1", "block_d7"])
def test_damped_default_path_matches_full_solve(name):
    """test_gpu_parity.test_eo_pre_elimination_matches_full_solve at lambda = 0.5 with a border of 1 and of 7 rows: the default path
    gives the oracle's full bordered solve, exterior orientations included, and so does the full-order build.
    Of the four scenes ONLY block_d7 is on the EO-reduced path (the damping of the UNREDUCED diagonal goes through the elimination
    with seven border rows beside it).  diag_d1, diag_d7 and block_d1 are full order by default, so there both halves factor the
    full damped system: they hold damping with a border of 1 and of 7 rows, not the reduced path.  d = 1 never reaches a reduced
    system: its recipe fixes the angles of an image, which rules the elimination out (create_plan.h, eo_columns_trailing).  Damping
    inside a reduced system at other d: test_forced_elimination_of_ordinary_images_with_a_border (d = 3, 4, 5, 7)."""
    import oracle
    fp = S.get_scene(name)
    U, d, s2, lam = fp.n_unknowns, fp.rank_defect, fp.sigma2apriori, 0.5
    dxo = oracle_pass(name, lam)[0]
    o = oracle.Oracle(fp)
    eng = engine.Engine(fp)
    eng.set_parameters(fp.values)
    eng.build(s2, lam)
    assert eng.reduced_order() == expected_order(name)
    dx = eng.solve(False)
    tol_m = 1e-6 * np.abs(dxo[:d]).max() + 1e-12
    err = float(np.abs(dx[d:] - dxo[d:]).max() / np.abs(dxo[d:]).max())
    np.testing.assert_allclose(dx[d:], dxo[d:], rtol=0, atol=1e-9 * np.abs(dxo[d:]).max())
    np.testing.assert_allclose(dx[:d], dxo[:d], rtol=0, atol=tol_m)
    om_o = o.omega(fp.values, s2, dxo)
    assert abs(eng.omega(s2, dx) - om_o) <= 1e-9 * om_o
    if eng.reduced_order() < U:
        with pytest.raises(engine.EngineError):
            eng.build(s2, lam); eng.solve(True)          # inverse needs the full system: prepare_inverse first
    eng.prepare_inverse(True); eng.build(s2, lam)
    assert eng.reduced_order() == U
    dxf = eng.solve(True)
    errf = float(np.abs(dxf[d:] - dxo[d:]).max() / np.abs(dxo[d:]).max())
    print(f"{name} lambda {lam}: default path (order {expected_order(name)}) {err:.2e}, full order {errf:.2e}")
    np.testing.assert_allclose(dxf[d:], dxo[d:], rtol=0, atol=1e-9 * np.abs(dxo[d:]).max())
    np.testing.assert_allclose(dxf[:d], dxo[:d], rtol=0, atol=tol_m)
    eng.close()


@pytest.mark.parametrize("name", ["diag_d3", "diag_d4", "diag_d5", "diag_d7"])
def test_forced_elimination_of_ordinary_images_with_a_border(name):
    """The diag scenes keep the full order by default; ordinary_group_elimination = 1 serves their images as blocks with a
    block-diagonal weight and eliminates the exterior orientations (tests/test_gpu_ordinary_elimination.py, which runs d = 0 and 6):
    the border of 3, 4, 5 and 7 rows inside that reduced system, undamped and damped, against the oracle's full bordered solve."""
    fp = S.get_scene(name)
    U, d, s2 = fp.n_unknowns, fp.rank_defect, fp.sigma2apriori
    for lam in (0.0, 0.5):
        dxo = oracle_pass(name, lam)[0]
        eng = engine.Engine(fp, ordinary_group_elimination=1)
        eng.set_parameters(fp.values)
        eng.build(s2, lam)
        assert eng.reduced_order() == U - 6 * fp.n_images
        dx = eng.solve(False)
        eng.close()
        print(f"{name} lambda {lam}: order {U - 6 * fp.n_images}, step vs oracle {np.abs(dx[d:] - dxo[d:]).max() / np.abs(dxo[d:]).max():.2e}")
        np.testing.assert_allclose(dx[d:], dxo[d:], rtol=0, atol=1e-9 * np.abs(dxo[d:]).max())
        np.testing.assert_allclose(dx[:d], dxo[:d], rtol=0, atol=1e-6 * np.abs(dxo[:d]).max() + 1e-12)


# ---- the whole loop ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["diag_d7", "block_d7", "block_d4"])
def test_estimate_matches_oracle_at_defects_7_and_4(name):
    """test_gpu_parity.test_estimate_matches_oracle: the same number of passes as the reference's loop, the parameters within 1e-9
    and the variance factor a posteriori Omega / f within 1e-11 relative (Omega is stationary at the solution: a parameter error
    of 1e-9 moves it in second order only).  A block case takes about 5 s, nearly all of it the seven passes of the oracle's loop
    (literal stacking of the dense dispersions); the diag case takes a moment."""
    import oracle
    fp = S.get_scene(name)
    vo, Qo, ro = oracle.Oracle(fp).estimate()
    eng = engine.Engine(fp)
    v, r = eng.estimate()
    assert r.state == ro.state == 1
    f = fp.degree_of_freedom
    perr = float((np.abs(v - vo) / np.maximum(np.abs(vo), 1e-3)).max())
    serr = abs(r.omega / f - ro.omega / f) / (ro.omega / f)
    U, d = fp.n_unknowns, fp.rank_defect
    Q = packed_to_full(eng.get_cofactor(), U); Qref = packed_to_full(Qo, U)
    qerr = float(np.abs(np.diag(Q)[d:] / np.diag(Qref)[d:] - 1.0).max())
    print(f"{name}: {r.iterations} passes (oracle {ro.iterations}), parameters {perr:.2e}, sigma0^2 {serr:.2e}, diag Q {qerr:.2e}")
    assert r.iterations == ro.iterations
    assert perr < 1e-9
    assert serr <= 1e-11
    assert qerr < 1e-8                                   # the bound of the test this one follows
    eng.close()


# ---- two shards ------------------------------------------------------------------------------------------------------------------------
def test_two_shards_sum_to_the_unsharded_system_at_defect_7():
    """test_gpu_parity.test_sharded_engines_sum_to_full on block_d7 (full-order path: N and n of the two shards add up to the
    unsharded accumulation), and the step as test_sharded_reduce_buffers_with_damping forms it (default path: the reduce buffers
    summed, every shard finalises the seven border rows and solves)."""
    import torch
    from bundle_adjustment_amd.distributed import DeviceArray
    name = "block_d7"
    fp = S.get_scene(name)
    s2, U, d = fp.sigma2apriori, fp.n_unknowns, fp.rank_defect
    h = fp.n_images // 2
    full = engine.Engine(fp); full.set_parameters(fp.values); full.prepare_inverse(True); full.accumulate(s2); N, n = full.get_normal()
    a = engine.Engine(fp, image_range=(0, h), apply_shared=True)
    b = engine.Engine(fp, image_range=(h, fp.n_images), apply_shared=False)
    for e_ in (a, b):
        e_.set_parameters(fp.values); e_.prepare_inverse(True); e_.accumulate(s2)
    Na, na = a.get_normal(); Nb, nb = b.get_normal()
    assert np.abs(N).max() > 0
    np.testing.assert_allclose(Na + Nb, N, rtol=1e-12, atol=1e-13 * np.abs(N).max())
    np.testing.assert_allclose(na + nb, n, rtol=1e-12, atol=1e-13 * np.abs(n).max())
    # the step: unsharded, default (EO-reduced) path
    full.prepare_inverse(engine.INVERT_NONE); full.build(s2, 0.0)
    e0 = full.reduced_order()
    assert e0 == U - 6 * fp.n_images
    dx_full = full.solve(False)
    dxo = oracle_pass(name, 0.0)[0]
    bufs = []
    for e_ in (a, b):
        e_.prepare_inverse(engine.INVERT_NONE)
        e_.accumulate(s2, 0.0)
        ptr, cnt = e_.reduce_buffer()
        bufs.append(torch.as_tensor(DeviceArray(ptr, cnt), device="cuda:0"))
    assert a.reduced_order() == e0 and bufs[0].numel() == e0 * (e0 + 1) // 2 + 2 * e0
    total = bufs[0] + bufs[1]
    bufs[0].copy_(total); bufs[1].copy_(total)
    torch.cuda.synchronize()
    dx = np.zeros(U)
    for e_ in (a, b):
        e_.finalize(s2, 0.0)
        part = e_.solve(False)
        np.testing.assert_allclose(part[d:e0], dx_full[d:e0], rtol=0, atol=1e-9 * np.abs(dx_full[d:]).max())
        dx[:e0] = part[:e0]
        dx[e0:] += part[e0:]
    print(f"{name}: shards vs unsharded step {np.abs(dx - dx_full)[d:].max() / np.abs(dx_full[d:]).max():.2e}, "
          f"vs oracle {np.abs(dx - dxo)[d:].max() / np.abs(dxo[d:]).max():.2e}")
    np.testing.assert_allclose(dx[d:], dx_full[d:], rtol=0, atol=1e-9 * np.abs(dx_full[d:]).max())
    np.testing.assert_allclose(dx[d:], dxo[d:], rtol=0, atol=1e-9 * np.abs(dxo[d:]).max())
    for e_ in (full, a, b):
        e_.close()


# ---- what consumes the border downstream ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DOWNSTREAM)
def test_redundancy_numbers_sum_to_the_degree_of_freedom_at_defects_7_and_4(name):
    """test_gpu_reliability.test_redundancy_numbers_sum_to_the_degree_of_freedom: f = n - u + d counts the border."""
    from test_gpu_reliability import check_bounds, inverting_pass
    fp = S.get_scene(name)
    eng, dx = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    res = eng.reliability(fp.sigma2apriori, dx)
    f = fp.degree_of_freedom
    print(f"{name}: sum r = {res.r.sum():.9f}, f = {f}")
    assert abs(res.r.sum() - f) <= 1e-8 * f, (res.r.sum(), f)
    check_bounds(fp, res)
    s = eng.reliability_summary()
    assert s[5] == 0.0
    assert s[0] == pytest.approx(res.r.sum(), rel=1e-12, abs=1e-9)
    assert s[4] == res.r.min()
    assert s[3] == np.isnan(res.t).sum()
    fin = np.flatnonzero(~np.isnan(res.t))
    assert s[1] == np.abs(res.t[fin]).max() and int(s[2]) == fin[np.argmax(np.abs(res.t[fin]))]
    eng.close()


def new_datum_mask(name):
    """block_d7: every second point from 0.  block_d4: every second point from 1 -- the fixed point 3 is flagged and must be passed
    over (BA:506), as the oracle passes it over."""
    fp = S.get_scene(name)
    m = np.zeros(fp.n_points, np.uint8)
    m[(1 if name == "block_d4" else 0)::2] = 1
    return m


@pytest.mark.parametrize("name", DOWNSTREAM)
def test_datum_transformation_at_defects_7_and_4(name):
    """The two checks of tests/test_gpu_datum.py on one subset of the points: the transformed matrix is the oracle's inverse in the
    new datum (1e-9 of max|Q_B|), and the new datum rows annihilate it (B' Q' = 0 to 16 times numpy's figure, B' Z = I, zero border
    block) -- with the SCALE row among them."""
    import oracle
    from test_gpu_datum import cofactor, inverting_pass, margin, oracle_inverse
    fp = S.get_scene(name)
    d = fp.rank_defect
    mask_b = new_datum_mask(name)
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    k = eng.cofactor_order()
    assert k == fp.n_unknowns
    QA = cofactor(eng)
    eng.datum_transform(mask_b)
    assert eng.cofactor_order() == k
    Q = cofactor(eng)
    QB, B = oracle_inverse(oracle, fp, mask_b)
    err = np.abs(Q - QB).max() / np.abs(QB).max()
    Qnp = datum_reference.transform(QA, B, d)
    qmax = np.abs(QA).max()
    r_dev = np.abs(B[:, d:] @ Q[d:, d:]).max()
    r_np = np.abs(B[:, d:] @ Qnp[d:, d:]).max()
    print(f"{name}: transformed vs the oracle's inverse in the new datum {err:.3e} of max|Q_B|; |B'Q'| device {r_dev:.3e}, numpy {r_np:.3e}, max|Q| {qmax:.3e}")
    assert np.abs(Q - QA).max() > 1e-6 * qmax                     # the datum did change
    assert err <= 1e-9
    idx = np.array([d, d + 4, k - 1, d + 1], np.int32)
    np.testing.assert_array_equal(eng.get_cofactor_sub(idx), Q[np.ix_(idx, idx)])
    np.testing.assert_array_equal(eng.get_dispersion_sub(0.37, idx), 0.37 * Q[np.ix_(idx, idx)])
    assert r_dev <= margin(r_dev, r_np, qmax)
    assert np.abs(B[:, d:] @ Q[d:, :d] - np.eye(d)).max() <= 1e-12
    assert np.all(Q[:d, :d] == 0)
    eng.close()


@pytest.mark.parametrize("name", DOWNSTREAM)
def test_point_precision_follows_a_datum_transformation_at_defects_7_and_4(name):
    """test_gpu_precision.test_every_call_follows_a_datum_transformation: after the transformation the figures of the points are
    those of the exported (transformed) matrix; at d = 4 the fixed point 3 gives zero axes."""
    from test_gpu_precision import K2, K3, S2, assert_worst, check_blocks, exported, inverting_pass
    fp = S.get_scene(name)
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    Q0 = exported(eng)
    before = eng.precision_points(S2, K3, K2)
    eng.datum_transform(new_datum_mask(name))
    Q = exported(eng)
    assert np.abs(Q - Q0).max() > 1e-6 * np.abs(Q0).max()
    pcol, ecol = np.asarray(fp.point_col).reshape(-1, 3), np.asarray(fp.eo_col).reshape(-1, 6)
    pts = eng.precision_points(S2, K3, K2)
    assert np.abs(pts.helmert - before.helmert).max() > 1e-3 * before.helmert.max()
    assert_worst(f"{name} after the transformation, points", check_blocks(pts, Q, pcol))
    assert_worst(f"{name} after the transformation, stations", check_blocks(eng.precision_stations(S2, K3, K2), Q, ecol[:, :3], ecol[:, 3:]))
    if name == "block_d4":
        assert pts.status[3] == engine.PREC_PARTIAL and not pts.semi_axes[3].any() and int((pts.status != 0).sum()) == 1
    else:
        assert not pts.status.any()
    eng.close()
