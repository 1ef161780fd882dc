"""Variance components of observation groups on the device (include/jaicov_vce.h, csrc/vce.hip).

The reference (tests/vce_reference.py, longdouble sums) is evaluated on the device's own v and r (jaicov_rel_get after the run) and
on the weights the device holds (get_block_weight), so that only the rounding of the sums separates the two:
|dOmega_g| <= 4 n_max 2^-53 S_g and |dr_g| <= 4 n_g 2^-53 R_g with n_max the rows of the largest weight block.  Largest ratios to these
bounds seen on an MI355X are in DESIGN.md 6p."""
import ctypes as C
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import helpers
import vce_reference as R
from bundle_adjustment_amd import engine, scene

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
BAD_ARGUMENT, BAD_STATE = -1, -2


def block_scene():
    return scene.make_scene(6, 120, 90, weights="block", control_dense=True)


SCENES = {
    "tiny": lambda: scene.config("tiny"),
    "tiny_block": lambda: scene.config("tiny_block"),
    "tiny_free": lambda: scene.config("tiny_free"),
    "block180": block_scene,
    "mixed": helpers.mixed_scene,
    "ragged": helpers.ragged_scene,
    "two_camera": lambda: helpers.two_camera_scene()[0],
    "cfg2": lambda: scene.config("cfg2"),
}


def inverting_pass(fp, invert=engine.INVERT_FULL, **kw):
    """build (lambda = 0) + inverting solve; returns the engine and the step (not applied)."""
    eng = engine.Engine(fp, device=0, **kw)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(invert)
    eng.build(fp.sigma2apriori, 0.0)
    dx = eng.solve(invert)
    return eng, dx


def groupings(fp, name):
    ones = lambda n, v=0: np.full(n, v, np.int32)
    out = {
        "kind": engine.vce_groups(fp, "kind"),
        "image": engine.vce_groups(fp, "image"),
        "all": engine.VceGroups(ones(fp.n_image_points), ones(fp.n_scale_bars), ones(fp.n_direct_groups), 1, None),
        # the images with an odd index, the scale bars and nothing else at -1; group 2 stays empty
        "partial": engine.VceGroups(np.where(fp.ip_image % 2 == 0, 1, -1).astype(np.int32), None, ones(fp.n_direct_groups), 3, None),
    }
    if name == "two_camera":
        out["camera"] = engine.vce_groups(fp, "camera")
    return out


class Truth:
    """blocks and the device's weights of a scene, formed once"""

    def __init__(self, eng, fp):
        self.fp, self.s0 = fp, fp.sigma2apriori
        self.blocks = R.weight_blocks(fp)
        self.P = R.block_weights(self.blocks, self.s0, eng)
        self.n_max = max(b.rows.size for b in self.blocks)

    def check(self, eng, groups, dx):
        """the table against the reference on the device's v, r; returns the largest ratios to the two bounds"""
        vc = eng.variance_components(groups, dx=dx)
        rel = eng.variance_components_reliability()
        ref = R.components(self.fp, groups, rel.v, rel.r, self.blocks, self.P, self.s0)
        np.testing.assert_array_equal(vc.n, ref.table[0])
        b_om = 4 * self.n_max * EPS * ref.S
        b_r = 4 * ref.table[0] * EPS * ref.R
        d_om, d_r = np.abs(vc.omega - ref.table[1]), np.abs(vc.r - ref.table[2])
        some = ref.table[0] > 0
        ratios = (float(np.max(d_om[some] / b_om[some], initial=0.0)), float(np.max(d_r[some] / b_r[some], initial=0.0)))
        print("ratios to the bounds (Omega, r):", ratios)
        assert np.all(d_om <= b_om), ratios
        assert np.all(d_r <= b_r), ratios
        np.testing.assert_array_equal(vc.status, ref.status)
        # the derived columns are exact functions of the device's own Omega_g and r_g
        for g in range(groups.n_groups):
            st, s2, k, sd = R.derived(vc.n[g], vc.omega[g], vc.r[g], self.s0)
            assert st == vc.status[g]
            np.testing.assert_array_equal(np.array([vc.s2[g], vc.k[g], vc.sd[g]]), np.array([s2, k, sd]))
        np.testing.assert_array_equal(np.isnan(vc.table), np.isnan(ref.table))
        # the totals: all rows, grouped or not
        s = vc.summary
        assert abs(s.omega - ref.omega_total) <= 4 * self.n_max * EPS * ref.S_total
        assert abs(s.sum_r - ref.r_total) <= 4 * self.fp.n_observations * EPS * ref.R_total
        assert s.rows_grouped == ref.table[0].sum() and s.rows_grouped + s.rows_ungrouped == self.fp.n_observations
        assert s.damping == 0.0
        return vc, ref, ratios


# ---- 1. against the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_matches_the_reference(name):
    fp = SCENES[name]()
    eng, dx = inverting_pass(fp)
    truth = Truth(eng, fp)
    worst = [0.0, 0.0]
    for gname, groups in groupings(fp, name).items():
        for step in (None, dx):
            vc, ref, ratios = truth.check(eng, groups, step)
            worst = [max(a, b) for a, b in zip(worst, ratios)]
            if gname == "partial":
                assert vc.status[2] == engine.VCE_EMPTY and vc.n[2] == 0 and np.all(np.isnan(vc.table[3:, 2]))
    print(name, "largest ratios to the bounds (Omega, r):", worst)
    if name == "tiny_free":                               # the single scale bar is a group of one row
        vc = eng.variance_components(engine.vce_groups(fp, "kind"))
        assert fp.n_scale_bars == 1 and vc.n[1] == 1
        # ... and the only source of scale of this free network: nothing controls it, r = 0 up to rounding
        assert abs(vc.r[1]) <= 1e-6 and vc.r[1] <= 1e-10 and vc.status[1] == engine.VCE_UNCONTROLLED and np.all(np.isnan(vc.table[3:, 1]))
    if name == "ragged":
        assert 6 in {b.rows.size for b in truth.blocks}   # a dense block smaller than a wave
    eng.close()


# ---- 2. invariants ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "tiny_free", "block180", "mixed", "cfg2"])
def test_complete_groupings_sum_to_omega_and_to_the_redundancy(name):
    fp = SCENES[name]()
    eng, dx = inverting_pass(fp)
    truth = Truth(eng, fp)
    n, s0 = fp.n_observations, fp.sigma2apriori
    for gname in ("kind", "image_and_rest"):
        groups = engine.vce_groups(fp, "kind")
        if gname == "image_and_rest":                     # every image a group, scale bars and direct rows two more
            I = fp.n_images
            groups = engine.VceGroups(fp.ip_image.astype(np.int32), np.full(fp.n_scale_bars, I, np.int32),
                                      np.full(fp.n_direct_groups, I + 1, np.int32), I + 2, None)
        for step in (None, dx):
            vc, ref, _ = truth.check(eng, groups, step)
            omega = eng.omega(s0, np.zeros(max(fp.n_unknowns, 1)) if step is None else step)
            sum_r = eng.reliability_summary()[0]
            d_om, b_om = abs(vc.omega.sum() - omega), 8 * n * EPS * ref.S.sum()
            d_r, b_r = abs(vc.r.sum() - sum_r), 8 * n * EPS * ref.R.sum()
            print(name, gname, "dx" if step is not None else "zero", "ratios to the bounds (Omega, sum r):", d_om / b_om, d_r / b_r)
            assert d_om <= b_om, (vc.omega.sum(), omega, d_om / b_om)
            assert d_r <= b_r, (vc.r.sum(), sum_r, d_r / b_r)
            f = fp.degree_of_freedom
            assert abs(vc.summary.sum_r - f) <= 1e-8 * f
    eng.close()


# ---- 3. chunked staging -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage", [64, 50, 1])
def test_staging_in_chunks_matches_the_single_stage(stage, monkeypatch):
    """JAICOV_VCE_STAGE lowers the residuals staged at a time: 2m = 180 runs 3, 4 and 180 stages."""
    fp = block_scene()
    eng, dx = inverting_pass(fp)
    truth = Truth(eng, fp)
    groups = engine.vce_groups(fp, "image")
    one, ref, _ = truth.check(eng, groups, dx)
    monkeypatch.setenv("JAICOV_VCE_STAGE", str(stage))
    many, _, _ = truth.check(eng, groups, dx)
    assert np.all(np.abs(many.omega - one.omega) <= 4 * truth.n_max * EPS * ref.S)
    np.testing.assert_array_equal(many.r, one.r)
    np.testing.assert_array_equal(many.n, one.n)
    eng.close()


# ---- 4. reproducibility -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "cfg2"])
def test_bits_repeat_permute_and_do_not_depend_on_the_other_groups(name):
    fp = SCENES[name]()
    eng, dx = inverting_pass(fp)
    groups = engine.VceGroups(fp.ip_image.astype(np.int32), None, np.full(fp.n_direct_groups, fp.n_images, np.int32), fp.n_images + 1, None)
    a = eng.variance_components(groups, dx=dx)
    b = eng.variance_components(groups, dx=dx)
    assert a.table.tobytes() == b.table.tobytes() and np.array_equal(a.status, b.status)
    perm = np.random.default_rng(5).permutation(groups.n_groups).astype(np.int32)      # old id -> new id
    c = eng.variance_components(groups._replace(ip=perm[groups.ip], dg=perm[groups.dg]), dx=dx)
    assert c.table[:, perm].tobytes() == a.table.tobytes() and np.array_equal(c.status[perm], a.status)
    keep = 3
    alone = eng.variance_components(groups._replace(ip=np.where(groups.ip == keep, keep, -1).astype(np.int32), dg=None), dx=dx)
    assert alone.table[:, keep].tobytes() == a.table[:, keep].tobytes()
    assert alone.summary.omega == a.summary.omega and alone.summary.sum_r == a.summary.sum_r
    assert alone.summary.rows_ungrouped == fp.n_observations - a.n[keep]
    eng.close()


# ---- 5. recovery of known factors -------------------------------------------------------------------------------------------------
RECOVERY = {
    "diag": lambda: scene.make_scene(20, 200, 200, weights="diag"),
    "block180": block_scene,
}


@pytest.mark.parametrize("name", list(RECOVERY))
def test_the_iteration_recovers_known_factors(name):
    """tests/test_vce_reference.py runs the same scenes on the CPU: both image groups have r_g >= 200 there."""
    fp, g = R.misstated(RECOVERY[name]())
    est = engine.estimate_variance_components(fp, engine.VceGroups(*g), tol=0.05, max_iter=10)
    K, r = est.factors, est.tables[-1].r
    print(name, "iterations", len(est.tables), "K", K, "K c", K * np.array(R.MISSTATED), "r", r)
    assert est.converged, [t.k for t in est.tables]
    assert r[0] >= 200 and r[1] >= 200, r
    for i in range(3):
        if r[i] >= 200:
            assert abs(K[i] * R.MISSTATED[i] - 1.0) <= 5.0 * np.sqrt(2.0 / r[i]), (i, K[i], r[i])
    # the engine returned is the last one, built from the problem returned
    again = est.engine.variance_components(engine.VceGroups(*g))
    assert again.table.tobytes() == est.tables[-1].table.tobytes()
    est.engine.close()


# ---- 6. states and arguments ------------------------------------------------------------------------------------------------------
def code_of(call):
    with pytest.raises(engine.EngineError) as err:
        call()
    return err.value.code, str(err.value)


def test_states_are_refused():
    fp = scene.config("tiny_block")       # every image a dense block: REDUCED eliminates the exterior orientations, the matrix is not all of Qxx
    groups = engine.vce_groups(fp, "kind")
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    assert code_of(lambda: eng.variance_components(groups))[0] == BAD_STATE       # before any inverting solve
    eng.prepare_inverse(engine.INVERT_REDUCED)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(engine.INVERT_REDUCED)
    assert eng.cofactor_order() == fp.n_unknowns - 6 * fp.n_images
    assert code_of(lambda: eng.variance_components(groups))[0] == BAD_STATE       # not all of Qxx
    table = np.zeros((engine.VCE_COLUMNS, 3)); status = np.zeros(3, np.int32)
    assert eng.L.jaicov_vce_get(eng._h, engine._p(table), status.ctypes.data_as(engine._pi), 3) == BAD_STATE
    eng.close()


def test_arguments_are_refused_and_the_previous_result_stays():
    fp = scene.config("tiny_block")
    eng, dx = inverting_pass(fp)
    groups = engine.vce_groups(fp, "kind")
    good = eng.variance_components(groups, dx=dx)
    rel = eng.variance_components_reliability()
    ip = groups.ip.copy()
    bad_high = groups._replace(ip=np.full(ip.size, 3, np.int32))
    bad_low = groups._replace(sb=None, dg=np.full(fp.n_direct_groups, -2, np.int32))
    split_all = groups._replace(ip=(np.arange(ip.size) % 2).astype(np.int32))
    first_of_3 = ip.copy(); first_of_3[fp.blk_ip_begin[3]] = 1
    split_3 = groups._replace(ip=first_of_3)
    for call, text in ((lambda: eng.variance_components(bad_high), "group id"),
                       (lambda: eng.variance_components(bad_low), "group id"),
                       (lambda: eng.variance_components(groups._replace(n_groups=0)), "n_groups"),
                       (lambda: eng.variance_components(groups._replace(n_groups=-1)), "n_groups"),
                       (lambda: eng.variance_components(groups, sigma2_test=0.0), "sigma2_test"),
                       (lambda: eng.variance_components(groups, sigma2_test=-1.0), "sigma2_test"),
                       (lambda: eng.variance_components(split_all), "block 0"),
                       (lambda: eng.variance_components(split_3), "block 3")):
        code, msg = code_of(call)
        assert code == BAD_ARGUMENT and text in msg, (code, msg, text)
        # the previous results are readable and unchanged
        table = np.zeros((engine.VCE_COLUMNS, 3)); status = np.zeros(3, np.int32)
        eng._chk(eng.L.jaicov_vce_get(eng._h, engine._p(table), status.ctypes.data_as(engine._pi), 3))
        assert table.tobytes() == good.table.tobytes() and np.array_equal(status, good.status)
        assert eng.variance_components_reliability().v.tobytes() == rel.v.tobytes()
    # get with another n_groups
    table = np.zeros((engine.VCE_COLUMNS, 4)); status = np.zeros(4, np.int32)
    assert eng.L.jaicov_vce_get(eng._h, engine._p(table), status.ctypes.data_as(engine._pi), 4) == BAD_ARGUMENT
    summ = np.zeros(5)
    assert eng.L.jaicov_vce_summary(eng._h, engine._p(summ), 4) == BAD_ARGUMENT
    # release is idempotent and takes the result away, not the reliability result
    eng.variance_components_release()
    eng.variance_components_release()
    assert eng.L.jaicov_vce_get(eng._h, engine._p(table), status.ctypes.data_as(engine._pi), 3) == BAD_STATE
    assert eng.variance_components_reliability().v.tobytes() == rel.v.tobytes()
    again = eng.variance_components(groups, dx=dx)
    assert again.table.tobytes() == good.table.tobytes()
    eng.close()


def test_an_empty_group_and_a_fixed_directly_observed_parameter():
    base = scene.config("tiny")
    c_slot = base.slot_io(0) + 2                           # the principal distance, fixed and directly observed: a zero row of A
    m = base.n_direct_rows
    fp = helpers.renumber(base, io_fixed=np.array([[False, False, True]]),
                          dg_slot=np.concatenate([base.dg_slot, [c_slot]]).astype(np.int32),
                          dg_row_begin=np.array([0, m, m + 1], np.int32), dg_obs=np.concatenate([base.dg_obs, [base.values[c_slot] + 0.002]]),
                          dg_var=np.concatenate([base.dg_var, [0.001 ** 2]]), dg_disp_offset=np.array([-1, -1], np.int64))
    eng, dx = inverting_pass(fp)
    groups = engine.VceGroups(None, None, np.array([0, 1], np.int32), 3, None)
    vc = eng.variance_components(groups, dx=dx)
    assert vc.n[1] == 1 and vc.r[1] == 1.0 and vc.status[1] == 0
    omega = fp.sigma2apriori / 0.001 ** 2 * 0.002 ** 2
    assert vc.omega[1] == pytest.approx(omega, rel=1e-9) and vc.k[1] == pytest.approx(omega / fp.sigma2apriori, rel=1e-9)
    assert vc.sd[1] == pytest.approx(vc.k[1] * np.sqrt(2.0), rel=1e-15)
    assert vc.status[2] == engine.VCE_EMPTY and vc.n[2] == 0 and vc.omega[2] == 0 and np.all(np.isnan(vc.table[3:, 2]))
    assert vc.summary.rows_grouped == m + 1 and vc.summary.rows_ungrouped == 2 * fp.n_image_points
    Truth(eng, fp).check(eng, groups, dx)
    eng.close()


# ---- 7. the C++ mirror and the example program ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example_base(tmp_path_factory):
    d = tmp_path_factory.mktemp("example")
    for f in ("ior", "eor", "obc", "scale"):
        shutil.copy(os.path.join(helpers.GOLDEN, "example", f"example.{f}"), d)
    with gzip.open(os.path.join(helpers.GOLDEN, "example", "example.phc.gz")) as src, open(d / "example.phc", "wb") as dst:
        dst.write(src.read())
    return str(d / "example")


def test_cpp_mirror_and_example_program(example_base):
    """varianceComponents through the pybind module returns the bits of the C calls on the mirror's own engine;
    host/example_variance_components adjusts the bundled block in a process of its own and is judged by its exit status (the groups
    by kind add up to the totals and to the degrees of freedom) and by its listing."""
    from bundle_adjustment_amd import host_api as H
    from test_host import example_adjustment
    host = os.path.join(os.path.dirname(os.path.dirname(helpers.GOLDEN)), "bundle-adjustment_amd", "host")
    if not os.path.exists(os.path.join(host, "example_variance_components")):
        subprocess.check_call(["make", "-C", host, "example_variance_components"], stdout=subprocess.DEVNULL)
    a = subprocess.run([os.path.join(host, "example_variance_components"), example_base], capture_output=True, text=True, timeout=600)
    print(a.stdout[-4000:])
    assert a.returncode == 0, (a.stdout[-2000:], a.stderr[-2000:])
    assert re.search(r"^image points\s+\d+", a.stdout, flags=re.M) and len(re.findall(r"^image \d+ ", a.stdout, flags=re.M)) == 10

    pr, ba = example_adjustment(H, example_base)
    assert ba.estimateModel() == H.EstimationStateType.ERROR_FREE_ESTIMATION, ba.lastError()
    n_ip = sum(len(im.coordinates()) for im in pr.camera.images())
    n_sb = len(pr.scaleBars())
    ip = np.zeros(n_ip, np.int32); sb = np.ones(n_sb, np.int32)
    tab, st, summ = ba.varianceComponents(ip.tolist(), sb.tolist(), [], 3, 0.0)
    L = engine.load_library()
    h = C.c_void_p(ba.nativeEngineHandle())
    assert L.jaicov_vce_run(h, ba.getVarianceFactorApriori(), None, ip.ctypes.data_as(engine._pi), sb.ctypes.data_as(engine._pi), None, 3, None) == 0
    t2 = np.zeros((engine.VCE_COLUMNS, 3)); s2 = np.zeros(3, np.int32); u2 = np.zeros(5)
    assert L.jaicov_vce_get(h, engine._p(t2), s2.ctypes.data_as(engine._pi), 3) == 0 and L.jaicov_vce_summary(h, engine._p(u2), 5) == 0
    assert tab.shape == (engine.VCE_COLUMNS, 3) and tab.tobytes() == t2.tobytes() and st.tobytes() == s2.tobytes() and summ.tobytes() == u2.tobytes()
    f = ba.getDegreeOfFreedom()
    assert st[0] == 0 and st[2] == engine.VCE_EMPTY and summ[3] == 0 and abs(summ[1] - f) <= 1e-6 * f
    assert tab[0, 0] == 2 * n_ip and tab[0, 1] == n_sb == 1
    # the block is a free network (d = 6) and its one scale bar the only source of scale: nothing controls it, r = 0 up to rounding
    assert abs(tab[2, 1]) <= 1e-6 and st[1] == engine.VCE_UNCONTROLLED and np.all(np.isnan(tab[3:, 1]))
    assert re.search(r"^scale bars\s+1\s+\S+\s+\S+\s+nan\s+nan\s+nan\s+2\s*$", a.stdout, flags=re.M)
    assert abs(tab[2, 0] - f) <= 1e-6 * f and np.all(np.isfinite(tab[3:, 0]))
