"""CPU: tests/vce_reference.py, the numpy restatement of include/jaicov_vce.h, held to the identities of the estimate without any
engine (the adjustment is the oracle's), and the iteration run on the scenes of tests/test_gpu_vce.py whose declared dispersions are
misstated by known factors: the inputs of the GPU test stay inside its statistical bound before the GPU is asked to."""
import numpy as np
import pytest

import vce_reference as R
from bundle_adjustment_amd import scene
from bundle_adjustment_amd.problem import scale_dispersions


def by_kind(fp):
    return R.Groups(np.zeros(fp.n_image_points, np.int32), np.full(fp.n_scale_bars, 1, np.int32), np.full(fp.n_direct_groups, 2, np.int32), 3, None)


@pytest.mark.parametrize("name,grouping", [("tiny_block", R.halves), ("tiny", R.halves), ("tiny_free", by_kind)])
def test_components_sum_to_omega_and_to_the_degree_of_freedom(oracle_mod, name, grouping):
    """Two image groups and the control group (by kind on the free network with its scale bar): a complete grouping."""
    fp = scene.config(name)
    groups = grouping(fp)
    comp, vals = R.cpu_components(oracle_mod, fp, groups)
    omega = oracle_mod.Oracle(fp).omega(vals, fp.sigma2apriori, np.zeros(fp.n_unknowns))
    assert abs(comp.table[1].sum() - omega) <= 1e-10 * omega, (comp.table[1].sum(), omega)
    assert abs(comp.table[1].sum() - comp.omega_total) <= 1e-10 * omega
    f = fp.degree_of_freedom                               # n - u + d
    assert abs(comp.table[2].sum() - f) <= 1e-10 * f, (comp.table[2].sum(), f)
    assert comp.table[0].sum() == fp.n_observations
    ok = comp.status == 0
    assert np.all(np.isfinite(comp.table[3:, ok])) and np.all(np.isnan(comp.table[3:, ~ok]))
    np.testing.assert_array_equal(comp.status[~ok], np.where(comp.table[0, ~ok] == 0, R.EMPTY, R.UNCONTROLLED))
    k = comp.table[4, ok]
    np.testing.assert_allclose(comp.table[3, ok], comp.table[1, ok] / comp.table[2, ok], rtol=1e-15)
    np.testing.assert_allclose(comp.table[5, ok], k * np.sqrt(2 / comp.table[2, ok]), rtol=1e-15)


def test_ungrouped_rows_leave_the_other_groups_alone(oracle_mod):
    fp = scene.config("tiny_block")
    full = R.halves(fp)
    part = full._replace(dg=None)
    a, _ = R.cpu_components(oracle_mod, fp, full)
    b, _ = R.cpu_components(oracle_mod, fp, part)
    np.testing.assert_array_equal(a.table[:, :2], b.table[:, :2])
    assert b.status[2] == R.EMPTY and np.all(np.isnan(b.table[3:, 2])) and b.table[0, 2] == 0
    assert a.omega_total == b.omega_total


def test_scale_dispersions_scales_what_it_says_and_nothing_else():
    fp = scene.make_scene(6, 40, 24, weights="block", n_control=4, control_dense=True, scale_bar=True)
    g = R.Groups((np.asarray(fp.ip_image) >= 3).astype(np.int32), np.full(1, 2, np.int32), np.full(1, 3, np.int32), 4, None)
    f = np.array([0.5, 3.0, np.nan, 7.0])
    out = scale_dispersions(fp, g, f)
    fi = f[g.ip]
    np.testing.assert_array_equal(out.ip_var_x, fp.ip_var_x * fi)
    np.testing.assert_array_equal(out.ip_var_y, fp.ip_var_y * fi)
    np.testing.assert_array_equal(out.ip_rho, fp.ip_rho)
    assert out.sigma2apriori == fp.sigma2apriori
    np.testing.assert_array_equal(out.sb_var, fp.sb_var)                   # a NaN factor keeps the group as it is
    np.testing.assert_array_equal(out.dg_var, 7.0 * fp.dg_var)
    np.testing.assert_array_equal(out.dg_disp, 7.0 * fp.dg_disp)
    for b in range(fp.n_image_blocks):
        lo, hi = int(fp.blk_disp_offset[b]), int(fp.blk_disp_offset[b]) + (2 * int(fp.blk_ip_begin[b + 1] - fp.blk_ip_begin[b])) ** 2
        np.testing.assert_array_equal(out.blk_disp[lo:hi], fp.blk_disp[lo:hi] * (0.5 if b < 3 else 3.0))
    np.testing.assert_array_equal(out.ip_x, fp.ip_x)
    split = g._replace(ip=np.arange(fp.n_image_points, dtype=np.int32) % 2)
    with pytest.raises(ValueError, match="block 0"):
        scale_dispersions(fp, split, f)


RECOVERY = {
    "diag": lambda: scene.make_scene(20, 200, 200, weights="diag"),
    "block180": lambda: scene.make_scene(6, 120, 90, weights="block", control_dense=True),
}


@pytest.mark.parametrize("name", list(RECOVERY))
def test_the_iteration_recovers_known_factors(oracle_mod, name):
    """Declared dispersions 1/4 and 2.25 times the true ones: the accumulated factors K must undo that within five standard
    deviations of chi^2_r / r, for every group with r_g >= 200; both image groups must be such groups."""
    fp, groups = R.misstated(RECOVERY[name]())
    K, tables, converged = R.cpu_estimate(oracle_mod, fp, groups, tol=0.05, max_iter=10)
    assert converged, [t.table[4] for t in tables]
    r = tables[-1].table[2]
    print(name, "iterations", len(tables), "K", K, "K c", K * np.array(R.MISSTATED), "r", r)
    assert r[0] >= 200 and r[1] >= 200, r
    for g in range(3):
        if r[g] >= 200:
            assert abs(K[g] * R.MISSTATED[g] - 1.0) <= 5.0 * np.sqrt(2.0 / r[g]), (g, K[g], r[g])
