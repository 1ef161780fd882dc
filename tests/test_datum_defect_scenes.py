"""CPU: the scene table of datum_defect_scenes.py and the reference on it, before the device is compared with either
(tests/test_gpu_datum_defects.py).

1. every recipe gives the stated defect and exactly the stated flags;
2. the oracle's step (packed Bunch-Kaufman on the preconditioned bordered system) is the exact solution of that system;
3. its cofactor matrix is the reflexive generalised inverse of N in the datum of the border: Q N Q = Q and B Q = 0;
4. its datum rows are BA:493-635, restated here in numpy: the SCALE row and the numbering of the rows with gaps included.

Bounds.  The device is held to 1e-9 of the oracle (step, Qxx) and to 2e-13 of the exact solution of its own system, so the oracle
has to sit well inside 1e-9 of what it stands for: 1e-11 for the step (set by the issue this table was written for; measured
<= 6e-13), 1e-10 for Q N Q = Q in the correlation scale of the Qxx asserts (a tenth of the device's bound; measured <= 2.2e-11,
on the block scenes at every d alike) and 1e-13 for B Q = 0 relative to max|Q| (B has unit rows; a thousand unit round-offs;
measured <= 3e-16).  Every figure is printed."""
import numpy as np
import pytest

import datum_defect_scenes as S
from bundle_adjustment_amd.problem import packed_to_full
from datum_reference import border_rows
from test_gpu_refinement import exact_solution


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------
def test_the_table_runs_every_defect_on_both_base_scenes():
    assert sorted(S.DEFECT[n] for n in S.NAMES if n.startswith("diag")) == list(range(8))
    assert sorted(S.DEFECT[n] for n in S.NAMES if n.startswith("block")) == list(range(8))
    assert S.NAMES == [f"{base}_d{d}" for base in S.BASES for d in S.DEFECTS] and list(S.EXPECTED_FLAGS) == S.NAMES
    for name in S.NAMES:                                          # the two literal tables and the table by conditions say the same
        assert S.EXPECTED_FLAGS[name] == S.FLAGS[S.DEFECT[name]]
    for d, f in S.FLAGS.items():
        assert bin(f).count("1") == d
    # the flag sets of d = 1 .. 5 leave gaps in TX .. SCALE, and SCALE occurs at d = 7, 4 and 1 only
    assert [d for d, f in S.FLAGS.items() if f & S.SCALE] == [7, 4, 1]
    assert all(not (S.FLAGS[d] & S.TX) for d in (5, 4, 3, 2, 1))


@pytest.mark.parametrize("name", S.NAMES)
def test_recipe_gives_the_stated_defect_and_flags(name):
    fp = S.get_scene(name)
    assert fp.rank_defect == S.DEFECT[name]
    assert fp.datum_flags == S.EXPECTED_FLAGS[name]
    assert fp.n_unknowns <= 240                                   # small: every GPU case takes a moment
    assert S.get_scene(name) is fp                                # cached
    # the angles fixed at d = 1, 2 take the exterior orientations out of the trailing 6 I columns
    assert S.eo_columns_are_trailing(fp) == (S.DEFECT[name] not in (1, 2))


@pytest.mark.parametrize("name", S.NAMES)
def test_plan_of_every_scene_takes_the_stated_path(name):
    """The engine's plan, device-free (jaicov_debug_create_plan): the block scenes of d in {0, 3, 4, 5, 6, 7} pre-eliminate the
    exterior orientations (reduced order U - 6 I, the border inside the reduced system); a fixed angle (d = 1, 2) and ordinary
    image groups of this size (every diag scene) keep the full order.  tests/test_gpu_datum_defects.py asserts the same of
    reduced_order() on the device."""
    from test_create_plan import plan
    fp = S.get_scene(name)
    rc, text, summary = plan(fp)
    assert rc == 0, text
    reduced = name.startswith("block") and S.DEFECT[name] not in (1, 2)
    assert summary["schur_ok"] == int(reduced)
    if reduced:
        assert summary["e0"] == fp.n_unknowns - 6 * fp.n_images


# ---- 2. the oracle's step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 0.5])
@pytest.mark.parametrize("name", S.NAMES)
def test_oracle_step_is_the_exact_solution_of_its_bordered_system(oracle_mod, name, lam):
    fp = S.get_scene(name)
    U, d = fp.n_unknowns, fp.rank_defect
    dx, _, N0, n0 = oracle_mod.Oracle(fp).step(fp.values, fp.sigma2apriori, lam, False)
    assert np.isfinite(dx).all()
    K = packed_to_full(N0, U)                                     # datum rows and damping applied, not preconditioned
    z = exact_solution(K, n0)
    err = float(np.abs(dx[d:] - z[d:]).max() / np.abs(z[d:]).max())
    mult = float(np.abs(dx[:d] - z[:d]).max() / np.abs(n0).max()) if d else 0.0
    print(f"{name} lambda {lam}: U = {U}, step vs exact {err:.2e}, multipliers {mult:.2e} of max|n|")
    assert err < 1e-11
    assert mult < 1e-11


# ---- 3. the oracle's cofactor matrix --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_oracle_cofactor_is_the_reflexive_inverse_in_the_datum_of_the_border(oracle_mod, name):
    fp = S.get_scene(name)
    U, d = fp.n_unknowns, fp.rank_defect
    o = oracle_mod.Oracle(fp)
    _, Qp, N0, _ = o.step(fp.values, fp.sigma2apriori, 0.0, True)
    Q = packed_to_full(Qp, U)[d:, d:]
    N = packed_to_full(N0, U)[d:, d:]
    assert np.isfinite(Q).all()
    sd = np.sqrt(np.abs(np.diag(Q)))
    assert (sd > 0).all()
    qnq = float((np.abs(Q @ N @ Q - Q) / np.outer(sd, sd)).max())
    bq = 0.0
    if d:
        B = border_rows(o, fp.values)[:, d:]
        np.testing.assert_allclose(np.linalg.norm(B, axis=1), 1.0, rtol=1e-14)
        bq = float(np.abs(B @ Q).max() / np.abs(Q).max())
    print(f"{name}: |Q N Q - Q| {qnq:.2e} (correlation scale), |B Q| {bq:.2e} of max|Q|")
    assert qnq < 1e-10
    assert bq < 1e-13


# ---- 4. the oracle's datum rows ---------------------------------------------------------------------------------------------------
def datum_rows_restated(fp, values):
    """addDatumConditionRows (BA:493-635) as a d x U matrix: the centroid over the datum points (datum flag set, X, Y and Z all
    free), the seven row patterns about it in flag order without gaps, each row divided by its norm."""
    U, d, f = fp.n_unknowns, fp.rank_defect, fp.datum_flags
    cols = np.asarray(fp.point_col).reshape(-1, 3)
    use = (np.asarray(fp.point_datum) != 0) & (cols >= 0).all(axis=1)
    assert use.sum() >= 3
    X = np.asarray(values)[:3 * fp.n_points].reshape(-1, 3)[use]
    c = cols[use]
    x, y, z = (X - X.sum(axis=0) / use.sum()).T
    one, nil = np.ones_like(x), np.zeros_like(x)
    patterns = {S.TX: (one, nil, nil), S.TY: (nil, one, nil), S.TZ: (nil, nil, one),
                S.RX: (nil, z, -y), S.RY: (-z, nil, x), S.RZ: (y, -x, nil), S.SCALE: (x, y, z)}
    B = np.zeros((d, U))
    row = 0
    for bit in S.CONDITIONS:
        if not f & bit:
            continue
        for a in range(3):
            B[row, c[:, a]] = patterns[bit][a]
        B[row] /= np.sqrt((B[row] ** 2).sum())
        row += 1
    assert row == d
    return B


@pytest.mark.parametrize("name", [n for n in S.NAMES if S.DEFECT[n] > 0])
def test_oracle_datum_rows_are_the_restated_condition_rows(oracle_mod, name):
    fp = S.get_scene(name)
    U, d = fp.n_unknowns, fp.rank_defect
    o = oracle_mod.Oracle(fp)
    Z = np.zeros(fp.packed_length); zn = np.zeros(U)
    o.finalize(fp.values, Z, zn, 0.0, False)                      # as test_gpu_refinement.bordered takes them
    full = packed_to_full(Z, U)
    assert not full[d:, d:].any() and not full[:d, :d].any() and not zn.any()
    B = full[:d, :]
    Br = datum_rows_restated(fp, fp.values)
    err = float(np.abs(B - Br).max())
    print(f"{name}: d = {d}, flags {fp.datum_flags}: rows vs restatement {err:.2e}")
    assert np.array_equal(B != 0, Br != 0)                        # the same columns in the same rows: no slip in the numbering
    assert err <= 4e-16                                           # unit rows: entries <= 1, a few roundings of the norm's sum apart
    # a fixed point carries no condition; a row is never empty
    fixed = np.asarray(fp.point_col).reshape(-1, 3)
    fixed = fixed[(fixed < 0).any(axis=1)]
    assert not B[:, fixed[fixed >= 0]].any()
    assert (np.abs(B).sum(axis=1) > 0).all()
    if fp.datum_flags & S.SCALE:                                  # the SCALE row is the last one and is no rotation row
        pc = np.asarray(fp.point_col).reshape(-1, 3)
        free = pc[(pc >= 0).all(axis=1)]
        assert (B[d - 1, free] != 0).all()
