"""CPU: the numpy restatement of include/jaicov_newpoints.h (tests/newpoint_reference.py) stands on its own feet before the device
is held against it: its F is the derivative of its own converged solution with respect to every shared parameter, the share of the
adjustment vanishes with Qxx, and the pair formulas are symmetric and degenerate where they must be."""
import numpy as np
import pytest

import newpoint_reference as R
import predict_reference as PR
from bundle_adjustment_amd.problem import packed_to_full

NAMES = ("block", "free")          # make_scene(40, 80, 30, DIST_FULL, "block", n_control=4) and the free network with a scale bar


@pytest.fixture(scope="module")
def cases(oracle_mod):
    """per scene: the problem, the oracle's Qxx at its values, three new points with 3, 4 and 6 rays and noise-free measurements made
    at the same values, and their converged solution"""
    out = {}
    for name in NAMES:
        fp = R.scene_of(name)
        _, Qp, _, _ = oracle_mod.Oracle(fp).step(fp.values, fp.sigma2apriori, 0.0, True)
        X = R.new_points(fp, 3)
        rb, ri = R.rays_of(fp, [3, 4, 6])
        xy = R.measure(fp, fp.values, X, rb, ri)
        disp = R.dispersions(fp, ri.size)
        Xc, st, it = R.iterate(oracle_mod, fp, fp.values, rb, ri, xy, disp, fp.sigma2apriori, X + 5.0)
        assert not st.any(), st
        Xc = R.refine(oracle_mod, fp, fp.values, rb, ri, xy, disp, fp.sigma2apriori, Xc)
        out[name] = dict(fp=fp, Q=packed_to_full(Qp, fp.n_unknowns), X=X, Xc=Xc, rb=rb, ri=ri, xy=xy, disp=disp, it=it)
    return out


def evaluate(oracle_mod, c, X, Q=None):
    fp = c["fp"]
    w, J = R.rows(oracle_mod, fp, fp.values, X, c["rb"], c["ri"], c["xy"])
    return [R.evaluate(fp, c["Q"] if Q is None else Q, w[c["rb"][i]:c["rb"][i + 1]], J[c["rb"][i]:c["rb"][i + 1]], c["ri"][c["rb"][i]:c["rb"][i + 1]],
                       c["disp"][c["rb"][i]:c["rb"][i + 1]], fp.sigma2apriori) for i in range(len(c["rb"]) - 1)]


@pytest.mark.parametrize("name", NAMES)
def test_new_points_fall_into_the_format_of_every_image(name):
    fp = R.scene_of(name)
    X = R.new_points(fp, 257)
    v = R.model_values(fp)
    for im in range(fp.n_images):
        xy = R.project(fp, v, X, np.full(X.shape[0], im))
        assert np.abs(xy[:, 0]).max() < PR.FORMAT_W / 2 and np.abs(xy[:, 1]).max() < PR.FORMAT_H / 2, (name, im)


@pytest.mark.parametrize("name", NAMES)
def test_noise_free_measurements_converge_to_the_point(cases, name):
    c = cases[name]
    print(f"{name}: iterations {c['it'].tolist()}, |X - truth| {np.abs(c['Xc'] - c['X']).max():.2e} mm")
    assert np.abs(c["Xc"] - c["X"]).max() <= 1e-8


@pytest.mark.parametrize("name", NAMES)
def test_F_is_the_derivative_of_the_converged_solution(oracle_mod, cases, name):
    """Central differences of the reference's own converged solution under a perturbation of every involved slot, at two step sizes
    h and h / 2.  The measurements are noise-free, so the second-order terms that F leaves out vanish, and what is left of the
    difference is the truncation of a second-order scheme: it must fall by about 4, asserted as <= 0.3 of the former.  h moves the
    point by about 1 mm (h = 1 mm / |F column|: the scale alone, whatever the unit of the slot), far above the rounding of X."""
    c = cases[name]
    fp = c["fp"]
    s0 = fp.sigma2apriori
    ev = evaluate(oracle_mod, c, c["Xc"])
    worst = 0.0
    for i, e in enumerate(ev):
        rb = np.array([0, c["rb"][i + 1] - c["rb"][i]], np.int32)
        k = slice(c["rb"][i], c["rb"][i + 1])
        ri, xy, disp = c["ri"][k], c["xy"][k], c["disp"][k]
        col2slot = {}
        for im in ri:
            for col, slot in zip(R.shared_columns(fp, im), R.shared_slots(fp, im)):
                if col >= 0:
                    col2slot[int(col)] = int(slot)
        assert sorted(col2slot) == e["cols"].tolist()
        dev = np.zeros((2, e["cols"].size))
        for a, col in enumerate(e["cols"]):
            s = col2slot[int(col)]
            h0 = 1.0 / np.abs(e["F"][:, a]).max()
            for t, h in enumerate((h0, 0.5 * h0)):
                Xpm = []
                for sign in (1.0, -1.0):
                    v = fp.values.copy(); v[s] += sign * h
                    Xpm.append(R.refine(oracle_mod, fp, v, rb, ri, xy, disp, s0, c["Xc"][i:i + 1], steps=4)[0])
                dev[t, a] = np.abs((Xpm[0] - Xpm[1]) / (2.0 * h) - e["F"][:, a]).max() * h0      # of dX/ds, in mm per h0
        ratio = dev[1].max() / dev[0].max()
        worst = max(worst, ratio)
        print(f"{name} point {i}: {e['cols'].size} columns, deviation of dX/ds {dev[0].max():.2e} at h, {dev[1].max():.2e} at h / 2 (mm per h), ratio {ratio:.3f}; "
              f"per column {np.sort(dev[1] / dev[0])[[0, -1]]}")
        assert ratio <= 0.3
    assert worst > 0.0


@pytest.mark.parametrize("name", NAMES)
def test_without_Qxx_the_cofactors_are_those_of_the_measurements(oracle_mod, cases, name):
    c = cases[name]
    for e, e0 in zip(evaluate(oracle_mod, c, c["Xc"]), evaluate(oracle_mod, c, c["Xc"], Q=np.zeros_like(c["Q"]))):
        assert not e0["Q_sys"].any() and np.array_equal(e0["Q_XX"], e0["Q_meas"])
        assert np.array_equal(e["Q_meas"], e0["Q_meas"])
        assert np.all(np.linalg.eigvalsh(e["Q_sys"]) >= -1e-12 * np.trace(e["Q_sys"])) and np.trace(e["Q_sys"]) > 0.0


@pytest.mark.parametrize("name", NAMES)
def test_pairs_are_symmetric_and_a_point_on_a_block_point_is_degenerate(oracle_mod, cases, name):
    c = cases[name]
    fp = c["fp"]
    ev = evaluate(oracle_mod, c, c["Xc"])
    mem = [R.new_member(c["Xc"][i], e) for i, e in enumerate(ev)] + [R.block_member(fp, fp.values, c["Q"], 5)]
    for a, b in ((0, 1), (1, 2), (0, 3), (3, 2)):
        ab, sab, _, _ = R.pair_figures(c["Q"], mem[a], mem[b], 1.3)
        ba, sba, _, _ = R.pair_figures(c["Q"], mem[b], mem[a], 1.3)
        assert sab == sba == 0
        assert np.allclose(ab, ba, rtol=1e-12, atol=0.0)
        assert ab[5] != ab[6]                                  # the members share the camera at least
    on = dict(mem[0], X=mem[3]["X"].copy())
    row, st, _, _ = R.pair_figures(c["Q"], mem[3], on, 1.0)
    assert st & R.PAIR_DEGENERATE and row[0] == 0.0 and np.isnan(row[[1, 5, 6]]).all() and np.isfinite(row[2:5]).all()
    # pulled apart, L -> 0 continuously
    for d in (1e-3, 1e-6):
        near = dict(mem[0], X=mem[3]["X"] + np.array([d, 0.0, 0.0]))
        row, st, _, _ = R.pair_figures(c["Q"], mem[3], near, 1.0)
        assert st == 0 and abs(row[0] - d) <= 1e-9 * d + 1e-13
