"""Every consumer of the cofactor matrix in every state of the engine that decides what it may read: a table of state x call.

The consumers (transform, reliability, datum, precision, parameters, forms, predict, new points, the getters of the engine) each test the same few facts about the matrix an
inverting solve leaves: is there one, is it the reduced one, is the engine a shard.  The table below is their status code and, for a
refusal, the whole text of jaicov_neq_last_error, written out from the consumers' sources and the order of refusals that the headers
under include/ state.  One engine walks through
    (a) solved without an inverse   (b) REDUCED   (c) FULL   (d) FULL_EXPANDED   (e) a further accumulate   (f) REDUCED again,
so that a fact one solve recorded and a later one did not overwrite shows; two shards and a network without a datum defect are added.
Every call is made once with valid arguments and once with one invalid argument: where the state is looked at first the refusal is
the state's.  Nothing here compares the bits of two solves."""
import ctypes as C

import numpy as np
import pytest

from bundle_adjustment_amd import engine, scene

pytestmark = pytest.mark.gpu

S2 = 0.83
OK = (0, None)
NO_FULL = (-2, "no full cofactor matrix: solve with JAICOV_INVERT_FULL or JAICOV_INVERT_FULL_EXPANDED first")
NO_Q = (-2, "no cofactor matrix: solve with invert != 0 first")
NO_Q_GET = (-2, "no cofactor matrix: solve with invert != 0 first (MatrixInversion.NONE, BA:1177)")
NO_STATIONS = (-2, "station precision needs the exterior orientations' columns: invert FULL or FULL_EXPANDED")
NO_S = (-2, "no datum transformation since the last inverting solve")
SHARD_REL = (-3, "reliability needs an engine that holds every observation (not a shard)")
SHARD_DATUM = (-3, "datum transformation on a sharded engine")
SHARD_PREC = (-3, "precision figures on a sharded engine")
SHARD_PAR = (-3, "parameter correlations and tests on a sharded engine")
SHARD_FORM = (-3, "forms on a sharded engine")
SHARD_PRED = (-3, "image predictions on a sharded engine")
SHARD_NEWPT = (-3, "new points on a sharded engine")
NO_ALL_PRED = (-2, "image predictions need all of Qxx on the device: solve with invert FULL or FULL_EXPANDED first")
NO_ALL_NEWPT = (-2, "new points need all of Qxx on the device: solve with invert FULL or FULL_EXPANDED first")
NO_DEFECT = (-3, "datum transformation: the network has no datum defect (d = 0)")
BAD_S2T = (-1, "sigma2_test must be positive and finite")
BAD_L0 = (-1, "lambda0 must be positive and finite")
BAD_POINT = (-1, "point index out of range")
BAD_MASK = (-1, "point_datum must hold one flag per object point")
BAD_ITEM = (-1, "precision: index out of range")
BAD_PAIR = (-1, "length precision: point index out of range")
BAD_K = (-1, "principal components: k must be 1 .. 4")
BAD_BITS = (-1, "correlation maxima: unknown bits in pair_mask or flags")
BAD_SLOT = (-1, "parameter tests: slot out of range")
BAD_MEMBER = (-1, "forms: point index out of range")
BAD_PRED = (-1, "image predictions: image or point index out of range")
BAD_RAY = (-1, "new points: image index out of range")
BAD_LEN = (-1, "cofactor buffer length must be order(order+1)/2 with order = jaicov_neq_cofactor_order()")
BAD_IDX = (-1, None)                # jaicov_neq_get_cofactor_sub names no reason for an index out of range

# state -> call -> (valid arguments, one invalid argument); datum_transform comes last: it is the one call that changes the matrix
TABLE = {
    "none": {                                            # (a), (e): no cofactor matrix
        "transform": (NO_FULL, NO_FULL),
        "reliability": (NO_FULL, BAD_S2T),               # reliability looks at its two arguments before the state
        "reliability_points": (NO_FULL, BAD_L0),
        "precision_points": (NO_Q, NO_Q),
        "precision_stations": (NO_Q, NO_Q),
        "precision_lengths": (NO_Q, NO_Q),
        "principal_components": (NO_Q, NO_Q),
        "correlation_maxima": (NO_Q, NO_Q),
        "parameter_tests": (NO_Q, NO_Q),
        "fit_forms": (NO_Q, NO_Q),
        "predict_image_points": (NO_ALL_PRED, NO_ALL_PRED),
        "check_image_points": (NO_ALL_PRED, NO_ALL_PRED),
        "intersect_new_points": (NO_ALL_NEWPT, NO_ALL_NEWPT),
        "get_cofactor": (NO_Q_GET, NO_Q_GET),
        "get_cofactor_sub": (NO_Q, NO_Q),
        "datum_transform": (NO_Q, NO_Q),
    },
    "reduced": {                                         # (b), (f): the inverse of the EO-reduced system
        "transform": (NO_FULL, NO_FULL),
        "reliability": (NO_FULL, BAD_S2T),
        "reliability_points": (NO_FULL, BAD_L0),
        "precision_points": (OK, BAD_ITEM),
        "precision_stations": (NO_STATIONS, NO_STATIONS),
        "precision_lengths": (OK, BAD_PAIR),
        "principal_components": (OK, BAD_K),
        "correlation_maxima": (OK, BAD_BITS),
        "parameter_tests": (OK, BAD_SLOT),
        "fit_forms": (OK, BAD_MEMBER),
        "predict_image_points": (NO_ALL_PRED, NO_ALL_PRED),
        "check_image_points": (NO_ALL_PRED, NO_ALL_PRED),
        "intersect_new_points": (NO_ALL_NEWPT, NO_ALL_NEWPT),
        "get_cofactor": (OK, BAD_LEN),
        "get_cofactor_sub": (OK, BAD_IDX),
        "datum_transform": (OK, BAD_MASK),
    },
    "full": {                                            # (c), (d): all of Qxx
        "transform": (OK, BAD_POINT),
        "reliability": (OK, BAD_S2T),
        "reliability_points": (OK, BAD_L0),
        "precision_points": (OK, BAD_ITEM),
        "precision_stations": (OK, BAD_ITEM),
        "precision_lengths": (OK, BAD_PAIR),
        "principal_components": (OK, BAD_K),
        "correlation_maxima": (OK, BAD_BITS),
        "parameter_tests": (OK, BAD_SLOT),
        "fit_forms": (OK, BAD_MEMBER),
        "predict_image_points": (OK, BAD_PRED),
        "check_image_points": (OK, BAD_PRED),
        "intersect_new_points": (OK, BAD_RAY),
        "get_cofactor": (OK, BAD_LEN),
        "get_cofactor_sub": (OK, BAD_IDX),
        "datum_transform": (OK, BAD_MASK),
    },
    "shard": {                                           # the transformation and the getters do not ask: a shard never has a matrix
        "transform": (NO_FULL, NO_FULL),
        "reliability": (SHARD_REL, SHARD_REL),
        "reliability_points": (SHARD_REL, SHARD_REL),
        "precision_points": (SHARD_PREC, SHARD_PREC),
        "precision_stations": (SHARD_PREC, SHARD_PREC),
        "precision_lengths": (SHARD_PREC, SHARD_PREC),
        "principal_components": (SHARD_PREC, SHARD_PREC),
        "correlation_maxima": (SHARD_PAR, SHARD_PAR),
        "parameter_tests": (SHARD_PAR, SHARD_PAR),
        "fit_forms": (SHARD_FORM, SHARD_FORM),
        "predict_image_points": (SHARD_PRED, SHARD_PRED),
        "check_image_points": (SHARD_PRED, SHARD_PRED),
        "intersect_new_points": (SHARD_NEWPT, SHARD_NEWPT),
        "get_cofactor": (NO_Q_GET, NO_Q_GET),
        "get_cofactor_sub": (NO_Q, NO_Q),
        "datum_transform": (SHARD_DATUM, SHARD_DATUM),
    },
}


def get_cofactor(eng, n):
    """jaicov_neq_get_cofactor itself (Engine.get_cofactor answers a missing matrix on its own)."""
    Q = np.zeros(n)
    eng._chk(eng.L.jaicov_neq_get_cofactor(eng._h, Q.ctypes.data_as(C.POINTER(C.c_double)), Q.size))
    return Q


def correlation_maxima(eng, n, pair_mask):
    """jaicov_par_maxima itself (Engine.correlation_maxima answers a missing matrix on its own)."""
    rho = np.zeros(n); partner = np.zeros(n, np.int32); status = np.zeros(n, np.int32)
    pi = C.POINTER(C.c_int32)
    eng._chk(eng.L.jaicov_par_maxima(eng._h, pair_mask, 0, rho.ctypes.data_as(C.POINTER(C.c_double)), partner.ctypes.data_as(pi),
                                     status.ctypes.data_as(pi), n))


def calls(eng, fp):
    """call -> (with valid arguments, with one invalid argument)"""
    P, I, U = fp.n_points, fp.n_images, fp.n_unknowns
    order = eng.cofactor_order() if eng.cofactor_order() >= 0 else U
    n = order * (order + 1) // 2
    first, cols = eng.point_column_range()
    rel = dict(omega=1.0, dof=fp.degree_of_freedom)
    var = [1e-6]
    rays = dict(ray_begin=[0, 2], xy=np.zeros((2, 2)), disp=[[1e-6, 1e-6, 0.0]] * 2, start=fp.values[0:3])
    return {
        "transform": (lambda: eng.transform([0, 1, 2], [(0, 1)], S2), lambda: eng.transform([0, P], [(0, 1)], S2)),
        "reliability": (lambda: eng.reliability(S2), lambda: eng.reliability(-1.0)),
        "reliability_points": (lambda: eng.reliability_points(S2, **rel), lambda: eng.reliability_points(S2, lambda0=-1.0, **rel)),
        "precision_points": (lambda: eng.precision_points(S2), lambda: eng.precision_points(S2, points=[P])),
        "precision_stations": (lambda: eng.precision_stations(S2), lambda: eng.precision_stations(S2, images=[I])),
        "precision_lengths": (lambda: eng.precision_lengths(S2, [(0, 1)]), lambda: eng.precision_lengths(S2, [(0, P)])),
        "principal_components": (lambda: eng.principal_components(3, first, cols, max_iterations=4),
                                 lambda: eng.principal_components(5, first, cols, max_iterations=4)),
        "correlation_maxima": (lambda: correlation_maxima(eng, order, engine.PAR_ALL_PAIRS),
                               lambda: correlation_maxima(eng, order, 1 << 16)),
        "parameter_tests": (lambda: eng.parameter_tests(S2, [[0, 1, 2]]), lambda: eng.parameter_tests(S2, [[0, fp.n_slots]])),
        "fit_forms": (lambda: eng.fit_forms(S2, [("plane", [0, 1, 2, 3])]), lambda: eng.fit_forms(S2, [("plane", [0, 1, 2, P])])),
        "predict_image_points": (lambda: eng.predict_image_points(S2, [0], [0]), lambda: eng.predict_image_points(S2, [0], [P])),
        "check_image_points": (lambda: eng.check_image_points([0], [0], np.zeros((1, 2)), var, var),
                               lambda: eng.check_image_points([0], [P], np.zeros((1, 2)), var, var)),
        "intersect_new_points": (lambda: eng.intersect_new_points(S2, ray_image=[0, 1], **rays),
                                 lambda: eng.intersect_new_points(S2, ray_image=[0, I], **rays)),
        "get_cofactor": (lambda: get_cofactor(eng, n), lambda: get_cofactor(eng, n + 1)),
        "get_cofactor_sub": (lambda: eng.get_cofactor_sub([0, order - 1]), lambda: eng.get_cofactor_sub([0, U + 7])),
        "datum_transform": (lambda: eng.datum_transform(np.ones(P)), lambda: eng.datum_transform(np.ones(P + 1))),
    }


def outcome(eng, fn):
    try:
        fn()
    except engine.EngineError as err:
        return err.code, eng.L.jaicov_neq_last_error(eng._h).decode()
    return OK


def check(label, eng, fp, row, order):
    """Every call of the row, the invalid argument first; the matrix keeps its bits until datum_transform is accepted."""
    assert eng.cofactor_order() == order, (label, eng.cofactor_order(), order)
    Q0 = eng.get_cofactor().tobytes() if order >= 0 else None
    fns = calls(eng, fp)
    assert list(row) == list(fns) and list(row)[-1] == "datum_transform"
    for name, expected in row.items():
        for which in (1, 0):
            got, want = outcome(eng, fns[name][which]), expected[which]
            print(f"{label} {name} {'invalid' if which else 'valid'}: {got}")
            assert got[0] == want[0] and (want[1] is None or got[1] == want[1]), (label, name, which, got, want)
            if Q0 is not None and (name, which) != ("datum_transform", 0):
                assert eng.get_cofactor().tobytes() == Q0, (label, name, which)
        assert eng.cofactor_order() == order, (label, name)


def solve(eng, fp, mode):
    eng.prepare_inverse(mode)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(mode)


def test_one_engine_through_every_state_of_its_cofactor_matrix():
    fp = scene.config("tiny_free")
    U = fp.n_unknowns
    assert fp.rank_defect == 6
    eng = engine.Engine(fp, device=0, ordinary_group_elimination=1)      # at this size the pre-elimination has to be asked for
    eng.set_parameters(fp.values)
    solve(eng, fp, engine.INVERT_NONE)
    check("(a) no inverse", eng, fp, TABLE["none"], -1)
    solve(eng, fp, engine.INVERT_REDUCED)
    reduced = eng.reduced_order()
    assert fp.rank_defect < reduced < U                  # the exterior orientations are pre-eliminated: REDUCED is not FULL here
    check("(b) REDUCED", eng, fp, TABLE["reduced"], reduced)
    solve(eng, fp, engine.INVERT_FULL)
    check("(c) FULL", eng, fp, TABLE["full"], U)
    solve(eng, fp, engine.INVERT_FULL_EXPANDED)
    check("(d) FULL_EXPANDED", eng, fp, TABLE["full"], U)
    # what (d) left with the engine: the results of the transformation and of the reliability run, S of the datum transformation
    kept = eng.transform_covariance().tobytes(), eng.reliability_summary().tobytes()
    x = np.linspace(-1.0, 1.0, U)
    Sx = eng.datum_apply(x)
    eng.accumulate(fp.sigma2apriori)                     # withdraws the matrix and nothing else
    check("(e) accumulate", eng, fp, TABLE["none"], -1)
    assert (eng.transform_covariance().tobytes(), eng.reliability_summary().tobytes()) == kept
    assert eng.datum_apply(x).tobytes() == Sx.tobytes()
    solve(eng, fp, engine.INVERT_REDUCED)                # results outlive an inverting solve, S does not
    assert (eng.transform_covariance().tobytes(), eng.reliability_summary().tobytes()) == kept
    assert outcome(eng, lambda: eng.datum_apply(x)) == NO_S
    check("(f) REDUCED again", eng, fp, TABLE["reduced"], reduced)
    assert (eng.transform_covariance().tobytes(), eng.reliability_summary().tobytes()) == kept
    eng.close()


@pytest.mark.parametrize("how", [dict(image_range=(0, 3)), dict(apply_shared=False)], ids=["image_range", "apply_shared"])
def test_a_shard_is_refused_before_state_and_arguments(how):
    fp = scene.config("tiny_free")
    sh = engine.Engine(fp, device=0, **how)
    check("shard", sh, fp, TABLE["shard"], -1)
    sh.close()


def test_no_datum_defect_is_refused_before_everything_else():
    ft = scene.config("tiny")
    assert ft.rank_defect == 0
    eng = engine.Engine(ft, device=0)
    P = ft.n_points
    for label in ("new", "FULL"):
        assert outcome(eng, lambda: eng.datum_transform(np.ones(P))) == NO_DEFECT, label
        assert outcome(eng, lambda: eng.datum_transform(np.ones(P + 1))) == NO_DEFECT, label
        if label == "new":
            eng.set_parameters(ft.values)
            solve(eng, ft, engine.INVERT_FULL)
    eng.close()
