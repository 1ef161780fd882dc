"""Device memory goes back.  DevBuf (csrc/devbuf.h) counts the bytes and allocations it holds, and nothing else in the library
allocates (tests/test_ownership_text.py), so jaicov_debug_device_census is complete: every case runs its scenario once as warm-up
(code objects, pooled streams), takes the census c0, runs the scenario again and asserts that the census is c0 again, both numbers,
with no tolerance.  The engine cases also assert that the byte count was above c0 while the engine was alive: a counter that never
counts fails.  Sizes are the smallest that reach the code; the count is exact, so nothing larger is needed."""
import ctypes as C
import dataclasses
import gc

import numpy as np
import pytest

import dlt_reference
import helpers
import intersect_reference
from bundle_adjustment_amd import engine, scene
from bundle_adjustment_amd.problem import full_to_packed

pytestmark = pytest.mark.gpu

MODES = {"reduced": engine.INVERT_REDUCED, "full": engine.INVERT_FULL, "full_expanded": engine.INVERT_FULL_EXPANDED}
_SCENES = {}


def scene_of(name):
    if name not in _SCENES:
        _SCENES[name] = helpers.base_scene() if name == "base" else scene.config(name)
    return _SCENES[name]


def census():
    """(bytes, allocations) that the library's owners hold in this process"""
    lib = engine.load_library()
    lib.jaicov_debug_device_census.argtypes = [C.POINTER(C.c_longlong)]
    lib.jaicov_debug_device_census.restype = None
    a = (C.c_longlong * 2)()
    lib.jaicov_debug_device_census(a)
    return int(a[0]), int(a[1])


def twice(scenario):
    """Warm-up, c0, the scenario again, the census must be c0 again.  The scenario calls peek() while its engine is alive; returns
    (c0, the censuses seen by peek in the second run)."""
    scenario(lambda: None)
    gc.collect()                       # an engine that an earlier test left to the collector goes now, not between the two readings
    c0 = census()
    seen = []
    scenario(lambda: seen.append(census()))
    c1 = census()
    print(f"census after warm-up {c0}, while alive {seen}, after the scenario {c1}")
    assert c1 == c0, (c0, c1)
    return c0, seen


def alive_above(c0, seen):
    assert seen and all(s[0] > c0[0] and s[1] > c0[1] for s in seen), (c0, seen)


def inverting_pass(fp, mode):
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(mode)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(mode)
    return eng


# ---- 1. an engine with both solvers, no inverse ------------------------------------------------------------------------------
def test_engine_without_an_inverse_gives_everything_back():
    fp = scene_of("base")

    def scenario(peek):
        eng = engine.Engine(fp, device=0)
        eng.set_parameters(fp.values)
        eng.build(fp.sigma2apriori, 0.0)
        eng.solve(False)
        peek()
        eng.close()

    alive_above(*twice(scenario))


# ---- 2. the inverse's squares ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_engine_with_an_inverse_gives_everything_back(mode):
    """Fails before the solver owned its inverse, for all three modes: the squares W and Q were allocated by hand into the solver's
    raw pointers and nothing freed them (2 squares of the reduced order for REDUCED, of the full order for FULL, both solvers'
    for FULL_EXPANDED)."""
    fp = scene_of("base")

    def scenario(peek):
        eng = inverting_pass(fp, MODES[mode])
        eng.get_cofactor_sub(np.arange(min(6, eng.cofactor_order()), dtype=np.int32))
        peek()
        eng.close()

    alive_above(*twice(scenario))


# ---- 3. the results an engine keeps: transformation, reliability, datum transformation -----------------------------------------------
@pytest.mark.parametrize("release_first", [False, True])
def test_kept_results_go_with_the_engine(release_first):
    fp, ft = scene_of("base"), scene_of("tiny_free")
    assert ft.rank_defect == 6
    P = ft.point_datum.size
    second = np.zeros(P, np.uint8); second[::2] = 1
    three = np.zeros(P, np.uint8); three[:3] = 1

    def scenario(peek):
        eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
        a = census()
        eng.transform(list(range(fp.point_col.shape[0])), [(0, 1), (0, 0)], fp.sigma2apriori)
        eng.transform_covariance()
        eng.transform_covariance_sub([0, 1, 2])
        eng.transform_point_blocks()
        b = census()
        assert b[0] > a[0] and b[1] == a[1] + 6, (a, b)          # the six buffers of XformState, none of the getters' left
        eng.reliability(fp.sigma2apriori)
        c = census()
        assert c[0] > b[0] and c[1] == b[1] + 1, (b, c)          # RelState::out; the run's work buffers are gone
        peek()
        if release_first:
            eng.transform_release()
            eng.reliability_release()
            assert census() == a
        eng.close()
        eng = inverting_pass(ft, engine.INVERT_FULL_EXPANDED)
        a = census()
        eng.datum_transform(second)
        b = census()
        assert b[0] > a[0] and b[1] == a[1] + 1, (a, b)          # DatumState::work
        eng.datum_transform(three)                               # the work buffer is used again, S is replaced
        assert census() == b
        peek()
        eng.close()

    alive_above(*twice(scenario))


# ---- 4. creation that fails --------------------------------------------------------------------------------------------------
def failing_create(fp, peek):
    """jaicov_neq_create as Engine.__init__ calls it, but the failed engine stays until peek() has looked: (status, text)"""
    lib = engine.load_library()
    desc, keep = fp.as_desc()
    opts = engine.EngineOptions()
    opts.struct_size = C.sizeof(engine.EngineOptions)
    opts.image_begin = opts.image_end = -1
    opts.apply_shared = 1
    h = C.c_void_p()
    rc = lib.jaicov_neq_create(C.byref(desc), C.byref(opts), C.byref(h))
    assert h
    msg = lib.jaicov_neq_last_error(h).decode()
    peek()
    lib.jaicov_neq_destroy(h)
    del keep
    return rc, msg


def test_creation_that_fails_on_the_device_gives_everything_back():
    fp = scene_of("base")
    D = fp.blk_disp.copy()
    D[fp.blk_disp_offset[1]] *= -1.0                             # first diagonal entry of one image block's dispersion: indefinite
    bad = dataclasses.replace(fp, blk_disp=D)

    def scenario(peek):
        rc, msg = failing_create(bad, peek)
        assert engine.STATUS[rc] == "SINGULAR" and "not positive definite" in msg, (rc, msg)

    alive_above(*twice(scenario))                                # structure and weights were on the device when the inversion failed


def test_a_refused_description_never_touches_the_device():
    bad, text = helpers.corrupt(scene_of("base"), "duplicate_column")

    def scenario(peek):
        rc, msg = failing_create(bad, peek)
        assert rc != 0 and text in msg, (rc, msg)

    c0, seen = twice(scenario)
    assert seen == [c0]


# ---- 5., 6. one-shot entries -----------------------------------------------------------------------------------------------------
def spd(n, seed):
    G = np.random.default_rng(seed).normal(size=(n, n + 20))
    return G @ G.T / n + np.eye(n)


def solve_packed(n):
    S = spd(n, n)
    b = np.random.default_rng(n + 1).normal(size=(3, n))
    x, ap, _ = engine.dense_spd_solve_packed(full_to_packed(S), b, invert=True)
    np.testing.assert_allclose(x, np.linalg.solve(S, b.T).T, rtol=1e-10, atol=1e-12)


def gemm_128():
    rng = np.random.default_rng(7)
    A, B, C0 = rng.normal(size=(128, 128)), rng.normal(size=(128, 128)), rng.normal(size=(128, 128))
    got, _ = engine.dense_gemm(0, 0, A, B, C0, 128, 128, 128, alpha=1.0, beta=0.0)
    assert np.isfinite(got).all()


def dlt_tiny():
    ob, xy, xyz, io, _ = dlt_reference.batch_from_scene(scene_of("tiny"))
    out, st, _ = engine.dlt_adjust(ob, xy, xyz, io)
    assert st.size == ob.size - 1


def intersect_tiny():
    fp = scene_of("tiny")
    rb, ri, xy, var, io, eo, _ = intersect_reference.batch_from_scene(fp)
    out = engine.intersect_points(rb, ri, xy, var, io, eo, sigma2apriori=fp.sigma2apriori)
    assert (out[1] == engine.ISECT_OK).all()


def newton_schulz_128():
    lib = engine.load_library()
    lib.jaicov_debug_newton_schulz.argtypes = [C.c_int] + [C.c_void_p] * 4
    lib.jaicov_debug_newton_schulz.restype = C.c_int
    M = np.ascontiguousarray(spd(128, 3))
    Q0 = np.ascontiguousarray(np.linalg.inv(M))
    Q = np.empty((128, 128))
    assert lib.jaicov_debug_newton_schulz(128, M.ctypes.data, Q0.ctypes.data, Q.ctypes.data, None) == 0


ONE_SHOT = {"dense_spd_solve_packed_200": lambda: solve_packed(200), "dense_gemm_128": gemm_128, "dlt_adjust": dlt_tiny,
            "intersect_points": intersect_tiny, "debug_newton_schulz_128": newton_schulz_128}


@pytest.mark.parametrize("name", list(ONE_SHOT))
def test_one_shot_entry_holds_nothing_after_it_returns(name):
    twice(lambda peek: ONE_SHOT[name]())


def test_dataflow_factorisation_holds_nothing_after_the_solve_returns(monkeypatch):
    """3 block columns under JAICOV_FLOW_MIN_BLOCKS=1: FlowFactor's buffers, its fine-grained flags included, are in the count"""
    monkeypatch.setenv("JAICOV_FLOW_MIN_BLOCKS", "1")
    twice(lambda peek: solve_packed(384))
