"""CPU: the C ABI of include/jaicov_newpoints.h is exported, declared and bound (Python: engine.NEWPT_EXPORTS, C++ mirror), the
header's constants are the binding's and the reference's, and a NULL engine is refused with every output untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import newpoint_reference as R
from bundle_adjustment_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jaicov_newpoints.h")


def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(jaicov_newpt_[a-z_0-9]+)\s*\(", src)))


def _lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def test_header_declaration_is_exported_and_bound():
    names = declared()
    assert names == sorted(engine.NEWPT_EXPORTS) == ["jaicov_newpt_intersect"]
    for other in (engine.EXPORTS, engine.XFORM_EXPORTS, engine.DLT_EXPORTS, engine.REL_EXPORTS, engine.REL_POINT_EXPORTS, engine.DATUM_EXPORTS,
                  engine.PREC_EXPORTS, engine.PARAM_EXPORTS, engine.FORM_EXPORTS, engine.PRED_EXPORTS, engine.ISECT_EXPORTS, engine.RESECT_EXPORTS,
                  engine.RELOR_EXPORTS, engine.SIMIL_EXPORTS, engine.LENS_EXPORTS):
        assert not set(names) & set(other)
    L = _lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    for n in names:
        assert hasattr(L, n), n
        assert re.search(r"\bT %s\b" % n, syms), f"{n} is declared but not exported"
    assert len(L.jaicov_newpt_intersect.argtypes) == 17
    assert callable(engine.Engine.intersect_new_points)
    from bundle_adjustment_amd import host_api
    assert hasattr(host_api.BundleAdjustment, "intersectNewPoints")


def test_the_headers_constants_are_the_bindings():
    text = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r"#define JAICOV_NEWPT_(\w+) (\d+)", text)}
    assert consts == {"PARTIAL": engine.NEWPT_PARTIAL, "NOT_CONVERGED": engine.NEWPT_NOT_CONVERGED, "TOO_FEW_RAYS": engine.NEWPT_TOO_FEW_RAYS,
                      "TOO_MANY": engine.NEWPT_TOO_MANY, "SINGULAR": engine.NEWPT_SINGULAR, "NOT_FINITE": engine.NEWPT_NOT_FINITE,
                      "PAIR_PARTIAL": engine.NEWPT_PAIR_PARTIAL, "PAIR_NEGATIVE": engine.NEWPT_PAIR_NEGATIVE,
                      "PAIR_NOT_FINITE": engine.NEWPT_PAIR_NOT_FINITE, "PAIR_DEGENERATE": engine.NEWPT_PAIR_DEGENERATE,
                      "COLUMNS": engine.NEWPT_COLUMNS, "PAIR_COLUMNS": engine.NEWPT_PAIR_COLUMNS, "MAX_RAYS": engine.NEWPT_MAX_RAYS,
                      "MAX_COLS": engine.NEWPT_MAX_COLS}
    assert (engine.NEWPT_COLUMNS, engine.NEWPT_PAIR_COLUMNS, engine.NEWPT_MAX_RAYS, engine.NEWPT_MAX_COLS) == (20, 7, 64, 448)
    assert (R.PARTIAL, R.NOT_CONVERGED, R.TOO_FEW_RAYS, R.TOO_MANY, R.SINGULAR, R.NOT_FINITE) == (
        engine.NEWPT_PARTIAL, engine.NEWPT_NOT_CONVERGED, engine.NEWPT_TOO_FEW_RAYS, engine.NEWPT_TOO_MANY, engine.NEWPT_SINGULAR, engine.NEWPT_NOT_FINITE)
    assert R.FAILED == engine.NEWPT_FAILED
    assert (R.PAIR_PARTIAL, R.PAIR_NEGATIVE, R.PAIR_NOT_FINITE, R.PAIR_DEGENERATE) == (
        engine.NEWPT_PAIR_PARTIAL, engine.NEWPT_PAIR_NEGATIVE, engine.NEWPT_PAIR_NOT_FINITE, engine.NEWPT_PAIR_DEGENERATE)
    assert (R.COLUMNS, R.PAIR_COLUMNS, R.MAX_RAYS, R.MAX_COLS) == (engine.NEWPT_COLUMNS, engine.NEWPT_PAIR_COLUMNS, engine.NEWPT_MAX_RAYS,
                                                                 engine.NEWPT_MAX_COLS)
    # the pair bits are those of the lengths of jaicov_precision.h
    prec = open(os.path.join(ROOT, "include", "jaicov_precision.h")).read()
    for name in ("PARTIAL", "NEGATIVE", "NOT_FINITE", "DEGENERATE"):
        assert int(re.search(r"#define JAICOV_PREC_%s (\d+)" % name, prec).group(1)) == consts["PAIR_" + name]
    assert 64 * 6 + 2 * (3 + engine.KROW - 12) <= engine.NEWPT_MAX_COLS          # 64 distinct images and two cameras of the largest size
    assert engine.NewPoints._fields == ("xyz", "cof_meas", "cof", "sigma", "omega", "dof", "status", "iterations", "ray_w", "lengths", "length_status")
    # the header states the order of the refusals
    order = [text.index(s) for s in ("NULL engine", "sharded engine", "not all of Qxx", "NULL or out-of-range arguments")]
    assert order == sorted(order)


def test_null_engine_is_refused_and_outputs_stay():
    L = _lib()
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    out = np.full(20, 3.0); st = np.full(1, 7, np.int32); it = np.full(1, 8, np.int32); rw = np.full(4, 2.0)
    pout = np.full(7, 5.0); pst = np.full(1, 9, np.int32)
    rb = np.array([0, 2], np.int32); ri = np.zeros(2, np.int32); xy = np.zeros(4); disp = np.tile([1.0, 1.0, 0.0], 2); start = np.zeros(3)
    pairs = np.array([0, -1], np.int32)
    assert L.jaicov_newpt_intersect(None, 1.0, 1, rb.ctypes.data_as(pi), ri.ctypes.data_as(pi), xy.ctypes.data_as(pd), disp.ctypes.data_as(pd),
                                    start.ctypes.data_as(pd), 20, pairs.ctypes.data_as(pi), 1, out.ctypes.data_as(pd), st.ctypes.data_as(pi),
                                    it.ctypes.data_as(pi), rw.ctypes.data_as(pd), pout.ctypes.data_as(pd), pst.ctypes.data_as(pi)) == -1
    assert np.all(out == 3.0) and st[0] == 7 and it[0] == 8 and np.all(rw == 2.0) and np.all(pout == 5.0) and pst[0] == 9
