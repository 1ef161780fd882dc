"""CPU: the C ABI of include/jaicov_predict.h is exported, declared and bound (Python: engine.PRED_EXPORTS, C++ mirror), the header's
constants are the binding's and the reference's, and a NULL engine is refused with every output untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import predict_reference as R
from bundle_adjustment_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jaicov_predict.h")


def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(jaicov_pred_[a-z_0-9]+)\s*\(", src)))


def _lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def test_header_declarations_are_exported_and_bound():
    names = declared()
    assert names == sorted(engine.PRED_EXPORTS) == ["jaicov_pred_check", "jaicov_pred_points"]
    for other in (engine.EXPORTS, engine.XFORM_EXPORTS, engine.DLT_EXPORTS, engine.REL_EXPORTS, engine.REL_POINT_EXPORTS, engine.DATUM_EXPORTS,
                  engine.PREC_EXPORTS, engine.PARAM_EXPORTS, engine.FORM_EXPORTS, engine.ISECT_EXPORTS, engine.RESECT_EXPORTS, engine.RELOR_EXPORTS,
                  engine.SIMIL_EXPORTS, engine.LENS_EXPORTS):
        assert not set(names) & set(other)
    L = _lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    for n in names:
        assert hasattr(L, n), n
        assert re.search(r"\bT %s\b" % n, syms), f"{n} is declared but not exported"
    for m in ("predict_image_points", "check_image_points"):
        assert callable(getattr(engine.Engine, m)), m
    from bundle_adjustment_amd import host_api
    for m in ("predictImagePoints", "checkImagePoints"):
        assert hasattr(host_api.BundleAdjustment, m), m


def test_the_headers_constants_are_the_bindings():
    text = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r"#define JAICOV_PRED_(\w+) (\d+)", text)}
    assert consts == {"PARTIAL": engine.PRED_PARTIAL, "NEGATIVE": engine.PRED_NEGATIVE, "NOT_FINITE": engine.PRED_NOT_FINITE,
                      "OBSERVED": engine.PRED_OBSERVED, "SINGULAR": engine.PRED_SINGULAR, "POINT_COLUMNS": engine.PRED_POINT_COLUMNS,
                      "CHECK_COLUMNS": engine.PRED_CHECK_COLUMNS, "GROUP_COLUMNS": engine.PRED_GROUP_COLUMNS, "MAX_GROUP": engine.PRED_MAX_GROUP}
    assert (R.PARTIAL, R.NEGATIVE, R.NOT_FINITE, R.OBSERVED, R.SINGULAR) == (engine.PRED_PARTIAL, engine.PRED_NEGATIVE, engine.PRED_NOT_FINITE,
                                                                             engine.PRED_OBSERVED, engine.PRED_SINGULAR)
    assert (R.POINT_COLUMNS, R.CHECK_COLUMNS, R.GROUP_COLUMNS, R.MAX_GROUP) == (engine.PRED_POINT_COLUMNS, engine.PRED_CHECK_COLUMNS,
                                                                                engine.PRED_GROUP_COLUMNS, engine.PRED_MAX_GROUP)
    assert R.KLOC == engine.KROW and len(engine.ImagePrediction._fields) == 6 and len(engine.ImageCheck._fields) == 6
    # the header states the order of the refusals
    order = [text.index(s) for s in ("NULL engine", "sharded engine", "not all of Qxx", "NULL, negative or out-of-range")]
    assert order == sorted(order)


def test_null_engine_is_refused_and_outputs_stay():
    L = _lib()
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    out = np.full(20, 3.0); st = np.full(2, 7, np.int32); idx = np.zeros(2, np.int32); gout = np.full(4, 5.0); gst = np.full(1, 9, np.int32)
    xy = np.zeros(4); disp = np.tile([1.0, 1.0, 0.0], 2); begin = np.array([0, 2], np.int32)
    assert L.jaicov_pred_points(None, 1.0, 1.0, idx.ctypes.data_as(pi), idx.ctypes.data_as(pi), 2, out.ctypes.data_as(pd), st.ctypes.data_as(pi)) == -1
    assert L.jaicov_pred_check(None, 1.0, idx.ctypes.data_as(pi), idx.ctypes.data_as(pi), xy.ctypes.data_as(pd), disp.ctypes.data_as(pd), 2,
                               begin.ctypes.data_as(pi), 1, out.ctypes.data_as(pd), st.ctypes.data_as(pi), gout.ctypes.data_as(pd),
                               gst.ctypes.data_as(pi)) == -1
    assert np.all(out == 3.0) and np.all(st == 7) and np.all(gout == 5.0) and gst[0] == 9
