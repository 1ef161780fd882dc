"""CPU: the C ABI of include/jaicov_calibration.h is exported, declared and bound (Python: engine.CALIB_EXPORTS, C++ mirror), the
header's constants are the binding's and the reference's, and a NULL engine is refused with every output untouched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import calib_reference as R
from bundle_adjustment_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jaicov_calibration.h")


def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(jaicov_calib_[a-z_0-9]+)\s*\(", src)))


def _lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def test_header_declarations_are_exported_and_bound():
    names = declared()
    assert names == sorted(engine.CALIB_EXPORTS) == ["jaicov_calib_compare", "jaicov_calib_field", "jaicov_calib_release"]
    for other in (engine.EXPORTS, engine.XFORM_EXPORTS, engine.DLT_EXPORTS, engine.REL_EXPORTS, engine.REL_POINT_EXPORTS, engine.DATUM_EXPORTS,
                  engine.PREC_EXPORTS, engine.PARAM_EXPORTS, engine.FORM_EXPORTS, engine.PRED_EXPORTS, engine.NEWPT_EXPORTS, engine.VCE_EXPORTS,
                  engine.ISECT_EXPORTS, engine.RESECT_EXPORTS, engine.RELOR_EXPORTS, engine.SIMIL_EXPORTS, engine.LENS_EXPORTS):
        assert not set(names) & set(other)
    L = _lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    for n in names + ["jaicov_debug_calib_timing"]:
        assert hasattr(L, n), n
        assert re.search(r"\bT %s\b" % n, syms), f"{n} is declared but not exported"
    assert len(L.jaicov_calib_field.argtypes) == 11 and len(L.jaicov_calib_compare.argtypes) == 13
    for m in ("calibration_field", "calibration_compare", "calibration_release"):
        assert callable(getattr(engine.Engine, m)), m
    assert callable(engine.sensor_grid) and callable(engine.radial_profile)
    from bundle_adjustment_amd import host_api
    for m in ("calibrationField", "compareCalibration"):
        assert hasattr(host_api.BundleAdjustment, m), m


def test_the_headers_constants_are_the_bindings():
    text = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r"#define JAICOV_CALIB_(\w+) (\d+)", text)}
    assert consts == {"PARTIAL": engine.CALIB_PARTIAL, "NEGATIVE": engine.CALIB_NEGATIVE, "NOT_FINITE": engine.CALIB_NOT_FINITE,
                      "SINGULAR": engine.CALIB_SINGULAR, "FIELD_COLUMNS": engine.CALIB_FIELD_COLUMNS,
                      "COMPARE_COLUMNS": engine.CALIB_COMPARE_COLUMNS, "SUMMARY_COLUMNS": engine.CALIB_SUMMARY_COLUMNS,
                      "MAX_COLUMNS": engine.CALIB_MAX_COLUMNS, "PRINCIPAL_POINT": engine.CALIB_PRINCIPAL_POINT,
                      "PRINCIPAL_DISTANCE": engine.CALIB_PRINCIPAL_DISTANCE, "KIND_SHIFT": engine.CALIB_KIND_SHIFT, "ALL": engine.CALIB_ALL,
                      "RELATIVE": engine.CALIB_RELATIVE}
    assert (R.PARTIAL, R.NEGATIVE, R.NOT_FINITE, R.SINGULAR) == (engine.CALIB_PARTIAL, engine.CALIB_NEGATIVE, engine.CALIB_NOT_FINITE,
                                                                  engine.CALIB_SINGULAR)
    assert (R.FIELD_COLUMNS, R.COMPARE_COLUMNS, R.SUMMARY_COLUMNS, R.MAX_COLUMNS) == (engine.CALIB_FIELD_COLUMNS, engine.CALIB_COMPARE_COLUMNS,
                                                                                      engine.CALIB_SUMMARY_COLUMNS, engine.CALIB_MAX_COLUMNS)
    assert (R.PRINCIPAL_POINT, R.PRINCIPAL_DISTANCE, R.KIND_SHIFT, R.ALL, R.RELATIVE) == (
        engine.CALIB_PRINCIPAL_POINT, engine.CALIB_PRINCIPAL_DISTANCE, engine.CALIB_KIND_SHIFT, engine.CALIB_ALL, engine.CALIB_RELATIVE)
    # the status bits have the values of jaicov_predict.h, every kind of coefficient has a bit within ALL, and the camera part of a row fits
    assert (engine.CALIB_PARTIAL, engine.CALIB_NEGATIVE, engine.CALIB_NOT_FINITE, engine.CALIB_SINGULAR) == (
        engine.PRED_PARTIAL, engine.PRED_NEGATIVE, engine.PRED_NOT_FINITE, engine.PRED_SINGULAR)
    assert engine.CALIB_ALL == (1 << (engine.CALIB_KIND_SHIFT + 10)) - 1 and engine.CALIB_MAX_COLUMNS == engine.KROW - 9
    assert engine.CalibrationField._fields == R.FIELD_FIELDS and engine.CalibrationCompare._fields == R.COMPARE_FIELDS
    assert engine.CalibrationSummary._fields == R.SUMMARY_FIELDS and len(R.SUMMARY_FIELDS) == engine.CALIB_SUMMARY_COLUMNS
    # the header states the order of the refusals
    order = [text.index(s) for s in ("NULL engine", "sharded engine", "no cofactor matrix on the device", "NULL, negative, non-finite or out-of-range")]
    assert order == sorted(order)


def test_null_engine_is_refused_and_outputs_stay():
    L = _lib()
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    out = np.full(28, 3.0); jac = np.full(92, 4.0); st = np.full(2, 7, np.int32); cams = np.zeros(2, np.int32); xy = np.ones(4); summ = np.full(8, 5.0)
    ref = np.ones(3)
    assert L.jaicov_calib_field(None, 1.0, 1.0, engine.CALIB_ALL, cams.ctypes.data_as(pi), xy.ctypes.data_as(pd), None, 2, out.ctypes.data_as(pd),
                                jac.ctypes.data_as(pd), st.ctypes.data_as(pi)) == -1
    assert L.jaicov_calib_compare(None, 1.0, 0, 0, ref.ctypes.data_as(pd), None, 0, xy.ctypes.data_as(pd), None, 2, out.ctypes.data_as(pd),
                                  st.ctypes.data_as(pi), summ.ctypes.data_as(pd)) == -1
    assert L.jaicov_calib_release(None) == -1
    assert L.jaicov_debug_calib_timing(None, 1, None) == -1
    assert np.all(out == 3.0) and np.all(jac == 4.0) and np.all(st == 7) and np.all(summ == 5.0)


def test_the_node_helpers():
    g = engine.sensor_grid(36.0, 24.0, 9, 7)
    assert g.shape == (63, 2) and g[0].tolist() == [-18.0, -12.0] and g[8].tolist() == [18.0, -12.0] and g[-1].tolist() == [18.0, 12.0]
    assert g[31].tolist() == [0.0, 0.0]
    p = engine.radial_profile(20.0, 20)
    assert p.shape == (20, 2) and np.array_equal(p[:, 0], np.arange(1.0, 21.0)) and not p[:, 1].any()
    q = engine.radial_profile(10.0, 5, azimuth=np.pi / 2)
    assert np.allclose(q[:, 1], [2.0, 4.0, 6.0, 8.0, 10.0]) and np.abs(q[:, 0]).max() < 1e-14
