"""CPU: the C ABI of include/jaicov_surfaces.h is exported, declared and bound (Python: engine.SURF_EXPORTS, C++ mirror), the header's
signature is the ctypes one, its constants are the binding's and the restatement's, and a NULL engine is refused with the outputs
untouched.  The family of jaicov_forms.h beside it stays what tests/test_forms_abi.py pins."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import surface_reference as R
from bundle_adjustment_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jaicov_surfaces.h")
HOST = os.path.join(ROOT, "bundle-adjustment_amd", "host")
CTYPE = {"jaicov_engine *": C.c_void_p, "double": C.c_double, "int32_t": C.c_int32, "const int32_t *": C.POINTER(C.c_int32),
         "const double *": C.POINTER(C.c_double), "double *": C.POINTER(C.c_double), "int32_t *": C.POINTER(C.c_int32),
         "float *": C.POINTER(C.c_float)}


def code():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def test_header_declarations_are_exported_and_bound():
    names = sorted(set(re.findall(r"\b(jaicov_surf_[a-z_0-9]+)\s*\(", code())))
    assert names == sorted(engine.SURF_EXPORTS) == ["jaicov_surf_fit"]
    for other in (engine.EXPORTS, engine.XFORM_EXPORTS, engine.DLT_EXPORTS, engine.REL_EXPORTS, engine.REL_POINT_EXPORTS, engine.DATUM_EXPORTS,
                  engine.PREC_EXPORTS, engine.PARAM_EXPORTS, engine.FORM_EXPORTS, engine.PRED_EXPORTS, engine.NEWPT_EXPORTS, engine.VCE_EXPORTS,
                  engine.ISECT_EXPORTS, engine.RESECT_EXPORTS, engine.RELOR_EXPORTS, engine.SIMIL_EXPORTS, engine.LENS_EXPORTS):
        assert not set(names) & set(other)
    L = _lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(re.findall(r"\bT (jaicov_surf_\w+)", syms)) == names          # exported, and nothing of the family undeclared
    assert hasattr(L, "jaicov_surf_fit") and callable(engine.Engine.fit_surfaces)
    assert '#include "jaicov_forms.h"' in code()                                # the status bits and the layouts are those of the forms


def test_header_signature_is_the_ctypes_one():
    m = re.search(r"\bint\s+jaicov_surf_fit\s*\(([^)]*)\)\s*;", code())
    assert m
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    kinds = [re.match(r"(.*?)(\w+)$", a).group(1).strip() for a in args]
    names = [re.match(r"(.*?)(\w+)$", a).group(2) for a in args]
    assert names == ["e", "sigma2", "n_forms", "form_type", "form_begin", "form_point", "start", "max_iterations", "tol", "out", "qpp",
                     "member_out", "status", "member_status", "ms_out"]
    assert [CTYPE[k] for k in kinds] == list(_lib().jaicov_surf_fit.argtypes)
    form = list(_lib().jaicov_form_fit.argtypes)                                # jaicov_form_fit with `start` behind form_point
    assert list(_lib().jaicov_surf_fit.argtypes) == form[:6] + [C.POINTER(C.c_double)] + form[6:]


def test_constants_match():
    consts = {k: int(v) for k, v in re.findall(r"#define JAICOV_SURF_(\w+) (\d+)", open(HEADER).read())}
    assert consts == {"CYLINDER": engine.SURF_CYLINDER, "CONE": engine.SURF_CONE}
    assert (R.CYLINDER, R.CONE) == (engine.SURF_CYLINDER, engine.SURF_CONE) == (engine.FORM_CIRCLE + 1, engine.FORM_CIRCLE + 2)
    assert R.KINDS == engine.SURF_KINDS and R.REPORTED == engine.SURF_REPORTED and len(engine.SURF_KINDS) == len(engine.SURF_REPORTED) == 6
    assert {k: v for k, v in engine.SURF_KINDS.items() if v <= engine.FORM_CIRCLE} == engine.FORM_KINDS
    assert engine.SURF_REPORTED[:4] == engine.FORM_REPORTED and max(engine.SURF_REPORTED) == engine.FORM_MAX_PARAMS
    assert max(R.FREE) == 6 and R.LEAST[4:] == R.FREE[4:] == (5, 6)             # wave_solve<6>; one condition per member
    assert [c * (engine.FORM_MAX_ROWS // c) for c in R.CONDITIONS] == [64] * 6


def test_the_cpp_host_mirrors_the_call():
    hpp = open(os.path.join(HOST, "jaicov.hpp")).read()
    cpp = open(os.path.join(HOST, "jaicov.cpp")).read()
    bind = open(os.path.join(HOST, "bindings.cpp")).read()
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert '#include "../../include/jaicov_surfaces.h"' in hpp
    assert re.search(r"\bfitSurfaces\s*\(", hpp) and re.search(r"BundleAdjustment::fitSurfaces\s*\(", cpp) and re.search(r"\bjaicov_surf_fit\s*\(engine_", cpp)
    # one pattern rule builds every program named in EXAMPLES
    assert '.def("fitSurfaces"' in bind and re.search(r"^EXAMPLES\s*:=.*\bexample_surfaces\b", mk, flags=re.M) and re.search(r"^example_%:", mk, flags=re.M)
    assert os.path.exists(os.path.join(HOST, "example_surfaces.cpp"))
    from bundle_adjustment_amd import host_api
    assert hasattr(host_api.BundleAdjustment, "fitSurfaces")


def test_null_engine_is_refused_and_outputs_stay():
    L = _lib()
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    out = np.full(28, 3.0); st = np.full(4, 7, np.int32); idx = np.zeros(4, np.int32); ms = C.c_float(5.0); start = np.full(7, 2.0)
    assert L.jaicov_surf_fit(None, 1.0, 1, idx.ctypes.data_as(pi), idx.ctypes.data_as(pi), idx.ctypes.data_as(pi), start.ctypes.data_as(pd), 10, 0.0,
                             out.ctypes.data_as(pd), out.ctypes.data_as(pd), out.ctypes.data_as(pd), st.ctypes.data_as(pi), st.ctypes.data_as(pi),
                             C.byref(ms)) == -1
    assert np.all(out == 3.0) and np.all(st == 7) and ms.value == 5.0 and np.all(start == 2.0)
