"""CPU: the C ABI of include/jaicov_reliability.h is exported, bound in Python (engine.REL_EXPORTS) and in Java (one native per
function, one Java_... twin per native), and its entry points refuse a NULL engine without touching their outputs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from bundle_adjustment_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jaicov_reliability.h")
SHIM = os.path.join(ROOT, "java", "jni", "jaicov_jni.c")
JAVA = os.path.join(ROOT, "java", "org", "applied_geodesy", "adjustment", "bundle", "nativeengine", "NativeNormalEquationEngine.java")


def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(jaicov_rel_[a-z_0-9]+)\s*\(", src)))


def _lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def test_header_declarations_are_exported_and_bound_in_python():
    names = declared()
    assert names == sorted(engine.REL_EXPORTS) and len(names) == 4
    assert not set(names) & set(engine.EXPORTS)
    L = _lib()
    for n in names:
        assert hasattr(L, n), n
    syms = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    for n in names:
        assert re.search(r"\bT %s\b" % n, syms), f"{n} is declared but not exported"


def test_every_reliability_function_has_one_native_and_one_shim_twin():
    shim = open(SHIM).read()
    assert set(re.findall(r"\b(jaicov_rel_\w+)\s*\(", shim)) == set(declared())
    java = open(JAVA).read()
    natives = re.findall(r"private static native \w+ (rel[A-Z]\w*)\(", java)
    twins = re.findall(r"JNIEXPORT \w+ JNICALL NAT\((rel[A-Z]\w*)\)", shim)
    assert sorted(natives) == sorted(twins) == ["relGet", "relRelease", "relRun", "relSummary"]
    for n in natives:                                     # each twin calls exactly one function of the header
        body = shim[shim.index("NAT(%s)" % n):].split("JNIEXPORT")[0]
        assert len(re.findall(r"\b(jaicov_rel_\w+)\s*\(", body)) == 1, n
    assert "SetIntArrayRegion(" not in shim               # the stub jni.h has none
    # the run reads U doubles of dx: the shim checks the Java array's length before it copies anything
    run = shim[shim.index("NAT(relRun)"):].split("JNIEXPORT")[0]
    assert "has_u_entries(e, h, dx)" in run and run.index("has_u_entries") < run.index("malloc")


def test_null_engine_is_refused_and_outputs_stay():
    L = _lib()
    n = C.c_int32(-7)
    dx = np.zeros(3)
    pd = C.POINTER(C.c_double)
    assert L.jaicov_rel_run(None, 1.0, dx.ctypes.data_as(pd), C.byref(n)) == -1
    assert L.jaicov_rel_run(None, 1.0, None, C.byref(n)) == -1
    assert n.value == -7
    bufs = [np.full(4, 5.0) for _ in range(4)]
    assert L.jaicov_rel_get(None, *[b.ctypes.data_as(pd) for b in bufs], 4) == -1
    assert all(np.all(b == 5.0) for b in bufs)
    out = np.full(6, 3.0)
    assert L.jaicov_rel_summary(None, out.ctypes.data_as(pd), 5) == -1
    assert L.jaicov_rel_summary(None, out.ctypes.data_as(pd), 6) == -1
    assert np.all(out == 3.0)
    assert L.jaicov_rel_release(None) == -1
