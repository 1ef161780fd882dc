"""CPU: the C ABI of include/jaicov_transform.h is exported, bound in Python (engine.XFORM_EXPORTS) and in Java (one native per
function, one Java_... twin per native), and its entry points refuse a NULL engine without touching a device."""
import ctypes as C
import os
import re
import subprocess

from bundle_adjustment_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jaicov_transform.h")
SHIM = os.path.join(ROOT, "java", "jni", "jaicov_jni.c")
JAVA = os.path.join(ROOT, "java", "org", "applied_geodesy", "adjustment", "bundle", "nativeengine", "NativeNormalEquationEngine.java")


def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(jaicov_xform_[a-z_0-9]+)\s*\(", src)))


def _lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def test_header_declarations_are_exported_and_bound_in_python():
    names = declared()
    assert names == sorted(engine.XFORM_EXPORTS) and len(names) == 6
    assert not set(names) & set(engine.EXPORTS)          # EXPORTS stays the list of jaicov_neq.h + jaicov_dense.h
    L = _lib()
    for n in names:
        assert hasattr(L, n), n
    syms = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    for n in names:
        assert re.search(r"\bT %s\b" % n, syms), f"{n} is declared but not exported"


def test_every_transform_function_has_one_native_and_one_shim_twin():
    shim = open(SHIM).read()
    used = set(re.findall(r"\b(jaicov_xform_\w+)\s*\(", shim))
    assert used == set(declared())
    java = open(JAVA).read()
    natives = re.findall(r"private static native \w+ (xform\w+)\(", java)
    twins = re.findall(r"JNIEXPORT \w+ JNICALL NAT\((xform\w+)\)", shim)
    assert sorted(natives) == sorted(twins) and len(natives) == 6
    for n in natives:                                     # each twin calls exactly one function of the header
        body = shim[shim.index("NAT(%s)" % n):].split("JNIEXPORT")[0]
        assert len(set(re.findall(r"\b(jaicov_xform_\w+)\s*\(", body))) == 1, n
    # no SetIntArrayRegion in the stub jni.h: the shim must not need it
    assert "SetIntArrayRegion(" not in shim
    # a packed covariance longer than a Java array is refused before it is allocated
    assert "Integer.MAX_VALUE" in java[java.index("getTransformedCovariance("):]


def test_null_engine_is_refused():
    L = _lib()
    n = C.c_int32(-7)
    pi = C.POINTER(C.c_int32)
    pts = (C.c_int32 * 1)(0)
    assert L.jaicov_xform_run(None, pts, 1, pts, pts, 1, 1.0, C.byref(n)) == -1
    assert n.value == -7
    assert L.jaicov_xform_get_coordinates(None, None, None, 0) == -1
    assert L.jaicov_xform_get_covariance(None, None, 0) == -1
    assert L.jaicov_xform_get_covariance_sub(None, C.cast(pts, pi), 1, None) == -1
    assert L.jaicov_xform_get_point_blocks(None, None, 0) == -1
    assert L.jaicov_xform_release(None) == -1
