"""CPU: the C ABI of include/jaicov_datum.h is exported, declared and bound (Python, C++ mirror, Java), and the numpy restatement of
the S-transformation (tests/datum_reference.py) turns the oracle's bordered inverse in one datum into the oracle's own inverse in
another datum at the same parameter values."""
import ctypes as C
import dataclasses
import gzip
import os
import re
import subprocess

import numpy as np

import datum_reference
from bundle_adjustment_amd import engine, scene
from bundle_adjustment_amd.problem import packed_to_full

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jaicov_datum.h")
SHIM = os.path.join(ROOT, "java", "jni", "jaicov_jni.c")
JAVA = os.path.join(ROOT, "java", "org", "applied_geodesy", "adjustment", "bundle", "nativeengine", "NativeNormalEquationEngine.java")
GOLDEN = os.path.join(ROOT, "tests", "golden", "example")


def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(jaicov_datum_[a-z_0-9]+)\s*\(", src)))


def _lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def test_header_declarations_are_exported_and_bound():
    names = declared()
    assert names == sorted(engine.DATUM_EXPORTS) == ["jaicov_datum_apply", "jaicov_datum_transform"]
    assert not set(names) & set(engine.EXPORTS)
    L = _lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    for n in names:
        assert hasattr(L, n), n
        assert re.search(r"\bT %s\b" % n, syms), f"{n} is declared but not exported"
    assert callable(getattr(engine.Engine, "datum_transform")) and callable(getattr(engine.Engine, "datum_apply"))
    from bundle_adjustment_amd import host_api
    assert hasattr(host_api.BundleAdjustment, "transformDatum")


def test_every_datum_function_has_one_native_and_one_shim_twin():
    shim = open(SHIM).read()
    assert set(re.findall(r"\b(jaicov_datum_\w+)\s*\(", shim)) == set(declared())
    java = open(JAVA).read()
    natives = re.findall(r"private static native \w+ (datum[A-Z]\w*)\(", java)
    twins = re.findall(r"JNIEXPORT \w+ JNICALL NAT\((datum[A-Z]\w*)\)", shim)
    assert sorted(natives) == sorted(twins) == ["datumApply", "datumTransform"]
    for n in natives:
        body = shim[shim.index("NAT(%s)" % n):].split("JNIEXPORT")[0]
        assert len(re.findall(r"\b(jaicov_datum_\w+)\s*\(", body)) == 1, n


def test_null_engine_is_refused_and_outputs_stay():
    L = _lib()
    mask = np.ones(4, np.uint8)
    assert L.jaicov_datum_transform(None, mask.ctypes.data_as(C.POINTER(C.c_uint8)), 4) == -1
    v = np.ones(8); out = np.full(8, 3.0)
    pd = C.POINTER(C.c_double)
    assert L.jaicov_datum_apply(None, v.ctypes.data_as(pd), out.ctypes.data_as(pd), 8) == -1
    assert np.all(out == 3.0)


# ---- the restatement against the oracle -------------------------------------------------------------------------------------------
def _oracle_inverse(oracle_mod, fp, values):
    o = oracle_mod.Oracle(fp)
    _, Q, _, _ = o.step(values, fp.sigma2apriori, 0.0, True)
    return packed_to_full(Q, fp.n_unknowns), o


def _check_restatement(oracle_mod, fp_a, mask_b):
    fp_b = dataclasses.replace(fp_a, point_datum=np.asarray(mask_b, np.uint8))
    x = fp_a.values
    QA, _ = _oracle_inverse(oracle_mod, fp_a, x)
    QB, ob = _oracle_inverse(oracle_mod, fp_b, x)
    B = datum_reference.border_rows(ob, x)
    d = fp_a.rank_defect
    Qt = datum_reference.transform(QA, B, d)
    err = np.abs(Qt - QB).max() / np.abs(QB).max()
    print(f"restatement vs oracle: {err:.3e} of max|Q_B| (border rows included)")
    assert err <= 1e-11
    return QA, QB, B


def test_restatement_reproduces_the_oracle_tiny_free_all_to_three_points(oracle_mod):
    fp = scene.config("tiny_free")
    P = fp.point_datum.size
    assert fp.rank_defect == 6 and fp.point_datum.all()
    mask = np.zeros(P, np.uint8); mask[:3] = 1
    QA, QB, B = _check_restatement(oracle_mod, fp, mask)
    # S v: the transformation of a step is the linear part of the datum change (B' S v = 0)
    d = fp.rank_defect
    v = np.random.default_rng(3).normal(size=fp.n_unknowns)
    sv = datum_reference.apply(QA, B, d, v)
    assert np.all(sv[:d] == 0) and np.abs(B[:, d:] @ sv[d:]).max() <= 1e-12 * np.abs(v).max()


def test_restatement_reproduces_the_oracle_bundled_block(oracle_mod, tmp_path):
    """The bundled block at AICON's adjusted values: ExampleReport's datum (66 points of <= 3-character names) -> AICON's (all 150)."""
    from bundle_adjustment_amd import host_api as H
    from bundle_adjustment_amd.host_api import flat_problem
    with gzip.open(os.path.join(GOLDEN, "example.htm.gz")) as src, open(tmp_path / "example.htm", "wb") as dst:
        dst.write(src.read())
    pr = H.read_aicon_report(str(tmp_path / "example.htm"))
    cam = pr.cameras()[0]
    for p in pr.points():
        if len(p.getName()) > 3:
            p.setDatum(False)
    ba = H.BundleAdjustment()
    ba.add(cam)
    for sb in pr.scaleBars():
        ba.add(sb)
    ba.useCentroidedCoordinates(False)
    ba.prepareUnknownParameters(); ba.flatten()
    fp = flat_problem(ba).validate()
    assert fp.rank_defect == 6 and int(fp.point_datum.sum()) == 66
    _check_restatement(oracle_mod, fp, np.ones(fp.point_datum.size, np.uint8))
