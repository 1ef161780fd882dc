"""CPU: the C ABI of include/jaicov_resect.h is exported, bound in Python (engine.RESECT_EXPORTS) and in Java (one native, one
Java_... twin); bad arguments are refused before any device is touched; a valid call without a GPU is NO_DEVICE.  The restatement in
tests/resection_reference.py is held to truth: it recovers noise-free spatial scenes and plane fields with c of both signs, its
derivatives agree with finite differences and its cofactor matrix with numpy's inverse, it withdraws exactly a planted gross error and
reports degenerate input, its orientations of the bundled block are start values from which the oracle's adjustment converges, and on
every input of the GPU parity test its two summation orders agree to a tenth of the GPU bound."""
import ctypes as C
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resection_reference as X
from bundle_adjustment_amd import engine, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jaicov_resect.h")
SHIM = os.path.join(ROOT, "java", "jni", "jaicov_jni.c")
JAVA = os.path.join(ROOT, "java", "org", "applied_geodesy", "adjustment", "bundle", "nativeengine", "NativeNormalEquationEngine.java")
GOLDEN = os.path.join(ROOT, "tests", "golden", "example")
EXTENT = 2000.0        # object extent of the synthetic scenes, mm


def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(jaicov_resect_[a-z_0-9]+)\s*\(", src)))


def _lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def test_header_declarations_are_exported_and_bound_in_python():
    names = declared()
    assert names == sorted(engine.RESECT_EXPORTS) == ["jaicov_resect_images"]
    for other in (engine.EXPORTS, engine.XFORM_EXPORTS, engine.DLT_EXPORTS, engine.REL_EXPORTS, engine.DATUM_EXPORTS, engine.ISECT_EXPORTS):
        assert not set(names) & set(other)
    L = _lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    for n in names:
        assert hasattr(L, n), n
        assert re.search(r"\bT %s\b" % n, syms), f"{n} is declared but not exported"
    assert [engine.RESECT_OK, engine.RESECT_NOT_CONVERGED, engine.RESECT_TOO_FEW_POINTS, engine.RESECT_SINGULAR, engine.RESECT_NOT_FINITE] == \
        [X.OK, X.NOT_CONVERGED, X.TOO_FEW_POINTS, X.SINGULAR, X.NOT_FINITE] == list(range(5))
    assert [engine.RESECT_START_GIVEN, engine.RESECT_START_SPACE, engine.RESECT_START_PLANE] == \
        [X.START_GIVEN, X.START_SPACE, X.START_PLANE] == list(range(3))
    hdr = open(HEADER).read()
    for k, name in enumerate(("OK", "NOT_CONVERGED", "TOO_FEW_POINTS", "SINGULAR", "NOT_FINITE")):
        assert re.search(r"JAICOV_RESECT_%s = %d\b" % (name, k), hdr), name
    for k, name in enumerate(("GIVEN", "SPACE", "PLANE")):
        assert re.search(r"JAICOV_RESECT_START_%s = %d\b" % (name, k), hdr), name
    assert re.search(r"#define JAICOV_RESECT_OUT_PER_IMAGE %d\b" % X.NOUT, hdr)
    assert callable(engine.resect_images) and callable(engine.resect_problem)


def test_the_resection_has_one_native_and_one_shim_twin():
    shim = open(SHIM).read()
    assert set(re.findall(r"\b(jaicov_resect_\w+)\s*\(", shim)) == set(declared())
    java = open(JAVA).read()
    natives = re.findall(r"private static native \w+ (resect\w+)\(", java)
    twins = re.findall(r"JNIEXPORT \w+ JNICALL NAT\((resect\w+)\)", shim)
    assert natives == twins == ["resectImages"]
    body = shim[shim.index("NAT(resectImages)"):].split("JNIEXPORT")[0]
    assert len(re.findall(r"\bjaicov_resect_images\s*\(", body)) == 1
    assert "public static long[] resectImages(" in java


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def _call(L, n=1, begin=(0, 4), m=4, xy=True, xyz=True, var=None, io=True, eo=None, s0=1.0, it=10, thr=0.0, mp=4, out=True, st=True):
    b = (C.c_int32 * len(begin))(*begin) if begin is not None else None
    k = max(n, 1)
    pxy = (C.c_double * (2 * m))() if xy else None
    pxyz = (C.c_double * (3 * m))(*[float(i * i % 7) for i in range(3 * m)]) if xyz else None
    pvar = (C.c_double * (3 * m))(*var) if var is not None else None
    pio = (C.c_double * (3 * k))(*([0.0, 0.0, 28.0] * k)) if io else None
    peo = (C.c_double * (6 * k))(*eo) if eo is not None else None
    pout = (C.c_double * (28 * k))() if out else None
    pst = (C.c_int32 * k)() if st else None
    return L.jaicov_resect_images(n, b, pxy, pxyz, pvar, pio, peo, s0, it, thr, mp, pout, pst, None, None, None, None, None)


def test_bad_arguments_are_refused_without_a_device():
    L = _lib()
    bad = -1
    unit = (1.0, 1.0, 0.0) * 4
    assert _call(L, n=-1) == bad                                 # a negative count
    assert _call(L, begin=(1, 4)) == bad                         # the CSR does not start at 0
    assert _call(L, n=2, begin=(0, 4, 3)) == bad                 # ... decreases
    assert _call(L, var=(0.0, 1.0, 0.0) + unit[3:]) == bad       # variance <= 0
    assert _call(L, var=(1.0, -1.0, 0.0) + unit[3:]) == bad
    assert _call(L, var=unit[:9] + (1.0, 1.0, 1.0)) == bad       # |rho| >= 1
    assert _call(L, var=unit[:9] + (1.0, 1.0, -1.5)) == bad
    assert _call(L, var=(float("nan"), 1.0, 0.0) + unit[3:]) == bad
    assert _call(L, s0=0.0) == bad                               # sigma2apriori <= 0
    assert _call(L, s0=-1.0) == bad
    assert _call(L, it=0) == bad                                 # max_iterations < 1
    assert _call(L, mp=2) == bad                                 # min_points < 3
    assert _call(L, thr=-1.0) == bad                             # reject_threshold < 0
    for missing in ("begin", "xy", "xyz", "io", "out", "st"):    # NULL where it is not allowed
        assert _call(L, **{missing: None if missing == "begin" else False}) == bad, missing
    import torch
    if not torch.cuda.is_available():
        assert _call(L, var=unit, mp=3, eo=[1.0] * 6) == -6      # the same call with valid arguments passes the checks


def test_valid_call_without_a_device_is_no_device():
    import torch
    L = _lib()
    rc = _call(L, var=(1.0, 2.0, 0.3) * 4, thr=5.0)
    assert rc == (0 if torch.cuda.is_available() else -6)
    if not torch.cuda.is_available():
        with pytest.raises(engine.EngineError) as ei:
            engine.resect_images([0, 4], np.zeros((4, 2)), np.arange(12.0).reshape(4, 3), None, [[0, 0, 28.0]])
        assert ei.value.code == -6
        with pytest.raises(engine.EngineError) as ei:
            engine.resect_problem(X.scene_of("tiny"))
        assert ei.value.code == -6
    with pytest.raises(engine.EngineError) as ei:                # sizes that do not agree never reach the library
        engine.resect_images([0, 4], np.zeros((4, 2)), np.zeros((3, 3)), None, [[0, 0, 28.0]])
    assert ei.value.code == -1


# ---- the restatement is held to truth ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "cfg2"])
@pytest.mark.parametrize("negative_c", [False, True])
def test_restatement_recovers_a_noise_free_scene(name, negative_c):
    """Noise-free pinhole observations: every image's true orientation to 1e-9 of the 2 000 mm extent and 1e-9 rad (north_star's
    figures; measured 1.1e-12 mm and 4.4e-16 rad).  The linear start is exact up to rounding, so one Gauss-Newton step confirms it;
    from 6 points on it is the space start."""
    ob, xy, xyz, _, io, eo = X.batch_from_scene(X.scene_of(name), exact=True, c=-scene.C_EX if negative_c else None)
    out, st, it, kind, used, q = X.resect(ob, xy, xyz, None, io)
    assert (st == X.OK).all() and (it <= 2).all() and used.all()
    dx, da = np.abs(out[:, :3] - eo[:, :3]).max(), np.abs(X.wrap(out[:, 3:6] - eo[:, 3:6])).max()
    print(f"{name} c {'<' if negative_c else '>'} 0: {dx:.2e} mm, {da:.2e} rad from the truth")
    assert dx < 1e-9 * EXTENT and da < 1e-9
    assert (kind[np.diff(ob) >= 6] == X.START_SPACE).all()


@pytest.mark.parametrize("negative_c", [False, True])
def test_restatement_recovers_a_plane_field(negative_c):
    """Every point on one tilted plane, 4, 5 and 12 points per image: the space start does not exist (its 11 x 11 system is rank
    deficient), the plane start is taken, and the truth comes back to the same bounds (measured 6.8e-12 mm, 1.8e-15 rad)."""
    c = -scene.C_EX if negative_c else scene.C_EX
    ob, xy, xyz, _, io, eo = X.plane_batch([4, 5, 12] * 4, c=c)
    out, st, it, kind, used, q = X.resect(ob, xy, xyz, None, io)
    assert (st == X.OK).all() and (kind == X.START_PLANE).all() and used.all()
    dx, da = np.abs(out[:, :3] - eo[:, :3]).max(), np.abs(X.wrap(out[:, 3:6] - eo[:, 3:6])).max()
    print(f"plane field c = {c:g}: {dx:.2e} mm, {da:.2e} rad from the truth")
    assert dx < 1e-9 * EXTENT and da < 1e-9


def test_derivatives_agree_with_finite_differences():
    """The six derivatives of PDF:165-171 and 183-189 against central differences of the computed image coordinates, step h = 1e-6
    in the reduced unknowns: the truncation error h^2 and the rounding error EPS / h of values of order |c| = 29 are both about
    1e-10 relative to the derivative's magnitude; bound 1e-7."""
    ob, xy, xyz, _, io, eo = X.batch_from_scene(X.scene_of("tiny"), exact=True)
    sl = slice(ob[0], ob[1])
    Xc = xyz[sl].mean(0); s = np.sqrt(((xyz[sl] - Xc) ** 2).sum(1).mean())
    P = (xyz[sl] - Xc) / s
    par = np.concatenate([(eo[0, :3] - Xc) / s, eo[0, 3:]]) + [0.01, -0.02, 0.015, 0.02, -0.03, 0.01]
    zero = np.zeros_like(xy[sl])
    ax, ay, w0, w1 = X.collinearity(par, P, zero, io[0])          # w = -computed
    h = 1e-6
    for k in range(6):
        d = np.zeros(6); d[k] = h
        _, _, p0, p1 = X.collinearity(par + d, P, zero, io[0])
        _, _, m0, m1 = X.collinearity(par - d, P, zero, io[0])
        fx, fy = -(p0 - m0) / (2 * h), -(p1 - m1) / (2 * h)
        scale = max(np.abs(ax[k]).max(), np.abs(ay[k]).max())
        err = max(np.abs(fx - ax[k]).max(), np.abs(fy - ay[k]).max()) / scale
        assert err < 1e-7, (k, err)


def test_cofactor_matrix_is_the_inverse_of_the_assembled_normal_matrix():
    """Q of the 28 values against numpy.linalg.inv of N assembled at the final values in the caller's units.  Bound: cond(N) EPS with
    cond(N) up to 1e9 in these units (mm against rad) leaves 1e-7 of the largest entry; measured 1e-11."""
    fp = X.scene_of("cfg2")
    ob, xy, xyz, var, io, _ = X.batch_from_scene(fp)
    for g in (0, 7):
        sl = slice(ob[g], ob[g + 1])
        out, st, *_ = X.resect_image(xy[sl], xyz[sl], var[sl], io[g], sigma2=fp.sigma2apriori)
        assert st == X.OK
        p11, p12, p22 = X.weights(var[sl], fp.sigma2apriori, ob[g + 1] - ob[g])
        par = np.concatenate([np.zeros(3), out[3:6]])             # reduction Xc = X0, s = 1: the caller's units
        N = X.normal(par, xyz[sl] - out[:3], xy[sl], io[g], p11, p12, p22, np.arange(ob[g + 1] - ob[g]), "plain")[0]
        Q = X.cofactor(out)
        err = np.abs(Q - np.linalg.inv(N)).max() / np.abs(Q).max()
        assert np.abs(Q @ N - np.eye(6)).max() < 1e-6 and err < 1e-7, err


def test_restatement_withdraws_exactly_the_planted_gross_error():
    """sigma2apriori = 1 makes q the squared residual in units of the observations' variance: threshold 5 is 5 sigma, the planted
    error 50 sigma in x and in y."""
    ob, xy, xyz, var, io, eo, planted = X.gross_error_batch(X.scene_of("cfg2"))
    out, st, it, kind, used, q = X.resect(ob, xy, xyz, var, io, reject_threshold=5.0, min_points=6)
    assert (st == X.OK).all()
    assert np.array_equal(np.flatnonzero(used == 0), np.sort(planted))
    assert q[used == 1].max() <= 25.0 < q[used == 0].min()
    assert np.abs(out[:, :3] - eo[:, :3]).max() < 1.0             # mm: the noise of 0.5 um leaves the orientations at the truth


def test_restatement_reports_degenerate_input():
    batch, expected = X.degenerate_batch()
    out, st, it, kind, used, q = X.resect(*batch)
    assert list(st) == expected == [X.OK, X.TOO_FEW_POINTS, X.SINGULAR, X.NOT_FINITE, X.OK]
    ob = batch[0]
    for g, e in enumerate(expected):
        s = slice(ob[g], ob[g + 1])
        assert np.isnan(out[g]).all() == (e != X.OK) and used[s].all() == (e == X.OK) and np.isnan(q[s]).all() == (e != X.OK)
    assert it[1] == 0 and kind[1] == 0
    # 3 points are enough with start values, and too few without
    ob, xy, xyz, var, io, eo = X.batch_from_scene(X.scene_of("tiny"), exact=True)
    sel = ob[0] + np.array([0, 5, 9])
    assert X.resect_image(xy[sel], xyz[sel], None, io[0])[1] == X.TOO_FEW_POINTS
    o, s_, *_ = X.resect_image(xy[sel], xyz[sel], None, io[0], eo[0] + [1.0, -1.0, 1.0, 0.001, -0.001, 0.001])
    assert s_ == X.OK and np.abs(o[:3] - eo[0, :3]).max() < 1e-6
    assert X.resect_image(xy[sel[:2]], xyz[sel[:2]], None, io[0], eo[0])[1] == X.TOO_FEW_POINTS


# ---- start values suffice --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example_base(tmp_path_factory):
    d = tmp_path_factory.mktemp("example")
    for f in ("ior", "eor", "obc", "scale"):
        shutil.copy(os.path.join(GOLDEN, f"example.{f}"), d)
    with gzip.open(os.path.join(GOLDEN, "example.phc.gz")) as src, open(d / "example.phc", "wb") as dst:
        dst.write(src.read())
    return str(d / "example")


def test_resected_orientations_of_the_bundled_block_are_sufficient_start_values(example_base, oracle_mod):
    """The block's 115 images resected from the .obc points and the .ior camera.  The resection models no distortion, so its
    orientations differ from the adjusted .eor values (the figure is printed, not asserted); from them the oracle reaches state 1
    with the sigma0 of the run from the .eor values, to 1e-9 relative."""
    fp = X.example_problem(example_base)
    out, st, it, kind, used, q = X.resect(*X.batch_from_problem(fp), sigma2=fp.sigma2apriori)
    assert (st == X.OK).all()
    v = np.array(fp.values, np.float64)
    e0 = fp.slot_eo(0)
    eor = v[e0:].reshape(-1, 6).copy()
    print(f"{len(st)} images, start kinds {np.bincount(kind, minlength=3)}: largest difference from .eor "
          f"{np.abs(out[:, :3] - eor[:, :3]).max():.3f} mm, {np.abs(X.wrap(out[:, 3:6] - eor[:, 3:6])).max():.6f} rad")
    v[e0:] = out[:, :6].ravel()
    _, _, r0 = oracle_mod.Oracle(fp).estimate(invert=False)
    _, _, r1 = oracle_mod.Oracle(fp).estimate(values=v, invert=False)
    assert r0.state == 1 and r1.state == 1
    s0, s1 = np.sqrt(r0.omega / fp.degree_of_freedom), np.sqrt(r1.omega / fp.degree_of_freedom)
    print(f"sigma0 from .eor {s0:.9f} in {r0.iterations} passes, from the resection {s1:.9f} in {r1.iterations} passes")
    assert abs(s1 - s0) < 1e-9 * s0


# ---- the parity inputs' own spread -------------------------------------------------------------------------------------------------------
def test_both_summation_orders_agree_on_every_parity_input(example_base):
    """On every input on which tests/test_gpu_resection.py holds the device against the restatement, the restatement in the kernel's
    summation order (lane-strided partial sums, then the butterfly) and in plain observation order agree in status, iterations, start
    kind and used flags, and in value to 1e-10 of a column's magnitude: a tenth of the GPU bound, so that bound is not spent on the
    input's own sensitivity to the order of its sums.  An input that fails this is replaced in resection_reference, not skipped."""
    worst = {}
    for name, batch, kw in X.parity_inputs(example_base):
        a = X.resect(*batch, **kw)
        b = X.resect(*batch, order="lanes", **kw)
        for k, what in ((1, "status"), (2, "iterations"), (3, "start kind"), (4, "used")):
            assert np.array_equal(a[k], b[k]), (name, what)
        err = 0.0
        for u, v in ((a[0], b[0]), (a[5][:, None], b[5][:, None])):
            assert np.array_equal(np.isnan(u), np.isnan(v)), name
            ok = ~np.isnan(u)
            col = np.nanmax(np.abs(np.where(ok, u, np.nan)), axis=0) if ok.any() else np.ones(u.shape[1])
            col = np.where(np.isnan(col) | (col == 0), 1.0, col)
            err = max(err, float((np.abs(np.where(ok, u - v, 0.0)) / col).max()))
        worst[name] = err
        print(f"{name}: {err:.2e}")
        assert err <= 1e-10, (name, err)
    assert "bundled block" in worst and len(worst) >= 14
