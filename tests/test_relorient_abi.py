"""CPU: the C ABI of include/jaicov_relorient.h is exported, bound in Python (engine.RELOR_EXPORTS) and in Java (one native, one
Java_... twin, counted in the documents); bad arguments are refused
before any device is touched; a valid call without a GPU is NO_DEVICE.  The restatement in tests/relorient_reference.py is held to
truth: it recovers noise-free pairs (c of both signs, two different cameras) and plane fields, its derivatives and weights agree
with finite differences and its cofactor matrix with the pseudo-inverse, it withdraws exactly a planted gross error and reports
degenerate input; and on every input of the GPU parity test its two summation orders agree to a tenth of the GPU bound, the choice
between the runs does not hang on rounding, and no q lies near the rejection threshold."""
import ctypes as C
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import relorient_reference as R
from bundle_adjustment_amd import engine, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "jaicov_relorient.h")
SHIM = os.path.join(ROOT, "java", "jni", "jaicov_jni.c")
JAVA = os.path.join(ROOT, "java", "org", "applied_geodesy", "adjustment", "bundle", "nativeengine", "NativeNormalEquationEngine.java")
GOLDEN = os.path.join(ROOT, "tests", "golden", "example")


def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(jaicov_relorient_[a-z_0-9]+)\s*\(", src)))


def _lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def test_header_declarations_are_exported_and_bound_in_python():
    names = declared()
    assert names == sorted(engine.RELOR_EXPORTS) == ["jaicov_relorient_pairs"]
    for other in (engine.EXPORTS, engine.XFORM_EXPORTS, engine.DLT_EXPORTS, engine.REL_EXPORTS, engine.DATUM_EXPORTS, engine.ISECT_EXPORTS,
                  engine.RESECT_EXPORTS):
        assert not set(names) & set(other)
    L = _lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True).stdout
    for n in names:
        assert hasattr(L, n), n
        assert re.search(r"\bT %s\b" % n, syms), f"{n} is declared but not exported"
    assert [engine.RELOR_OK, engine.RELOR_NOT_CONVERGED, engine.RELOR_TOO_FEW_POINTS, engine.RELOR_SINGULAR, engine.RELOR_NOT_FINITE] == \
        [R.OK, R.NOT_CONVERGED, R.TOO_FEW_POINTS, R.SINGULAR, R.NOT_FINITE] == list(range(5))
    assert [engine.RELOR_START_GIVEN, engine.RELOR_START_SPACE, engine.RELOR_START_PLANE] == \
        [R.START_GIVEN, R.START_SPACE, R.START_PLANE] == list(range(3))
    hdr = open(HEADER).read()
    for k, name in enumerate(("OK", "NOT_CONVERGED", "TOO_FEW_POINTS", "SINGULAR", "NOT_FINITE")):
        assert re.search(r"JAICOV_RELOR_%s = %d\b" % (name, k), hdr), name
    for k, name in enumerate(("GIVEN", "SPACE", "PLANE")):
        assert re.search(r"JAICOV_RELOR_START_%s = %d\b" % (name, k), hdr), name
    assert re.search(r"#define JAICOV_RELOR_OUT_PER_PAIR %d\b" % R.NOUT, hdr)
    assert callable(engine.relorient_pairs) and callable(engine.relorient_problem)


def test_the_relative_orientation_has_one_native_and_one_shim_twin():
    shim = open(SHIM).read()
    assert set(re.findall(r"\b(jaicov_relorient_\w+)\s*\(", shim)) == set(declared())
    java = open(JAVA).read()
    natives = re.findall(r"private static native \w+ (orient\w+)\(", java)
    twins = re.findall(r"JNIEXPORT \w+ JNICALL NAT\((orient\w+)\)", shim)
    assert natives == twins == ["orientPairs"]
    body = shim[shim.index("NAT(orientPairs)"):].split("JNIEXPORT")[0]
    assert len(re.findall(r"\bjaicov_relorient_pairs\s*\(", body)) == 1
    assert "public static long[] orientPairs(" in java
    # the natives count of the documents is the number of natives there are, this one included
    n = len(re.findall(r"private static native ", java))
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        for claimed in re.findall(r"(\d+) natives", open(os.path.join(ROOT, doc)).read()):
            assert int(claimed) == n, (doc, claimed)


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def _call(L, n=1, begin=(0, 6), m=6, xa=True, xb=True, va=None, vb=None, io=True, start=None, s0=1.0, it=10, thr=0.0, mp=6, out=True, st=True):
    b = (C.c_int32 * len(begin))(*begin) if begin is not None else None
    k = max(n, 1)
    pxa = (C.c_double * (2 * m))(*[float(i * i % 7) for i in range(2 * m)]) if xa else None
    pxb = (C.c_double * (2 * m))(*[float(i * i % 5) for i in range(2 * m)]) if xb else None
    pva = (C.c_double * (3 * m))(*va) if va is not None else None
    pvb = (C.c_double * (3 * m))(*vb) if vb is not None else None
    pio = (C.c_double * (6 * k))(*([0.0, 0.0, 28.0, 0.0, 0.0, -28.0] * k)) if io else None
    pst = (C.c_double * (6 * k))(*start) if start is not None else None
    pout = (C.c_double * (28 * k))() if out else None
    pstat = (C.c_int32 * k)() if st else None
    return L.jaicov_relorient_pairs(n, b, pxa, pxb, pva, pvb, pio, pst, s0, it, thr, mp, pout, pstat, None, None, None, None, None)


def test_bad_arguments_are_refused_without_a_device():
    L = _lib()
    bad = -1
    unit = (1.0, 1.0, 0.0) * 6
    assert _call(L, n=-1) == bad                                 # a negative count
    assert _call(L, begin=(1, 6)) == bad                         # the CSR does not start at 0
    assert _call(L, n=2, begin=(0, 6, 5)) == bad                 # ... decreases
    for side in ("va", "vb"):                                    # the variances of either image
        assert _call(L, **{side: (0.0, 1.0, 0.0) + unit[3:]}) == bad       # variance <= 0
        assert _call(L, **{side: (1.0, -1.0, 0.0) + unit[3:]}) == bad
        assert _call(L, **{side: unit[:15] + (1.0, 1.0, 1.0)}) == bad      # |rho| >= 1
        assert _call(L, **{side: unit[:15] + (1.0, 1.0, -1.5)}) == bad
        assert _call(L, **{side: (float("nan"), 1.0, 0.0) + unit[3:]}) == bad
    assert _call(L, s0=0.0) == bad                               # sigma2apriori <= 0
    assert _call(L, s0=-1.0) == bad
    assert _call(L, it=0) == bad                                 # max_iterations < 1
    assert _call(L, mp=4) == bad                                 # min_points < 5
    assert _call(L, thr=-1.0) == bad                             # reject_threshold < 0
    for missing in ("begin", "xa", "xb", "io", "out", "st"):     # NULL where it is not allowed
        assert _call(L, **{missing: None if missing == "begin" else False}) == bad, missing
    import torch
    if not torch.cuda.is_available():
        assert _call(L, va=unit, vb=unit, mp=5, start=[1.0] * 6) == -6     # the same call with valid arguments passes the checks


def test_valid_call_without_a_device_is_no_device():
    import torch
    L = _lib()
    rc = _call(L, va=(1.0, 2.0, 0.3) * 6, thr=5.0)
    assert rc == (0 if torch.cuda.is_available() else -6)
    if not torch.cuda.is_available():
        with pytest.raises(engine.EngineError) as ei:
            engine.relorient_pairs([0, 6], np.zeros((6, 2)), np.ones((6, 2)), None, None, [[0, 0, 28.0, 0, 0, 28.0]])
        assert ei.value.code == -6
        with pytest.raises(engine.EngineError) as ei:
            engine.relorient_problem(R.scene_of("tiny"), 0, 1)
        assert ei.value.code == -6
    with pytest.raises(engine.EngineError) as ei:                # sizes that do not agree never reach the library
        engine.relorient_pairs([0, 6], np.zeros((6, 2)), np.zeros((5, 2)), None, None, [[0, 0, 28.0, 0, 0, 28.0]])
    assert ei.value.code == -1


# ---- the restatement is held to truth ------------------------------------------------------------------------------------------------
CAMERAS = {"c > 0": {}, "c < 0": dict(c=-scene.C_EX), "two cameras": dict(c=scene.C_EX, c_b=-1.7 * scene.C_EX)}


@pytest.mark.parametrize("name", ["tiny", "cfg2"])
@pytest.mark.parametrize("cameras", list(CAMERAS))
def test_restatement_recovers_noise_free_pairs(name, cameras):
    """Noise-free pinhole observations of four pairs: the true base direction to 1e-9 and the true rotation to 1e-9 rad (north_star's
    figure; measured 1.3e-15 and 7e-16).  The difference of two rotations is taken between their matrices."""
    batch, truth, _ = R.pairs_of_scene(R.scene_of(name), R.SCENE_PAIRS, exact=True, **CAMERAS[cameras])
    out, st, it, kind, used, q = R.relorient(*batch[:3], None, None, *batch[5:])
    assert (st == R.OK).all() and used.all()
    db, dr = R.pose_error(out, truth)
    print(f"{name} {cameras}: base {db:.2e}, rotation {dr:.2e} from the truth, iterations {it}, start kinds {kind}")
    assert db < 1e-9 and dr < 1e-9


@pytest.mark.parametrize("thickness", [0.0, 0.01])
def test_restatement_recovers_plane_fields(thickness):
    """6, 8, 12 and 40 points on a plane or within 1 % of the extent of it: the plane start is taken (on the exact plane the space
    start does not exist), and the truth comes back to the same bounds.  (The exact fields of this seed have one solution in front
    of both cameras; where both decompositions are, Omega cannot choose, as the header says.)"""
    batch, truth, _ = R.plane_batch([6, 8, 12, 40], thickness=thickness)
    out, st, it, kind, used, q = R.relorient(*batch[:3], None, None, *batch[5:])
    assert (st == R.OK).all() and used.all()
    if thickness == 0.0:
        assert (kind == R.START_PLANE).all() and (out[:, 27] / scene.C_EX ** 2 < 1e-20).all()
    db, dr = R.pose_error(out, truth)
    print(f"plane field, thickness {thickness}: base {db:.2e}, rotation {dr:.2e} from the truth, start kinds {kind}")
    assert db < 1e-9 and dr < 1e-9


def _condition(par, ua, va, ub, vb):
    """g of every point, written from the header: d_b' R' [b]x d_a"""
    Rm = scene.rotation(*par[3:])
    da = np.stack([ua, va, np.ones_like(ua)], 1); db = np.stack([ub, vb, np.ones_like(ub)], 1)
    return np.einsum("ij,ij->i", db @ Rm.T, np.cross(par[:3], da))


def test_derivatives_and_weights_agree_with_finite_differences():
    """N = sum p a a', n = -sum p a g and p = 1 / (j' Q j) of the restatement against central differences of g, step h = 1e-6: the
    truncation error h^2 and the rounding error EPS / h are both about 1e-10 of values of order 1; bound 1e-7."""
    rng = np.random.default_rng(0)
    m = 9
    ua, va, ub, vb = rng.normal(0, 0.3, (4, m))
    qa = (rng.uniform(1, 2, m), rng.uniform(-0.5, 0.5, m), rng.uniform(1, 2, m))
    qb = (rng.uniform(1, 2, m), rng.uniform(-0.5, 0.5, m), rng.uniform(1, 2, m))
    par = np.array([0.6, -0.2, 0.77, 0.1, -0.3, 0.5]); par[:3] /= np.linalg.norm(par[:3])
    e1, e2 = R.tangent(par[:3])
    h = 1e-6
    J = np.zeros((m, 5))
    for j in range(5):
        d = np.zeros(6)
        if j < 2:
            d[:3] = h * np.array(e1 if j == 0 else e2)
        else:
            d[1 + j] = h
        J[:, j] = (_condition(par + d, ua, va, ub, vb) - _condition(par - d, ua, va, ub, vb)) / (2 * h)
    obs = [ua, va, ub, vb]
    G = np.zeros((m, 4))
    for j in range(4):
        hi = [o.copy() for o in obs]; lo = [o.copy() for o in obs]
        hi[j] = hi[j] + h; lo[j] = lo[j] - h
        G[:, j] = (_condition(par, *hi) - _condition(par, *lo)) / (2 * h)
    cof = (qa[0] * G[:, 0] ** 2 + 2 * qa[1] * G[:, 0] * G[:, 1] + qa[2] * G[:, 1] ** 2 +
           qb[0] * G[:, 2] ** 2 + 2 * qb[1] * G[:, 2] * G[:, 3] + qb[2] * G[:, 3] ** 2)
    g = _condition(par, ua, va, ub, vb)
    N, n, omega, q = R.normal(par, e1, e2, (ua, va, ub, vb, qa, qb), np.arange(m), "plain")
    assert np.abs(q * cof / g ** 2 - 1.0).max() < 1e-7
    Nf, nf = (J.T / cof) @ J, -(J.T / cof) @ g
    assert np.abs(N - Nf).max() < 1e-7 * np.abs(N).max() and np.abs(n - nf).max() < 1e-7 * np.abs(n).max()
    assert abs(omega - (g ** 2 / cof).sum()) < 1e-7 * omega
    assert abs(np.dot(e1, par[:3])) < 1e-15 and abs(np.dot(e2, par[:3])) < 1e-15 and abs(np.dot(e1, e2)) < 1e-15


def test_cofactor_matrix_has_rank_five_and_inverts_the_normal_matrix():
    """The 6 x 6 cofactor matrix of a noisy pair: b is its null vector (the base length is not estimable), and on the tangent basis it
    is the inverse of N assembled at the returned values.  Bound: cond(N) EPS, cond(N) < 1e6 here, leaves 1e-9; asked 1e-7."""
    fp = R.scene_of("cfg2")
    batch = R.pairs_of_scene(fp, R.SCENE_PAIRS[:1])[0]
    out, st, *_ = R.relorient(*batch, sigma2=fp.sigma2apriori)
    assert st[0] == R.OK
    Q = R.X.cofactor(out[0])
    assert np.abs(Q[:, :3] @ out[0, :3]).max() < 1e-12 * np.abs(Q).max()
    e1, e2 = R.tangent(out[0, :3])
    J = np.zeros((6, 5)); J[:3, 0] = e1; J[:3, 1] = e2; J[3:, 2:] = np.eye(3)
    m = batch[0][1]
    ua, va = -(batch[1][:, 0] - batch[5][0, 0]) / batch[5][0, 2], -(batch[1][:, 1] - batch[5][0, 1]) / batch[5][0, 2]
    ub, vb = -(batch[2][:, 0] - batch[5][0, 3]) / batch[5][0, 5], -(batch[2][:, 1] - batch[5][0, 4]) / batch[5][0, 5]
    obs = (ua, va, ub, vb, R.cofactors(batch[3], fp.sigma2apriori, batch[5][0, 2], m), R.cofactors(batch[4], fp.sigma2apriori, batch[5][0, 5], m))
    N = R.normal(out[0, :6], e1, e2, obs, np.arange(m), "plain")[0]
    Q5 = J.T @ Q @ J
    assert np.abs(Q5 @ N - np.eye(5)).max() < 1e-7 and np.abs(J @ Q5 @ J.T - Q).max() < 1e-12 * np.abs(Q).max()
    assert np.linalg.matrix_rank(Q, tol=1e-10 * np.abs(Q).max()) == 5


def test_restatement_withdraws_exactly_the_planted_gross_error():
    """sigma2apriori = 1 makes q the squared misclosure in units of its variance: threshold 5 is 5 sigma, the planted error 50 sigma
    in x and in y of image b."""
    batch, planted = R.gross_error_batch()
    out, st, it, kind, used, q = R.relorient(*batch, reject_threshold=5.0, min_points=8)
    assert (st == R.OK).all()
    assert np.array_equal(np.flatnonzero(used == 0), np.sort(planted))
    assert q[used == 1].max() <= 25.0 < q[used == 0].min()


def test_restatement_reports_degenerate_input():
    batch, expected = R.degenerate_batch()
    out, st, it, kind, used, q = R.relorient(*batch)
    assert list(st) == expected == [R.OK, R.SINGULAR, R.NOT_FINITE, R.TOO_FEW_POINTS, R.OK]
    ob = batch[0]
    for g, e in enumerate(expected):
        s = slice(ob[g], ob[g + 1])
        assert np.isnan(out[g]).all() == (e != R.OK) and used[s].all() == (e == R.OK) and np.isnan(q[s]).all() == (e != R.OK)
    assert it[3] == 0 and kind[3] == 0
    # 5 points are enough with start values, and too few without; 4 are too few either way
    (ob, xa, xb, va, vb, io, _), truth, _ = R.pairs_of_scene(R.scene_of("tiny"), R.SCENE_PAIRS[:1], exact=True)
    sel = np.array([0, 3, 6, 9, 12])
    assert R.relorient_pair(xa[sel], xb[sel], None, None, io[0])[1] == R.TOO_FEW_POINTS
    o, s_, *_ = R.relorient_pair(xa[sel], xb[sel], None, None, io[0], truth[0] + [0.01, -0.01, 0.01, 0.001, -0.001, 0.001])
    assert s_ == R.OK and R.pose_error(o[None], truth)[0] < 1e-6
    assert R.relorient_pair(xa[sel[:4]], xb[sel[:4]], None, None, io[0], truth[0])[1] == R.TOO_FEW_POINTS


# ---- the parity inputs -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example_base(tmp_path_factory):
    d = tmp_path_factory.mktemp("example")
    for f in ("ior", "eor", "obc", "scale"):
        shutil.copy(os.path.join(GOLDEN, f"example.{f}"), d)
    with gzip.open(os.path.join(GOLDEN, "example.phc.gz")) as src, open(d / "example.phc", "wb") as dst:
        dst.write(src.read())
    return str(d / "example")


@pytest.fixture(scope="module")
def parity_runs(example_base):
    """every parity input once in each summation order, with the plain order's runs: shared by the tests below"""
    runs = []
    for name, batch, kw in R.parity_inputs(example_base):
        info = {}
        a = R.relorient(*batch, info=info, **kw)
        b = R.relorient(*batch, order="lanes", **kw)
        runs.append((name, batch, kw, a, b, info))
    return runs


def test_both_summation_orders_agree_on_every_parity_input(parity_runs):
    """On every input on which tests/test_gpu_relorient.py holds the device against the restatement, the restatement in the kernel's
    summation order and in plain observation order agree in status, iterations, start kind and used flags, and in value to 1e-10 of a
    column's magnitude: a tenth of the GPU bound (the sibling's bound).  An input that fails this is replaced in relorient_reference,
    not skipped."""
    worst = {}
    for name, batch, kw, a, b, _ in parity_runs:
        for k, what in ((1, "status"), (2, "iterations"), (3, "start kind"), (4, "used")):
            assert np.array_equal(a[k], b[k]), (name, what, a[k][:12], b[k][:12])
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
    assert "bundled block" in worst and len(worst) >= 15


def test_no_choice_on_a_parity_input_hangs_on_rounding(parity_runs):
    """Where a pair of a parity input has more than one run, the returned one either ends in a better status than every other, or its
    Omega lies below the other's by more than 1e-6 relative, or the other is the same pose (base direction and rotation matrix within
    1e-6): then rounding of 1e-16 cannot change what is returned."""
    compared = 0
    for name, batch, kw, a, b, info in parity_runs:
        for g, inf in info.items():
            runs = inf.get("runs", [])
            if len(runs) < 2:
                continue
            w = runs[inf["win"]]
            for k, r in enumerate(runs):
                if k == inf["win"]:
                    continue
                compared += 1
                same_pose = max(R.pose_error(w[3][None], r[3][None])) < 1e-6
                assert same_pose or w[1] < r[1] or (w[1] == r[1] and w[2] < r[2] * (1.0 - 1e-6)), (name, g, w[:3], r[:3])
    assert compared >= 40


def test_no_q_of_a_parity_input_lies_near_the_rejection_threshold(parity_runs):
    """On the parity inputs with rejection, no q that rejection could still take (a used observation of a pair above min_points) lies
    within 1 % of threshold^2: rounding cannot change a decision."""
    seen = 0
    for name, batch, kw, a, b, _ in parity_runs:
        if not kw.get("reject_threshold"):
            continue
        seen += 1
        thr2 = kw["reject_threshold"] ** 2
        counts = np.diff(batch[0])
        nused = np.add.reduceat(a[4].astype(np.int64), batch[0][:-1].astype(np.intp))
        can_go = np.repeat(nused > kw["min_points"], counts) & (a[4] == 1)
        q = a[5][can_go]
        assert not ((q > 0.99 * thr2) & (q < 1.01 * thr2)).any(), name
        assert (a[4] == 0).sum() > 0, name
    assert seen >= 2
