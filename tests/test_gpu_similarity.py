"""GPU: the absolute orientation of include/jaicov_simil.h against the restatement in tests/similarity_reference.py: parity on every
input of similarity_reference.parity_inputs, exact recovery (plane fields, angles near pi and coordinates of 1e6 included), point counts
at the lane and chunk boundaries with rejection, degenerate input, given and closed starts in one batch, batch independence and
determinism, jaicov_simil_apply against numpy, the device's memory census, the chain relative orientation, intersection, resection,
intersection, absolute orientation on an exact scene, the C++ mirror, and host/example_absolute on the bundled block."""
import copy
import ctypes as C
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import similarity_reference as S
from bundle_adjustment_amd import engine, scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "example")
EXTENT = 2000.0        # object extent of the synthetic scenes, mm


def same(dev, ref, rtol=1e-9):
    """same() of tests/test_gpu_resection.py: NaN positions equal, values within rtol of each column's magnitude over the batch"""
    dev = np.asarray(dev, np.float64).reshape(len(dev), -1)
    ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    assert np.array_equal(np.isnan(dev), np.isnan(ref))
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    col = np.nanmax(np.abs(np.where(ok, ref, np.nan)), axis=0)
    col = np.where(np.isnan(col) | (col == 0), 1.0, col)
    err = float((np.abs(np.where(ok, dev - ref, 0.0)) / col).max())
    assert err <= rtol, err
    return err


def check(batch, **kw):
    """one device call against the restatement: status, iterations, start kind and pt_used equal, values and q within same()"""
    dev = engine.similarity_models(*batch, **kw)
    ref = S.similarity(*batch, **kw)
    for k, what in ((1, "status"), (2, "iterations"), (3, "start kind"), (4, "used")):
        assert np.array_equal(dev[k], ref[k]), (what, np.flatnonzero(dev[k] != ref[k])[:5], dev[k][:12], ref[k][:12])
    worst = max(same(dev[0], ref[0]), same(dev[5][:, None], ref[5][:, None]))
    return dev, ref, worst


def test_parity_with_the_restatement():
    """Every input of similarity_reference.parity_inputs.  The summation orders differ (lanes and a butterfly here, point order
    there), so bit parity is not asked; tests/test_similarity_abi.py holds the restatement's own spread between the two orders on these
    inputs below a tenth of this bound."""
    names = []
    for name, batch, kw in S.parity_inputs():
        dev, ref, worst = check(batch, **kw)
        print(f"{name}: status {np.bincount(dev[1], minlength=5)}, start kinds {np.bincount(dev[3], minlength=2)}, iterations {dev[2][:12]}, "
              f"{int((dev[4] == 0).sum())} not used, worst relative difference to the restatement {worst:.2e}")
        names.append(name)
    assert len(names) >= 12


EXACT = {"space": dict(counts=[3, 4, 12, 200]), "plane": dict(counts=[4, 40], plane=True),
         "near pi": dict(counts=[3, 4, 12, 200], angles=S.NEAR_PI),
         "offset 1e6": dict(counts=[3, 4, 12, 200], offset=1.0e6), "plane, offset 1e6": dict(counts=[4, 40], plane=True, offset=1.0e6)}


@pytest.mark.parametrize("case", list(EXACT))
@pytest.mark.parametrize("weights", ["none", "cofactors"])
def test_exact_transformations_are_recovered(case, weights):
    """Noise-free point sets: T to 1e-9 of the coordinate magnitude (the extent, or the offset where it is larger), m to 1e-9 relative,
    the rotation matrix to 1e-9 (the restatement reaches 1e-12 or better)."""
    kw = EXACT[case]
    batch, truth = S.models(seed=3, **kw)
    out, st, it, kind, used, q = engine.similarity_models(*(batch[:3] if weights == "none" else batch[:5]))
    assert (st == engine.SIMIL_OK).all() and used.all() and (kind == engine.SIMIL_START_CLOSED).all()
    dt, dm, dr = S.pose_error(out, truth, max(1000.0, kw.get("offset", 0.0)))
    print(f"{case}, {weights}: T {dt:.2e}, m {dm:.2e}, R {dr:.2e} from the truth, iterations {it}")
    assert dt < 1e-9 and dm < 1e-9 and dr < 1e-9


def test_point_counts_at_the_lane_and_chunk_boundaries():
    """3, 4 (start values given), 5, 63, 64, 65, 127, 128, 129, 200 points: every model is solved; with rejection the rounds restart
    inside the kernel on resident (<= 128) and on chunked models alike, and exactly the planted errors go."""
    batch, counts, truth = S.lane_batch()
    assert sorted(counts) == S.COUNTS
    dev, ref, worst = check(batch)
    assert (dev[1] == engine.SIMIL_OK).all()
    assert (dev[3][counts == 4] == engine.SIMIL_START_GIVEN).all() and (dev[3][counts != 4] == engine.SIMIL_START_CLOSED).all()
    batch, counts, bad = S.lane_batch_with_gross_errors()
    dev, ref, _ = check(batch, reject_threshold=8.0, min_points=4)
    assert np.array_equal(np.flatnonzero(dev[4] == 0), np.sort(bad))
    print(f"counts {sorted(counts)}: worst relative difference to the restatement {worst:.2e}; {bad.size} planted errors withdrawn")


def test_given_and_closed_starts_in_one_batch():
    batch = S.mixed_start_batch()
    dev, ref, worst = check(batch)
    assert (dev[1] == engine.SIMIL_OK).all()
    assert (dev[3][0::2] == engine.SIMIL_START_GIVEN).all() and (dev[3][1::2] == engine.SIMIL_START_CLOSED).all()
    free = engine.similarity_models(*batch[:5])
    assert same(dev[0][:, :7], free[0][:, :7], 1e-7) < 1e-7    # both starts end at the same values, to the convergence criterion


def test_planted_gross_errors_are_withdrawn():
    """100 sigma on one point per model, threshold 6 (the cofactors are the noise's own: q in units of the variance), min_points 5."""
    batch, planted = S.gross_error_batch()
    dev, ref, worst = check(batch, reject_threshold=6.0, min_points=5)
    assert np.array_equal(np.flatnonzero(dev[4] == 0), np.sort(planted))
    assert (dev[1] == engine.SIMIL_OK).all()
    print(f"rejection: {planted.size} points withdrawn, worst relative difference to the restatement {worst:.2e}")


def test_degenerate_input_does_not_disturb_its_neighbours():
    batch, expected = S.degenerate_batch()
    dev, ref, _ = check(batch)
    out, st, it, kind, used, q = dev
    pb = batch[0]
    assert list(st) == expected
    for g, e in enumerate(expected):
        s = slice(pb[g], pb[g + 1])
        if e == S.OK:
            assert np.isfinite(out[g]).all() and used[s].all() and np.isfinite(q[s]).all()
        else:
            assert np.isnan(out[g]).all() and not used[s].any() and np.isnan(q[s]).all() and kind[g] == 0
    assert out[0].tobytes() == out[4].tobytes() and q[pb[0]:pb[1]].tobytes() == q[pb[4]:pb[5]].tobytes()
    # max_iterations = 1 on noisy data: values are returned all the same
    dev, ref, _ = check(S.models([12, 40], seed=5, sigma=S.SIGMA)[0], max_iterations=1)
    assert (dev[1] == engine.SIMIL_NOT_CONVERGED).all() and np.isfinite(dev[0]).all()


def test_batch_independence_and_determinism():
    """The lane-boundary models with gross errors, four more and the degenerate ones, twice over, with rejection.  Two runs give the
    same bits; a model alone gives the bits it gives inside the batch."""
    lb = S.lane_batch_with_gross_errors()[0]
    mx = S.mixed_start_batch()
    dg = S.degenerate_batch()[0]
    begin, *arrays = S.cat([mx, lb, dg] * 2)
    assert begin.size - 1 == 38
    kw = dict(reject_threshold=8.0, min_points=4)
    a = engine.similarity_models(begin, *arrays, **kw)
    b = engine.similarity_models(begin, *arrays, **kw)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    for g in (0, 1, 4, 7, 9, 13, 14, 15, 16, 20, 37):
        s = slice(begin[g], begin[g + 1])
        o = engine.similarity_models([0, begin[g + 1] - begin[g]], arrays[0][s], arrays[1][s], arrays[2][s], arrays[3][s], arrays[4][g:g + 1], **kw)
        assert o[0].tobytes() == a[0][g:g + 1].tobytes() and all(o[k][0] == a[k][g] for k in (1, 2, 3)), g
        assert o[4].tobytes() == a[4][s].tobytes() and o[5].tobytes() == a[5][s].tobytes(), g


def test_apply_against_numpy():
    """Points, their cofactors and image orientations of five models, one of them with a NaN parameter and one without images: against
    the header's formulas in numpy.  Bounds: coordinates to 1e-12 of their magnitude, cofactors to 1e-12 of theirs, rotations (compared
    between matrices, the angles near +-pi included) to 1e-12."""
    rng = np.random.default_rng(1)
    n = 5
    par = np.column_stack([rng.uniform(-5000, 5000, (n, 3)), rng.uniform(0.5, 300.0, n), rng.uniform(-3.1, 3.1, n), rng.uniform(-1.3, 1.3, n),
                           rng.uniform(-3.1, 3.1, n)])
    par[3, 5] = np.nan
    pb = np.array([0, 7, 7, 300, 310, 1000], np.int32)
    ib = np.array([0, 3, 4, 4, 6, 40], np.int32)
    xyz = rng.uniform(-1000, 1000, (pb[-1], 3))
    cof = S.random_cofactors(rng, pb[-1], 0.1)[0]
    eo = np.column_stack([rng.uniform(-1000, 1000, (ib[-1], 3)), rng.uniform(-3.1, 3.1, ib[-1]), rng.uniform(-1.3, 1.3, ib[-1]),
                          rng.uniform(-3.1, 3.1, ib[-1])])
    x, q, e = engine.similarity_apply(par, pb, xyz, cof, ib, eo)
    xr, qr, er = S.apply(par, pb, xyz, cof, ib, eo)
    for dev, ref in ((x, xr), (q, qr), (e, er)):
        assert np.array_equal(np.isnan(dev), np.isnan(ref))
    assert np.isnan(x[pb[3]:pb[4]]).all() and np.isnan(q[pb[3]:pb[4]]).all() and np.isnan(e[ib[3]:ib[4]]).all()
    ok = ~np.isnan(xr[:, 0])
    dx = np.abs(x[ok] - xr[ok]).max() / np.abs(xr[ok]).max()
    dq = (np.abs(q[ok] - qr[ok]).max(axis=1) / np.abs(qr[ok]).max(axis=1)).max()
    oke = ~np.isnan(er[:, 0])
    de = np.abs(e[oke, :3] - er[oke, :3]).max() / np.abs(er[oke, :3]).max()
    dr = max(np.abs(scene.rotation(*u[3:]) - scene.rotation(*v[3:])).max() for u, v in zip(e[oke], er[oke]))
    print(f"apply: points {dx:.2e}, cofactors {dq:.2e}, projection centres {de:.2e}, rotations {dr:.2e} from numpy")
    assert dx < 1e-12 and dq < 1e-12 and de < 1e-12 and dr < 1e-12
    # either range set may be absent, and the full output of similarity_models is taken as it is
    x2, q2, e2 = engine.similarity_apply(np.pad(par, ((0, 0), (0, 29))), pb, xyz)
    assert q2 is None and e2 is None and x2.tobytes() == x.tobytes()
    x3, q3, e3 = engine.similarity_apply(par, None, None, None, ib, eo)
    assert x3 is None and q3 is None and e3.tobytes() == e.tobytes()


def test_device_memory_returns_to_its_census():
    L = engine.load_library()
    L.jaicov_debug_device_census.argtypes = [C.POINTER(C.c_longlong)]
    L.jaicov_debug_device_census.restype = None

    def census():
        a = (C.c_longlong * 2)()                              # bytes, allocations held by the library right now
        L.jaicov_debug_device_census(a)
        return list(a)
    batch = S.lane_batch()[0]
    out = engine.similarity_models(*batch)[0]                 # the runtime's own first-call allocations are made
    engine.similarity_apply(out, batch[0], batch[1], batch[3])
    before = census()
    engine.similarity_models(*batch, reject_threshold=8.0)
    engine.similarity_apply(out, batch[0], batch[1], batch[3], [0] * 10 + [2], np.zeros((2, 6)))
    with pytest.raises(engine.EngineError):                   # a refused call: a zero on the diagonal of cof_dst
        engine.similarity_models(batch[0], batch[1], batch[2], None, np.zeros_like(batch[4]))
    assert census() == before


def test_a_model_is_carried_onto_the_object_frame():
    """relorient_problem with base length 1, intersect_problem, resect_problem, intersect_problem on a distortion-free exact scene (12
    images x 200 points) give a model in the frame of image 0; similarity_models onto the true object coordinates of five points and
    similarity_apply carry it into the object frame: every point and projection centre within 1e-9 of the extent of the truth, every
    rotation within 1e-9 rad (between rotation matrices)."""
    import dlt_reference as D
    import relorient_reference as R
    fp0 = R.scene_of("all_points")
    pts, io, eo = D.scene_truth(fp0)
    ob, xy, _, _, _ = D.batch_from_scene(fp0, exact=True)
    fp = copy.copy(fp0)
    order = np.argsort(np.asarray(fp0.ip_image), kind="stable")
    x, y = np.array(fp0.ip_x, np.float64), np.array(fp0.ip_y, np.float64)
    x[order] = xy[:, 0]; y[order] = xy[:, 1]
    fp.ip_x, fp.ip_y = x, y
    a, b = 0, 1
    v = np.full(len(fp.values), np.nan)
    c0 = 3 * fp.n_points
    v[c0:fp.slot_eo(0)] = np.asarray(fp.values, np.float64)[c0:fp.slot_eo(0)]          # the camera, and nothing else
    v, out, st = engine.relorient_problem(fp, a, b, base_length=1.0, values=v, with_status=True)
    assert st == engine.RELOR_OK
    seen = np.isin(np.asarray(fp.ip_image), (a, b))
    fp2 = copy.copy(fp)                                       # the image points of the two oriented images only
    for name in ("ip_image", "ip_point", "ip_x", "ip_y", "ip_var_x", "ip_var_y", "ip_rho"):
        setattr(fp2, name, np.asarray(getattr(fp, name))[seen])
    v = engine.intersect_problem(fp2, values=v, min_rays=2)
    v = engine.resect_problem(fp, values=v)
    v = engine.intersect_problem(fp, values=v)
    model_pts, model_eo = v[:c0].reshape(-1, 3), v[fp.slot_eo(0):].reshape(-1, 6)
    assert np.isfinite(model_pts).all() and np.isfinite(model_eo).all()
    five = np.array([3, 50, 97, 140, 199])
    sim, st, it, kind, used, q = engine.similarity_models([0, 5], model_pts[five], pts[five])
    assert st[0] == engine.SIMIL_OK and used.all()
    base = np.linalg.norm(eo[b, :3] - eo[a, :3])
    assert abs(sim[0, 3] - base) < 1e-9 * base               # the scale is the base length the pair could not give
    xo, _, eo_out = engine.similarity_apply(sim, [0, fp.n_points], model_pts, None, [0, fp.n_images], model_eo)
    dp = np.abs(xo - pts).max()
    dx = np.abs(eo_out[:, :3] - eo[:, :3]).max()
    dr = max(np.abs(scene.rotation(*eo_out[i, 3:]) - scene.rotation(*eo[i, 3:])).max() for i in range(fp.n_images))
    print(f"scale {sim[0, 3]:.6f} (base {base:.6f}), {it[0]} steps: points {dp:.2e} mm, projection centres {dx:.2e} mm, "
          f"rotations {dr:.2e} from the truth")
    assert dp < 1e-9 * EXTENT and dx < 1e-9 * EXTENT and dr < 1e-9


@pytest.fixture(scope="module")
def example_base(tmp_path_factory):
    d = tmp_path_factory.mktemp("example")
    for f in ("ior", "eor", "obc", "scale"):
        shutil.copy(os.path.join(GOLDEN, f"example.{f}"), d)
    with gzip.open(os.path.join(GOLDEN, "example.phc.gz")) as src, open(d / "example.phc", "wb") as dst:
        dst.write(src.read())
    return str(d / "example")


def test_cpp_mirror_carries_a_block_into_another_frame(example_base):
    """SimilarityTransformation of the C++ mirror on the bundled block's .obc points and .eor orientations: a known transformation is
    estimated from every third point (the 36 values are engine.similarity_models' on the same arrays, bit for bit) and apply() writes
    every point and every orientation where numpy puts them, to 1e-9 of the extent and 1e-9 between rotation matrices."""
    from bundle_adjustment_amd import host_api as H
    pr = H.read_aicon_flat(example_base)
    pts, images = list(pr.points()), list(pr.camera.images())
    T = H.ParameterType
    EO = (T.CAMERA_COORDINATE_X, T.CAMERA_COORDINATE_Y, T.CAMERA_COORDINATE_Z, T.CAMERA_OMEGA, T.CAMERA_PHI, T.CAMERA_KAPPA)
    xyz = np.array([[p.getX().getValue(), p.getY().getValue(), p.getZ().getValue()] for p in pts])
    eo = np.array([[im.getExteriorOrientation().get(t).getValue() for t in EO] for im in images])
    truth = np.array([[120.0, -340.0, 56.0, 3.5, 0.4, -0.3, 2.9]])
    target, _, eo_ref = S.apply(truth, [0, len(pts)], xyz, None, [0, len(images)], eo)
    model = H.SimilarityTransformation.Model()
    model.points = pts[::3]
    model.target = [list(t) for t in target[::3]]
    r = H.SimilarityTransformation.estimateAll([model])[0]
    assert r.status == engine.SIMIL_OK and r.startKind == engine.SIMIL_START_CLOSED and r.pointsUsed == r.points == len(pts[::3]) and all(r.used)
    out = engine.similarity_models([0, r.points], xyz[::3], target[::3])[0]
    assert np.array(r.values()).tobytes() == out[0].tobytes()
    ext = np.ptp(target, axis=0).max()
    dt, dm, dr = S.pose_error(out, truth, ext)
    assert dt < 1e-9 and dm < 1e-9 and dr < 1e-9
    assert H.SimilarityTransformation.apply(r, pts, images)
    got = np.array([[p.getX().getValue(), p.getY().getValue(), p.getZ().getValue()] for p in pts])
    got_eo = np.array([[im.getExteriorOrientation().get(t).getValue() for t in EO] for im in images])
    dp, dx = np.abs(got - target).max() / ext, np.abs(got_eo[:, :3] - eo_ref[:, :3]).max() / ext
    da = max(np.abs(scene.rotation(*u[3:]) - scene.rotation(*v[3:])).max() for u, v in zip(got_eo, eo_ref))
    print(f"mirror: T {dt:.2e}, m {dm:.2e}, R {dr:.2e} from the truth; points {dp:.2e}, projection centres {dx:.2e} of the extent, rotations {da:.2e}")
    assert dp < 1e-9 and dx < 1e-9 and da < 1e-9


def test_native_example_absolute_program(example_base):
    """host/example_absolute builds the bundled block's model from its image measurements and the .ior camera alone (pair, intersection
    and resection in alternation, base length 1), carries it onto the .obc coordinates by the similarity transformation over all common
    points with rejection on, and reaches the sigma0 that host/example_flatfiles reaches from the .obc and .eor values with REDUCED, to
    1e-9 relative."""
    host = os.path.join(ROOT, "bundle-adjustment_amd", "host")
    subprocess.check_call(["make", "-C", host, "example_absolute", "example_flatfiles"], stdout=subprocess.DEVNULL)
    a = subprocess.run([os.path.join(host, "example_absolute"), example_base], capture_output=True, text=True, timeout=600)
    b = subprocess.run([os.path.join(host, "example_flatfiles"), example_base, "REDUCED"], capture_output=True, text=True, timeout=600)
    print(a.stdout[-3000:])
    assert a.returncode == 0 and b.returncode == 0, (a.stdout[-2000:], a.stderr[-2000:])
    s0 = [float(re.search(r"sigma0 a-posteriori\s+(\S+)", t).group(1)) for t in (a.stdout, b.stdout)]
    assert abs(s0[0] - s0[1]) <= 1e-9 * s0[1], s0
    assert re.search(r"similarity transformation\s+status 0", a.stdout) and re.search(r"scale m\s+\S+\s+\+-", a.stdout)
