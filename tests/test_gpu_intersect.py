"""GPU: the forward intersection of include/jaicov_intersect.h against the restatement in tests/intersect_reference.py: noise-free
scenes (exact recovery), the synthetic configs with distortion and noise (parity), ray counts at the lane and chunk boundaries, batch
independence and determinism, rejection of a planted gross error, degenerate input, end to end from DLT orientations to the adjustment,
and the bundled block (tests/golden/example) through the C++ mirror."""
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dlt_reference as D
import intersect_reference as X
from bundle_adjustment_amd import engine, scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "example")
EXTENT = 2000.0        # object extent of the synthetic scenes, mm

_SCENES = {}


def scene_of(name):
    if name not in _SCENES:
        _SCENES[name] = scene.make_scene(200, 40, 40) if name == "all_rays" else scene.config(name)
    return _SCENES[name]


def same(dev, ref, rtol=1e-9):
    """same() of tests/test_gpu_dlt.py: NaN positions equal, values within rtol of each column's magnitude over the batch; the angle
    (last column of an (n, 11) result) within rtol rad"""
    dev = np.asarray(dev, np.float64).reshape(len(dev), -1)
    ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    assert np.array_equal(np.isnan(dev), np.isnan(ref))
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    col = np.nanmax(np.abs(np.where(ok, ref, np.nan)), axis=0)
    col = np.where(np.isnan(col) | (col == 0), 1.0, col)
    if ref.shape[1] == X.NOUT:
        col[10] = 1.0
    err = float((np.abs(np.where(ok, dev - ref, 0.0)) / col).max())
    assert err <= rtol, err
    return err


def check(batch, **kw):
    """one device call against the restatement: status, ray_used and iterations equal, values and q within same()"""
    rb, ri, xy, var, io, eo = batch
    dev = engine.intersect_points(rb, ri, xy, var, io, eo, **kw)
    kr = {("sigma2" if k == "sigma2apriori" else k): v for k, v in kw.items()}
    ref = X.intersect(rb, ri, xy, var, io, eo, **kr)
    assert np.array_equal(dev[1], ref[1]), np.flatnonzero(dev[1] != ref[1])[:5]
    assert np.array_equal(dev[3], ref[3]), np.flatnonzero(dev[3] != ref[3])[:5]
    assert np.array_equal(dev[2], ref[2]), np.flatnonzero(dev[2] != ref[2])[:5]
    worst = max(same(dev[0], ref[0]), same(dev[4][:, None], ref[4][:, None]))
    return dev, ref, worst


@pytest.mark.parametrize("negative_c", [False, True])
def test_exact_scene_is_recovered(negative_c):
    """Noise- and distortion-free observations of cfg2 (200 points x 20 rays), c of both signs.  Bound: that of the DLT's exact test,
    1e-10 of the 2 000 mm extent (the restatement reaches 6.7e-13 mm); the linear start is exact, so one step confirms it."""
    rb, ri, xy, _, io, eo, pts = X.batch_from_scene(scene_of("cfg2"), exact=True, c=-scene.C_EX if negative_c else None)
    out, st, it, used, q = engine.intersect_points(rb, ri, xy, None, io, eo)
    assert (st == engine.ISECT_OK).all() and used.all()
    err = np.abs(out[:, :3] - pts).max()
    print(f"c {'<' if negative_c else '>'} 0: max distance from the truth {err:.2e} mm, iterations {np.bincount(it)}")
    assert err < 1e-10 * EXTENT
    assert (it <= 2).all()


@pytest.mark.parametrize("name", ["tiny", "cfg2"])
def test_parity_with_the_restatement(name):
    """Distortion and noise (the intersection models neither); tiny carries 2 x 2 weights, cfg2 diagonal ones; unit weights as well.
    The summation orders differ (lanes and a butterfly here, ray order there), so bit parity is not asked."""
    fp = scene_of(name)
    rb, ri, xy, var, io, eo, _ = X.batch_from_scene(fp)
    for v, s0 in ((var, fp.sigma2apriori), (var, 1.0), (None, 1.0)):
        dev, ref, worst = check((rb, ri, xy, v, io, eo), sigma2apriori=s0)
        assert (dev[1] == engine.ISECT_OK).all()
        print(f"{name} weights={'unit' if v is None else 'var'} s0={s0:g}: worst relative difference to the restatement {worst:.2e}")


COUNTS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 200]


def lane_batch(exact=False):
    """70 points in shuffled order from a scene whose 40 points are seen by all 200 images; point k keeps the first COUNTS[k % 11] of
    its rays: the lane width (64), the LDS chunk (128) and both sides of each"""
    fp = scene_of("all_rays")
    rb, ri, xy, var, io, eo, _ = X.batch_from_scene(fp, exact=exact)
    assert (np.diff(rb) == 200).all()
    order = np.random.default_rng(3).permutation(70)
    keep = [np.arange(rb[k % 40], rb[k % 40] + COUNTS[k % 11]) for k in order]
    begin = np.concatenate([[0], np.cumsum([len(s) for s in keep])]).astype(np.int32)
    sel = np.concatenate(keep)
    return (begin, ri[sel], xy[sel], var[sel], io, eo), np.array([COUNTS[k % 11] for k in order])


def test_ray_counts_at_the_lane_boundaries():
    batch, counts = lane_batch()
    dev, ref, worst = check(batch, sigma2apriori=1.0)
    assert (dev[1][counts < 2] == engine.ISECT_TOO_FEW_RAYS).all() and (dev[2][counts < 2] == 0).all()
    assert (dev[1][counts >= 2] == engine.ISECT_OK).all()
    assert np.isnan(dev[0][counts < 2]).all()
    print(f"ray counts {sorted(set(counts))}: worst relative difference to the restatement {worst:.2e}")
    # with rejection, on distortion-free rays with N(0, 0.0005) noise (so that Omega and q are residuals, not rounding of zero) and one
    # gross error of 1 mm = 2 000 sigma: the rounds restart inside the kernel on resident (<= 128 rays) and on chunked points alike,
    # and the first used ray changes where ray 0 is the one withdrawn.  Threshold 30 sigma: no kept q comes near 900.
    (rb, ri, xy, var, io, eo), counts = lane_batch(exact=True)
    xy = xy + np.random.default_rng(5).normal(0, 0.0005, xy.shape)
    big = np.flatnonzero(counts >= 63)
    bad = rb[big] + np.where(np.arange(big.size) % 2 == 0, 0, 70 % counts[big])
    xy[bad] += 1.0
    dev, ref, _ = check((rb, ri, xy, var, io, eo), sigma2apriori=1.0, reject_threshold=30.0, min_rays=3)
    assert np.array_equal(np.flatnonzero(dev[3] == 0), np.sort(np.concatenate([bad, np.flatnonzero(np.repeat(counts < 2, counts))])))
    assert ref[4][ref[3] == 1].max() < 0.5 * 900.0


def test_batch_independence_and_determinism():
    (rb, ri, xy, var, io, eo), counts = lane_batch()
    a = engine.intersect_points(rb, ri, xy, var, io, eo)
    b = engine.intersect_points(rb, ri, xy, var, io, eo)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    for p in [int(np.flatnonzero(counts == c)[0]) for c in (2, 64, 65, 129, 200)]:
        s = slice(rb[p], rb[p + 1])
        o = engine.intersect_points([0, rb[p + 1] - rb[p]], ri[s], xy[s], var[s], io, eo)
        assert o[0].tobytes() == a[0][p:p + 1].tobytes() and o[1][0] == a[1][p] and o[2][0] == a[2][p]
        assert o[3].tobytes() == a[3][s].tobytes() and o[4].tobytes() == a[4][s].tobytes()


def test_planted_gross_errors_are_withdrawn():
    """The CPU case of tests/test_intersect_abi.py on the device: threshold 5 (sigma2apriori = 1: q in units of the variance),
    min_rays 3.  No q of a kept ray lies within 1 % of threshold^2 (checked here on the restatement's q), so rounding cannot change a
    decision."""
    rb, ri, xy, var, io, eo, planted = X.gross_error_batch(scene_of("cfg2"))
    dev, ref, worst = check((rb, ri, xy, var, io, eo), sigma2apriori=1.0, reject_threshold=5.0, min_rays=3)
    kept = ref[4][ref[3] == 1]
    assert not ((kept > 25.0 * 0.99) & (kept < 25.0 * 1.01)).any()
    assert np.array_equal(np.flatnonzero(dev[3] == 0), np.sort(planted))
    assert (dev[1] == engine.ISECT_OK).all()
    print(f"rejection: {planted.size} rays withdrawn, worst relative difference to the restatement {worst:.2e}")


def test_degenerate_input():
    fp = scene_of("cfg2")
    rb, ri, xy, var, io, eo, _ = X.batch_from_scene(fp)
    good = slice(rb[0], rb[1])
    ng = rb[1] - rb[0]
    # one good point, the same ray twice, one ray, no ray
    begin = np.array([0, ng, ng + 2, ng + 3, ng + 3], np.int32)
    img = np.concatenate([ri[good], ri[[0, 0]], ri[[1]]])
    pxy = np.concatenate([xy[good], xy[[0, 0]], xy[[1]]])
    pvar = np.concatenate([var[good], var[[0, 0]], var[[1]]])
    dev, ref, _ = check((begin, img, pxy, pvar, io, eo), sigma2apriori=1.0)
    out, st, it, used, q = dev
    assert list(st) == [engine.ISECT_OK, engine.ISECT_SINGULAR, engine.ISECT_TOO_FEW_RAYS, engine.ISECT_TOO_FEW_RAYS]
    assert np.isnan(out[1:]).all() and not used[ng:].any() and np.isnan(q[ng:]).all() and used[:ng].all()
    alone = engine.intersect_points([0, ng], ri[good], xy[good], var[good], io, eo, sigma2apriori=1.0)
    assert alone[0].tobytes() == out[:1].tobytes() and alone[4].tobytes() == q[:ng].tobytes()     # untouched by its neighbours
    # max_iterations = 1 on noisy data: values are returned all the same
    dev, ref, _ = check((rb, ri, xy, var, io, eo), sigma2apriori=1.0, max_iterations=1)
    assert (dev[1] == engine.ISECT_NOT_CONVERGED).all() and (dev[2] == 1).all() and np.isfinite(dev[0]).all()
    # a point at a projection centre (N = 0 in the collinearity equations): no values, and no fault
    eo2 = np.vstack([eo[0], eo[0] + [0, 0, 0, 0.3, 0.2, 0.1]])
    dev, ref, _ = check(([0, 2], [0, 1], np.tile(io[0, :2], (2, 1)), None, io[:2], eo2))
    assert dev[1][0] in (engine.ISECT_SINGULAR, engine.ISECT_NOT_FINITE) and np.isnan(dev[0]).all()


def relative_parameter_error(fp, got, ref):
    """tests/test_gpu_termination.py: coordinates against the 2 000 mm extent, every other parameter against its magnitude (floor 1)"""
    P3, I6 = 3 * fp.n_points, 6 * fp.n_images
    den = np.maximum(np.abs(ref), 1.0)
    den[:P3] = EXTENT
    den[-I6:].reshape(-1, 6)[:, :3] = EXTENT
    return float((np.abs(got - ref) / den).max())


def test_end_to_end_from_dlt_orientations():
    """cfg2 on the device alone: engine.dlt_adjust (x0, y0, c held at the camera's start values, the scene's start points as
    control), engine.intersect_problem from those orientations, Engine.estimate from both.  It reaches the converged parameters of the
    run from fp.values within 1e-9 (test_gpu_termination's bound)."""
    fp = scene_of("cfg2")
    P = fp.n_points
    ob, xy, _, _, _ = D.batch_from_scene(fp)
    io = np.tile(fp.values[3 * P:3 * P + 3], (fp.n_images, 1))
    xyz = fp.values[:3 * P].reshape(P, 3)[fp.ip_point]
    dl, st, _ = engine.dlt_adjust(ob, xy, xyz, io, io_fixed=np.ones((fp.n_images, 3), np.uint8),
                                  restrictions=(D.FIXED_X0, D.FIXED_Y0, D.FIXED_C_X, D.FIXED_C_Y))
    assert (st == engine.DLT_CONVERGED).all()
    v = fp.values.copy()
    v[fp.slot_eo(0):] = dl[:, 14:20].ravel()
    v[:3 * P] = np.nan                                           # every point must come from the intersection
    v, out, ist = engine.intersect_problem(fp, v, with_status=True)
    assert (ist == engine.ISECT_OK).all() and np.isfinite(v).all()
    ref = engine.Engine(fp)
    v0, r0 = ref.estimate(invert=engine.INVERT_NONE)
    ref.close()
    eng = engine.Engine(fp)
    v1, r1 = eng.estimate(values=v, invert=engine.INVERT_NONE)
    eng.close()
    err = relative_parameter_error(fp, v1, v0)
    print(f"start values {np.abs(v[:3 * P] - fp.truth[:3 * P]).max():.2f} mm from the truth; passes {r1.iterations} "
          f"(from fp.values {r0.iterations}); parameters {err:.2e}")
    assert r0.state == 1 and r1.state == 1
    assert err < 1e-9


# ---- the bundled block ------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def example_base(tmp_path):
    for f in ("ior", "eor", "obc", "scale"):
        shutil.copy(os.path.join(GOLDEN, f"example.{f}"), tmp_path)
    with gzip.open(os.path.join(GOLDEN, "example.phc.gz")) as src, open(tmp_path / "example.phc", "wb") as dst:
        dst.write(src.read())
    return str(tmp_path / "example")


def _example(H, base):
    """ExampleFlatFiles' setup (A3, Cx, Cy fixed, datum = names of <= 3 characters), as example_flatfiles does it"""
    pr = H.read_aicon_flat(base)
    cam = pr.camera
    cam.getDistortionModel(H.DistortionModelType.RADIAL_DISTORTION).get(3).setColumn(H.COLUMN_FIXED)
    aff = cam.getDistortionModel(H.DistortionModelType.AFFINITY_AND_SHEAR)
    aff.getCx().setColumn(H.COLUMN_FIXED); aff.getCy().setColumn(H.COLUMN_FIXED)
    for p in pr.points():
        if len(p.getName()) > 3:
            p.setDatum(False)
    return pr, cam


def _rays(H, cam):
    """the mirror's batch rebuilt in Python: points in first-seen order, a point's rays in the images' order"""
    T = H.ParameterType
    index, per, io, eo = {}, [], [], []
    ior = cam.getInteriorOrientation()
    for i, im in enumerate(cam.images()):
        io.append([ior.getPrinciplePointX().getValue(), ior.getPrinciplePointY().getValue(), ior.getPrincipleDistance().getValue()])
        e = im.getExteriorOrientation()
        eo.append([e.get(t).getValue() for t in (T.CAMERA_COORDINATE_X, T.CAMERA_COORDINATE_Y, T.CAMERA_COORDINATE_Z, T.CAMERA_OMEGA,
                                                  T.CAMERA_PHI, T.CAMERA_KAPPA)])
        for ic in im.coordinates():
            name = ic.getObjectCoordinate().getName()
            if name not in index:
                index[name] = len(per); per.append([])
            per[index[name]].append((i, ic.getX().getValue(), ic.getY().getValue(), ic.getX().getVariance(), ic.getY().getVariance(),
                                     ic.getCorrelationCoefficientXY()))
    rb = np.concatenate([[0], np.cumsum([len(r) for r in per])]).astype(np.int32)
    flat = np.array([r for rs in per for r in rs])
    return list(index), rb, flat[:, 0].astype(np.int32), flat[:, 1:3], flat[:, 3:6], np.array(io), np.array(eo)


def _adjust(H, pr, cam):
    ba = H.BundleAdjustment()
    ba.add(cam)
    for s in pr.scaleBars():
        ba.add(s)
    ba.setInvertNormalEquation(H.MatrixInversion.REDUCED)
    state = ba.estimateModel()
    pts = {p.getName(): [p.getX().getValue(), p.getY().getValue(), p.getZ().getValue()] for p in ba.getObjectCoordinates()}
    return state, ba.getVarianceFactorAposteriori(), pts, ba


def rigid_fit(A, B):
    """B moved onto A by the best rotation and translation (Kabsch)"""
    ca, cb = A.mean(0), B.mean(0)
    U, _, Vt = np.linalg.svd((B - cb).T @ (A - ca))
    Rm = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    return (B - cb) @ Rm + ca


def test_example_block_from_intersected_start_values(example_base):
    """The bundled block through the C++ mirror: .eor orientations, every point by ForwardIntersection::intersectAll (the .obc values are
    overwritten).  Statuses and values equal the restatement's on the same rays; REDUCED from those start values reaches the sigma0 of
    the run from .obc to 1e-9 relative and its points to 1e-9 of the extent (the bounds of test_example_block_from_dlt_start_values).

    The points are compared after a rigid fit of one result onto the other.  The block is a free network whose datum (inner constraints
    over the points with short names) is carried by the START values of those points, and here, unlike in the DLT's test, the points'
    start values change: up to 2.44 mm from .obc.  The two adjusted blocks are therefore the same shape in two datums.  Measured with
    the oracle on the CPU from the restatement's points: both runs state 1 in 4 passes, sigma0 equal to 5.9e-14 relative, points
    5.5e-4 of the extent apart as they stand (0.81 mm) and 4.7e-16 of the extent after the rigid fit."""
    from bundle_adjustment_amd import host_api as H
    pr, cam = _example(H, example_base)
    names, rb, ri, xy, var, io, eo = _rays(H, cam)
    obc = {p.getName(): [p.getX().getValue(), p.getY().getValue(), p.getZ().getValue()] for p in pr.points()}
    res = H.ForwardIntersection.intersectAll([cam])
    assert [r.point.getName() for r in res] == names
    ref = X.intersect(rb, ri, xy, var, io, eo)
    assert np.array_equal([r.status for r in res], ref[1]) and np.array_equal([r.iterations for r in res], ref[2])
    assert np.array_equal([r.rays for r in res], np.diff(rb)) and all(r.raysUsed == r.rays for r in res)
    dev = np.array([r.values() for r in res])
    worst = same(dev, ref[0])
    assert (ref[1] == X.OK).all()
    got = np.array([[r.point.getX().getValue(), r.point.getY().getValue(), r.point.getZ().getValue()] for r in res])
    assert got.tobytes() == dev[:, :3].tobytes()                 # written into the points
    d0 = np.sqrt(((got - np.array([obc[n] for n in names])) ** 2).sum(1)).max()
    print(f"{len(res)} points, {ri.size} rays: worst relative difference to the restatement {worst:.2e}; start values up to {d0:.3f} mm from .obc")
    st_i, s2_i, pts_i, ba_i = _adjust(H, pr, cam)
    pr2, cam2 = _example(H, example_base)
    st_o, s2_o, pts_o, _ = _adjust(H, pr2, cam2)
    assert st_i == st_o == H.EstimationStateType.ERROR_FREE_ESTIMATION, ba_i.lastError()
    assert abs(np.sqrt(s2_i) - np.sqrt(s2_o)) < 1e-9 * np.sqrt(s2_o)
    A = np.array([pts_o[n] for n in names]); B = np.array([pts_i[n] for n in names])
    ext = np.ptp(A, axis=0).max()
    raw, fit = np.abs(B - A).max() / ext, np.abs(rigid_fit(A, B) - A).max() / ext
    print(f"intersected start vs .obc start after REDUCED: sigma0 {abs(np.sqrt(s2_i) / np.sqrt(s2_o) - 1):.2e} relative, "
          f"points {raw:.2e} of the extent as they stand, {fit:.2e} in one datum")
    assert fit < 1e-9


def test_native_example_intersection_program(example_base):
    """host/example_intersection prints the sigma0 that host/example_flatfiles prints for the same base with REDUCED."""
    host = os.path.join(ROOT, "bundle-adjustment_amd", "host")
    subprocess.check_call(["make", "-C", host, "example_intersection", "example_flatfiles"], stdout=subprocess.DEVNULL)
    a = subprocess.run([os.path.join(host, "example_intersection"), example_base], capture_output=True, text=True, timeout=600)
    b = subprocess.run([os.path.join(host, "example_flatfiles"), example_base, "REDUCED"], capture_output=True, text=True, timeout=600)
    assert a.returncode == 0 and b.returncode == 0, (a.stdout[-2000:], a.stderr[-2000:])
    s0 = [re.search(r"sigma0 a-posteriori\s+(\S+)", t).group(1) for t in (a.stdout, b.stdout)]
    assert s0[0] == s0[1], s0
    assert re.search(r"status ok / not converged\s+150 / 0", a.stdout)
    print(a.stdout[-1200:])
