"""GPU: the batched DLT of include/jaicov_dlt.h against the restatement in tests/dlt_reference.py (the reference's arithmetic, dspsv
through the oracle), on noise-free scenes (exact recovery), on the synthetic configs with distortion and noise (parity), at the loop
control's edges, on degenerate input, and end to end on the bundled block (tests/golden/example) through the C++ mirror."""
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dlt_reference as R
from bundle_adjustment_amd import engine, scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "example")
EXTENT = 2000.0        # object extent of the synthetic scenes, mm

SINGLE = [(t,) for t in range(6)]
SETS = [()] + SINGLE + [(R.FIXED_X0, R.FIXED_Y0), (0, 1, 2, 3, 4, 5)]


@pytest.fixture()
def example_base(tmp_path):
    for f in ("ior", "eor", "obc", "scale"):
        shutil.copy(os.path.join(GOLDEN, f"example.{f}"), tmp_path)
    with gzip.open(os.path.join(GOLDEN, "example.phc.gz")) as src, open(tmp_path / "example.phc", "wb") as dst:
        dst.write(src.read())
    return str(tmp_path / "example")


_SCENES = {}


def scene_of(name):
    if name not in _SCENES:
        if name == "cfg4":     # config 4's geometry (500 images x 500 points of 5 000); its noise drawn diagonal, which is all the DLT reads
            _SCENES[name] = scene.make_scene(500, 5000, 500, dist=scene.DIST_FULL, weights="diag", n_control=15)
        else:
            _SCENES[name] = scene.config(name)
    return _SCENES[name]


def same(dev, ref, rtol=1e-9):
    """status-level NaN positions equal, values within rtol of each column's magnitude over the batch"""
    assert np.array_equal(np.isnan(dev), np.isnan(ref))
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    col = np.nanmax(np.abs(np.where(ok, ref, np.nan)), axis=0)
    col = np.where(np.isnan(col) | (col == 0), 1.0, col)
    d = np.abs(np.where(ok, dev - ref, 0.0))
    d[:, 17:20] = np.abs(R.wrap(np.where(ok[:, 17:20], dev[:, 17:20] - ref[:, 17:20], 0.0)))
    err = float((d / col).max())
    assert err <= rtol, err
    return err


@pytest.mark.parametrize("rs", [(), (R.FIXED_X0,), (R.FIXED_Y0,), (R.FIXED_C_X,), (R.FIXED_C_Y,), (R.IDENTICAL,), (R.ROTATION,),
                                (0, 1, 2, 3, 4, 5)])
def test_exact_scene_is_recovered(rs):
    """Noise- and distortion-free observations of cfg2 (20 images x 200 points), c > 0, restrictions the truth satisfies.  Bound: the
    DLT is a linear least-squares fit of exact data, so its error is rounding amplified by the conditioning of the preconditioned
    normal equations (~1e5 here): the restatement reaches 4e-12 mm on X0; 1e-10 of the 2 000 mm extent (2e-7 mm) and 1e-10 rad / mm
    on the angles and the interior orientation leave room for that and nothing more."""
    ob, xy, xyz, io, eo = R.batch_from_scene(scene_of("cfg2"), exact=True)
    out, st, sv = engine.dlt_adjust(ob, xy, xyz, io, restrictions=rs)
    assert (st == engine.DLT_CONVERGED).all()
    assert np.abs(out[:, 14:17] - eo[:, :3]).max() < 1e-10 * EXTENT
    assert np.abs(R.wrap(out[:, 17:20] - eo[:, 3:])).max() < 1e-10
    assert np.abs(out[:, 11:14] - io).max() < 1e-10


@pytest.mark.parametrize("name", ["tiny", "cfg2", "cfg3", "cfg4"])
def test_parity_with_the_restatement(name):
    """Distortion and noise (the DLT models neither); every restriction set.  The device sums and rounds in the restatement's order
    with contraction off, so status and solves agree exactly; values agree to 1e-9 of each column's magnitude (what is left is the
    last bit of the device's atan2 / asin against the host's libm).  Two runs are bitwise equal."""
    ob, xy, xyz, io, _ = R.batch_from_scene(scene_of(name))
    worst = 0.0
    for rs in SETS:
        out, st, sv = engine.dlt_adjust(ob, xy, xyz, io, restrictions=rs)
        ro, rst, rsv = R.adjust(ob, xy, xyz, io, restrictions=rs)
        assert np.array_equal(st, rst), (rs, np.flatnonzero(st != rst)[:5])
        assert np.array_equal(sv, rsv), (rs, np.flatnonzero(sv != rsv)[:5])
        worst = max(worst, same(out, ro))
        out2, st2, sv2 = engine.dlt_adjust(ob, xy, xyz, io, restrictions=rs)
        assert out2.tobytes() == out.tobytes() and np.array_equal(st2, st) and np.array_equal(sv2, sv)
    print(f"{name}: worst relative difference to the restatement {worst:.2e}")


@pytest.mark.parametrize("rs", [(), (R.FIXED_X0, R.FIXED_C_X)])
def test_loop_control_at_small_max_iterations(rs):
    ob, xy, xyz, io, _ = R.batch_from_scene(scene_of("tiny"))
    for it in (0, 1, 2, 3):
        out, st, sv = engine.dlt_adjust(ob, xy, xyz, io, restrictions=rs, max_iterations=it)
        ro, rst, rsv = R.adjust(ob, xy, xyz, io, restrictions=rs, max_iterations=it)
        assert np.array_equal(st, rst) and np.array_equal(sv, rsv), (it, st, rst, sv, rsv)
        if not rs and it < 3:
            assert (st == engine.DLT_NOT_CONVERGED).all()
        same(out, ro)


def _concat(parts):
    """[(xy, xyz)] -> CSR batch"""
    begin = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in parts])]).astype(np.int32)
    xy = np.concatenate([p[0] for p in parts]).reshape(-1, 2) if begin[-1] else np.zeros((0, 2))
    xyz = np.concatenate([p[1] for p in parts]).reshape(-1, 3) if begin[-1] else np.zeros((0, 3))
    return begin, xy, xyz


def _images(name="tiny"):
    ob, xy, xyz, io, _ = R.batch_from_scene(scene_of(name))
    return [(xy[ob[g]:ob[g + 1]], xyz[ob[g]:ob[g + 1]]) for g in range(ob.size - 1)], io[0]


def test_too_few_points_leave_neighbours_alone():
    imgs, io = _images()
    parts = [imgs[0], (np.zeros((0, 2)), np.zeros((0, 3))), imgs[1], (imgs[2][0][:5], imgs[2][1][:5]), imgs[3]]
    ob, xy, xyz = _concat(parts)
    out, st, sv = engine.dlt_adjust(ob, xy, xyz, np.tile(io, (5, 1)), restrictions=(R.ROTATION,))
    assert list(st[[1, 3]]) == [engine.DLT_TOO_FEW_POINTS] * 2 and list(sv[[1, 3]]) == [0, 0]
    assert np.isnan(out[[1, 3]]).all()
    ob2, xy2, xyz2 = _concat([imgs[0], imgs[1], imgs[3]])
    out2, st2, _ = engine.dlt_adjust(ob2, xy2, xyz2, np.tile(io, (3, 1)), restrictions=(R.ROTATION,))
    assert out[[0, 2, 4]].tobytes() == out2.tobytes() and np.array_equal(st[[0, 2, 4]], st2)


def test_degenerate_control_matches_the_restatement():
    """Control on a plane (Z = 0 exactly: three columns of N are zero, dsptrf meets a zero pivot -> SINGULAR), on a line, and one point
    repeated: the device reports what the restatement reports."""
    rng = np.random.default_rng(5)
    m = 40
    plane = np.stack([rng.uniform(-500, 500, m), rng.uniform(-500, 500, m), np.zeros(m)], 1)
    line = np.stack([rng.uniform(-500, 500, m), np.zeros(m), np.zeros(m)], 1)
    dup = np.tile([[100.0, 50.0, -30.0]], (m, 1))
    xy = np.stack([rng.uniform(-10, 10, m), rng.uniform(-10, 10, m)], 1)
    parts = [(xy, plane), (xy, line), (np.tile(xy[:1], (m, 1)), dup)]
    ob, bxy, bxyz = _concat(parts)
    io = np.tile([0.01, 0.05, 28.8], (3, 1))
    for rs in [(), (0, 1, 2, 3, 4, 5)]:
        out, st, sv = engine.dlt_adjust(ob, bxy, bxyz, io, restrictions=rs)
        ro, rst, rsv = R.adjust(ob, bxy, bxyz, io, restrictions=rs)
        assert np.array_equal(st, rst) and np.array_equal(sv, rsv), (rs, st, rst)
        assert st[0] == engine.DLT_SINGULAR and np.isnan(out[0]).all()
        bad = st >= engine.DLT_TOO_FEW_POINTS
        assert np.isnan(out[bad]).all()
        same(out[~bad], ro[~bad])


def test_duplicated_restriction_ids_are_dropped():
    ob, xy, xyz, io, _ = R.batch_from_scene(scene_of("tiny"))
    a = engine.dlt_adjust(ob, xy, xyz, io, restrictions=(4, 4, 0, 4, 0))
    b = engine.dlt_adjust(ob, xy, xyz, io, restrictions=(4, 0))
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    c = engine.dlt_adjust(ob, xy, xyz, io, restrictions=(2, 3, 0, 1))       # IDENTICAL dropped beside both FIXED_PRINCIPLE_DISTANCE_*
    d = engine.dlt_adjust(ob, xy, xyz, io, restrictions=(2, 3, 1))
    assert c[0].tobytes() == d[0].tobytes()


def test_one_large_image_among_small_ones():
    """25 000 observations (196 LDS chunks) between images of 24."""
    imgs, io = _images()
    rng = np.random.default_rng(11)
    big = 25000
    pts = np.stack([rng.uniform(-1000, 1000, big), rng.uniform(-150, 150, big), rng.uniform(-1000, 1000, big)], 1)
    eo = np.array([100.0, -2500.0, 50.0, 1.5, 0.1, 0.3])
    x, y, N = scene.project(scene.C_EX, scene.X0_EX, scene.Y0_EX, eo, pts, scene.R0_EX, [])
    assert (N < 0).all()
    xy_big = np.stack([x, y], 1) + rng.normal(0, 5e-4, (big, 2))
    parts = [imgs[0], (xy_big, pts), imgs[1]]
    ob, xy, xyz = _concat(parts)
    for rs in [(), (R.FIXED_X0, R.FIXED_Y0, R.ROTATION)]:
        out, st, sv = engine.dlt_adjust(ob, xy, xyz, np.tile(io, (3, 1)), restrictions=rs)
        ro, rst, rsv = R.adjust(ob, xy, xyz, np.tile(io, (3, 1)), restrictions=rs)
        assert np.array_equal(st, rst) and np.array_equal(sv, rsv)
        same(out, ro)
        assert np.abs(out[1, 14:17] - eo[:3]).max() < 0.1           # 0.5 um noise on 25 000 rays, no distortion


def test_fixed_interior_orientation_returns_the_cameras_values():
    """Q2: a fixed x0 / y0 / c comes back as given (the reference would return it divided by scale)."""
    ob, xy, xyz, io, _ = R.batch_from_scene(scene_of("cfg2"))
    fixed = np.ones((io.shape[0], 3), np.uint8)
    out, st, _ = engine.dlt_adjust(ob, xy, xyz, io, io_fixed=fixed, restrictions=(R.FIXED_X0, R.FIXED_C_Y))
    ro, rst, _ = R.adjust(ob, xy, xyz, io, io_fixed=fixed, restrictions=(R.FIXED_X0, R.FIXED_C_Y))
    assert np.array_equal(st, rst)
    assert out[:, 11:14].tobytes() == io.tobytes()
    same(out, ro)


def test_q1_negative_principal_distance():
    """A c < 0 camera (AICON): the device returns what the restatement returns, |c| and kappa + pi; projecting with the returned
    (c, EO) reproduces the observations."""
    fp = scene_of("cfg2")
    ob, xy, xyz, io, eo = R.batch_from_scene(fp, exact=True, c=-scene.C_EX)
    out, st, sv = engine.dlt_adjust(ob, xy, xyz, io)
    ro, rst, rsv = R.adjust(ob, xy, xyz, io)
    assert np.array_equal(st, rst) and (st == engine.DLT_CONVERGED).all()
    same(out, ro)
    assert np.abs(out[:, 13] - scene.C_EX).max() < 1e-10
    assert np.abs(R.wrap(out[:, 19] - eo[:, 5] - np.pi)).max() < 1e-10
    assert np.abs(out[:, 14:17] - eo[:, :3]).max() < 1e-10 * EXTENT
    for g in range(ob.size - 1):
        x, y, _ = scene.project(out[g, 13], out[g, 11], out[g, 12], out[g, 14:20], xyz[ob[g]:ob[g + 1]], scene.R0_EX, [])
        assert np.abs(np.stack([x, y], 1) - xy[ob[g]:ob[g + 1]]).max() < 1e-9


# ---- the bundled block ------------------------------------------------------------------------------------------------------------
def _example(H, base):
    """ExampleFlatFiles' setup (A3, Cx, Cy fixed, datum = names of <= 3 characters), as example_flatfiles / example_dlt do it"""
    pr = H.read_aicon_flat(base)
    cam = pr.camera
    cam.getDistortionModel(H.DistortionModelType.RADIAL_DISTORTION).get(3).setColumn(H.COLUMN_FIXED)
    aff = cam.getDistortionModel(H.DistortionModelType.AFFINITY_AND_SHEAR)
    aff.getCx().setColumn(H.COLUMN_FIXED); aff.getCy().setColumn(H.COLUMN_FIXED)
    for p in pr.points():
        if len(p.getName()) > 3:
            p.setDatum(False)
    return pr, cam


def _adjust(H, pr, cam):
    ba = H.BundleAdjustment()
    ba.add(cam)
    for s in pr.scaleBars():
        ba.add(s)
    ba.setInvertNormalEquation(H.MatrixInversion.REDUCED)
    state = ba.estimateModel()
    pts = np.array([[p.getX().getValue(), p.getY().getValue(), p.getZ().getValue()] for p in ba.getObjectCoordinates()])
    T = H.ParameterType
    eo = np.array([[im.getExteriorOrientation().get(t).getValue() for t in (T.CAMERA_COORDINATE_X, T.CAMERA_COORDINATE_Y,
                   T.CAMERA_COORDINATE_Z, T.CAMERA_OMEGA, T.CAMERA_PHI, T.CAMERA_KAPPA)] for im in cam.images()])
    return state, ba.getVarianceFactorAposteriori(), pts, eo, ba


def test_example_block_from_dlt_start_values(example_base):
    """DLT start values against the .eor file, then REDUCED from those start values reaches the sigma0 and the parameters that the
    .eor start values reach.  Measured: images 48 and 54 have fewer than 6 points (TOO_FEW_POINTS, their .eor
    orientation is kept); the other 113 differ from the .eor orientation by up to 138.3 mm and 0.380 rad -- the DLT ignores the
    lens distortion and several images see few, clustered points -- so the bounds are 200 mm and 0.5 rad (without Q1 kappa would be
    off by pi)."""
    from bundle_adjustment_amd import host_api as H
    pr, cam = _example(H, example_base)
    eor = np.array([[im.getExteriorOrientation().get(t).getValue() for t in (H.ParameterType.CAMERA_COORDINATE_X, H.ParameterType.CAMERA_COORDINATE_Y,
                    H.ParameterType.CAMERA_COORDINATE_Z, H.ParameterType.CAMERA_OMEGA, H.ParameterType.CAMERA_PHI, H.ParameterType.CAMERA_KAPPA)]
                    for im in cam.images()])
    coefs = [H.DLTCoefficients(im) for im in cam.images()]
    ok = H.DirectLinearTransformation.adjustAll(coefs, pr)
    few = sorted(im.getId() for c, im in zip(coefs, cam.images()) if c.status == engine.DLT_TOO_FEW_POINTS)
    assert few == [48, 54]
    assert all(o == (c.status == engine.DLT_CONVERGED) for o, c in zip(ok, coefs))
    assert all(c.status == engine.DLT_CONVERGED for c in coefs if c.getReference().getId() not in few)
    used = np.array([c.status == engine.DLT_CONVERGED for c in coefs])
    assert all(c.values()[13] > 0 for c in coefs if c.status == engine.DLT_CONVERGED)   # Q1: the DLT's c > 0, the camera's is not
    for c, im in zip(coefs, cam.images()):
        if c.status == engine.DLT_CONVERGED:
            H.DirectLinearTransformation.applyExteriorOrientation(c, im.getExteriorOrientation())
    T = H.ParameterType
    dlt = np.array([[im.getExteriorOrientation().get(t).getValue() for t in (T.CAMERA_COORDINATE_X, T.CAMERA_COORDINATE_Y,
                    T.CAMERA_COORDINATE_Z, T.CAMERA_OMEGA, T.CAMERA_PHI, T.CAMERA_KAPPA)] for im in cam.images()])
    dX = np.abs(dlt[used, :3] - eor[used, :3]).max()
    dA = np.abs(R.wrap(dlt[used, 3:] - eor[used, 3:])).max()
    print(f"DLT vs .eor: max |dX0| {dX:.4f} mm, max |dangle| {dA:.3e} rad")
    assert dX < 200.0 and dA < 0.5
    st_d, s2_d, pts_d, eo_d, ba_d = _adjust(H, pr, cam)
    pr2, cam2 = _example(H, example_base)
    st_e, s2_e, pts_e, eo_e, _ = _adjust(H, pr2, cam2)
    assert st_d == st_e == H.EstimationStateType.ERROR_FREE_ESTIMATION, ba_d.lastError()
    assert abs(np.sqrt(s2_d) - np.sqrt(s2_e)) < 1e-9 * np.sqrt(s2_e)
    ext = np.ptp(pts_e, axis=0).max()
    dp, de, da = np.abs(pts_d - pts_e).max(), np.abs(eo_d[:, :3] - eo_e[:, :3]).max(), np.abs(R.wrap(eo_d[:, 3:] - eo_e[:, 3:])).max()
    print(f"DLT start vs .eor start after REDUCED: points {dp / ext:.2e}, projection centres {de / ext:.2e} of the extent, angles {da:.2e} rad")
    assert dp < 1e-9 * ext
    # Finding: the projection centres differ by up to 2.5e-6 mm = 1.7e-9 of the extent although both runs end with
    # steps of ~1e-12 and equal omega to 11 digits: rounding in the two different iteration histories of a free network, not another
    # minimum.  The bounds are the measurements (1.7e-9 of the extent, 4.3e-9 rad) with margin.
    assert de < 5e-9 * ext
    assert da < 1e-8


def test_native_example_dlt_program(example_base):
    """host/example_dlt prints the sigma0 that host/example_flatfiles prints for the same base and mode."""
    host = os.path.join(ROOT, "bundle-adjustment_amd", "host")
    subprocess.check_call(["make", "-C", host, "example_dlt", "example_flatfiles"], stdout=subprocess.DEVNULL)
    a = subprocess.run([os.path.join(host, "example_dlt"), example_base, "REDUCED"], capture_output=True, text=True, timeout=600)
    b = subprocess.run([os.path.join(host, "example_flatfiles"), example_base, "REDUCED"], capture_output=True, text=True, timeout=600)
    assert a.returncode == 0 and b.returncode == 0, (a.stdout[-2000:], a.stderr[-2000:])
    s0 = [re.search(r"sigma0 a-posteriori\s+(\S+)", t).group(1) for t in (a.stdout, b.stdout)]
    assert s0[0] == s0[1], s0
    assert "images without DLT result     2" in a.stdout          # images 48 and 54: fewer than 6 points
    print(a.stdout[-1200:])
