"""GPU: the relative orientation of include/jaicov_relorient.h against the restatement in tests/relorient_reference.py: noise-free
pairs (exact recovery, c of both signs, two different cameras), plane fields, parity on every input of
relorient_reference.parity_inputs, observation counts at the lane and chunk boundaries, given and linear starts in one batch,
rejection, degenerate input, batch independence and determinism, the device's memory census, and the chain relative orientation,
intersection, resection, intersection on an exact scene."""
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


def device(batch, **kw):
    kd = {("sigma2apriori" if k == "sigma2" else k): v for k, v in kw.items()}
    return engine.relorient_pairs(*batch, **kd)


def check(batch, **kw):
    """one device call against the restatement: status, iterations, start kind and obs_used equal, values and q within same()"""
    dev = device(batch, **kw)
    ref = R.relorient(*batch, **kw)
    for k, what in ((1, "status"), (2, "iterations"), (3, "start kind"), (4, "used")):
        assert np.array_equal(dev[k], ref[k]), (what, np.flatnonzero(dev[k] != ref[k])[:5], dev[k][:12], ref[k][:12])
    worst = max(same(dev[0], ref[0]), same(dev[5][:, None], ref[5][:, None]))
    return dev, ref, worst


@pytest.fixture(scope="module")
def example_base(tmp_path_factory):
    d = tmp_path_factory.mktemp("example")
    for f in ("ior", "eor", "obc", "scale"):
        shutil.copy(os.path.join(GOLDEN, f"example.{f}"), d)
    with gzip.open(os.path.join(GOLDEN, "example.phc.gz")) as src, open(d / "example.phc", "wb") as dst:
        dst.write(src.read())
    return str(d / "example")


CAMERAS = {"c > 0": {}, "c < 0": dict(c=-scene.C_EX), "two cameras": dict(c=scene.C_EX, c_b=-1.7 * scene.C_EX)}


@pytest.mark.parametrize("name", ["tiny", "cfg2"])
@pytest.mark.parametrize("cameras", list(CAMERAS))
def test_exact_pairs_are_recovered(name, cameras):
    """Noise- and distortion-free observations: the true base direction to 1e-9 and the true rotation to 1e-9 rad (north_star's
    figures; the restatement reaches 1.3e-15 and 7e-16).  The difference of two rotations is taken between their matrices, whose
    entries change by at most the angle between them."""
    batch, truth, _ = R.pairs_of_scene(R.scene_of(name), R.SCENE_PAIRS, exact=True, **CAMERAS[cameras])
    out, st, it, kind, used, q = device(batch[:3] + (None, None) + batch[5:])
    assert (st == engine.RELOR_OK).all() and used.all() and (kind != engine.RELOR_START_GIVEN).all()
    db, dr = R.pose_error(out, truth)
    print(f"{name} {cameras}: base {db:.2e}, rotation {dr:.2e} from the truth, iterations {it}, start kinds {kind}")
    assert db < 1e-9 and dr < 1e-9
    assert np.abs(np.linalg.norm(out[:, :3], axis=1) - 1.0).max() < 1e-14


def test_plane_fields_return_the_truth():
    """6, 8 and 12 points within 1 % of the extent of a plane: the truth comes back to the bounds of the exact pairs.  An exactly planar
    field: status OK and Omega below 1e-20 in the units of the rays (Omega over c^2 with unit weights); its pose is one of the two
    exact solutions and is not asserted."""
    batch, truth, _ = R.plane_batch([6, 8, 12], thickness=0.01)
    out, st, it, kind, used, q = device(batch[:3] + (None, None) + batch[5:])
    db, dr = R.pose_error(out, truth)
    print(f"plane field of 1 %: base {db:.2e}, rotation {dr:.2e} from the truth, iterations {it}, start kinds {kind}")
    assert (st == engine.RELOR_OK).all() and db < 1e-9 and dr < 1e-9
    batch, truth, _ = R.plane_batch([6, 8, 12, 40], thickness=0.0)
    out, st, it, kind, used, q = device(batch[:3] + (None, None) + batch[5:])
    print(f"exact plane: Omega / c^2 {out[:, 27] / scene.C_EX ** 2}, start kinds {kind}, distance from the truth {R.pose_error(out, truth)}")
    assert (st == engine.RELOR_OK).all() and (kind == engine.RELOR_START_PLANE).all()
    assert (out[:, 27] / scene.C_EX ** 2 < 1e-20).all()


def test_parity_with_the_restatement(example_base):
    """Every input of relorient_reference.parity_inputs, the bundled block included.  The summation orders differ (lanes and a
    butterfly here, observation order there), so bit parity is not asked; tests/test_relorient_abi.py holds the restatement's own
    spread between the two orders on these inputs below a tenth of this bound."""
    names = []
    for name, batch, kw in R.parity_inputs(example_base):
        dev, ref, worst = check(batch, **kw)
        print(f"{name}: status {np.bincount(dev[1], minlength=5)}, start kinds {np.bincount(dev[3], minlength=3)}, "
              f"{int((dev[4] == 0).sum())} not used, worst relative difference to the restatement {worst:.2e}")
        names.append(name)
    assert "bundled block" in names and len(names) >= 15


def test_observation_counts_at_the_lane_boundaries():
    """5 (start values given), 6, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200 common points: every pair is solved; with rejection the
    rounds restart inside the kernel on resident (<= 128) and on chunked pairs alike, and exactly the planted errors go."""
    batch, counts, truth = R.lane_batch()
    assert sorted(counts) == R.COUNTS
    dev, ref, worst = check(batch)
    assert (dev[1] == engine.RELOR_OK).all()
    assert (dev[3][counts == 5] == engine.RELOR_START_GIVEN).all() and (dev[3][counts > 5] != engine.RELOR_START_GIVEN).all()
    assert (dev[3][(counts > 5) & (counts < 8)] == engine.RELOR_START_PLANE).all()
    batch, counts, bad = R.lane_batch_with_gross_errors()
    dev, ref, _ = check(batch, reject_threshold=30.0, min_points=6)
    assert np.array_equal(np.flatnonzero(dev[4] == 0), np.sort(bad))
    print(f"counts {sorted(counts)}: worst relative difference to the restatement {worst:.2e}; {bad.size} planted errors withdrawn")


def test_given_and_linear_starts_in_one_batch():
    batch = R.mixed_start_batch()
    dev, ref, worst = check(batch)
    assert (dev[1] == engine.RELOR_OK).all()
    assert (dev[3][0::2] == engine.RELOR_START_GIVEN).all() and (dev[3][1::2] != engine.RELOR_START_GIVEN).all()
    free = device(batch[:6] + (None,))
    assert same(dev[0], free[0]) < 1e-9                       # both starts end at the same pose


def test_batch_independence_and_determinism():
    """cfg2's pairs, the 12 lane-boundary pairs and the degenerate ones, twice over, with rejection.  Two runs give the same bits; a
    pair alone gives the bits it gives inside the batch."""
    lb = R.lane_batch_with_gross_errors()[0]
    sc = R.pairs_of_scene(R.scene_of("cfg2"), R.SCENE_PAIRS)[0]
    dg = R.degenerate_batch()[0]
    begin, *arrays = R.cat([sc, lb, dg] * 2)
    assert begin.size - 1 == 42
    kw = dict(reject_threshold=30.0, min_points=6)
    a = engine.relorient_pairs(begin, *arrays, **kw)
    b = engine.relorient_pairs(begin, *arrays, **kw)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    for g in (0, 3, 4, 9, 15, 17, 18, 20, 25, 41):
        s = slice(begin[g], begin[g + 1])
        o = engine.relorient_pairs([0, begin[g + 1] - begin[g]], arrays[0][s], arrays[1][s], arrays[2][s], arrays[3][s], arrays[4][g:g + 1],
                                   arrays[5][g:g + 1], **kw)
        assert o[0].tobytes() == a[0][g:g + 1].tobytes() and all(o[k][0] == a[k][g] for k in (1, 2, 3)), g
        assert o[4].tobytes() == a[4][s].tobytes() and o[5].tobytes() == a[5][s].tobytes(), g


def test_planted_gross_errors_are_withdrawn():
    """50 sigma in one observation per pair, threshold 5 (sigma2apriori = 1: q in units of the variance of g), min_points 8."""
    batch, planted = R.gross_error_batch()
    dev, ref, worst = check(batch, reject_threshold=5.0, min_points=8)
    assert np.array_equal(np.flatnonzero(dev[4] == 0), np.sort(planted))
    assert (dev[1] == engine.RELOR_OK).all()
    print(f"rejection: {planted.size} observations withdrawn, worst relative difference to the restatement {worst:.2e}")


def test_degenerate_input_does_not_disturb_its_neighbours():
    batch, expected = R.degenerate_batch()
    dev, ref, _ = check(batch)
    out, st, it, kind, used, q = dev
    ob = batch[0]
    assert list(st) == expected
    for g, e in enumerate(expected):
        s = slice(ob[g], ob[g + 1])
        if e == R.OK:
            assert np.isfinite(out[g]).all() and used[s].all() and np.isfinite(q[s]).all()
        else:
            assert np.isnan(out[g]).all() and not used[s].any() and np.isnan(q[s]).all() and kind[g] == 0
    assert out[0].tobytes() == out[4].tobytes() and q[ob[0]:ob[1]].tobytes() == q[ob[4]:ob[5]].tobytes()
    s = slice(ob[0], ob[1])
    alone = engine.relorient_pairs([0, ob[1]], batch[1][s], batch[2][s], batch[3][s], batch[4][s], batch[5][:1])
    assert alone[0].tobytes() == out[:1].tobytes() and alone[5].tobytes() == q[s].tobytes()
    # max_iterations = 1 on noisy data: values are returned all the same
    dev, ref, _ = check(R.pairs_of_scene(R.scene_of("cfg2"), R.SCENE_PAIRS)[0], max_iterations=1)
    assert (dev[1] == engine.RELOR_NOT_CONVERGED).all() and np.isfinite(dev[0]).all()


def test_device_memory_returns_to_its_census():
    L = engine.load_library()
    L.jaicov_debug_device_census.argtypes = [C.POINTER(C.c_longlong)]
    L.jaicov_debug_device_census.restype = None

    def census():
        a = (C.c_longlong * 2)()                              # bytes, allocations held by the library right now
        L.jaicov_debug_device_census(a)
        return list(a)
    batch = R.lane_batch()[0]
    device(batch)                                             # the runtime's own first-call allocations are made
    before = census()
    device(batch, reject_threshold=30.0)
    with pytest.raises(engine.EngineError):
        engine.relorient_pairs([0, 6], np.zeros((6, 2)), np.zeros((6, 2)), np.zeros((6, 3)), None, [[0, 0, 28.0, 0, 0, 28.0]])   # variance 0
    assert census() == before


def test_a_block_grows_from_image_measurements_alone():
    """relorient_problem, intersect_problem, resect_problem, intersect_problem on a distortion-free exact scene (12 images x 200 points)
    with the true base length: every orientation and every point equals the truth expressed in the frame of image a, to 1e-9 of the
    extent and 1e-9 rad (between rotation matrices)."""
    import copy
    import dlt_reference as D
    fp0 = R.scene_of("all_points")
    pts, io, eo = D.scene_truth(fp0)
    ob, xy, _, _, _ = D.batch_from_scene(fp0, exact=True)
    fp = copy.copy(fp0)
    order = np.argsort(np.asarray(fp0.ip_image), kind="stable")
    x, y = np.array(fp0.ip_x, np.float64), np.array(fp0.ip_y, np.float64)
    x[order] = xy[:, 0]; y[order] = xy[:, 1]
    fp.ip_x, fp.ip_y = x, y
    a, b = 0, 1
    truth, base = R.relative_truth(eo[a], eo[b])
    v = np.full(len(fp.values), np.nan)
    c0 = 3 * fp.n_points
    v[c0:fp.slot_eo(0)] = np.asarray(fp.values, np.float64)[c0:fp.slot_eo(0)]          # the camera, and nothing else
    v, out, st = engine.relorient_problem(fp, a, b, base_length=base, values=v, with_status=True)
    assert st == engine.RELOR_OK
    seen = np.isin(np.asarray(fp.ip_image), (a, b))
    fp2 = copy.copy(fp)                                       # the image points of the two oriented images only
    for name in ("ip_image", "ip_point", "ip_x", "ip_y", "ip_var_x", "ip_var_y", "ip_rho"):
        setattr(fp2, name, np.asarray(getattr(fp, name))[seen])
    v = engine.intersect_problem(fp2, values=v, min_rays=2)
    assert np.isfinite(v[:c0]).all()
    v = engine.resect_problem(fp, values=v)
    v = engine.intersect_problem(fp, values=v)
    Ra = scene.rotation(*eo[a, 3:])
    pts_a = (pts - eo[a, :3]) @ Ra
    dp = np.abs(v[:c0].reshape(-1, 3) - pts_a).max()
    e = v[fp.slot_eo(0):].reshape(-1, 6)
    dx = max(np.abs(e[i, :3] - Ra.T @ (eo[i, :3] - eo[a, :3])).max() for i in range(fp.n_images))
    dr = max(np.abs(scene.rotation(*e[i, 3:]) - Ra.T @ scene.rotation(*eo[i, 3:])).max() for i in range(fp.n_images))
    print(f"pair ({a}, {b}), base {base:.3f}: points {dp:.2e} mm, projection centres {dx:.2e} mm, rotations {dr:.2e} from the truth")
    assert dp < 1e-9 * EXTENT and dx < 1e-9 * EXTENT and dr < 1e-9


def test_native_example_relative_program(example_base):
    """host/example_relative builds the bundled block's start values from its image measurements and the .ior camera alone (pair,
    intersection and resection in alternation, scale bar) and reaches the sigma0 that host/example_flatfiles reaches from the .obc and
    .eor values with REDUCED, to 1e-9 relative."""
    host = os.path.join(ROOT, "bundle-adjustment_amd", "host")
    subprocess.check_call(["make", "-C", host, "example_relative", "example_flatfiles"], stdout=subprocess.DEVNULL)
    a = subprocess.run([os.path.join(host, "example_relative"), example_base], capture_output=True, text=True, timeout=600)
    b = subprocess.run([os.path.join(host, "example_flatfiles"), example_base, "REDUCED"], capture_output=True, text=True, timeout=600)
    print(a.stdout[-2500:])
    assert a.returncode == 0 and b.returncode == 0, (a.stdout[-2000:], a.stderr[-2000:])
    s0 = [float(re.search(r"sigma0 a-posteriori\s+(\S+)", t).group(1)) for t in (a.stdout, b.stdout)]
    assert abs(s0[0] - s0[1]) <= 1e-9 * s0[1], s0
    assert re.search(r"oriented images / points\s+115 of 115", a.stdout)
