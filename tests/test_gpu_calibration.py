"""GPU: the distortion field of a camera and the comparison of two calibrations (include/jaicov_calibration.h, csrc/calibration.hip)
against the numpy restatement of tests/calib_reference.py on the cofactor matrix that the same engine exports (get_cofactor_sub).

Scenes (calib_reference.SCENES): those of predict_reference -- a free network (d = 6, radial terms only: depth may be NULL), two cameras
with 11 and 5 coefficients, a fixed c (PARTIAL) -- and one camera with Zernike X, Y and gradient terms and a fixed c, whose centre
node is NOT_FINITE.  Node lists hold 1, 63, 65 and 257 nodes, the cameras interleaved at random, one node twice, node 1 on the principal
point, node 3 with a NaN depth.  Every matrix mode is used: the EO-reduced one, all of Qxx, and all of Qxx expanded from the reduced
system.  Every test prints the worst figure it saw before it asserts."""
import ctypes as C
import gc

import numpy as np
import pytest

import calib_reference as R
import predict_reference as PR
from bundle_adjustment_amd import engine

pytestmark = pytest.mark.gpu

NAMES = list(R.SCENES)
MODES = {"REDUCED": engine.INVERT_REDUCED, "FULL": engine.INVERT_FULL, "FULL_EXPANDED": engine.INVERT_FULL_EXPANDED}
COUNTS = (1, 63, 65, 257)
S2, K2 = 0.83, 1.7
_pd, _pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def inverting_pass(fp, mode):
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(mode)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(mode)
    return eng


def exported(eng):
    return eng.get_cofactor_sub(np.arange(eng.cofactor_order(), dtype=np.int32))


def node_list(fp, count):
    """the nodes of one call; the scenes without distance-dependent terms take the 63-node list without depths"""
    cams, xy, depth = R.nodes(fp, count, seed=3 + count)
    if count >= 5:
        depth[3] = np.nan
    if count == 63 and not any(R.has_di(fp, k) for k in range(fp.n_cameras)):
        depth = None
    return cams, xy, depth


@pytest.fixture(scope="module")
def ref(oracle_mod):
    """per scene and count, once: the nodes with their reference rows at the start values"""
    out = {}
    for name in NAMES:
        fp = R.scene_of(name)
        lists = {}
        for count in COUNTS:
            cams, xy, depth = node_list(fp, count)
            w, J = R.rows(oracle_mod, fp, fp.values, cams, xy, depth)
            lists[count] = dict(cams=cams, xy=xy, depth=depth, w=w, J=J)
        out[name] = dict(fp=fp, lists=lists)
    return out


def delta(K):
    """the entrywise bound of J Q J' relative to the sum of absolute terms: twice the row parity bound, and a fixed-order sum of K^2 terms
    (tests/test_gpu_predict.py, K the staged columns)"""
    return 2.0 * R.ROW_PARITY + np.asarray(K, float) ** 2 * R.U53


def of_bound(err, bound):
    """the largest err / bound; where the bound is zero (no term at all) the error must be zero"""
    with np.errstate(all="ignore"):
        return float(np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf)).max(initial=0.0))


def bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def field_bits(f, k=slice(None)):
    return bits(f.delta[k], f.cof[k], f.sigma[k], f.ellipse[k], f.direction[k], f.radial[k], f.sigma_radial[k], f.status[k], f.jac[k])


def compare_bits(c, k=slice(None)):
    return bits(c.d[k], c.M[k], c.q[k], c.T_prio[k], c.T_post[k], c.status[k])


def same(a, b):
    """equal, NaN where the other has NaN"""
    return np.array_equal(a, b, equal_nan=True)


def perturbed(fp, k, seed=11):
    """(reference values of camera k near its own, a covariance of them): a certificate"""
    rng = np.random.default_rng(seed)
    th = fp.values[R.camera_slots(fp, k)]
    sig = 1e-4 * np.abs(th) + 1e-14
    B = sig[:, None] * rng.normal(size=(th.size, th.size))
    return th + sig * rng.normal(size=th.size), B @ B.T


# ---- 1. the field against the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_the_field_matches_the_reference_on_the_exported_matrix(ref, name, mode):
    fp = ref[name]["fp"]
    eng = inverting_pass(fp, MODES[mode])
    Q = exported(eng)
    kinds = sorted(set(fp.dist_kind.tolist()))
    masks = [R.ALL, R.PRINCIPAL_DISTANCE, R.PRINCIPAL_POINT | (1 << (R.KIND_SHIFT + kinds[-1]))]
    for count in COUNTS:
        c = ref[name]["lists"][count]
        for columns in masks if count == 65 else masks[:1]:
            got = eng.calibration_field(S2, c["cams"], c["xy"], c["depth"], K2, columns=columns, jacobian=True)
            out, status, sabs, K = R.field(fp, Q, c["w"], c["J"], c["cams"], c["xy"], S2, K2, columns)
            fin = (status & R.NOT_FINITE) == 0
            assert got.delta.shape == (count, 2) and got.cof.shape == (count, 3) and got.jac.shape == (count, 2, R.MAX_COLUMNS)
            exy = np.abs(got.delta - out[:, 0:2])[fin].max(initial=0.0)
            ratio = of_bound(np.abs(got.cof - out[:, 2:5])[fin], delta(K)[fin, None] * sabs[fin])
            scale = np.abs(c["J"]).max(axis=(1, 2))
            okj = np.isfinite(scale)
            ejac = (np.abs(got.jac - c["J"])[okj].max(axis=(1, 2), initial=0.0) / scale[okj]).max(initial=0.0)
            # the figures derived from C, against numpy on the call's own C and correction
            g = got.cof[fin]
            l = np.array([PR.ellipse(*q) for q in g]).reshape(-1, 3)
            tr = np.maximum(g[:, 0] + g[:, 2], 1e-300)[:, None]                    # a fixed c alone leaves C = 0
            sig = np.sqrt(S2 * np.maximum(g[:, [0, 2]], 0.0))
            ell = K2 * np.sqrt(S2 * np.maximum(l[:, 0:2], 0.0))
            e_fig = max(np.abs(got.sigma[fin] - sig).max(initial=0.0) / max(sig.max(initial=0.0), 1e-300),
                        (np.abs(got.ellipse[fin] ** 2 - ell ** 2) / (K2 * K2 * S2 * tr)).max(initial=0.0))
            xs, ys = c["xy"][fin, 0], c["xy"][fin, 1]
            r = np.hypot(xs, ys)
            pos = r > 0.0
            with np.errstate(all="ignore"):
                dr = (xs * got.delta[fin, 0] + ys * got.delta[fin, 1]) / r
                dt = (-ys * got.delta[fin, 0] + xs * got.delta[fin, 1]) / r
                qrr = (xs * xs * g[:, 0] + 2.0 * xs * ys * g[:, 1] + ys * ys * g[:, 2]) / (r * r)
                qtt = (ys * ys * g[:, 0] - 2.0 * xs * ys * g[:, 1] + xs * xs * g[:, 2]) / (r * r)
            e_rad = max(np.abs(got.radial[fin][pos] - np.stack([dr, dt], 1)[pos]).max(initial=0.0),
                        (np.abs(got.sigma_radial[fin][pos] ** 2 - S2 * np.maximum(np.stack([qrr, qtt], 1)[pos], 0.0)) / (S2 * tr[pos])).max(initial=0.0))
            print(f"{name} {mode} {count} nodes, columns {columns:#x}: correction {exy:.2e} mm, C {ratio:.2e} of the bound, jacobian {ejac:.2e} of the "
                  f"row's scale, sigma and ellipse {e_fig:.2e}, radial {e_rad:.2e}, K {sorted(set(K.tolist()))}, status {sorted(set(got.status.tolist()))}")
            assert exy <= 1e-13
            assert ratio <= 1.0
            assert ejac <= R.ROW_PARITY
            assert e_fig <= 1e-12 and e_rad <= 1e-12
            assert np.array_equal(got.status, status), (got.status, status)
            assert np.isnan(got.delta[~fin]).all() and np.isnan(got.cof[~fin]).all() and np.isnan(got.sigma_radial[~fin]).all()
            assert np.all(got.ellipse[fin, 0] >= got.ellipse[fin, 1]) and np.all((got.direction[fin] >= 0.0) & (got.direction[fin] < np.pi))
            assert np.isnan(got.radial[fin][~pos]).all() and np.isnan(got.sigma_radial[fin][~pos]).all() and np.isfinite(got.sigma[fin][~pos]).all()
            beyond = np.arange(R.MAX_COLUMNS)[None, :] >= K[:, None]
            assert not np.nan_to_num(got.jac.transpose(0, 2, 1)[beyond]).any()                # zero behind the camera's K
            if count >= 5 and c["depth"] is not None:
                assert status[3] & R.NOT_FINITE                          # the NaN depth
            if name == "zernike" and count >= 2:
                assert status[1] & R.NOT_FINITE                          # the centre node, by m / r^2
            elif count >= 2:
                assert not status[1] & R.NOT_FINITE
            if name in ("partial", "zernike"):                           # the fixed c
                assert np.all((got.status & R.PARTIAL) != 0) == bool(columns & R.PRINCIPAL_DISTANCE)
            else:
                assert not (got.status & R.PARTIAL).any()
    if name == "two_camera":
        assert len(set(K.tolist())) == 2
    eng.close()


# ---- 2. the comparison against the reference, the summary included ---------------------------------------------------------------------------
def check_compare(tag, got, exp, s0, s2post, n):
    out, status, sabs, K = exp
    fin = (status & R.NOT_FINITE) == 0
    ed = np.abs(got.d - out[:, 0:2])[fin].max(initial=0.0)
    ratio = of_bound(np.abs(got.M - out[:, 2:5])[fin], float(delta(K)) * sabs[fin])
    # q and the T values, against numpy on the call's own d and C_d.  The determinant m_xx m_yy - m_xy^2 cancels: its relative error, and
    # that of q, is the rounding of the products times m_xx m_yy / det, so 1e-12 (the figure of tests/test_gpu_predict.py) times that
    good = fin & ((got.status & R.SINGULAR) == 0)
    d, M = got.d[good], got.M[good]
    q = (M[:, 2] * d[:, 0] ** 2 - 2.0 * M[:, 1] * d[:, 0] * d[:, 1] + M[:, 0] * d[:, 1] ** 2) / (M[:, 0] * M[:, 2] - M[:, 1] ** 2)
    qs = np.maximum(np.abs(q), 1e-300) * (M[:, 0] * M[:, 2]) / (M[:, 0] * M[:, 2] - M[:, 1] ** 2)
    eq = max((np.abs(got.q[good] - q) / qs).max(initial=0.0), (np.abs(got.T_prio[good] - q / (2.0 * s0)) / (qs / (2.0 * s0))).max(initial=0.0),
             (np.abs(got.T_post[good] - q / (2.0 * s2post)) / (qs / (2.0 * s2post))).max(initial=0.0))
    # the summary, against longdouble sums over the device's own per-node output
    raw = np.column_stack([got.d, got.M, got.q, got.T_prio, got.T_post])
    summ, (sum_d2, abs_tr, sum_tr) = R.summary(raw, got.status, s0)
    s = got.summary
    tree = 4.0 * R.U53 + 2.0 * n * R.U53 ** 2
    e_rms = abs(s.rms - summ[1]) / (tree * summ[1]) if summ[1] > 0.0 else float(s.rms != summ[1])
    e_exp = abs(s.rms_expected - summ[2]) / (tree * summ[2] * abs_tr / sum_tr) if summ[2] > 0.0 else float(not same(s.rms_expected, summ[2]))
    print(f"{tag}: d {ed:.2e} mm, C_d {ratio:.2e} of the bound, q and T {eq:.2e} relative, K {K}; summary: {s.n_finite} finite nodes, rms {s.rms:.3e} "
          f"({e_rms:.2e} of the tree's bound), expected {s.rms_expected:.3e} ({e_exp:.2e}), max |d| {s.max_d:.3e} at {s.max_d_node}, max T_prio "
          f"{s.max_T_prio:.3f} at {s.max_T_node}, {s.n_singular} singular; status {sorted(set(got.status.tolist()))}")
    assert ed <= 1e-13
    assert ratio <= 1.0
    assert eq <= 1e-12
    assert np.array_equal(got.status, status), (got.status, status)
    assert np.isnan(raw[~fin]).all() and np.isnan(got.q[fin & ~good]).all()
    assert (s.n_finite, s.max_d_node, s.max_T_node, s.n_singular) == (int(summ[0]), int(summ[4]), int(summ[6]), int(summ[7]))
    assert same(s.max_T_prio, summ[5])
    assert same(s.max_d, summ[3]) or abs(s.max_d - summ[3]) <= 2.0 * R.U53 * summ[3]          # the square root of the same key: one rounding
    assert e_rms <= 1.0 and e_exp <= 1.0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_the_comparison_and_its_summary_match_the_reference(ref, oracle_mod, name, mode):
    fp = ref[name]["fp"]
    s0, s2post = fp.sigma2apriori, 1.3 * fp.sigma2apriori
    eng = inverting_pass(fp, MODES[mode])
    Q = exported(eng)
    cam_a = fp.n_cameras - 1
    cam_b = 0
    ref_values, ref_cov = perturbed(fp, cam_b)
    vB = R.with_camera(fp, fp.values, cam_b, ref_values)
    for count in COUNTS:
        c = ref[name]["lists"][count]
        cams = np.full(count, cam_a, np.int32)
        wA, JA = R.rows(oracle_mod, fp, fp.values, cams, c["xy"], c["depth"])
        # a certificate with its covariance; relative positions in the 65-node call, but not for the purely radial camera of the free
        # network: without x0, y0 its rows are (xs, ys) g(r), C_d has rank 1 and SINGULAR is left to the rounding (test_exact_answers)
        relative = count == 65 and name != "free"
        cov = None if count == 63 else ref_cov
        wB, JB = R.rows(oracle_mod, fp, fp.values, cams, c["xy"], c["depth"], row_cams=cam_b, row_values=vB)
        got = eng.calibration_compare(cam_a, cam_b, c["xy"], c["depth"], ref_values=ref_values, ref_cov=cov, sigma2_post=s2post, relative=relative)
        exp = R.compare(fp, Q, fp.values, wA, JA, wB, JB, cam_a, cam_b, s0, s2post, ref_values=ref_values, ref_cov=cov, relative=relative)
        check_compare(f"{name} {mode} {count} nodes, camera {cam_a} against a certificate of camera {cam_b}", got, exp, s0, s2post, count)
        only = eng.calibration_compare(cam_a, cam_b, c["xy"], c["depth"], ref_values=ref_values, ref_cov=cov, sigma2_post=s2post, relative=relative,
                                       nodes=False)
        assert only.d is None and bits(*only.summary) == bits(*got.summary)          # the summary alone, without the download
        if fp.n_cameras > 1:
            wB, JB = R.rows(oracle_mod, fp, fp.values, cams, c["xy"], c["depth"], row_cams=cam_b)
            got = eng.calibration_compare(cam_a, cam_b, c["xy"], c["depth"], sigma2_post=s2post, relative=relative)
            exp = R.compare(fp, Q, fp.values, wA, JA, wB, JB, cam_a, cam_b, s0, s2post, relative=relative)
            check_compare(f"{name} {mode} {count} nodes, camera {cam_a} against camera {cam_b} of the engine", got, exp, s0, s2post, count)
    if fp.n_cameras > 1:
        # compare(a, b) and compare(b, a) on the same rays: d changes its sign, C_d agrees to the covariance bound (the sums run in another order)
        c = ref[name]["lists"][257]
        io = fp.values[fp.slot_io(0):fp.slot_io(0) + 3 * fp.n_cameras].reshape(-1, 3)
        ab = eng.calibration_compare(cam_a, cam_b, c["xy"], c["depth"], sigma2_post=s2post)
        ba = eng.calibration_compare(cam_b, cam_a, c["xy"] * (io[cam_b, 2] / io[cam_a, 2]), c["depth"], sigma2_post=s2post)
        _, _, sabs, K = R.compare(fp, Q, fp.values, wA, JA, wB, JB, cam_a, cam_b, s0, s2post)
        fin = (ab.status & R.NOT_FINITE) == 0
        ed = np.abs(ab.d + ba.d)[fin].max()
        ratio = of_bound(np.abs(ab.M - ba.M)[fin], 2.0 * float(delta(K)) * sabs[fin])
        print(f"{name} {mode}: compare(a, b) against compare(b, a): d + d' {ed:.2e} mm, C_d {ratio:.2e} of twice the bound")
        assert ed <= 2e-13 and ratio <= 1.0 and np.array_equal(ab.status, ba.status)
    eng.close()


# ---- 3. exact answers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_exact_answers_bit_for_bit(ref, name, mode):
    fp = ref[name]["fp"]
    eng = inverting_pass(fp, MODES[mode])
    Q = exported(eng)
    c = ref[name]["lists"][257]
    # the principal point alone: J is the unit matrix, C the exported block of x0, y0 at every node
    got = eng.calibration_field(S2, c["cams"], c["xy"], c["depth"], K2, columns=R.PRINCIPAL_POINT)
    fin = (got.status & R.NOT_FINITE) == 0
    cols = fp.io_col[c["cams"]]
    want = np.stack([Q[cols[:, 0], cols[:, 0]], Q[cols[:, 1], cols[:, 0]], Q[cols[:, 1], cols[:, 1]]], 1)
    assert fin.sum() >= 250 and bits(got.cof[fin]) == bits(want[fin])
    # a camera against its own current values: a zero field
    vals = eng.get_parameters()
    for k in range(fp.n_cameras):
        own = vals[R.camera_slots(fp, k)]
        for relative in (False, True):
            z = eng.calibration_compare(k, k, c["xy"], c["depth"], ref_values=own, relative=relative)
            fin = (z.status & R.NOT_FINITE) == 0
            sing = (z.status & R.SINGULAR) != 0
            assert fin.sum() >= 250
            assert not z.d[fin].any() and not z.q[fin & ~sing].any() and not z.T_prio[fin & ~sing].any() and np.isnan(z.q[sing]).all()
            if not relative:
                assert not sing.any()
            else:
                # without x0, y0 the centre node has no column left (C_d = 0), and the rows of a purely radial camera (free) are
                # (xs, ys) g(r): C_d has rank 1 at every node, and whether its determinant rounds above zero is left to the rounding
                if name == "zernike":                             # its centre node is NOT_FINITE before anything else
                    assert not fin[1] and not sing.any()
                elif name == "free":
                    assert sing[1] and not z.M[1].any()
                    assert np.all(np.abs(z.M[fin, 0] * z.M[fin, 2] - z.M[fin, 1] ** 2) <= 1e-12 * z.M[fin, 0] * z.M[fin, 2])
                else:
                    assert sing[1] and not z.M[1].any() and sing.sum() == 1
            s = z.summary
            cand = np.flatnonzero(fin & ~sing)
            assert s.n_finite == fin.sum() and s.rms == 0.0 and s.max_d == 0.0 and s.max_d_node == 0 and s.n_singular == sing.sum()
            assert s.max_T_node == (cand[0] if cand.size else -1) and (s.max_T_prio == 0.0 if cand.size else np.isnan(s.max_T_prio))
            assert s.rms_expected > 0.0
    eng.close()


# ---- 4. determinism and shape ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_two_runs_shuffled_doubled_and_single_calls_give_the_same_bits(ref, name):
    fp = ref[name]["fp"]
    eng = inverting_pass(fp, engine.INVERT_REDUCED)
    c = ref[name]["lists"][257]
    cams, xy, depth = c["cams"], c["xy"], c["depth"]
    a = eng.calibration_field(S2, cams, xy, depth, K2, jacobian=True)
    assert field_bits(a) == field_bits(eng.calibration_field(S2, cams, xy, depth, K2, jacobian=True))
    perm = np.random.default_rng(21).permutation(cams.size)
    assert field_bits(a, perm) == field_bits(eng.calibration_field(S2, cams[perm], xy[perm], depth[perm], K2, jacobian=True))
    twice = np.concatenate([np.arange(cams.size), np.arange(cams.size)[::-1]])
    assert field_bits(a, twice) == field_bits(eng.calibration_field(S2, cams[twice], xy[twice], depth[twice], K2, jacobian=True))
    for k in (0, 1, 5, 200):
        assert field_bits(a, slice(k, k + 1)) == field_bits(eng.calibration_field(S2, cams[k:k + 1], xy[k:k + 1], depth[k:k + 1], K2, jacobian=True))
    ref_values, ref_cov = perturbed(fp, 0)
    ka = fp.n_cameras - 1
    for kw in (dict(ref_values=ref_values, ref_cov=ref_cov), dict(ref_values=ref_values, relative=True)) + ((dict(),) if ka != 0 else ()):
        b = eng.calibration_compare(ka, 0, xy, depth, **kw)
        b2 = eng.calibration_compare(ka, 0, xy, depth, **kw)
        assert compare_bits(b) == compare_bits(b2) and bits(*b.summary) == bits(*b2.summary)
        assert compare_bits(b, perm) == compare_bits(eng.calibration_compare(ka, 0, xy[perm], depth[perm], **kw))
        assert compare_bits(b, twice) == compare_bits(eng.calibration_compare(ka, 0, xy[twice], depth[twice], **kw))
        assert compare_bits(b, slice(5, 6)) == compare_bits(eng.calibration_compare(ka, 0, xy[5:6], depth[5:6], **kw))
    eng.close()


# ---- 5. state and arguments --------------------------------------------------------------------------------------------------------------------
def raw_field(eng, sigma2, k2, columns, cams, xy, depth, n, out, jac, status):
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)      # noqa: E731
    return eng.L.jaicov_calib_field(eng._h, sigma2, k2, columns, p(cams, _pi), p(xy, _pd), p(depth, _pd), n, p(out, _pd), p(jac, _pd), p(status, _pi))


def raw_compare(eng, s2post, cam_a, cam_b, ref_values, ref_cov, flags, xy, depth, n, out, status, summ):
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)      # noqa: E731
    return eng.L.jaicov_calib_compare(eng._h, s2post, cam_a, cam_b, p(ref_values, _pd), p(ref_cov, _pd), flags, p(xy, _pd), p(depth, _pd), n,
                                      p(out, _pd), p(status, _pi), p(summ, _pd))


def test_refusals_leave_the_outputs_and_the_matrix_untouched(ref):
    fp = ref["two_camera"]["fp"]
    cams = np.array([0, 1, 1, 0], np.int32); xy = np.array([[1.0, 2.0], [-3.0, 4.0], [5.0, -6.0], [0.5, 0.25]]); depth = np.full(4, -900.0)
    out = np.full((4, 14), 3.0); jac = np.full((4, 2, 23), 4.0); st = np.full(4, 7, np.int32); summ = np.full(8, 5.0)
    K0 = R.n_columns(fp, 0)
    own = fp.values[R.camera_slots(fp, 0)].copy()
    cov = np.eye(K0) * 1e-12

    def untouched():
        return np.all(out == 3.0) and np.all(jac == 4.0) and np.all(st == 7) and np.all(summ == 5.0)

    ok_f = (1.0, 1.0, R.ALL, cams, xy, depth, 4, out, jac, st)
    ok_c = (1.0, 0, 1, None, None, 0, xy, depth, 4, out, st, summ)
    # no inverting solve: BAD_STATE; a shard: UNSUPPORTED, looked at before the state and the arguments
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    assert raw_field(eng, *ok_f) == -2 and raw_compare(eng, *ok_c) == -2 and untouched()
    assert raw_field(eng, 1.0, 1.0, R.ALL, cams, xy, depth, -1, out, jac, st) == -2              # the state comes before the arguments
    eng.close()
    for kw in (dict(image_range=(0, 3)), dict(apply_shared=False)):
        sh = engine.Engine(fp, device=0, **kw)
        assert raw_field(sh, *ok_f) == -3 and raw_compare(sh, *ok_c) == -3 and untouched()
        sh.close()
    # bad arguments
    eng = inverting_pass(fp, engine.INVERT_REDUCED)
    idx = np.arange(eng.cofactor_order(), dtype=np.int32)
    before = eng.get_cofactor_sub(idx).tobytes()
    bad_cam = cams.copy(); bad_cam[2] = fp.n_cameras
    neg_cam = cams.copy(); neg_cam[0] = -1
    cases = []
    for pos, vals in ((0, (-1.0, np.nan)), (1, (-1.0, np.nan)), (2, (0, R.ALL + 1, 1 << 20)), (3, (None, bad_cam, neg_cam)), (4, (None,)),
                      (5, (None,)), (6, (-1,)), (7, (None,)), (9, (None,))):       # depth NULL: the cameras have D_i terms
        for v in vals:
            a = list(ok_f); a[pos] = v
            cases.append(a)
    for a in cases:
        assert raw_field(eng, *a) == -1, a
        assert untouched()
    bad_ref = own.copy(); bad_ref[3] = np.inf
    bad_cov = cov.copy(); bad_cov[2, 1] = np.nan
    cases = []
    for pos, vals in ((0, (0.0, -1.0, np.nan, np.inf)), (1, (-1, fp.n_cameras)), (2, (-1, fp.n_cameras, 0)), (4, (cov,)), (5, (2, 3)), (6, (None,)),
                      (7, (None,)), (8, (-1,))):
        for v in vals:
            a = list(ok_c); a[pos] = v
            cases.append(a)
    cases.append([1.0, 0, 0, None, None, 0, xy, depth, 4, out, st, summ])                  # cam_b == cam_a without ref_values
    cases.append([1.0, 0, 0, bad_ref, None, 0, xy, depth, 4, out, st, summ])
    cases.append([1.0, 0, 0, own, bad_cov, 0, xy, depth, 4, out, st, summ])
    for a in cases:
        assert raw_compare(eng, *a) == -1, a
        assert untouched()
    assert eng.get_cofactor_sub(idx).tobytes() == before
    # the upper part of ref_cov is not read; an empty call is a call, and writes the summary of no nodes
    up = cov.copy(); up[1, 2] = np.nan
    assert raw_compare(eng, 1.0, 0, 0, own, up, 0, xy, depth, 4, None, None, None) == 0
    assert raw_field(eng, 1.0, 1.0, R.ALL, None, None, None, 0, None, None, None) == 0 and untouched()
    assert raw_compare(eng, 1.0, 0, 1, None, None, 0, None, None, 0, None, None, summ) == 0
    assert summ[0] == 0 and np.isnan(summ[[1, 2, 3, 5]]).all() and summ[4] == summ[6] == -1 and summ[7] == 0
    e = eng.calibration_field(1.0, [], np.zeros((0, 2)))
    assert e.delta.shape == (0, 2) and e.status.size == 0
    # the radial scene without depths is a call; with them it gives the same correction where the depth is -c
    fr = ref["free"]["fp"]
    e2 = inverting_pass(fr, engine.INVERT_REDUCED)
    a = e2.calibration_field(1.0, 0, xy)
    b = e2.calibration_field(1.0, 0, xy, np.full(4, -fr.values[fr.slot_io(0) + 2]))
    assert field_bits(a._replace(jac=np.zeros(0))) == field_bits(b._replace(jac=np.zeros(0))) and not a.status.any()
    e2.close()
    assert eng.get_cofactor_sub(idx).tobytes() == before
    eng.close()


# ---- 6. ownership --------------------------------------------------------------------------------------------------------------------------------
def census():
    lib = engine.load_library()
    lib.jaicov_debug_device_census.argtypes = [C.POINTER(C.c_longlong)]
    lib.jaicov_debug_device_census.restype = None
    a = (C.c_longlong * 2)()
    lib.jaicov_debug_device_census(a)
    return int(a[0]), int(a[1])


def test_the_work_buffers_go_with_release_and_with_the_engine(ref):
    fp = ref["two_camera"]["fp"]
    c = ref["two_camera"]["lists"][257]

    def scenario(release):
        eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
        a = census()
        eng.calibration_field(1.0, c["cams"], c["xy"], c["depth"], jacobian=True)
        b = census()
        assert b[0] > a[0] and b[1] == a[1] + 4, (a, b)          # tab, rows, vals and out of CalibState
        eng.calibration_compare(1, 0, c["xy"][:100], c["depth"][:100])
        assert census()[1] == b[1]
        if release:
            eng.calibration_release()
            assert census() == a                                  # back to the value before the first call
            eng.calibration_release()                             # releasing nothing is no error
        eng.close()

    scenario(True)
    gc.collect()
    c0 = census()
    scenario(False)
    c1 = census()
    print(f"census after warm-up {c0}, after the scenario {c1}")
    assert c1 == c0


# ---- 7. the C++ mirror -----------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_returns_the_bits_of_the_c_calls(tmp_path):
    """calibrationField and compareCalibration through the pybind module return the bits of the C calls on the mirror's own engine (the
    bundled block, MatrixInversion.REDUCED)"""
    import gzip
    import os
    import shutil
    from bundle_adjustment_amd import host_api as H
    from test_host import example_adjustment
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example")
    for f in ("ior", "eor", "obc", "scale"):
        shutil.copy(os.path.join(golden, f"example.{f}"), tmp_path)
    with gzip.open(os.path.join(golden, "example.phc.gz")) as src, open(tmp_path / "example.phc", "wb") as dst:
        dst.write(src.read())
    keep, ba = example_adjustment(H, str(tmp_path / "example"))
    ba.setInvertNormalEquation(H.MatrixInversion.REDUCED)
    assert ba.estimateModel() == H.EstimationStateType.ERROR_FREE_ESTIMATION, ba.lastError()
    s2 = ba.getVarianceFactorAposteriori()
    xy = engine.sensor_grid(36.0, 24.0, 9, 7)
    n = xy.shape[0]
    cams = np.zeros(n, np.int32)
    tab, st, jac = ba.calibrationField(s2, cams.tolist(), xy.ravel().tolist(), k2=2.0, withJacobian=True)
    L = engine.load_library()
    h = C.c_void_p(ba.nativeEngineHandle())
    o = np.zeros((n, 14)); s = np.zeros(n, np.int32); j = np.zeros((n, 2, 23))
    assert L.jaicov_calib_field(h, s2, 2.0, R.ALL, cams.ctypes.data_as(_pi), xy.ctypes.data_as(_pd), None, n, o.ctypes.data_as(_pd), j.ctypes.data_as(_pd),
                                s.ctypes.data_as(_pi)) == 0
    assert tab.shape == (n, 14) and tab.tobytes() == o.tobytes() and st.tobytes() == s.tobytes() and jac.tobytes() == j.tobytes()
    assert np.isfinite(np.delete(o, 31, 0)).all() and np.isfinite(o[31, :10]).all() and np.isnan(o[31, 10:]).all()      # node 31 is the centre
    refv = np.array(ba.cameraValues(0)); refv[2] *= 1.0 + 1e-5
    ctab, cst, summ = ba.compareCalibration(0, 0, xy.ravel().tolist(), refValues=refv.tolist(), sigma2Post=s2, relative=True)
    co = np.zeros((n, 8)); cs = np.zeros(n, np.int32); sm = np.zeros(8)
    assert L.jaicov_calib_compare(h, s2, 0, 0, refv.ctypes.data_as(_pd), None, R.RELATIVE, xy.ctypes.data_as(_pd), None, n, co.ctypes.data_as(_pd),
                                  cs.ctypes.data_as(_pi), sm.ctypes.data_as(_pd)) == 0
    assert ctab.tobytes() == co.tobytes() and cst.tobytes() == cs.tobytes() and summ.tobytes() == sm.tobytes()
    assert sm[0] == n and sm[1] > 0.0 and sm[3] >= sm[1]
    del keep
