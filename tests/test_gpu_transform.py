"""CoordinateTransformationExteriorOrientation.transform on the device (include/jaicov_transform.h, csrc/transform.hip).

Independent check in numpy: the rows are enumerated in Python, J is formed by complex-step differentiation of
X_T = X0_T + R_T R_S' (X - X0_S) (exact to rounding), Q comes from get_cofactor / get_cofactor_sub, and every device entry must
satisfy |C_dev - C_ref| <= 64 eps sigma2 (|J| |Q| |J|') -- the same bound for the coordinates."""
import dataclasses

import numpy as np
import pytest

from bundle_adjustment_amd import engine, scene
from bundle_adjustment_amd.problem import packed_to_full

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
H = 1e-30


# ---- independent reference ----------------------------------------------------------------------------------------------------
def rot(o, p, k):
    """R(omega, phi, kappa), elementwise for arrays (complex allowed): shape (..., 3, 3)."""
    so, co, sp, cp, sk, ck = np.sin(o), np.cos(o), np.sin(p), np.cos(p), np.sin(k), np.cos(k)
    return np.stack([np.stack([cp * ck, -cp * sk, sp], -1),
                     np.stack([co * sk + so * sp * ck, co * ck - so * sp * sk, -so * cp], -1),
                     np.stack([so * sk - co * sp * ck, so * ck + co * sp * sk, co * cp], -1)], -2)


def xt(q):
    """q (n, 15) = [X Y Z | X0 Y0 Z0 omega phi kappa of src | the same of ref] -> X_T (n, 3)."""
    RS = rot(q[:, 6], q[:, 7], q[:, 8])
    RT = rot(q[:, 12], q[:, 13], q[:, 14])
    d = q[:, 0:3] - q[:, 3:6]
    u = np.einsum("nji,nj->ni", RS, d)
    return q[:, 9:12] + np.einsum("nij,nj->ni", RT, u)


def slot_eo(fp, i):
    return 3 * fp.point_col.shape[0] + 3 * fp.io_col.shape[0] + fp.dist_col.size + 6 * i


def enumerate_rows(fp, points, pairs):
    seen = {}
    for im, pt in zip(fp.ip_image, fp.ip_point):
        seen.setdefault(int(im), set()).add(int(pt))
    return np.array([(p, s, t) for t, s in pairs for p in points if p in seen.get(s, ())], np.int32).reshape(-1, 3)


def reference_rows(fp, vals, ids):
    """Coordinates (n, 3), J values (n, 3, 15) and columns (n, 15) (-1 = no column)."""
    n = len(ids)
    q = np.zeros((n, 15))
    cols = np.full((n, 15), -1, np.int64)
    for t, (p, s, r) in enumerate(ids):
        q[t, 0:3] = vals[3 * p:3 * p + 3]
        q[t, 3:9] = vals[slot_eo(fp, s):slot_eo(fp, s) + 6]
        q[t, 9:15] = vals[slot_eo(fp, r):slot_eo(fp, r) + 6]
        cols[t, 0:3] = fp.point_col[p]
        if s != r:
            cols[t, 3:9] = fp.eo_col[s]
            cols[t, 9:15] = fp.eo_col[r]
    X = xt(q)
    J = np.zeros((n, 3, 15))
    for k in range(15):
        qc = q.astype(complex)
        qc[:, k] += 1j * H
        J[:, :, k] = xt(qc).imag / H
    same = ids[:, 1] == ids[:, 2]
    X[same] = q[same, 0:3]
    J[same] = 0.0
    J[same, 0, 0] = J[same, 1, 1] = J[same, 2, 2] = 1.0
    J[cols[:, None, :].repeat(3, 1) < 0] = 0.0
    # the coordinate bound: |X0_T| + |R_T| |R_S'| (|X| + |X0_S|)
    RS = np.abs(rot(q[:, 6], q[:, 7], q[:, 8])); RT = np.abs(rot(q[:, 12], q[:, 13], q[:, 14]))
    xb = np.abs(q[:, 9:12]) + np.einsum("nij,nkj,nk->ni", RT, RS, np.abs(q[:, 0:3]) + np.abs(q[:, 3:6]))
    return X, J, cols, xb


def dense_J(J, cols, U):
    n = J.shape[0]
    D = np.zeros((3 * n, U))
    for t in range(n):
        for k in range(15):
            if cols[t, k] >= 0:
                D[3 * t:3 * t + 3, cols[t, k]] += J[t, :, k]
    return D


def check_full(eng, fp, points, pairs, sigma2):
    vals = eng.get_parameters()
    xyz, ids = eng.transform(points, pairs, sigma2)
    want = enumerate_rows(fp, points, pairs)
    np.testing.assert_array_equal(ids, want)
    X, J, cols, xb = reference_rows(fp, vals, want)
    assert np.all(np.abs(xyz - X) <= 64 * EPS * xb)
    U = fp.n_unknowns
    Q = packed_to_full(eng.get_cofactor(), U)
    D = dense_J(J, cols, U)
    C = sigma2 * (D @ Q @ D.T)
    B = abs(sigma2) * (np.abs(D) @ np.abs(Q) @ np.abs(D).T)
    R = 3 * len(want)
    Cd = packed_to_full(eng.transform_covariance(), R) if R else np.zeros((0, 0))
    assert Cd.shape == C.shape
    assert np.all(np.abs(Cd - C) <= 64 * EPS * B), float(np.max(np.abs(Cd - C) / np.maximum(B, 1e-300)))
    return xyz, ids, Cd


def inverting_pass(fp, invert, **kw):
    eng = engine.Engine(fp, device=0, **kw)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(invert)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(invert)
    assert eng.cofactor_order() == fp.n_unknowns
    return eng


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def test_tiny_full_every_pair():
    fp = scene.config("tiny")
    eng = inverting_pass(fp, engine.INVERT_FULL)
    I, P = fp.eo_col.shape[0], fp.point_col.shape[0]
    pairs = [(t, s) for t in range(I) for s in range(I)]
    points = list(np.random.default_rng(3).permutation(P))           # the caller's order, not the index order
    xyz, ids, C = check_full(eng, fp, points, pairs, 2.5)
    assert 0 < len(ids) < len(points) * len(pairs)                      # some points are not seen by some images: skipped
    eng.close()


def test_tiny_free_border_columns():
    fp = scene.config("tiny_free")
    assert fp.rank_defect == 6
    eng = inverting_pass(fp, engine.INVERT_FULL)
    I, P = fp.eo_col.shape[0], fp.point_col.shape[0]
    check_full(eng, fp, list(range(P)), [(1, 0), (1, 1), (1, 4), (3, 2)], 0.7)
    eng.close()


def test_ref_equals_src_rows_are_bit_identical():
    fp = scene.config("tiny")
    eng = inverting_pass(fp, engine.INVERT_FULL)
    P = fp.point_col.shape[0]
    s2 = 1.7
    xyz, ids = eng.transform(list(range(P)), [(2, 2), (2, 0)], s2)
    same = np.nonzero(ids[:, 1] == 2)[0]
    assert same.size > 0 and np.all(ids[same, 2] == 2)
    vals = eng.get_parameters()
    pts = ids[same, 0]
    np.testing.assert_array_equal(xyz[same], vals[:3 * P].reshape(P, 3)[pts])
    rows = (3 * same[:, None] + np.arange(3)).ravel().astype(np.int32)
    qcols = fp.point_col[pts].ravel().astype(np.int32)
    np.testing.assert_array_equal(eng.transform_covariance_sub(rows), s2 * eng.get_cofactor_sub(qcols))
    eng.close()


def fix_columns(fp, points, images):
    """The same problem with the columns of `points` and of the exterior orientations of `images` FIXED, the rest renumbered."""
    pc, ec = fp.point_col.copy(), fp.eo_col.copy()
    pc[points] = -1
    ec[images] = -1
    old = np.concatenate([pc.ravel(), fp.io_col.ravel(), fp.dist_col.ravel(), ec.ravel()])
    free = np.sort(old[old >= 0])
    new = np.full(fp.n_unknowns, -1, np.int64)
    new[free] = fp.rank_defect + np.arange(free.size)
    ren = lambda a: np.where(a >= 0, new[np.maximum(a, 0)], -1).astype(np.int32)
    return dataclasses.replace(fp, n_unknowns=int(fp.rank_defect + free.size), point_col=ren(pc), io_col=ren(fp.io_col),
                               dist_col=ren(fp.dist_col), eo_col=ren(ec)).validate()


def test_fixed_point_and_eo_columns_contribute_nothing():
    fp0 = scene.config("tiny")
    control = set((fp0.dg_slot // 3).tolist()) if fp0.dg_slot.size else set()
    pfix = [p for p in range(fp0.point_col.shape[0]) if p not in control and p < 3 * fp0.point_col.shape[0]][:2]
    fp = fix_columns(fp0, pfix, [3])
    eng = inverting_pass(fp, engine.INVERT_FULL)
    P = fp.point_col.shape[0]
    xyz, ids, C = check_full(eng, fp, list(range(P)), [(3, 0), (0, 3), (3, 3), (1, 2)], 1.3)
    # a fixed point seen from its own image: zero rows; a fixed EO pair: only the point columns remain
    for t, (p, s, r) in enumerate(ids):
        if p in pfix and s == r:
            assert np.all(C[3 * t:3 * t + 3] == 0.0)
    eng.close()


def test_cfg3_block_full_expanded():
    fp = scene.config("cfg3_block")
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    P = fp.point_col.shape[0]
    xyz, ids, C = check_full(eng, fp, list(range(P)), [(0, 0), (0, 1), (0, 2)], fp.sigma2apriori)
    assert 2000 <= C.shape[0] <= 6000
    eng.close()


def test_cfg4_blocks_entries_and_bit_reproducibility(cfg4_scene):
    fp = cfg4_scene
    eng = inverting_pass(fp, engine.INVERT_FULL_EXPANDED)
    P = fp.point_col.shape[0]
    pairs = [(0, 0), (0, 1), (0, 2), (0, 3)]
    s2 = 1.9
    vals = eng.get_parameters()
    xyz, ids = eng.transform(list(range(P)), pairs, s2)
    want = enumerate_rows(fp, list(range(P)), pairs)
    np.testing.assert_array_equal(ids, want)
    R = 3 * len(ids)
    assert 4500 <= R <= 7500, R
    X, J, cols, xb = reference_rows(fp, vals, want)
    assert np.all(np.abs(xyz - X) <= 64 * EPS * xb)
    involved = np.unique(cols[cols >= 0])
    pos = np.full(fp.n_unknowns, -1, np.int64)
    pos[involved] = np.arange(involved.size)
    Qs = eng.get_cofactor_sub(involved.astype(np.int32))
    lc = np.where(cols >= 0, pos[np.maximum(cols, 0)], 0)
    Jr = J.reshape(R, 15)                 # row 3t + c: J[t, c, :]
    lr = np.repeat(lc, 3, axis=0)         # its local columns

    def entries(ri, rj):
        q = Qs[lr[ri][:, :, None], lr[rj][:, None, :]]
        c = s2 * np.einsum("nk,nkl,nl->n", Jr[ri], q, Jr[rj])
        b = s2 * np.einsum("nk,nkl,nl->n", np.abs(Jr[ri]), np.abs(q), np.abs(Jr[rj]))
        return c, b

    n = len(ids)
    for t0 in range(0, n, 500):
        ts = np.arange(t0, min(n, t0 + 500))
        for t in ts:
            rows = np.arange(3 * t, 3 * t + 3, dtype=np.int32)
            blk = eng.transform_covariance_sub(rows)
            ri, rj = np.repeat(rows, 3), np.tile(rows, 3)
            c, b = entries(ri, rj)
            assert np.all(np.abs(blk.ravel() - c) <= 64 * EPS * b), t
    blocks = eng.transform_point_blocks()                                   # all 3 x 3 diagonal blocks in one call
    assert blocks.shape == (n, 3, 3)
    for t in range(0, n, 97):
        rows = np.arange(3 * t, 3 * t + 3, dtype=np.int32)
        np.testing.assert_array_equal(blocks[t], eng.transform_covariance_sub(rows))
    rng = np.random.default_rng(7)
    ri, rj = rng.integers(0, R, 2000), rng.integers(0, R, 2000)
    ap = eng.transform_covariance()
    hi, lo = np.maximum(ri, rj), np.minimum(ri, rj)
    dev = ap[hi * (hi + 1) // 2 + lo]
    c, b = entries(ri, rj)
    assert np.all(np.abs(dev - c) <= 64 * EPS * b)
    xyz2, ids2 = eng.transform(list(range(P)), pairs, s2)
    np.testing.assert_array_equal(xyz2, xyz)
    np.testing.assert_array_equal(eng.transform_covariance(), ap)          # deterministic: the same bits
    eng.close()


def _code(fn):
    with pytest.raises(engine.EngineError) as ei:
        fn()
    return ei.value.code


def test_errors_state_arguments_and_lifetime():
    fp = scene.make_scene(6, 40, 24, dist=scene.DIST_FULL, weights="block", n_control=4)
    s2 = fp.sigma2apriori
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    assert _code(lambda: eng.transform([0, 1], [(0, 1)], 1.0)) == -2                  # no inverting solve yet
    eng.prepare_inverse(engine.INVERT_REDUCED)
    eng.build(s2, 0.0)
    eng.solve(engine.INVERT_REDUCED)
    assert eng.cofactor_order() < fp.n_unknowns                                    # the exterior orientations were eliminated
    assert _code(lambda: eng.transform([0, 1], [(0, 1)], 1.0)) == -2                  # REDUCED leaves no full Qxx
    assert _code(lambda: eng.transform_covariance()) == -2                            # nothing to read yet
    eng.prepare_inverse(engine.INVERT_FULL_EXPANDED)
    eng.build(s2, 0.0)
    eng.solve(engine.INVERT_FULL_EXPANDED)
    P, I = fp.point_col.shape[0], fp.eo_col.shape[0]
    xyz, ids = eng.transform(list(range(P)), [(0, 1), (0, 0)], s2)
    C = eng.transform_covariance()
    assert _code(lambda: eng.transform([P], [(0, 1)], 1.0)) == -1                     # point out of range
    assert _code(lambda: eng.transform([-1], [(0, 1)], 1.0)) == -1
    assert _code(lambda: eng.transform([0], [(0, I)], 1.0)) == -1                     # image out of range
    assert _code(lambda: eng.transform([0], [(-1, 0)], 1.0)) == -1
    assert _code(lambda: eng.transform([0, 2, 0], [(0, 1)], 1.0)) == -1               # duplicate point (a Set in the reference)
    assert "duplicate" in eng.L.jaicov_neq_last_error(eng._h).decode()
    # the refused runs left the previous result in place
    np.testing.assert_array_equal(eng.transform_covariance(), C)
    R = 3 * len(ids)
    pd, pi = engine.C.POINTER(engine.C.c_double), engine.C.POINTER(engine.C.c_int32)
    buf = np.zeros(C.size + 1)
    assert eng.L.jaicov_xform_get_covariance(eng._h, buf.ctypes.data_as(pd), buf.size) == -1
    assert eng.L.jaicov_xform_get_covariance(eng._h, buf.ctypes.data_as(pd), C.size - 1) == -1
    xb, ib = np.zeros(3 * len(ids) + 3), np.zeros(3 * len(ids) + 3, np.int32)
    assert eng.L.jaicov_xform_get_coordinates(eng._h, xb.ctypes.data_as(pd), ib.ctypes.data_as(pi), len(ids) + 1) == -1
    assert _code(lambda: eng.transform_covariance_sub([R])) == -1
    assert _code(lambda: eng.transform_covariance_sub([-1])) == -1
    # the result survives a later build and solve
    eng.prepare_inverse(engine.INVERT_NONE)
    eng.build(s2, 0.0)
    eng.solve(False)
    np.testing.assert_array_equal(eng.transform_covariance(), C)
    np.testing.assert_array_equal(eng.transform_covariance_sub([0, 1, 2]), packed_to_full(C, R)[:3, :3])
    # zero transformed points: a valid, empty result (the non-inverting solve above released Qxx: invert once more)
    eng.prepare_inverse(engine.INVERT_FULL_EXPANDED)
    eng.build(s2, 0.0)
    eng.solve(engine.INVERT_FULL_EXPANDED)
    xyz0, ids0 = eng.transform([], [(0, 1)], s2)
    assert xyz0.shape == (0, 3) and eng.transform_covariance().size == 0
    eng.transform_release()
    assert _code(lambda: eng.transform_covariance()) == -2
    eng.transform_release()                                                         # idempotent
    eng.close()


def test_host_mirror_on_the_example_block(tmp_path):
    import gzip
    import os
    import shutil
    from bundle_adjustment_amd import host_api as Hm
    G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "example")
    for f in ("ior", "eor", "obc", "scale"):
        shutil.copy(os.path.join(G, f"example.{f}"), tmp_path)
    with gzip.open(os.path.join(G, "example.phc.gz")) as src, open(tmp_path / "example.phc", "wb") as dst:
        dst.write(src.read())
    pr = Hm.read_aicon_flat(str(tmp_path / "example"))
    cam = pr.camera
    ba = Hm.BundleAdjustment()
    ba.add(cam)
    for s in pr.scaleBars():
        ba.add(s)
    ba.setInvertNormalEquation(Hm.MatrixInversion.FULL)
    assert ba.estimateModel() == Hm.EstimationStateType.ERROR_FREE_ESTIMATION
    images = cam.images()
    points = pr.points()[:60]
    align = [(images[0], [images[1], images[0], images[2]]), (images[3], [images[4]])]
    s2 = ba.getVarianceFactorAposteriori()
    tr = Hm.CoordinateTransformationExteriorOrientation.getInstance()
    tr.transform(points, align, s2, ba)
    out = tr.getTransformedCoordinates()
    seen = {im.getId(): {c.getObjectCoordinate().getName() for c in im.coordinates()} for im in images[:5]}
    names = [f"{p.getName()} {s.getId()} {t.getId()}" for t, srcs in align for s in srcs for p in points if p.getName() in seen[s.getId()]]
    assert [o.getName() for o in out] == names and len(names) > 0
    assert [o.getX().getColumn() for o in out] == [3 * i for i in range(len(out))]
    assert [o.getZ().getColumn() for o in out] == [3 * i + 2 for i in range(len(out))]
    # the same call through the C ABI on the adjustment's engine: the same indices give the same bits
    h = engine.C.c_void_p(ba.nativeEngineHandle())
    L = engine.load_library()
    C_host = np.asarray(tr.getCovarianceMatrix())
    R = 3 * len(out)
    assert C_host.size == R * (R + 1) // 2
    pidx = {p.getName(): i for i, p in enumerate(ba.getObjectCoordinates())}
    iidx = {im.getId(): i for i, im in enumerate(images)}
    pts = np.array([pidx[p.getName()] for p in points], np.int32)
    ref = np.array([iidx[t.getId()] for t, srcs in align for s in srcs], np.int32)
    src = np.array([iidx[s.getId()] for t, srcs in align for s in srcs], np.int32)
    pi, pd = engine.C.POINTER(engine.C.c_int32), engine.C.POINTER(engine.C.c_double)
    n = engine.C.c_int32(0)
    assert L.jaicov_xform_run(h, pts.ctypes.data_as(pi), pts.size, ref.ctypes.data_as(pi), src.ctypes.data_as(pi), ref.size, s2, engine.C.byref(n)) == 0
    assert n.value == len(out)
    C_abi = np.zeros(R * (R + 1) // 2)
    assert L.jaicov_xform_get_covariance(h, C_abi.ctypes.data_as(pd), C_abi.size) == 0
    np.testing.assert_array_equal(C_host, C_abi)
    xyz, ids = np.zeros((n.value, 3)), np.zeros((n.value, 3), np.int32)
    assert L.jaicov_xform_get_coordinates(h, xyz.ctypes.data_as(pd), ids.ctypes.data_as(pi), n.value) == 0
    # the mirror's coordinates are in the frame of the objects' values: the engine's plus the centring shift of each point
    vals = np.zeros(L.jaicov_neq_num_slots(h))
    assert L.jaicov_neq_get_parameters(h, vals.ctypes.data_as(pd), vals.size) == 0
    ocs = ba.getObjectCoordinates()
    for t, o in enumerate(out):
        p = ocs[ids[t, 0]]
        shift = np.array([p.getX().getValue(), p.getY().getValue(), p.getZ().getValue()]) - vals[3 * ids[t, 0]:3 * ids[t, 0] + 3]
        got = np.array([o.getX().getValue(), o.getY().getValue(), o.getZ().getValue()])
        np.testing.assert_allclose(got, xyz[t] + shift, rtol=1e-12, atol=1e-9)
