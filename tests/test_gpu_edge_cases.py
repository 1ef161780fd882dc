"""GPU parity on the irregular inputs the reference's object model allows: fixed parameters (column = Integer.MAX_VALUE,
UnknownParameter.java:27 -- no column, but the VALUE still enters the model), several cameras with their own distortion
sets (Camera.java:45-83), jointly dispersed and ordinary images in one adjustment, ragged image sizes."""
import numpy as np
import pytest

from bundle_adjustment_amd import engine, scene
from bundle_adjustment_amd.problem import packed_to_full
from helpers import mixed_scene, ragged_scene, renumber, two_camera_scene

pytestmark = pytest.mark.gpu


def check_against_oracle(oracle_mod, fp, invert=True, **engine_options):
    o = oracle_mod.Oracle(fp)
    s2 = fp.sigma2apriori
    U, d = fp.n_unknowns, fp.rank_defect
    No, no, _ = o.build(fp.values, s2, 0.0)
    dxo, Qo, _, _ = o.step(fp.values, s2, 0.0, invert)
    eng = engine.Engine(fp, **engine_options)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(engine.INVERT_FULL)
    eng.build(s2, 0.0)
    N, n = eng.get_normal()
    Nf, Nof = packed_to_full(N, U), packed_to_full(No, U)
    dg = np.sqrt(np.abs(np.diag(Nof))); dg[dg == 0] = 1.0
    assert (np.abs(Nf - Nof) / np.outer(dg, dg)).max() < 1e-11
    np.testing.assert_allclose(n, no, rtol=0, atol=1e-11 * np.abs(no).max())
    dx = eng.solve(engine.INVERT_FULL if invert else engine.INVERT_NONE)
    np.testing.assert_allclose(dx[d:], dxo[d:], rtol=0, atol=1e-9 * np.abs(dxo[d:]).max())
    if invert:
        q, qo = np.diag(packed_to_full(eng.get_cofactor(), U))[d:], np.diag(packed_to_full(Qo, U))[d:]
        qerr = float(np.abs(q / qo - 1.0).max())
        if qerr >= 1e-9:
            # Two fp64 assemblies of the same N differ in the last bits of its entries (the sums run in different orders), and the
            # variances of a system with cond ~ 1e7 move by 1e-9 ... 1e-8 for that (measured here: 1.2e-9, 2.8e-9, 8.0e-9).  So: the
            # device's inverse must be the exact inverse of ITS N to 1e-9 (Newton steps in extended precision give that inverse), and
            # its distance from the oracle's must be what the two N's exact inverses differ by -- not more.
            def newton_ld(K, X0):
                Kl, X = K.astype(np.longdouble), X0.astype(np.longdouble)
                I2 = 2 * np.eye(K.shape[0], dtype=np.longdouble)
                for _ in range(4):
                    Xn = X @ (I2 - Kl @ X)
                    last = float(np.abs(np.diag(Xn)[d:] / np.diag(X)[d:] - 1).max())
                    X = Xn
                assert last < 1e-12, last             # converged: the exact inverse of K to cond * 2^-64, a thousand times below what is tested
                return X
            Xo, Xd = packed_to_full(Qo, U), packed_to_full(eng.get_cofactor(), U)
            To, Td = newton_ld(Nof, Xo), newton_ld(Nf, Xd)
            dev_inversion = float(np.abs(np.diag(Xd)[d:] / np.diag(Td)[d:] - 1).max())
            oracle_inversion = float(np.abs(np.diag(Xo)[d:] / np.diag(To)[d:] - 1).max())
            assembly = float(np.abs(np.diag(Td)[d:] / np.diag(To)[d:] - 1).max())
            assert dev_inversion < 1e-9, (dev_inversion, oracle_inversion)
            assert qerr <= 1.2 * assembly + dev_inversion + oracle_inversion, (qerr, assembly, dev_inversion, oracle_inversion)
    # the default route of the engine (EO pre-elimination where the problem allows it) gives the same step
    eng.prepare_inverse(engine.INVERT_NONE)
    eng.build(s2, 0.0)
    dx2 = eng.solve(False)
    np.testing.assert_allclose(dx2[d:], dxo[d:], rtol=0, atol=1e-9 * np.abs(dxo[d:]).max())
    reduced = eng.reduced_order() < U
    eng.close()
    return reduced


@pytest.mark.parametrize("weights", ["diag", "block"])
def test_fixed_parameters(oracle_mod, weights):
    fp = scene.make_scene(7, 50, 30, dist=scene.DIST_FULL, weights=weights, n_control=5, control_dense=True)
    P, I, nd = fp.n_points, fp.n_images, fp.dist_kind.size
    pf = np.zeros((P, 3), bool); pf[3, 2] = True; pf[7, :] = True
    iof = np.zeros((1, 3), bool); iof[0, 0] = True
    df = np.zeros(nd, bool); df[1] = True; df[nd - 1] = True
    ef = np.zeros((I, 6), bool); ef[2, 5] = True; ef[0, :] = True
    # the fixed point must not be a control point (its directly observed rows would have no column)
    ctrl = set(int(s) // 3 for s in fp.dg_slot)
    assert 7 not in ctrl and 3 not in ctrl
    fx = renumber(fp, point_fixed=pf, io_fixed=iof, dist_fixed=df, eo_fixed=ef)
    assert fx.n_unknowns == fp.n_unknowns - (1 + 3 + 1 + 2 + 1 + 6)
    reduced = check_against_oracle(oracle_mod, fx)
    assert not reduced            # EO columns are no longer 6 per image: the full-order route is taken


def test_two_cameras_with_different_distortion_sets(oracle_mod):
    two, _ = two_camera_scene()
    reduced = check_against_oracle(oracle_mod, two)
    assert reduced                 # every image still has a dense group and six trailing EO columns


def test_dense_and_ordinary_images_in_one_adjustment(oracle_mod):
    reduced = check_against_oracle(oracle_mod, mixed_scene())
    assert reduced                 # round 4: the ordinary images are pre-eliminated too (block-diagonal weights, test_gpu_ordinary_elimination.py)


def test_ragged_images(oracle_mod):
    """Images with very different numbers of points (3 ... 45) in jointly dispersed groups."""
    reduced = check_against_oracle(oracle_mod, ragged_scene())
    assert reduced


def test_incomplete_distortion_model_is_rejected():
    """A lone Bx (TangentialDistortionModel always owns Bx and By, TDF:39-134) must not silently drop out of the model."""
    base = scene.make_scene(6, 40, 24, dist=scene.DIST_FULL, weights="diag", n_control=4)
    nd = base.dist_kind.size
    keep = np.arange(nd) < 3                       # Cx, Cy, Bx
    s = 3 * base.n_points + 3
    bad = renumber(base, cam_dist_begin=np.array([0, 3], np.int32), dist_kind=base.dist_kind[keep].copy(),
                   dist_order=base.dist_order[keep].copy(), truth=None,
                   values=np.concatenate([base.values[:s], base.values[s:s + nd][keep], base.values[s + nd:]]))
    with pytest.raises(engine.EngineError) as ei:
        engine.Engine(bad)
    assert ei.value.code == -1


def test_an_engine_holds_one_cu_masked_hardware_queue_and_the_pool_keeps_two():
    """A CU-masked stream is a hardware queue of its own, idle or not; with ~20 of them in a process the scheduler time-slices ALL queues and a
    factorisation of 94 block columns takes 29 ms instead of 19 (32 of them: 58 ms; scripts/queue_count_probe.py) -- and the bounded waits of
    the dataflow factorisation start to run out (round 5: the GPU suite's "rare stalls", DESIGN.md section 4 "Hardware queues").  Until then
    every solver held two such streams, every engine has two solvers, and the pool kept them all for the life of the process.  Now: the
    dataflow solver holds ONE (the chain workgroups'), the EO-reduced solver shares the full-order solver's, and the pool keeps at most two
    idle ones of a kind."""
    import ctypes as C
    lib = engine.load_library()

    def census():
        a = (C.c_int * 8)()
        lib.jaicov_debug_stream_census(a)
        return list(a)

    fp = scene.config("cfg3")              # 24 block columns after the elimination: the dataflow factorisation, full-order and reduced solver
    before = census()
    engs = [engine.Engine(fp) for _ in range(5)]
    for e in engs:
        e.set_parameters(fp.values)
        e.build(fp.sigma2apriori, 0.0)
        e.solve(False)
    alive = census()
    held = [alive[k] - alive[4 + k] for k in range(4)]                 # streams in the hands of the five engines, per kind
    assert held[2] == 0 and held[3] == 5, (before, alive)              # no masked stream for trailing updates, one for the chain workgroups each
    for e in engs:
        e.close()
    after = census()
    assert after[2] <= 2 and after[3] <= 2 and after[6] == after[2] and after[7] == after[3], after    # all idle, and no more than two of a kind left
