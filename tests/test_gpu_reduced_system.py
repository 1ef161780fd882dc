"""The EO-reduced normal equations as the device assembles them (schur.hip: blk_elim, blk_pprime, blk_tfix, blk_diagcorr[_det],
blk_backsub; assemble.hip: blk_T*, blk_cc*, blk_pc*, blk_pp* and the two gathers), entry by entry against the extended-precision
truth of tests/reduced_truth.py.

The bound of every assert is MARGIN times the distance of the REFERENCE's fp64 route (build, precondition,
reduceNormalEquationSystem, BA:1197-1342) from the same truth, computed here for the scene and damping of the case: nothing in
it comes from the device.  tests/test_reduced_truth.py shows on the host that these asserts tell an entry off by 1e-10, a dropped
point x point contribution, a damping of S's own diagonal and an fp32 inv(N_EE) from a right matrix.  Run with -s for the figures
(DESIGN.md section 5 keeps the table).

The right-hand side and the EO step are held to the truth of the engine's OWN misclosures (reduced_truth.misclosure_shift): the
truth's rows are the oracle's fp64 rows, which the reference shares to the bit, and two correct fp64 evaluations of a misclosure
differ in its last bits.  What the engine contributes to that truth is bounded from outside: its misclosures
are held to the oracle's within W_ULPS ulps of the largest image coordinate, and the figures against the truth of the ORACLE's
misclosures to the suite's standing 1e-11."""
import numpy as np
import pytest

import reduced_truth as rt
from bundle_adjustment_amd import engine
from bundle_adjustment_amd.problem import packed_to_full

pytestmark = pytest.mark.gpu

MARGIN = rt.MARGIN
FORCE = 1           # ordinary_group_elimination: as tests/test_gpu_ordinary_elimination.py
# A misclosure is observed - (x0 + xs + sum of the distortion terms): sums of numbers of the size of the image coordinate.  Each
# evaluation rounds the collinearity quotient, the distortion sum and the final difference at that size (3 ... 4 half ulps), the
# engine contracts to FMAs where the oracle does not: two evaluations differ by up to about 4 ulps of the coordinate; twice that.
W_ULPS = 8
STANDING = 1e-11    # the suite's bound on n against the oracle (test_gpu_parity.py, test_gpu_edge_cases.py)


@pytest.fixture(autouse=True)
def _extended_precision(oracle_mod):
    rt.require_extended_precision()


def reduced_of(eng, U):
    """The leading block of the engine's N, n: the reduced system of the last build / accumulate."""
    N, n = eng.get_normal()
    e0 = eng.reduced_order()
    return packed_to_full(N, U)[:e0, :e0], n[:e0]


def misclosures_of(eng, name):
    """The engine's own misclosures of every image point (jaicov_neq_get_rows), held to the oracle's."""
    fp = rt.get_scene(name)
    w, _ = eng.get_rows(0, fp.n_image_points)
    wo = rt.oracle_misclosures(name)
    bound = W_ULPS * 2.0 ** -52 * max(np.abs(fp.ip_x).max(), np.abs(fp.ip_y).max())
    diff = float(np.abs(w - wo).max())
    print(f"misclosures: {name}: max |w - w_oracle| {diff:.2e}, bound {bound:.2e} ({W_ULPS} ulps of the largest image coordinate), max |w| {np.abs(wo).max():.2e}")
    assert diff <= bound, (diff, bound)
    return w


def hold(tag, name, lam, S, s, w):
    """The three figures of (S, s) against the truth, beside the reference's; each at most MARGIN times the reference's.  The right-hand
    side is held to the truth of the engine's own misclosures w (the reference's figure is its distance from the truth of ITS
    misclosures), and to the standing bound against the truth of the oracle's."""
    T = rt.truth_of(name, lam)
    _, _, ref = rt.reference_of(name, lam)
    assert S.shape == T.St.shape
    dev = T.err_full(S), T.err_own(S), T.with_misclosures(w).err_rhs(s)
    oracle_w = T.err_rhs(s)
    start = T.errors(T.Nt[:T.e0, :T.e0], T.nt[:T.e0])                # N_RR, n_R: what an assembly that eliminated nothing would score
    print(f"{tag}: {name} lambda {lam}: err_full start {start[0]:.1e} reference {ref[0]:.2e} device {dev[0]:.2e} | "
          f"err_own start {start[1]:.1e} reference {ref[1]:.2e} device {dev[1]:.2e} | rhs start {start[2]:.1e} reference {ref[2]:.2e} device {dev[2]:.2e}"
          f" (with the oracle's misclosures {oracle_w:.2e})")
    assert dev[0] <= MARGIN * ref[0], ("err_full", dev[0], ref[0])
    assert dev[1] <= MARGIN * ref[1], ("err_own", dev[1], ref[1])
    assert dev[2] <= MARGIN * ref[2], ("rhs", dev[2], ref[2])
    assert oracle_w <= STANDING, ("rhs, oracle's misclosures", oracle_w)


def check(tag, name, lam, **options):
    fp = rt.get_scene(name)
    eng = engine.Engine(fp, **options)
    eng.set_parameters(fp.values)
    eng.build(fp.sigma2apriori, lam)
    assert eng.reduced_order() == fp.n_unknowns - 6 * fp.n_images
    S, s = reduced_of(eng, fp.n_unknowns)
    w = misclosures_of(eng, name)
    eng.close()
    hold(tag, name, lam, S, s, w)


@pytest.mark.parametrize("lam", [0.0, 0.5])
@pytest.mark.parametrize("deterministic", [None, False])
def test_jointly_dispersed_images(lam, deterministic):
    """8 images of 40 points with a dense dispersion each, dense control group: the default (deterministic) and the arrival-order assembly."""
    check("default" if deterministic is None else "arrival order", "block8", lam, deterministic=deterministic)


@pytest.mark.parametrize("lam", [0.0, 0.5])
def test_free_network_with_scale_bar(lam):
    """d = 6: the datum border in front, the scale bar in N_RR."""
    assert rt.get_scene("free8").rank_defect == 6
    check("free network", "free8", lam)


@pytest.mark.parametrize("form", ["t_vector", "no_fork", "materialise"])
def test_assembly_forms(form, monkeypatch):
    monkeypatch.setenv("JAICOV_ASSEMBLY_FORM", form)            # read when the engine is created
    check(f"form {form}", "block8", 0.5)


@pytest.mark.parametrize("lam", [0.0, 0.5])
@pytest.mark.parametrize("deterministic", [True, False])
@pytest.mark.parametrize("name", ["tiny", "tiny_free"])
def test_ordinary_image_groups(name, deterministic, lam):
    """Ordinary image groups through the same elimination: 2 x 2 weights (tiny) and diagonal weights in a free network (tiny_free, d = 6)."""
    check(f"ordinary, deterministic {deterministic}", name, lam, ordinary_group_elimination=FORCE, deterministic=deterministic)


@pytest.mark.parametrize("lam", [0.0, 0.5])
@pytest.mark.parametrize("name", ["mixed", "ragged", "two_cameras"])
def test_irregular_scenes(name, lam):
    """Dense and ordinary images in one adjustment; 3 ... 45 points per image; two cameras with different distortion sets."""
    check(name, name, lam)


@pytest.mark.parametrize("deterministic", [True, False])
def test_strips_with_partner_ranges_longer_than_a_wave(deterministic):
    """Several 64-lane segments per strip, most (image, strip) pairs empty: the regime that was only compared with the other device path."""
    assert rt.longest_partner_range(rt.get_scene("strips")) > 64
    check(f"strips, deterministic {deterministic}", "strips", 0.0, ordinary_group_elimination=FORCE, deterministic=deterministic)


def test_two_shards_sum_to_the_truth():
    fp = rt.get_scene("block8")
    a = engine.Engine(fp, image_range=(0, 3), apply_shared=True)
    b = engine.Engine(fp, image_range=(3, fp.n_images), apply_shared=False)
    whole = engine.Engine(fp)
    whole.set_parameters(fp.values)
    w = misclosures_of(whole, "block8")
    whole.close()
    parts = []
    for e_ in (a, b):
        e_.set_parameters(fp.values)
        e_.accumulate(fp.sigma2apriori)
        assert e_.reduced_order() == fp.n_unknowns - 6 * fp.n_images
        parts.append(reduced_of(e_, fp.n_unknowns))
        e_.close()
    hold("two shards", "block8", 0.0, parts[0][0] + parts[1][0], parts[0][1] + parts[1][1], w)


@pytest.mark.parametrize("lam", [0.0, 0.5])
@pytest.mark.parametrize("name", ["block8", "tiny"])
def test_eo_back_substitution(oracle_mod, name, lam):
    """blk_backsub_kernel: dx_E of the solve against Ei (n_E - C' dx_R) in long double with the device's own dx_R, per image relative to
    the largest EO component of that image's truth.  Floor: the same formula in plain fp64 numpy from the oracle's fp64 N."""
    fp = rt.get_scene(name)
    T = rt.truth_of(name, lam)
    assert T.d == 0
    eng = engine.Engine(fp, ordinary_group_elimination=FORCE) if name == "tiny" else engine.Engine(fp)
    eng.set_parameters(fp.values)
    eng.build(fp.sigma2apriori, lam)
    e0 = eng.reduced_order()
    assert e0 == T.e0
    dx = eng.solve(False)
    w = misclosures_of(eng, name)
    eng.close()
    ref = dx.copy()
    ref[e0:] = rt.numpy_eo_step(oracle_mod, fp, fp.values, fp.sigma2apriori, lam, dx[:e0]).ravel()
    dev, floor = T.with_misclosures(w).err_eo_step(dx), T.err_eo_step(ref)         # each against the n_E of its own misclosures
    oracle_w = T.err_eo_step(dx)
    print(f"EO back-substitution: {name} lambda {lam}: reference {floor:.2e} device {dev:.2e} (with the oracle's misclosures {oracle_w:.2e})")
    assert dev <= MARGIN * floor, (dev, floor)
    assert oracle_w <= STANDING, oracle_w
