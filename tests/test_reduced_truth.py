"""The extended-precision truth of the EO-reduced normal equations (tests/reduced_truth.py) on the host: it is consistent with the
full system it was reduced from, the reference's fp64 route stays inside the caps on every scene of the GPU matrix
(tests/test_gpu_reduced_system.py), and the asserts of that matrix -- a figure of at most MARGIN times the reference's -- tell a
reduced system that is subtly wrong from one that is right.  No device."""
import functools

import numpy as np
import pytest

import reduced_truth as rt

LD, MARGIN = rt.LD, rt.MARGIN

EPS_LD = float(np.finfo(LD).eps)


@pytest.fixture(autouse=True)
def _extended_precision(oracle_mod):
    rt.require_extended_precision()


def solve_ld(K, f):
    """K x = f with x in long double: fp64 LU, residuals and the running solution in long double, until it stops moving."""
    K64 = K.astype(np.float64)
    x = np.zeros(f.size, LD)
    for _ in range(8):
        dx = np.linalg.solve(K64, (f - K @ x).astype(np.float64)).astype(LD)
        x = x + dx
        if np.abs(dx).max() <= 4 * EPS_LD * np.abs(x).max():
            break
    return x


@pytest.mark.parametrize("name,lam", [("block8", 0.0), ("block8", 0.5), ("free8", 0.0), ("tiny_free", 0.5), ("ragged", 0.0), ("mixed", 0.5)])
def test_reduced_truth_is_consistent_with_the_full_system(name, lam):
    """[x_R; x_E] solves the damped, bordered full truth system; then St x_R = st and x_E = Ei (n_E - C' x_R).

    The bound.  An entry of St is the difference of long-double numbers up to A = max N_ii / S_ii times its own size (A is about 450
    on the small scenes at lambda = 0, 3700 on the ragged one, 2.2 at lambda = 0.5), each rounded to an ulp, and a row of the
    products sums up to e0 ~ 200 such terms (sqrt(200) ~ 14 ulps): 16 A ulps of long double relative to |St| |x_R| + |st|.  At
    the worst (ragged) that is 6e-15, four orders below the reference's own distance from this truth."""
    T = rt.truth_of(name, lam)
    x = solve_ld(T.Nt, np.concatenate([np.zeros(T.d, LD), T.nt[T.d:]]))
    d, e0 = T.d, T.e0
    xR, xE = x[:e0], x[e0:].reshape(-1, 6)
    amp = float(((T.g / T.h) ** 2).max())
    bound = 16 * amp * EPS_LD
    r = np.abs(T.St @ xR - T.st) / (np.abs(T.St) @ np.abs(xR) + np.abs(T.st))
    xt = rt.eo_step_truth(T.blocks, xR)
    eo = (np.abs(xE - xt).max(axis=1) / np.abs(xt).max(axis=1)).max()
    print(f"{name} lambda {lam}: A = {amp:.0f}, St x_R - st {float(r[d:].max()) / EPS_LD:.0f} ulps, EO step {float(eo) / EPS_LD:.0f} ulps, "
          f"bound {bound / EPS_LD:.0f} ulps = {bound:.1e}")
    assert r[d:].max() <= bound
    assert eo <= bound


@pytest.mark.parametrize("name,lam", rt.MATRIX)
def test_reference_stays_inside_the_caps(name, lam):
    """The floor of every GPU assert is the reference's own distance from the truth: it has to be a distance worth holding the
    device to.  1e-12 in the measure of every other N assert of the suite (they use 1e-11)."""
    _, _, (full, own, rhs) = rt.reference_of(name, lam)
    print(f"{name} lambda {lam}: reference err_full {full:.2e} err_own {own:.2e} rhs {rhs:.2e}")
    assert full < 1e-12
    assert np.isfinite(own) and np.isfinite(rhs)


def test_strips_scene_has_partner_ranges_longer_than_a_wave():
    """The assertion of test_gather_with_partner_ranges_longer_than_a_wave (test_gpu_parity.py) on the strips scene used here."""
    fp = rt.get_scene("strips")
    assert rt.longest_partner_range(fp) > 64


# ---- discrimination: what the GPU asserts would say to a reduced matrix that is nearly right ---------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_normal(name, lam):
    """The oracle's damped fp64 N of a scene, full storage."""
    import oracle
    from bundle_adjustment_amd.problem import packed_to_full
    fp = rt.get_scene(name)
    N, _, _ = oracle.Oracle(fp).build(fp.values, fp.sigma2apriori, lam)
    return packed_to_full(N, fp.n_unknowns)


def image_term(name, lam, img, inverse=np.linalg.inv):
    """C inv(N_EE) C' of one image in fp64 from the oracle's damped fp64 N (e0 x e0)."""
    fp = rt.get_scene(name)
    Nf = oracle_normal(name, lam)
    e0 = fp.n_unknowns - 6 * fp.n_images
    c = e0 + 6 * img
    C = Nf[:e0, c:c + 6]
    return C @ inverse(Nf[c:c + 6, c:c + 6]) @ C.T


def one_entry_off(name, lam, S):
    """One diagonal entry off by a relative 1e-10: the entry where S_ii / N_ii is smallest, i.e. where err_full sees the least of it."""
    T = rt.truth_of(name, lam)
    i = T.d + int(np.argmin(T.h / T.g))
    S[i, i] *= 1 + 1e-10


def dropped_block(name, lam, S):
    """Image 2's contribution to the block of the first two object points it sees is never subtracted."""
    fp = rt.get_scene(name)
    img = 2
    p, q = np.unique(fp.ip_point[fp.ip_image == img])[:2]
    rp, rq = fp.point_col.reshape(-1, 3)[p], fp.point_col.reshape(-1, 3)[q]
    assert (rp >= 0).all() and (rq >= 0).all()
    G = image_term(name, lam, img)
    S[np.ix_(rp, rq)] += G[np.ix_(rp, rq)]
    S[np.ix_(rq, rp)] += G[np.ix_(rq, rp)]


def own_diagonal_damped(name, lam, S):
    """lambda diag(S) instead of lambda diag(N): what blk_diagcorr exists to prevent."""
    assert lam > 0
    S0, _, _ = rt.reference_of(name, 0.0)
    S[:, :] = S0
    i = np.arange(S.shape[0])
    S[i, i] *= 1 + lam


def inverse_rounded_to_fp32(name, lam, S):
    """Image 1's inv(N_EE) carried in fp32."""
    S += image_term(name, lam, 1) - image_term(name, lam, 1, lambda E: np.linalg.inv(E).astype(np.float32).astype(np.float64))


DEFECTS = {"one_entry_1e-10": one_entry_off, "dropped_point_block": dropped_block, "own_diagonal_damped": own_diagonal_damped,
           "fp32_inverse": inverse_rounded_to_fp32}


def defect_cases():
    for name, lam in (("block8", 0.0), ("block8", 0.5), ("tiny", 0.0), ("tiny", 0.5), ("ragged", 0.0), ("ragged", 0.5)):
        for defect in DEFECTS:
            if defect == "own_diagonal_damped" and lam == 0:
                continue                                  # no damping, no such defect
            if defect == "one_entry_1e-10" and (name, lam) == ("ragged", 0.0):
                continue                                  # the reference itself is 2.3e-10 from the truth in err_own there (images of 3 and 4 points)
            yield name, lam, defect


@pytest.mark.parametrize("name,lam,defect", list(defect_cases()))
def test_the_gpu_asserts_tell_nearly_right_from_right(name, lam, defect):
    """Each defect, put into the reference's fp64 S, must exceed MARGIN times the reference's figure in at least one measure: then
    the same assert on the device's S binds.  (One case is out of reach: see defect_cases.)"""
    S, s, (full, own, _) = rt.reference_of(name, lam)
    T = rt.truth_of(name, lam)
    bad = S.copy()
    DEFECTS[defect](name, lam, bad)
    bfull, bown = T.err_full(bad), T.err_own(bad)
    print(f"{name} lambda {lam} {defect}: err_full {bfull:.2e} (reference {full:.2e}), err_own {bown:.2e} (reference {own:.2e})")
    assert T.err_full(S) <= MARGIN * full and T.err_own(S) <= MARGIN * own          # the unperturbed matrix passes
    assert bfull > MARGIN * full or bown > MARGIN * own
