"""Extended-precision truth of the EO-reduced normal equations S = N_RR - N_RE inv(N_EE) N_ER, s = n_R - N_RE inv(N_EE) n_E
(host only: numpy long double on the oracle's extended-precision N, n; no device).

The full-order N, n come from ``Oracle.exact_accumulate`` (``oracle/ba_exact.c``: weights sigma0^2 inv(D) and every sum in x87
extended precision, returned as (hi, lo) pairs); the datum rows and the damping are applied as ``oracle_finalize`` applies them
(BA:493-635, BA:814-822).  The exterior orientations are then eliminated image by image in long double, with a long-double
Cholesky inverse of each 6 x 6 N_EE -- the plain Schur complement, not the rank-6 downdate of the weight matrix the device runs.

Two measures of a reduced matrix against that truth, both over the parameter rows and columns [d, e0):
``err_full``: max |S - St|_ij / (g_i g_j) with g = sqrt(diag) of the damped FULL truth -- the scale of every N assert of the suite;
``err_own``:  the same with h = sqrt(|diag St|) -- the Jacobi scale the solver of the reduced system works in (S_ii / N_ii goes
down to about 2e-3 on the small scenes, so this one is up to 500 times sharper).
The right-hand side: max |s - st| / max |st|.
"""
import functools

import numpy as np
import pytest

from bundle_adjustment_amd import scene
from bundle_adjustment_amd.problem import packed_to_full
from helpers import mixed_scene, ragged_scene, two_camera_scene

LD = np.longdouble
MARGIN = 8          # the project's figure (test_gpu_inverse_refinement.py): a device figure may be this many times the reference's


def require_extended_precision():
    """numpy's long double must be the x87 80-bit format (64-bit significand) for the truth to be one."""
    nmant = np.finfo(LD).nmant
    if nmant < 63:
        pytest.skip(f"numpy long double has a {nmant + 1}-bit significand on this machine: no extended-precision truth "
                    f"(needs the 64 bits of the x87 format)")


# ---- the scenes of the GPU matrix (tests/test_gpu_reduced_system.py), by name; the CPU test holds the reference on every one ----
def _block8():
    return scene.make_scene(8, 60, 40, dist=scene.DIST_FULL, weights="block", n_control=5, control_dense=True)


def _free8():
    return scene.make_scene(8, 60, 40, dist=scene.DIST_FULL, weights="block", n_control=0, scale_bar=True)


def _strips():
    """A block flown in strips, 150 points per image, ordinary (diagonal) weights.  With 600 object points (min S_ii / N_ii = 6e-5, one
    image's scaled N_EE at cond 8e4) the reference's fp64 route is 2.1e-12 from the truth in err_full: outside the 1e-12 cap.  With 500
    it is 7e-15, and the partner ranges are as long (86 of one image in 256 columns)."""
    return scene.make_scene(40, 500, 150, layout="strips", dist=scene.DIST_FULL, weights="diag", n_control=8)


def longest_partner_range(fp):
    """The most points of one image within one strip of 256 columns (test_gather_with_partner_ranges_longer_than_a_wave)."""
    pc = fp.point_col.reshape(-1, 3)[:, 0]
    longest = 0
    for img in range(fp.n_images):
        cols = pc[fp.ip_point[fp.ip_image == img]]
        longest = max(longest, int(np.bincount(cols[cols >= 0] // 256).max()))
    return longest


SCENES = {"block8": _block8, "free8": _free8, "tiny": lambda: scene.config("tiny"), "tiny_free": lambda: scene.config("tiny_free"),
          "mixed": mixed_scene, "ragged": ragged_scene, "two_cameras": lambda: two_camera_scene()[0], "strips": _strips}
# scene x damping as the GPU matrix runs them
MATRIX = [(name, lam) for name in SCENES for lam in (0.0, 0.5) if not (name == "strips" and lam)]


@functools.lru_cache(maxsize=None)
def get_scene(name):
    return SCENES[name]()


# ---- truth ------------------------------------------------------------------------------------------------------------
def full_truth(fp, values, sigma2, lam):
    """(Nt, nt): the full bordered, damped system in long double.  Rows / columns 0 .. d-1 carry the datum conditions."""
    import oracle
    o = oracle.Oracle(fp)
    U = fp.n_unknowns
    Nh, Nl, nh, nl = o.exact_accumulate(values, sigma2)
    Nt = packed_to_full(Nh, U).astype(LD) + packed_to_full(Nl, U).astype(LD)
    nt = nh.astype(LD) + nl.astype(LD)
    d = fp.rank_defect
    if d:                            # oracle_finalize writes the datum rows into the zero rows 0 .. d-1 (fp64 values, exact in long double)
        Z = np.zeros(fp.packed_length); zn = np.zeros(U)
        o.finalize(values, Z, zn, 0.0, False)
        B = packed_to_full(Z, U)
        Nt[:d, :] = B[:d, :]; Nt[:, :d] = B[:, :d]
    if lam > 0:                      # BA:814-822: every parameter column, i.e. every column but the datum border
        idx = np.arange(d, U)
        Nt[idx, idx] = Nt[idx, idx] * (LD(1) + LD(lam))
    return Nt, nt


def spd_inverse_ld(E):
    """inv(E) of a small SPD matrix by Cholesky E = L L', Y = inv(L), inv(E) = Y' Y, every operation in long double."""
    m = E.shape[0]
    L = np.zeros((m, m), LD)
    for j in range(m):
        v = E[j, j] - (L[j, :j] * L[j, :j]).sum()
        assert v > 0, "N_EE is not positive definite"
        L[j, j] = np.sqrt(v)
        for i in range(j + 1, m):
            L[i, j] = (E[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    Y = np.zeros((m, m), LD)
    for c in range(m):
        for i in range(c, m):
            Y[i, c] = ((LD(1) if i == c else LD(0)) - (L[i, c:i] * Y[c:i, c]).sum()) / L[i, i]
    return Y.T @ Y


def reduced_truth(fp, values, sigma2, lam, full=None):
    """(St, st, blocks): the reduced system of order e0 = U - 6 images in long double, and (Ei, C, n_E) of every image with
    Ei = inv(N_EE), C = N_RE (e0 x 6), for eo_step_truth.  full: (Nt, nt) of full_truth for the same arguments, if at hand."""
    Nt, nt = full_truth(fp, values, sigma2, lam) if full is None else full
    U, I = fp.n_unknowns, fp.n_images
    e0 = U - 6 * I
    assert np.array_equal(np.asarray(fp.eo_col).ravel(), np.arange(e0, U)), "the EO columns must be the trailing six per image"
    St, st = Nt[:e0, :e0].copy(), nt[:e0].copy()
    blocks = []
    for i in range(I):
        c = e0 + 6 * i
        off = np.delete(Nt[c:c + 6, e0:], np.s_[6 * i:6 * i + 6], axis=1)
        assert not off.any(), "two images' exterior orientations are coupled"
        Ei = spd_inverse_ld(Nt[c:c + 6, c:c + 6])
        C, nE = Nt[:e0, c:c + 6].copy(), nt[c:c + 6].copy()
        rows = np.flatnonzero((C != 0).any(axis=1))         # the image's own points and its camera: everything else is zero
        F = C[rows] @ Ei
        St[np.ix_(rows, rows)] -= F @ C[rows].T
        st[rows] -= F @ nE
        blocks.append((Ei, C, nE))
    return St, st, blocks


def eo_step_truth(blocks, dx_R):
    """Ei (n_E - C' dx_R) of every image, long double, (images, 6)."""
    x = np.asarray(dx_R).astype(LD)
    return np.stack([Ei @ (nE - C.T @ x) for Ei, C, nE in blocks])


def misclosure_shift(fp, values, sigma2, w):
    """A' P (w - w_o) over all image points in long double, w_o the oracle's fp64 misclosures: what the truth's n moves by when the
    misclosures are `w` (n_image_points x 2).

    The truth is exact in its SUMS; its rows A, w are the oracle's fp64 ones (ba_exact.c), which the reference's route shares to the bit.
    A misclosure is observed minus computed, a difference of numbers a thousand times its size, so two correct fp64 evaluations of
    it differ by about 1e-13 of it -- and the right-hand side of an engine that evaluates its own rows would be held to a floor that
    does not contain that rounding.  With this shift the right-hand side is held to the truth OF ITS OWN MISCLOSURES, as the
    reference's is."""
    import oracle
    o = oracle.Oracle(fp)
    n_ip = fp.n_image_points
    rows = [o.rows(values, ip, sigma2) for ip in range(n_ip)]
    dw = np.asarray(w, np.float64).astype(LD) - np.stack([r[0] for r in rows]).astype(LD)
    dn = np.zeros(fp.n_unknowns, LD)
    point_col, io_col, dist_col, eo_col = (np.asarray(a).ravel() for a in (fp.point_col, fp.io_col, fp.dist_col, fp.eo_col))

    def add(ip, t):                                     # dn += A_ip' t, local layout of oracle_rows: point, io, eo, distortion
        img, pt = int(fp.ip_image[ip]), int(fp.ip_point[ip])
        cam = int(fp.image_camera[img])
        jb, je = int(fp.cam_dist_begin[cam]), int(fp.cam_dist_begin[cam + 1])
        cols = np.concatenate([point_col[3 * pt:3 * pt + 3], io_col[3 * cam:3 * cam + 3], eo_col[6 * img:6 * img + 6], dist_col[jb:je]])
        a = rows[ip][1][:, :cols.size].astype(LD).T @ t
        ok = cols >= 0
        np.add.at(dn, cols[ok], a[ok])

    in_block = np.zeros(n_ip, bool)
    for b in range(fp.n_image_blocks):
        b0, b1 = int(fp.blk_ip_begin[b]), int(fp.blk_ip_begin[b + 1])
        in_block[b0:b1] = True
        Ph, Pl = o.exact_block_weight(sigma2, b)
        t = (Ph.astype(LD) + Pl.astype(LD)) @ dw[b0:b1].ravel()
        for k, ip in enumerate(range(b0, b1)):
            add(ip, t[2 * k:2 * k + 2])
    for ip in np.flatnonzero(~in_block):
        add(ip, rows[ip][2].astype(LD) @ dw[ip])
    return dn


# ---- the reference's own fp64 route -----------------------------------------------------------------------------------------
def reference_reduced(oracle, fp, values, sigma2, lam):
    """(S, s) as the reference computes them: createNormalEquation, applyPrecondition, reduceNormalEquationSystem (BA:1197-1342)
    in fp64 -- the oracle's build, precondition, reduce -- and the preconditioner taken off again."""
    o = oracle.Oracle(fp)
    U = fp.n_unknowns
    e0 = U - 6 * fp.n_images
    N, n, V = o.build(values, sigma2, lam)
    o.precondition(V, N, n)
    o.reduce(N, n, False)
    S = packed_to_full(N, U)[:e0, :e0] / np.outer(V[:e0], V[:e0])
    return S, n[:e0] / V[:e0]


def numpy_eo_step(oracle, fp, values, sigma2, lam, dx_R):
    """The EO step Ei (n_E - C' dx_R) in plain fp64 numpy from the oracle's fp64 N, n: the floor of the back-substitution."""
    o = oracle.Oracle(fp)
    U = fp.n_unknowns
    e0 = U - 6 * fp.n_images
    N, n, _ = o.build(values, sigma2, lam)
    Nf = packed_to_full(N, U)
    x = np.asarray(dx_R, np.float64)
    return np.stack([np.linalg.solve(Nf[c:c + 6, c:c + 6], n[c:c + 6] - Nf[:e0, c:c + 6].T @ x) for c in range(e0, U, 6)])


# ---- measures ---------------------------------------------------------------------------------------------------------------------
class Truth:
    """Truth of one scene at one damping, with the scales of the two measures."""

    def __init__(self, fp, lam, values=None, sigma2=None):
        self.fp, self.lam = fp, lam
        self.values = fp.values if values is None else values
        self.sigma2 = fp.sigma2apriori if sigma2 is None else sigma2
        Nt, nt = full_truth(fp, self.values, self.sigma2, lam)
        self.Nt, self.nt = Nt, nt
        self.St, self.st, self.blocks = reduced_truth(fp, self.values, self.sigma2, lam, full=(Nt, nt))
        self.d, self.e0 = fp.rank_defect, self.St.shape[0]
        sl = slice(self.d, self.e0)
        self.g = np.sqrt(np.abs(np.diag(Nt)))[sl]
        self.h = np.sqrt(np.abs(np.diag(self.St)))[sl]
        assert (self.g > 0).all() and (self.h > 0).all()
        self.sl = sl

    def _err(self, S, scale):
        D = np.abs(np.asarray(S).astype(LD)[self.sl, self.sl] - self.St[self.sl, self.sl])
        return float((D / np.outer(scale, scale)).max())

    def err_full(self, S):
        return self._err(S, self.g)

    def err_own(self, S):
        return self._err(S, self.h)

    def err_rhs(self, s):
        sl = self.sl
        return float(np.abs(np.asarray(s).astype(LD)[sl] - self.st[sl]).max() / np.abs(self.st[sl]).max())

    def errors(self, S, s):
        return self.err_full(S), self.err_own(S), self.err_rhs(s)

    def with_misclosures(self, w):
        """The same truth for the misclosures `w` of the image points instead of the oracle's: st and every n_E move, nothing else."""
        import copy
        dn = misclosure_shift(self.fp, self.values, self.sigma2, w)
        T = copy.copy(self)
        T.nt = self.nt + dn
        T.st = T.nt[:self.e0].copy()
        T.blocks = []
        for i, (Ei, C, _) in enumerate(self.blocks):
            nE = T.nt[self.e0 + 6 * i:self.e0 + 6 * i + 6].copy()
            T.st -= C @ (Ei @ nE)
            T.blocks.append((Ei, C, nE))
        return T

    def err_eo_step(self, dx):
        """max over the images of |dx_E - truth| / (largest component of that image's truth), the truth formed with dx's own dx_R."""
        xt = eo_step_truth(self.blocks, dx[:self.e0])
        xe = np.asarray(dx[self.e0:]).astype(LD).reshape(-1, 6)
        return float((np.abs(xe - xt).max(axis=1) / np.abs(xt).max(axis=1)).max())


@functools.lru_cache(maxsize=None)
def oracle_misclosures(name):
    """The oracle's fp64 misclosures of every image point of a scene of the matrix, (n_image_points, 2)."""
    import oracle
    fp = get_scene(name)
    o = oracle.Oracle(fp)
    return np.stack([o.rows(fp.values, ip, fp.sigma2apriori)[0] for ip in range(fp.n_image_points)])


@functools.lru_cache(maxsize=None)
def truth_of(name, lam):
    return Truth(get_scene(name), lam)


@functools.lru_cache(maxsize=None)
def reference_of(name, lam):
    """(S, s) of the reference's fp64 route on a scene of the matrix, and its three figures."""
    import oracle
    fp = get_scene(name)
    S, s = reference_reduced(oracle, fp, fp.values, fp.sigma2apriori, lam)
    return S, s, truth_of(name, lam).errors(S, s)
