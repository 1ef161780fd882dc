/*
 * jaicov_relorient.h -- C ABI of the relative orientation on the device: the orientation of image b of many image pairs in the frame of
 * image a, each from the image points the two images share and their known interior orientations, in one call.
 *
 * The call has no counterpart in the reference, which has no relative orientation.  It closes the chain of start values for a block
 * without control points: jaicov_relorient_pairs gives the first two orientations (up to the base length), jaicov_isect_points the
 * points they see, jaicov_resect_images the next image from those points, and so on.  Where a formula is the reference's, its lines
 * are given (PDF = derivation/PartialDerivativeFactory.java, NES = NormalEquationSystem.java).  Every pair of the call is worked by one
 * wave of one kernel launch (bundle-adjustment_amd/csrc/relorient.hip), the linear starts, every Gauss-Newton run and the rejection
 * rounds included.  It is a stand-alone call with no engine, like jaicov_resect_images.
 *
 * Semantics, per pair g (observations obs_begin[g] .. obs_begin[g+1]-1 in the caller's order; observation k is one object point seen
 * at xy_a[2k], xy_a[2k+1] in image a and at xy_b[2k], xy_b[2k+1] in image b).  Every sum runs over the used observations.
 *   Frame.  X0_a = 0, R_a = I.  The unknowns are b = X0 of image b with |b| = 1 (the base length is not estimable) and the angles
 *     omega, phi, kappa of R = R_b (PDF:125-135).
 *   Rays.  d = (u, v, 1) with u = -(x - x0) / c, v = -(y - y0) / c per image; c may have either sign and the two cameras may differ.  An
 *     object point X is seen where X = lambda_a d_a and R'(X - b) = lambda_b d_b; it lies in front of a camera where c lambda < 0.
 *   Fewer than 6 used observations, or fewer than 5 of a pair with given start values: JAICOV_RELOR_TOO_FEW_POINTS.
 *   Condition.  g = d_b' R' [b]x d_a = (R d_b) . (b x d_a) = 0, one per point, in the Gauss-Helmert form linearised at the observed
 *     values: the cofactor of g is j_a' Q_a j_a + j_b' Q_b j_b with j = dg / d(x, y) of the image point (dg/dd_a = (R d_b) x b,
 *     dg/dd_b = R'(b x d_a), dd/dx = -1/c) and Q = the 2 x 2 dispersion of the image point over sigma2apriori (PDF:308-319 inverted:
 *     var_x, rho sqrt(var_x var_y), var_y; var == NULL: Q = I).  p = 1 / that cofactor, q_k = p_k g_k^2, Omega = sum q_k.  The weights are
 *     recomputed at the current values in every pass; their dependence on the unknowns is not differentiated.
 *   Unknowns of a step: alpha, beta (moves of b along e1, e2), domega, dphi, dkappa.  e = the unit axis i with the smallest |b_i| (the
 *     lowest index on a tie), e1 = b x e / |b x e|, e2 = b x e1.  After a step b <- (b + alpha e1 + beta e2) / |.|.  The derivatives
 *     are analytic: with r = R d_b, p = b x d_a, s = R'p:  dg/dalpha = r . (e1 x d_a), dg/dbeta = r . (e2 x d_a),
 *     dg/domega = p_z r_y - p_y r_z, dg/dphi = p . ((0, cos omega, sin omega) x r), dg/dkappa = u_b s_y - v_b s_x.
 *   Step.  N = sum p a a', n = -sum p a g (5 x 5), Jacobi-preconditioned as NES:82-91 (V = 1/sqrt(diag) where diag > EPS = 2^-53, else 1)
 *     and solved by Cholesky.  NaN or Inf in the system: JAICOV_RELOR_NOT_FINITE; a pivot of the preconditioned matrix <= sqrt(EPS):
 *     JAICOV_RELOR_SINGULAR (a pure rotation without base, and phi = +-90 deg, end here).  Converged when the largest of the five
 *     corrections is <= sqrt(EPS).  max_iterations steps of one run without convergence: JAICOV_RELOR_NOT_CONVERGED; the values are
 *     returned all the same.
 *   Start values.  start != NULL and all six values of the pair finite: X0 / |X0| and the three angles are the only start
 *     (start_kind 0).  Otherwise up to three starts from two linear solutions, each a pair (M, b) with M = R' in twelve fixed slots:
 *     Space (at least 8 used points, slots 0-3).  The 9 x 9 matrix sum k k' with k = d_b (x) d_a (k[3i + j] = d_b[i] d_a[j]) is brought
 *       to diagonal form by 10 sweeps of cyclic Jacobi (rotations (p, q), p < q, row by row; a rotation with a_pq == 0 is skipped).  E
 *       (3 x 3, row-major) is sqrt(2) times the eigenvector of the smallest eigenvalue (the lowest index among equal ones); a
 *       normalisation E33 = 1 would fail in the ordinary stereo case.  The candidates do not exist where the second-smallest eigenvalue
 *       is not > sqrt(EPS) times the largest: the plane case.  n = the eigenvector of the smallest eigenvalue of E'E by 6 sweeps of
 *       cyclic Jacobi of order 3 (rows sorted by falling eigenvalue, the last flipped so that the determinant is +1).  With C = the
 *       cofactor matrix of E (row i = E_i+1 x E_i+2) and D_i = E_i x n:  slots 0-3 = (C - D, n), (C - D, -n), (C + D, n), (C + D, -n).
 *       M is used as it stands (it is orthogonal only where E has two equal singular values; the angles taken from it are a start).
 *     Plane (at least 4 used points, slots 4-11).  The homography (u_a, v_a) -> (u_b, v_b), 8 unknowns h11 .. h32 with h33 = 1, two rows
 *       per point, unit weights, solved like the step's system (a pivot <= sqrt(EPS): no plane candidates).  Eigenvalues l1 >= l2 >= l3
 *       and eigenvectors v1 v2 v3 of H'H by the Jacobi routine of order 3; H <- H / sqrt(l2), l <- l / l2.  No candidates unless
 *       l1 - l3 > sqrt(EPS) (no base).  For s = +1, -1:  u = (sqrt(1 - l3) v1 + s sqrt(l1 - 1) v3) / sqrt(l1 - l3), n = v2 x u; for
 *       sg = +1, -1 (the sign of H is not known where c may have either sign):  w1 = sg H v2, w2 = sg H u, w3 = w1 x w2,
 *       M = w1 v2' + w2 u' + w3 n', t = sg H n - w3, b = -M't / |.| (|.| = 0: the two do not exist); the slots take (M, b), (M, -b)
 *       in the order s, sg, sign of b.
 *     Cheirality.  A point's depths solve the 2 x 2 normal equations of lambda_a M d_a - lambda_b d_b = M b; it counts for a slot where
 *       their determinant is > 0 and c_a lambda_a < 0 and c_b lambda_b < 0.  Of slots 0-3 the one with the highest count goes on
 *       (start_kind 1); of slots 4-11 those whose count equals the highest of them, two at the most (start_kind 2); ties go to the
 *       lowest slot.  The angles of a start are omega = atan2(-r23, r33), phi = asin(r13), kappa = atan2(-r12, r11) of R = M'.
 *     Choice.  Every start (three at the most, in the order space, plane, plane) runs Gauss-Newton to its end and is evaluated there.
 *       One that ends SINGULAR or NOT_FINITE, or with an Omega that is not finite, is dropped.  The one that ends OK with the smallest
 *       Omega is returned, or where none ends OK the NOT_CONVERGED one with the smallest Omega; a tie goes to the first.  Two runs
 *       that end in the same minimum differ in Omega by their rounding, so a tie is taken as wide as the convergence criterion: a
 *       later run replaces an earlier one of the same status only where Omega < Omega_earlier - sqrt(EPS) Omega_earlier.  None left:
 *       JAICOV_RELOR_SINGULAR, or JAICOV_RELOR_NOT_FINITE where NaN or Inf was met in the round.
 *   Evaluation at the returned values: q_k of every observation, Omega, N and Q5 = N^-1; the 6 x 6 cofactor matrix of (X0, Y0, Z0,
 *     omega, phi, kappa) is J Q5 J' with J = [e1 e2 0; 0 0 I3] at the returned b.  It has rank 5.
 *   Rejection (off when reject_threshold == 0).  While more than min_points observations are used and the largest q_k of a used one
 *     exceeds reject_threshold^2, that observation is withdrawn (among equal values the lowest index) and the pair starts again from
 *     its starts: one observation per round.  The status is that of the last round.
 *   TOO_FEW_POINTS, SINGULAR and NOT_FINITE give NaN in all 28 values, 0 in obs_used, NaN in obs_q and 0 in start_kind of the pair.
 *   Determinism.  Every sum has a fixed order (observation k is summed by lane k mod 64, the lanes are combined in a fixed butterfly):
 *     two runs give the same bits, and a pair's result does not depend on what else is in the batch.
 *   Not resolved.  For an exactly planar field both decompositions of the homography are exact relative orientations, and with 5
 *     points there is no redundancy: Omega cannot tell such solutions apart, and the first in the order above is returned.  Not
 *     modelled: lens distortion in the rays; the adjustment's first passes remove what is left.  jaicov_lens_correct (jaicov_lens.h)
 *     reduces measured image points to the distortion-free camera beforehand, with their dispersions.
 *
 * Output out[28 g + k]: X0, Y0, Z0, omega, phi, kappa of image b; the 21 entries of the cofactor matrix, upper triangle row by row in
 * that order; Omega.
 */
#ifndef JAICOV_RELORIENT_H
#define JAICOV_RELORIENT_H

#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-pair outcome in status[] */
enum {
    JAICOV_RELOR_OK = 0,
    JAICOV_RELOR_NOT_CONVERGED = 1,  /* max_iterations steps in the returned run; values are returned          */
    JAICOV_RELOR_TOO_FEW_POINTS = 2, /* fewer than 6 used points, or fewer than 5 with given start values      */
    JAICOV_RELOR_SINGULAR = 3,       /* no start exists, or every run met a pivot <= sqrt(EPS)                  */
    JAICOV_RELOR_NOT_FINITE = 4      /* NaN / Inf in the input, in a step or in the result                      */
};

/* start_kind[] */
enum { JAICOV_RELOR_START_GIVEN = 0, JAICOV_RELOR_START_SPACE = 1, JAICOV_RELOR_START_PLANE = 2 };

#define JAICOV_RELOR_OUT_PER_PAIR 28

/* n_pairs >= 0 pairs; obs_begin[n_pairs + 1]: CSR offsets, obs_begin[0] == 0, non-decreasing; xy_a[2 n_obs], xy_b[2 n_obs];
 * var_a[3 n_obs], var_b[3 n_obs] (either may be NULL: Q = I for that image): var_x > 0, var_y > 0, |rho| < 1 per observation;
 * pair_io[6 n_pairs]: x0, y0, c of image a's camera, then of image b's (c == 0 ends as JAICOV_RELOR_NOT_FINITE); start[6 n_pairs] (may be
 * NULL): X0 Y0 Z0 omega phi kappa of image b, used where all six are finite; sigma2apriori > 0; max_iterations >= 1 per run;
 * reject_threshold >= 0 (0: no rejection); min_points >= 5.  out[28 n_pairs], status[n_pairs]; iterations[n_pairs] (may be NULL):
 * Gauss-Newton solves over all runs and rounds; start_kind[n_pairs] (may be NULL); obs_used[n_obs] (may be NULL): 1 / 0 per observation;
 * obs_q[n_obs] (may be NULL): q of every observation at the returned values, withdrawn ones included; ms_out (may be NULL): kernel
 * time.  Bad arguments are JAICOV_ERR_BAD_ARGUMENT before any device is touched; without a device JAICOV_ERR_NO_DEVICE (there is no CPU
 * fallback).  The return code covers the call; the outcome of each pair is in status. */
int jaicov_relorient_pairs(int32_t n_pairs, const int32_t *obs_begin, const double *xy_a, const double *xy_b, const double *var_a,
                           const double *var_b, const double *pair_io, const double *start, double sigma2apriori,
                           int32_t max_iterations, double reject_threshold, int32_t min_points, double *out, int32_t *status,
                           int32_t *iterations, int32_t *start_kind, uint8_t *obs_used, double *obs_q, double *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_RELORIENT_H */
