/*
 * jaicov_resect.h -- C ABI of the spatial resection on the device: start values of the exterior orientation of many images, each from
 * the known object points it sees and its known interior orientation, in one call.
 *
 * The call has no counterpart in the reference, which has no resection.  It stands beside jaicov_dlt_adjust (orientations from at
 * least 6 spatial control points, interior orientation estimated with them) and jaicov_isect_points (points from oriented images):
 * resection and intersection in alternation grow a block image by image.  Unlike the DLT it needs 4 points, works on a plane field
 * of points, keeps the camera it is given and takes c of either sign.  Where a formula is the reference's, its lines are given
 * (PDF = derivation/PartialDerivativeFactory.java, NES = NormalEquationSystem.java).  Every image of the call is worked by one wave of
 * one kernel launch (bundle-adjustment_amd/csrc/resect.hip), the linear start, the whole Gauss-Newton loop and the rejection rounds
 * included.  It is a stand-alone call with no engine, like jaicov_dlt_adjust.
 *
 * Semantics, per image g (observations obs_begin[g] .. obs_begin[g+1]-1 in the caller's order; observation k is the image point
 * xy[2k], xy[2k+1] of the object point xyz[3k .. 3k+2], which is taken as free of error).  Every sum runs over the used observations.
 *   Model.  The collinearity equations PDF:137-152 with the rotation R(omega, phi, kappa) of PDF:125-135, without distortion.  c may
 *     have either sign.  Weights per observation (PDF:308-319) as in jaicov_intersect.h; var == NULL: P = I.
 *   Fewer than 4 observations, or fewer than 3 of an image with given start values: JAICOV_RESECT_TOO_FEW_POINTS.
 *   Reduction.  Xc = centroid of the used object points, s = their root mean square distance from Xc (s^2 = trace of the scatter
 *     matrix sum (X - Xc)(X - Xc)' over the number of used points); P = (X - Xc) / s.  s == 0: JAICOV_RESECT_SINGULAR.  With
 *     u = -(x - x0) / c, v = -(y - y0) / c the model reads u = p1 / p3, v = p2 / p3, p = M P + t, M = R', and X0 = Xc - s R t.
 *   Start values.  eo_start != NULL and all six values of the image finite: they are the start (start_kind 0).  Otherwise the linear
 *     start, in two forms:
 *     Space (at least 6 used points).  The 11 unknowns m11 m12 m13 t1 m21 m22 m23 t2 m31 m32 m33 of [M~ | t~] with t3 = 1, two rows per
 *       point (m1.P + t1 - u m3.P = u, m2.P + t2 - v m3.P = v), unit weights.  The normal equations are Jacobi-preconditioned as
 *       NES:82-91 (V = 1/sqrt(diag) where diag > EPS = 2^-53, else 1) and solved by Cholesky; a pivot of the preconditioned matrix
 *       <= sqrt(EPS) means that this candidate does not exist (the plane case).  det M~ < 0: M~ and t~ change sign.  M = the
 *       orthogonal polar factor of M~ by 10 steps of Newton's iteration X <- (X + X^-T) / 2 from X = M~ / sqrt(|M~|_F^2 / 3);
 *       t = t~ / (trace(M' M~) / 3).
 *     Plane (at least 4 used points).  The eigenvectors of the scatter matrix by 6 sweeps of cyclic Jacobi, sorted by falling
 *       eigenvalue: e1, e2, n; n is flipped so that det [e1 e2 n] = +1.  With a = e1.P, b = e2.P the 8 unknowns h11 h12 h13 h21 h22
 *       h23 h31 h32 of the homography (h33 = 1) are solved the same way.  lambda = (|h1| + |h2|) / 2 over its columns,
 *       r1 = h1 / lambda, r2 = h2 / lambda, t = h3 / lambda; of the two signs of (r1, r2, t) the one with c t3 < 0 is taken (a point in
 *       front of the camera has c N < 0, N of PDF:143, for c of either sign).  M = polar factor of [r1 r2 r1 x r2] times [e1 e2 n]'.
 *     Choice.  Both candidates are evaluated; one whose Omega is not finite does not exist.  The one with the smaller weighted Omega
 *       at its start values is taken, on a tie the plane start.  Neither exists: JAICOV_RESECT_SINGULAR (JAICOV_RESECT_NOT_FINITE
 *       where NaN or Inf was met).  Angles: omega = atan2(-r23, r33), phi = asin(r13), kappa = atan2(-r12, r11); X0 = -R t (reduced).
 *   Gauss-Newton on (X0 reduced, omega, phi, kappa).  A (2 x 6) = PDF:165-171 and 183-189 in the reduced coordinates,
 *     w = observed - computed, N = sum A'PA, n = sum A'Pw, solved by Jacobi preconditioning and Cholesky as above.  NaN or Inf in the
 *     system: JAICOV_RESECT_NOT_FINITE; a pivot <= sqrt(EPS): JAICOV_RESECT_SINGULAR (phi = +-90 deg ends here).  Converged when
 *     max(|dX0| / s, |domega|, |dphi|, |dkappa|) <= sqrt(EPS).  max_iterations steps of one round without convergence:
 *     JAICOV_RESECT_NOT_CONVERGED; the values are returned all the same (as the DLT and the intersection do).
 *   Evaluation at the final values: q_k = w_k' P_k w_k of every observation, Omega = sum of q_k over the used ones, and, in the last
 *     round, N at the final values and Q = N^-1, brought back to the caller's units (X0 rows and columns times s).
 *   Rejection (off when reject_threshold == 0).  While more than min_points observations are used and the largest q_k of a used one
 *     exceeds reject_threshold^2, that observation is withdrawn (among equal values the lowest index) and the image starts again
 *     from its start (the given values, or the linear start over the remaining points): one observation per round.  The status is
 *     that of the last round.
 *   TOO_FEW_POINTS, SINGULAR and NOT_FINITE give NaN in all 28 values, 0 in obs_used, NaN in obs_q and 0 in start_kind of the image.
 *   Determinism.  Every sum has a fixed order (observation k is summed by lane k mod 64, the lanes are combined in a fixed butterfly):
 *     two runs give the same bits, and an image's result does not depend on what else is in the batch.
 *   Not resolved: the two-fold ambiguity of the pose of a plane field seen nearly head-on (both poses fit within the noise; the
 *     start with the smaller Omega is taken and Gauss-Newton stays in its basin).  4 or 5 points that do not lie in a plane have the
 *     plane start only, which need not lie in the basin of the true pose: Omega tells.  Not modelled: lens distortion, as in the DLT
 *     and the intersection; the adjustment's first passes remove what is left.  jaicov_lens_correct (jaicov_lens.h) reduces measured
 *     image points to the distortion-free camera beforehand, with their dispersions.
 *
 * Output out[28 g + k]: X0, Y0, Z0, omega, phi, kappa; the 21 entries of Q, upper triangle row by row in that parameter order; Omega.
 */
#ifndef JAICOV_RESECT_H
#define JAICOV_RESECT_H

#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-image outcome in status[] */
enum {
    JAICOV_RESECT_OK = 0,
    JAICOV_RESECT_NOT_CONVERGED = 1,  /* max_iterations steps in the last round; values are returned        */
    JAICOV_RESECT_TOO_FEW_POINTS = 2, /* fewer than 4 points, or fewer than 3 with given start values       */
    JAICOV_RESECT_SINGULAR = 3,       /* no start exists, or a pivot <= sqrt(EPS) in a step                  */
    JAICOV_RESECT_NOT_FINITE = 4      /* NaN / Inf in the input, in a step or in the result                  */
};

/* start_kind[] */
enum { JAICOV_RESECT_START_GIVEN = 0, JAICOV_RESECT_START_SPACE = 1, JAICOV_RESECT_START_PLANE = 2 };

#define JAICOV_RESECT_OUT_PER_IMAGE 28

/* n_images >= 0 images; obs_begin[n_images + 1]: CSR offsets, obs_begin[0] == 0, non-decreasing; xy[2 n_obs]; xyz[3 n_obs];
 * var[3 n_obs] (may be NULL: unit weights): var_x > 0, var_y > 0, |rho| < 1 per observation; image_io[3 n_images]: x0, y0, c of each
 * image's camera (c == 0 ends as JAICOV_RESECT_NOT_FINITE); eo_start[6 n_images] (may be NULL): X0 Y0 Z0 omega phi kappa, used where
 * all six are finite; sigma2apriori > 0; max_iterations >= 1 per round; reject_threshold >= 0 (0: no rejection); min_points >= 3.
 * out[28 n_images], status[n_images]; iterations[n_images] (may be NULL): Gauss-Newton solves over all rounds; start_kind[n_images]
 * (may be NULL); obs_used[n_obs] (may be NULL): 1 / 0 per observation; obs_q[n_obs] (may be NULL): q of every observation at the final
 * values, withdrawn ones included; ms_out (may be NULL): kernel time.  Bad arguments are JAICOV_ERR_BAD_ARGUMENT before any device is
 * touched; without a device JAICOV_ERR_NO_DEVICE (there is no CPU fallback).  The return code covers the call; the outcome of each
 * image is in status. */
int jaicov_resect_images(int32_t n_images, const int32_t *obs_begin, const double *xy, const double *xyz, const double *var,
                         const double *image_io, const double *eo_start, double sigma2apriori, int32_t max_iterations,
                         double reject_threshold, int32_t min_points, double *out, int32_t *status, int32_t *iterations,
                         int32_t *start_kind, uint8_t *obs_used, double *obs_q, double *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_RESECT_H */
