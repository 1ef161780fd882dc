/*
 * jaicov_intersect.h -- C ABI of the spatial forward intersection on the device: start values of many object points, each from the
 * image rays that see it, in one call.
 *
 * The call has no counterpart in the reference: JAICOV takes the start values of its object points from a file.  Together with
 * jaicov_dlt_adjust (start values of the orientations from known points) it closes the way from oriented images and measured image
 * points to jaicov_neq_create.  Where a formula is the reference's, its lines are given (PDF = derivation/PartialDerivativeFactory.java,
 * NES = NormalEquationSystem.java).  Every point of the call is worked by one wave of one kernel launch
 * (bundle-adjustment_amd/csrc/intersect.hip), the whole Gauss-Newton loop and the rejection rounds included.  It is a stand-alone call
 * with no engine, like jaicov_dlt_adjust.
 *
 * Semantics, per point p (rays ray_begin[p] .. ray_begin[p+1]-1, in the caller's order; ray k is the image point xy[2k], xy[2k+1] in
 * image ray_image[k])
 *   Model.  The collinearity equations PDF:137-152 with the rotation R(omega, phi, kappa) of PDF:125-135, without distortion (the DLT
 *     models none either; the adjustment's first passes remove what is left).  c may have either sign (AICON: c < 0).
 *     jaicov_lens_correct (jaicov_lens.h) reduces measured image points to this model beforehand, with their dispersions.
 *     Weights per ray (PDF:308-319): rho == 0: P = diag(s0/var_x, s0/var_y); else inv = s0 / ((1 - rho^2) var_x var_y),
 *     P = [[inv var_y, -inv rho sqrt(var_x var_y)], [., inv var_x]], s0 = sigma2apriori.  var == NULL: P = I.
 *   Fewer than 2 rays: JAICOV_ISECT_TOO_FEW_RAYS.
 *   Reduction.  All coordinates are taken relative to Xc, the projection centre of the point's first used ray; Xc is added back at the end.
 *   Linear start.  With u = x - x0, v = y - y0 and r1, r2, r3 the columns of R, every used ray gives the rows
 *     (u r3 + c r1) . (X - X0) = 0 and (v r3 + c r2) . (X - X0) = 0; with unit weights they go into 3 x 3 normal equations.
 *   Solve (the start and every later step).  Jacobi preconditioning as NES:82-91 (V = 1/sqrt(diag) where diag > EPS = 2^-53, else 1),
 *     then Cholesky.  NaN or Inf in the system: JAICOV_ISECT_NOT_FINITE.  A pivot of the preconditioned matrix <= sqrt(EPS):
 *     JAICOV_ISECT_SINGULAR (such a pivot is the squared sine of the angle the rays span: below it the point is numerically at infinity).
 *   Gauss-Newton.  A (2 x 3) = d(x, y)/d(X, Y, Z) of PDF:157-159 and 175-177, w = observed - computed, N = sum A'PA, n = sum A'Pw,
 *     X += dx.  Converged when max|dx| <= sqrt(EPS) max(1, max|X - Xc|).  max_iterations steps of one round without convergence:
 *     JAICOV_ISECT_NOT_CONVERGED; the values are returned all the same (as the DLT does).
 *   Evaluation at the final X: w and q_k = w_k' P_k w_k of every ray, Omega = sum of q_k over the used rays, N at the final X, and the
 *     cofactor matrix Q = inverse of that N.
 *   Rejection (off when reject_threshold == 0).  When more than min_rays rays are used and the largest q_k of a used ray exceeds
 *     reject_threshold^2, that ray is withdrawn (among equal values the lowest index) and the point starts again from the linear start
 *     over the remaining rays: one ray per round.  The status is that of the last round.
 *   Quality.  The largest angle between two used rays, atan2(|d_i x d_j|, d_i . d_j) with d = X - X0 (well conditioned at small angles).
 *   TOO_FEW_RAYS, SINGULAR and NOT_FINITE give NaN in all 11 values, 0 in ray_used and NaN in ray_q of the point (deviation Q3 of the DLT).
 *   Determinism.  Every sum has a fixed order (ray k is summed by lane k mod 64, the lanes are combined in a fixed butterfly): two runs
 *     give the same bits, and a point's result does not depend on what else is in the batch.
 *
 * Output out[11 p + k]: X, Y, Z, qXX, qXY, qXZ, qYY, qYZ, qZZ, Omega, largest angle [rad].
 */
#ifndef JAICOV_INTERSECT_H
#define JAICOV_INTERSECT_H

#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-point outcome in status[] */
enum {
    JAICOV_ISECT_OK = 0,
    JAICOV_ISECT_NOT_CONVERGED = 1,  /* max_iterations steps in the last round; values are returned */
    JAICOV_ISECT_TOO_FEW_RAYS = 2,   /* fewer than 2 rays                                           */
    JAICOV_ISECT_SINGULAR = 3,       /* a pivot <= sqrt(EPS): the rays do not span an angle         */
    JAICOV_ISECT_NOT_FINITE = 4      /* NaN / Inf in a step or in the result                        */
};

#define JAICOV_ISECT_OUT_PER_POINT 11

/* n_points >= 0 points; ray_begin[n_points + 1]: CSR offsets, ray_begin[0] == 0, non-decreasing; ray_image[n_rays] in [0, n_images);
 * xy[2 n_rays]; var[3 n_rays] (may be NULL: unit weights): var_x > 0, var_y > 0, |rho| < 1 per ray; image_io[3 n_images]: x0, y0, c of
 * each image's camera; image_eo[6 n_images]: X0 Y0 Z0 omega phi kappa; sigma2apriori > 0; max_iterations >= 1 per round;
 * reject_threshold >= 0 (0: no rejection); min_rays >= 2.
 * out[11 n_points], status[n_points]; iterations[n_points] (may be NULL): Gauss-Newton solves over all rounds; ray_used[n_rays] (may
 * be NULL): 1 / 0 per ray; ray_q[n_rays] (may be NULL): q of every ray at the final X, withdrawn rays included; ms_out (may be NULL):
 * kernel time.  Bad arguments are JAICOV_ERR_BAD_ARGUMENT before any device is touched; without a device JAICOV_ERR_NO_DEVICE (there
 * is no CPU fallback).  The return code covers the call; the outcome of each point is in status. */
int jaicov_isect_points(int32_t n_points, const int32_t *ray_begin, const int32_t *ray_image, const double *xy, const double *var,
                        int32_t n_images, const double *image_io, const double *image_eo, double sigma2apriori, int32_t max_iterations,
                        double reject_threshold, int32_t min_rays, double *out, int32_t *status, int32_t *iterations, uint8_t *ray_used,
                        double *ray_q, double *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_INTERSECT_H */
