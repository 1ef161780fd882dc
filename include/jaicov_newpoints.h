/*
 * jaicov_newpoints.h -- C ABI of the object-space reader of the cofactor matrix on the device: object points that were not part of
 * the adjustment (a probe tip, a later target, a check point, the ends of a length artefact), intersected from measurements in
 * the adjusted images, with the uncertainty of the cameras and stations that all such points share carried in from Qxx, and the
 * lengths between such points (and points of the block) with the correlations this sharing causes.
 *
 * The reference has no such call; jaicov_isect_points (jaicov_intersect.h) intersects without distortion and with error-free
 * orientations, so its cofactors hold measurement noise only.  Everything here is a read-only consumer of the matrix an inverting
 * solve left on the device (bundle-adjustment_amd/csrc/newpoints.hip): it is the counterpart of jaicov_predict.h, and its
 * conventions are the same: host pointers, jaicov_status return codes, one engine externally synchronised; every refusal leaves
 * the outputs, the engine and the cofactor matrix bit-identical.
 *
 * Rays.  ray_begin[n_points + 1] is a CSR over the rays: it starts at 0 and ascends.  Ray k is the measurement xy[2k], xy[2k + 1] in
 * image ray_image[k] of the problem with the dispersion disp[3k .. 3k + 2] = (var_x, var_y, rho).  A point may name an image more
 * than once: a repeated measurement is legitimate.
 *
 * Semantics, per new point with the rays k = 0 .. m - 1
 *   Model.  The adjustment's own rows (jaicov_neq_get_rows) at the engine's current slot vector, all distortion families included:
 *     J (2 x K) and w = l - f of every ray are computed by the kernel that computes the rows of the adjustment, with the new point
 *     in the place of the object point.  Local columns as in jaicov_predict.h: A_k = J[:, 0:3] for the new point, B_k = J[:, 3:K]
 *     for x0, y0, c of the image's camera, X0 .. kappa of the image and the camera's distortion coefficients.  A fixed parameter
 *     (JAICOV_COL_FIXED) contributes no term, and the point gets JAICOV_NEWPT_PARTIAL.
 *   Weights.  P_k as in jaicov_intersect.h with s0 the a-priori variance factor the engine recorded for the inverted build, so
 *     that the cofactors below are on the scale of Qxx.
 *   Gauss-Newton on X alone.  N = sum A_k' P_k A_k, n = sum A_k' P_k w_k (k ascending over the lanes of a fixed butterfly), Jacobi
 *     preconditioning and Cholesky as jaicov_intersect.h states them (a pivot <= sqrt(EPS): JAICOV_NEWPT_SINGULAR; NaN or Inf:
 *     JAICOV_NEWPT_NOT_FINITE), X += inv(N) n.  Converged when max|dx| <= sqrt(EPS) max(1, max|X - X0|), X0 the projection centre of
 *     the point's first ray.  max_iterations steps without convergence: JAICOV_NEWPT_NOT_CONVERGED, the values are returned all the
 *     same.  Fewer than 2 rays: JAICOV_NEWPT_TOO_FEW_RAYS.  More than JAICOV_NEWPT_MAX_RAYS rays or more than JAICOV_NEWPT_MAX_COLS
 *     distinct shared columns (64 distinct images and two cameras of the largest size fit): JAICOV_NEWPT_TOO_MANY.  Gross errors
 *     are not rejected.
 *   At the final X.  Q_meas = inv(N).  H_k = -inv(N) A_k' P_k B_k (3 x |S_k|) is dX/ds of the converged solution with respect to the
 *     shared parameters of ray k; the terms with second derivatives times residuals are left out, as everywhere in a Gauss-Newton
 *     adjustment.  The point's column list c_0 < c_1 < .. is the sorted union of the (not fixed) columns of its rays,
 *     F[:, a] = sum_k H_k[:, local(c_a)] over the rays in ascending k, and
 *       Q_sys = sum_a ( q(c_a, c_a) F_a F_a' + sum_{b < a} q(c_a, c_b) (F_a F_b' + F_b F_a') ),     Q_XX = Q_meas + Q_sys.
 *     The plus sign says that the new measurements are independent of the adjustment's observations.  Naming an image point of the
 *     adjustment as a "new" measurement makes it wrong (the point's rays and the unknowns are then correlated), as the plus sign of
 *     jaicov_pred_check is for an observed pair; the call cannot know and does not refuse.
 *
 * Pairs.  pairs[2j], pairs[2j + 1] are two members A, B.  A member >= 0 is a new point of this call; a member -1 - P is object point
 * P of the problem: columns point_col[P], F = I, Q_meas = 0, X from the slot vector.  The cross block is
 * Q_AB = F_A Q[cols_A, cols_B] F_B', Q6 the 6 x 6 block with both members' Q_XX on the diagonal, and D = X_B - X_A, L, u, g = [-u, u]
 * and the formulas are those of jaicov_prec_lengths.  A pair of two block points belongs to jaicov_prec_lengths and is
 * JAICOV_ERR_BAD_ARGUMENT; so is a pair that names the same member twice.
 *
 * Refusals, checked in this order
 *   NULL engine                                                              JAICOV_ERR_BAD_ARGUMENT
 *   sharded engine                                                           JAICOV_ERR_UNSUPPORTED
 *   not all of Qxx on the device (no inverting solve since the last accumulate, or JAICOV_INVERT_REDUCED)
 *                                                                            JAICOV_ERR_BAD_STATE
 *   NULL or out-of-range arguments: n_points or n_pairs negative; ray_begin not ascending from 0; an image or a member outside the
 *   call; var <= 0, |rho| >= 1, NaN; sigma2 negative or NaN; max_iterations < 1  JAICOV_ERR_BAD_ARGUMENT
 * A start value that is not finite is no refusal: its point ends as JAICOV_NEWPT_NOT_FINITE.
 *
 * Determinism.  Every output is a fixed-order sum over the point's (the pair's) own rays and columns: two runs give the same
 * bits, and a point's or a pair's figures are the same bits whatever else is in the call and wherever it stands in it.
 */
#ifndef JAICOV_NEWPOINTS_H
#define JAICOV_NEWPOINTS_H

#include <stddef.h>
#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status bits of a new point */
#define JAICOV_NEWPT_PARTIAL 1         /* a shared column of a ray is fixed: it contributes no term */
#define JAICOV_NEWPT_NOT_CONVERGED 2   /* max_iterations steps; the values are returned */
#define JAICOV_NEWPT_TOO_FEW_RAYS 4    /* fewer than 2 rays */
#define JAICOV_NEWPT_TOO_MANY 8        /* more than JAICOV_NEWPT_MAX_RAYS rays or JAICOV_NEWPT_MAX_COLS shared columns */
#define JAICOV_NEWPT_SINGULAR 16       /* a pivot of the preconditioned N <= sqrt(EPS): the rays do not span an angle */
#define JAICOV_NEWPT_NOT_FINITE 32     /* NaN / Inf in a step or in the result */
/* with one of these the 20 columns of the point are NaN */
#define JAICOV_NEWPT_FAILED (JAICOV_NEWPT_TOO_FEW_RAYS | JAICOV_NEWPT_TOO_MANY | JAICOV_NEWPT_SINGULAR | JAICOV_NEWPT_NOT_FINITE)

/* status bits of a pair: the values of JAICOV_PREC_PARTIAL, _NEGATIVE, _NOT_FINITE and _DEGENERATE (jaicov_precision.h) */
#define JAICOV_NEWPT_PAIR_PARTIAL 1     /* a member is a block point with a fixed coordinate, or a new point that is PARTIAL */
#define JAICOV_NEWPT_PAIR_NEGATIVE 2    /* a negative variance of L or of a coordinate difference (its sigma is 0) */
#define JAICOV_NEWPT_PAIR_NOT_FINITE 4  /* a member has failed, or a gathered entry is not finite: the figures are NaN */
#define JAICOV_NEWPT_PAIR_DEGENERATE 8  /* L == 0: sigma_L and both q_L are NaN */

#define JAICOV_NEWPT_COLUMNS 20
#define JAICOV_NEWPT_PAIR_COLUMNS 7
#define JAICOV_NEWPT_MAX_RAYS 64
#define JAICOV_NEWPT_MAX_COLS 448

/* n_points >= 0 new points (0 is a valid empty call); start[3 n_points]: start values (required; the Python wrapper obtains them
 * from jaicov_lens_correct and jaicov_isect_points); sigma2 scales the sigmas only.  out[i][0 .. 19] =
 *   0 ..  2  X, Y, Z
 *   3 ..  8  Q_meas (xx, xy, xz, yy, yz, zz)
 *   9 .. 14  Q_XX in the same order
 *   15       Omega = sum w_k' P_k w_k
 *   16       2m - 3
 *   17 .. 19 sigma_X, sigma_Y, sigma_Z = sqrt(sigma2 max(q_kk, 0)) of Q_XX
 * status[n_points]; iterations[n_points] (may be NULL): the Gauss-Newton steps taken; ray_w[2 n_rays] (may be NULL): the final
 * misclosures, NaN for the rays of a failed point.  With TOO_FEW_RAYS, TOO_MANY, SINGULAR or NOT_FINITE: NaN in all 20 columns; the
 * return value stays JAICOV_OK.
 * pairs, pout, pstatus are needed only with n_pairs > 0.  pout[j][0 .. 6] =
 *   0        L
 *   1        sigma_L = sqrt(sigma2 max(q_L, 0))
 *   2 ..  4  sigma of D_X, D_Y, D_Z
 *   5        q_L = g' Q6 g, not scaled
 *   6        q_L with the cross block set to zero: what neglecting the correlations between the two members gives
 * pstatus[j]: JAICOV_NEWPT_PAIR_* bits. */
int jaicov_newpt_intersect(jaicov_engine *e, double sigma2, int32_t n_points, const int32_t *ray_begin, const int32_t *ray_image,
                           const double *xy, const double *disp, const double *start, int32_t max_iterations, const int32_t *pairs,
                           int32_t n_pairs, double *out, int32_t *status, int32_t *iterations, double *ray_w, double *pout, int32_t *pstatus);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_NEWPOINTS_H */
