/*
 * jaicov_predict.h -- C ABI of the image-space readers of the cofactor matrix on the device: where an adjusted object point appears
 * in an image that has not measured it, with its confidence ellipse (search windows), and the test of check measurements that
 * were withheld from the adjustment, pair by pair and jointly for groups of pairs.
 *
 * The reference has neither: it prints sigmas of the unknowns only.  Everything here is a read-only consumer of the matrix an
 * inverting solve left on the device (bundle-adjustment_amd/csrc/predict.hip).  Conventions are those of jaicov_precision.h: host
 * pointers, jaicov_status return codes, one engine externally synchronised; every refusal leaves the outputs, the engine and the
 * cofactor matrix bit-identical.
 *
 * A pair (I, P) is an image index and an object point index of the problem; it need not be an image point of the adjustment.
 *
 * Local columns of a pair.  With k = image_camera[I], in the local row layout of the adjustment's own rows (jaicov_neq_get_rows):
 *    0 ..  2  X, Y, Z of P                                  (point_col)
 *    3 ..  5  x0, y0, c of camera k                         (io_col)
 *    6 .. 11  X0, Y0, Z0, omega, phi, kappa of I            (eo_col)
 *   12 ..     the distortion coefficients cam_dist_begin[k] .. cam_dist_begin[k + 1] of camera k   (dist_col)
 * K = 12 + n_dist(k) <= 32 columns, the problem's own column numbers (the d border rows included).  A fixed parameter
 * (JAICOV_COL_FIXED) contributes no term, as in jaicov_xform_run.  Entry (a, b) of the cofactor matrix is Q[max(a, b)][min(a, b)]:
 * only the lower part is valid.
 *
 * The rows.  J (2 x K) and the misclosure w = l - f(x) of a pair are computed by the kernel that computes the rows of the
 * adjustment, at the engine's current slot vector, all distortion families included: for an image point of the adjustment given
 * its own measurement they are the bits of jaicov_neq_get_rows.
 *
 * C = J Qxx J' (2 x 2).  With p the point's columns and s the camera's and image's (local 3 ..), for r, t in {x, y}:
 *   pp_t[a] = sum_{b<3} Q(p_a, p_b) J_t[b],   w_t[a] = sum_{b in s} Q(p_a, s_b) J_t[b],   ss_t[a] = sum_{b in s} Q(s_a, s_b) J_t[b]
 *   C_rt = sum_{a<3} J_r[a] (pp_t[a] + w_t[a]) + sum_{b<3} J_t[b] w_r[b] + sum_{a in s} J_r[a] ss_t[a]
 * every sum with its index ascending, the three parts added from left to right.
 *
 * Refusals common to both calls, checked in this order
 *   NULL engine                                                              JAICOV_ERR_BAD_ARGUMENT
 *   sharded engine (image_begin / image_end, or apply_shared == 0)          JAICOV_ERR_UNSUPPORTED
 *   not all of Qxx on the device (no inverting solve since the last accumulate, or JAICOV_INVERT_REDUCED: the columns of the
 *   exterior orientations are needed)                                       JAICOV_ERR_BAD_STATE
 *   NULL, negative or out-of-range arguments                                JAICOV_ERR_BAD_ARGUMENT
 *
 * Determinism.  Every output entry is one fixed-order sum over the pair's (or the group's) own local columns: two runs give the
 * same bits, and a pair's or a group's figures are the same bits whatever else is in the call and wherever it stands in it.
 */
#ifndef JAICOV_PREDICT_H
#define JAICOV_PREDICT_H

#include <stddef.h>
#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status bits of a pair or a group */
#define JAICOV_PRED_PARTIAL 1     /* a local column is fixed: it contributes no term */
#define JAICOV_PRED_NEGATIVE 2    /* the smaller eigenvalue of C is below -1e-12 times its trace */
#define JAICOV_PRED_NOT_FINITE 4  /* a gathered entry, a row entry or a factor is not finite: the figures are NaN */
#define JAICOV_PRED_OBSERVED 8    /* the pair is an image point of the adjustment */
#define JAICOV_PRED_SINGULAR 16   /* M (a pair of jaicov_pred_check) or M_G (a group) has no Cholesky factor: q and the T values are NaN */

/* columns of one row of the outputs */
#define JAICOV_PRED_POINT_COLUMNS 10
#define JAICOV_PRED_CHECK_COLUMNS 8
#define JAICOV_PRED_GROUP_COLUMNS 4
/* pairs of one group of jaicov_pred_check */
#define JAICOV_PRED_MAX_GROUP 32

/* Predicted image coordinates of n pairs (images[i], points[i]); pairs may repeat and come in any order, n == 0 is a valid empty
 * call.  out[i][0 .. 9] =
 *   0, 1     x, y: the image coordinates of the model, -w of the rows computed with a zero measurement
 *   2 .. 4   q_xx, q_xy, q_yy of C = J Qxx J' (not scaled by sigma2)
 *   5, 6     sigma_x, sigma_y = sqrt(sigma2 max(q, 0))
 *   7, 8     semi-axes A >= B = k2 sqrt(sigma2 max(L, 0)), L = (q_xx + q_yy) / 2 +- hypot((q_xx - q_yy) / 2, q_xy)
 *   9        direction of A in [0, pi), from +x towards +y: atan2(2 q_xy, q_xx - q_yy) / 2, plus pi when negative
 * (7 .. 9 are the formulas of columns 16 .. 18 of jaicov_prec_points; k2 is the caller's expansion factor, no quantile is
 * evaluated.)  status[i]: JAICOV_PRED_PARTIAL, _NEGATIVE, _NOT_FINITE, _OBSERVED.  For an observed pair C is the cofactor block of
 * its adjusted observation.  A point behind the camera is no error: its figures are finite or NOT_FINITE.
 * JAICOV_ERR_BAD_ARGUMENT: n < 0; with n > 0 a NULL pointer or an index outside the problem; sigma2 or k2 negative or NaN. */
int jaicov_pred_points(jaicov_engine *e, double sigma2, double k2, const int32_t *images, const int32_t *points, int32_t n, double *out,
                       int32_t *status);

/* Test of n check measurements xy[2 i], xy[2 i + 1] of the pairs (images[i], points[i]) with the dispersions
 * disp[3 i .. 3 i + 2] = (var_x, var_y, rho).  s0 is the a-priori variance factor the engine recorded for the inverted build;
 * Q_ll = [[var_x, rho sqrt(var_x var_y)], [., var_y]] / s0.  A check measurement l is independent of the adjusted unknowns, so
 * d = l - f(x) has the cofactor matrix M = Q_ll + J Qxx J' (plus).  out[i][0 .. 7] =
 *   0, 1     d_x, d_y: the misclosure of the rows with the measurement given
 *   2 .. 4   m_xx, m_xy, m_yy
 *   5        q = d' M^-1 d = (m_yy d_x^2 - 2 m_xy d_x d_y + m_xx d_y^2) / (m_xx m_yy - m_xy^2); without a positive
 *            determinant JAICOV_PRED_SINGULAR and NaN in 5 .. 7
 *   6        T_prio = q / (2 s0): F(2, inf) under the null hypothesis
 *   7        T_post = q / (2 sigma2_post): F(2, f), f the redundancy of the adjustment sigma2_post was estimated from
 * No quantile is evaluated.  status[i] as above, JAICOV_PRED_OBSERVED included: for an image point of the adjustment l and x are
 * correlated, the plus sign is wrong (jaicov_rel_run has the right matrix, Q_ll - J Qxx J'), and the call does not refuse.
 *
 * Groups.  group_begin[n_groups + 1] is a CSR over the pairs in the caller's order: it starts at 0, ascends and ends at n; a group
 * holds 1 .. JAICOV_PRED_MAX_GROUP pairs (one check point in all its images, say).  group_begin == NULL with n_groups == 0: no
 * groups.  For a group of m pairs M_G is the 2m x 2m matrix with J_i Qxx J_j' in every block and the pairs' Q_ll added on the
 * diagonal blocks, d_G the 2m misclosures.  gout[g][0 .. 3] =
 *   0        q_G = d_G' M_G^-1 d_G by a Cholesky factor
 *   1        T_prio = q_G / (2m s0): F(2m, inf)
 *   2        T_post = q_G / (2m sigma2_post): F(2m, f)
 *   3        2m
 * gstatus[g]: JAICOV_PRED_PARTIAL, _NOT_FINITE (NaN in 0 .. 2), _SINGULAR (no Cholesky factor: NaN in 0 .. 2; the return value
 * stays JAICOV_OK).  A block of M_G is summed in the group's own fixed order, so a group of one pair agrees with the pair's q to
 * rounding, not to the bit.
 * JAICOV_ERR_BAD_ARGUMENT: n < 0 or n_groups < 0; with n > 0 a NULL pointer (gout and gstatus only with n_groups > 0) or an index
 * outside the problem; sigma2_post not positive or NaN; var <= 0 or NaN; |rho| >= 1 or NaN; group_begin not ascending from 0 to n,
 * an empty group, a group of more than JAICOV_PRED_MAX_GROUP pairs. */
int jaicov_pred_check(jaicov_engine *e, double sigma2_post, const int32_t *images, const int32_t *points, const double *xy, const double *disp,
                      int32_t n, const int32_t *group_begin, int32_t n_groups, double *out, int32_t *status, double *gout, int32_t *gstatus);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_PREDICT_H */
