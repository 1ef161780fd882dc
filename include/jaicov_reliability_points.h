/*
 * jaicov_reliability_points.h -- C ABI of the leave-one-out diagnostics of every image point, beside the one-dimensional test of
 * jaicov_reliability.h (whose conventions, rows, weights, residuals and lifetime rules hold here unchanged).
 *
 * Both coordinates of an image point are one measurement of one target, and with correlated weights they are correlated with each
 * other and with the other points of their image: the unit of a decision about a blunder is the image point, not the row.  The table
 * below answers "what happens if this point is taken out" for every image point without a second adjustment, from what the
 * reliability run forms anyway (P, G = A Qxx A' P, P v, Qxx).  The declarations live in a header of their own because
 * jaicov_reliability.h is pinned to its four functions.
 *
 * Two identities carry it (standard least-squares theory; they hold with dense weight blocks and with a datum border):
 *   Estimating a 2-vector gross error nabla in the rows S of one image point is the same adjustment as deleting those two rows AND
 *   the matching rows and columns of the dispersion D (P = sigma0^2 inv(D) formed anew from the smaller D).
 *   With g = (P v)_S, M = (P Q_vv P)_SS and nabla^ = -inv(M) g the deleted adjustment has Omega' = Omega - g' inv(M) g and the step
 *   dx' = dx - Qxx A' P[:, S] nabla^.
 *
 * Semantics
 *   For image point k in the caller's order: S = {2k, 2k+1}; P the weight the engine assembles with (2 x 2, or the dense block of
 *   the image); v as in jaicov_rel_run; g = (P v)_S; P_S = P_SS; M = P_S - (P A Qxx A' P)_SS.
 *     0      q          g' inv(M) g: the drop of Omega when the point is deleted
 *     1      T_prio     q / (2 sigma2_test)  (one row instead of two would give t^2)
 *     2      T_post     (q / 2) / ((omega - q) / (dof - 2)); NaN when dof <= 2, omega <= 0 or omega - q <= 0
 *     3, 4   nabla_x, nabla_y   nabla^ = -inv(M) g: the estimated gross error in observation units (an uncorrelated row: -v / r)
 *     5-7    Mxx, Mxy, Myy      the block M itself
 *     8, 9   mdb_major, mdb_minor   sqrt(lambda0 sigma2_test / mu_min), sqrt(lambda0 sigma2_test / mu_max), mu the eigenvalues of M:
 *                       the semi-axes of the ellipse of minimal detectable bias nabla' M nabla = lambda0 sigma2_test
 *     10     delta_ext  sqrt(lambda0 (lambda_max(inv(M) P_S) - 1)): external reliability.  P_S - M is positive semidefinite; a
 *                       negative rounding residue counts as 0
 *     11-13  dX, dY, dZ the rows P(k) of -Qxx A' P[:, S] nabla^: the shift of the point's own object coordinates if the image point
 *                       is deleted (a fixed coordinate has shift 0)
 *   Not controlled.  When mu_min <= 1e-10 max(P_xx, P_yy) (the threshold of the one-dimensional test) columns 0-4 and 8-13 are NaN
 *   and columns 5-7 are still written.  A point seen by exactly two images is the typical case: four rows, three unknowns, M of
 *   rank 1.
 *   The eigenvalues of M and of inv(M) P_S are closed forms of the 2 x 2 entries, without iteration.
 *   Rows outside image points (scale bars, directly observed parameters) keep what jaicov_rel_run gives them: a one-row group has
 *   nothing to add.  The shift of parameters other than the point's own coordinates is not formed (the identity gives all of it;
 *   one U-vector per image point would not fit).
 *
 * Determinism.  Every entry is one fixed-order sum, whatever the number of images per batch: two runs give the same bits.
 */
#ifndef JAICOV_RELIABILITY_POINTS_H
#define JAICOV_RELIABILITY_POINTS_H

#include <stddef.h>
#include <stdint.h>

#include "jaicov_reliability.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JAICOV_REL_POINT_COLUMNS 14
/* Everything jaicov_rel_run does (same four vectors, same summary, same states and errors), and the table above for every image
 * point.  lambda0 > 0 finite (non-centrality, e.g. 17.075; else JAICOV_ERR_BAD_ARGUMENT); omega, dof: the Omega = v'Pv of the same dx
 * (jaicov_neq_omega) and the degrees of freedom; dof <= 2 or omega <= 0 switches T_post off (NaN).  *n_rows, *n_image_points may
 * be NULL. */
int jaicov_rel_run_points(jaicov_engine *e, double sigma2_test, const double *dx, double lambda0, double omega, int32_t dof,
                          int32_t *n_rows, int32_t *n_image_points);
/* out[JAICOV_REL_POINT_COLUMNS][n] column by column (SoA), n = n_image_points of the last jaicov_rel_run_points;
 * JAICOV_ERR_BAD_STATE when the last run was a plain jaicov_rel_run or there is none.  jaicov_rel_get and jaicov_rel_summary work
 * after either run; jaicov_rel_release frees both results. */
int jaicov_rel_get_points(jaicov_engine *e, double *out, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_RELIABILITY_POINTS_H */
