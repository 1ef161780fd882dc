/*
 * jaicov_simil.h -- C ABI of the absolute orientation on the device: the spatial similarity transformation (seven parameters) between
 * two sets of the same points, for many models in one call, and the call that carries a model's points and image orientations into
 * the target frame.
 *
 * The calls have no counterpart in the reference, which has no absolute orientation.  jaicov_relorient_pairs, jaicov_isect_points and
 * jaicov_resect_images build a model in the frame of its first image with base length 1; jaicov_simil_models brings such a model
 * onto control points or onto another model, jaicov_simil_apply moves what the model holds.  Where a formula is the reference's, its
 * lines are given (PDF = derivation/PartialDerivativeFactory.java, NES = NormalEquationSystem.java).  Every model of the call is worked
 * by one wave of one kernel launch (bundle-adjustment_amd/csrc/simil.hip), the closed start, the Gauss-Newton steps and the rejection
 * rounds included.  Both are stand-alone calls with no engine, like jaicov_relorient_pairs.
 *
 * Semantics of jaicov_simil_models, per model g (points pt_begin[g] .. pt_begin[g+1]-1 in the caller's order; point k is s_k =
 * src[3k .. 3k+2] in the model's frame and d_k = dst[3k .. 3k+2] in the target frame).  Every sum runs over the used points.
 *   Model.  d = T + m R s with R = R(omega, phi, kappa) of PDF:125-135 (= Rx(omega) Ry(phi) Rz(kappa)) and m > 0.  A round works in the
 *     centred form d = T_c + m R (s - sbar), sbar = (sum s_k) / n the plain mean of the round's used source points: the system stays
 *     well-conditioned where the coordinates lie far from the origin.  T = T_c - m R sbar is returned.  A mean that is not finite:
 *     JAICOV_SIMIL_NOT_FINITE.
 *   Fewer than 3 used points: JAICOV_SIMIL_TOO_FEW_POINTS.
 *   Condition (Gauss-Helmert, linearised at the observed values, as in the relative orientation).  With s' = s_k - sbar and r = R s':
 *     e_k = (d_k - T_c) - m r,  C_k = Q_d,k + m^2 R Q_s,k R',  P_k = adj(C_k) / det(C_k),  q_k = e_k' P_k e_k,  Omega = sum q_k.
 *     Q_s,k and Q_d,k are the 3 x 3 cofactor matrices of the point in the two frames (cof_src == NULL: 0, the model is error-free;
 *     cof_dst == NULL: I).  The weights are recomputed at the current values in every pass; their dependence on the unknowns is not
 *     differentiated.  A used point whose C_k has a leading minor (c11, c11 c22 - c12^2, det) that is not > 0 ends the model as
 *     JAICOV_SIMIL_SINGULAR (a NaN off the diagonal of a cofactor matrix ends here too).
 *   Step.  Unknowns dT_c (3), dm, domega, dphi, dkappa.  A_k (3 x 7) = [I | r | m (0, -r_z, r_y)' | m (0, cos omega, sin omega)' x r |
 *     m R (-s'_y, s'_x, 0)'], the analytic derivatives of T_c + m R s'.  N = sum A'PA, n = sum A'Pe (7 x 7), Jacobi-preconditioned
 *     as NES:82-91 (V = 1/sqrt(diag) where diag > EPS = 2^-53, else 1) and solved by Cholesky.  NaN or Inf in the system or in the
 *     corrections: JAICOV_SIMIL_NOT_FINITE; a pivot of the preconditioned matrix <= sqrt(EPS): JAICOV_SIMIL_SINGULAR (phi = +-90 deg
 *     ends here); m not > 0 after a step, or in given start values: JAICOV_SIMIL_SINGULAR.  Converged when the largest of the seven
 *     corrections is <= sqrt(EPS).  max_iterations steps of one round without convergence: JAICOV_SIMIL_NOT_CONVERGED; the values are
 *     returned all the same.
 *   Start values.  start != NULL and all seven values of the model (Tx Ty Tz m omega phi kappa) finite: they are the start
 *     (start_kind 0), T_c = T + m R sbar.  Otherwise the closed start with unit weights (start_kind 1):
 *       dbar = (sum d_k) / n;  M = sum (d_k - dbar)(s_k - sbar)',  ss = sum |s_k - sbar|^2.  Not finite: JAICOV_SIMIL_NOT_FINITE.
 *       Eigenvalues l1 >= l2 >= l3 and eigenvector rows v1 v2 v3 (det +1) of M'M by 6 sweeps of cyclic Jacobi of order 3.
 *       Not l2 > sqrt(EPS) l1: JAICOV_SIMIL_SINGULAR (collinear or coincident points).
 *       u1 = M v1 / |.|;  u2 = M v2 - (u1 . M v2) u1, normalised;  u3 = u1 x u2;  R = u1 v1' + u2 v2' + u3 v3': the Kabsch rotation,
 *       proper by construction and valid for plane point fields, where M has rank 2.  R is used as it stands: it is not made
 *       orthogonal again, m is taken with it and the angles are read from it.
 *       omega = atan2(-r23, r33), phi = asin(r13), kappa = atan2(-r12, r11).
 *       m = sum (d_k - dbar) . R (s_k - sbar) / ss, taken as (sum_ij r_ij M_ij) / ss, which is the same sum.  m not > 0:
 *       JAICOV_SIMIL_SINGULAR.  T_c = dbar.
 *     With equal isotropic cofactors the closed start is the least-squares solution already.
 *   Evaluation at the returned values: q_k of every point (withdrawn ones included), Omega, N and Q7 = N^-1; the 7 x 7 cofactor matrix of
 *     (Tx, Ty, Tz, m, omega, phi, kappa) is J Q7 J' with J = the identity except dT/dm = -R sbar and dT/dangle = -m dR/dangle sbar.
 *   Rejection (off when reject_threshold == 0).  While more than min_points points are used and the largest q_k of a used one exceeds
 *     reject_threshold^2, that point is withdrawn (among equal values the lowest index) and the model starts again from its start:
 *     sbar and the closed start are computed again, one point goes per round.  The status is that of the last round.
 *   TOO_FEW_POINTS, SINGULAR and NOT_FINITE give NaN in all 36 values, 0 in pt_used, NaN in pt_q and 0 in start_kind of the model.
 *   Determinism.  Every sum has a fixed order (point k is summed by lane k mod 64, the lanes are combined in a fixed xor butterfly):
 *     two runs give the same bits, and a model's result does not depend on what else is in the batch.
 *   Not resolved.  phi = +-90 deg ends SINGULAR, as in the sibling calls.  A mirrored point set is not detected as such: the rotation
 *     stays proper, and what comes back is a poor fit with a large Omega.
 *
 * Output out[36 g + k]: Tx, Ty, Tz, m, omega, phi, kappa; the 28 entries of their cofactor matrix, upper triangle row by row in that
 * order; Omega.
 *
 * jaicov_simil_apply carries the points and the image orientations of every model into the target frame, one thread per item:
 *   point:        X' = T + m R X,  Q' = m^2 R Q R' (cofactors qXX qXY qXZ qYY qYZ qZZ, as jaicov_isect_points returns them);
 *   orientation:  X0' = T + m R X0,  R'_img = R R_img, its angles by the three formulas of the closed start.
 * The dispersion of the seven parameters is not propagated: Q' is the cofactor matrix of the point inside its model, turned and scaled.
 * A model one of whose seven parameters is not finite gives NaN for all of its items.
 */
#ifndef JAICOV_SIMIL_H
#define JAICOV_SIMIL_H

#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-model outcome in status[] */
enum {
    JAICOV_SIMIL_OK = 0,
    JAICOV_SIMIL_NOT_CONVERGED = 1,  /* max_iterations steps in the last round; values are returned                     */
    JAICOV_SIMIL_TOO_FEW_POINTS = 2, /* fewer than 3 used points                                                         */
    JAICOV_SIMIL_SINGULAR = 3,       /* collinear points, a pivot <= sqrt(EPS), m not > 0, a cofactor matrix not positive */
    JAICOV_SIMIL_NOT_FINITE = 4      /* NaN / Inf in the input, in a step or in the result                               */
};

/* start_kind[] */
enum { JAICOV_SIMIL_START_GIVEN = 0, JAICOV_SIMIL_START_CLOSED = 1 };

#define JAICOV_SIMIL_OUT_PER_MODEL 36

/* n_models >= 0 models; pt_begin[n_models + 1]: CSR offsets, pt_begin[0] == 0, non-decreasing; src[3 n_pts], dst[3 n_pts];
 * cof_src[6 n_pts] (may be NULL: 0): qXX qXY qXZ qYY qYZ qZZ per point, no diagonal entry negative; cof_dst[6 n_pts] (may be NULL: I):
 * every diagonal entry > 0; start[7 n_models] (may be NULL): Tx Ty Tz m omega phi kappa, used where all seven are finite;
 * max_iterations >= 1 per round; reject_threshold >= 0 and finite (0: no rejection); min_points >= 3.  out[36 n_models],
 * status[n_models]; iterations[n_models] (may be NULL): Gauss-Newton solves over all rounds; start_kind[n_models] (may be NULL);
 * pt_used[n_pts] (may be NULL): 1 / 0 per point; pt_q[n_pts] (may be NULL): q of every point at the returned values, withdrawn
 * ones included; ms_out (may be NULL): kernel time.  Bad arguments are JAICOV_ERR_BAD_ARGUMENT before any device is touched; without
 * a gfx950 device JAICOV_ERR_NO_DEVICE (there is no CPU fallback).  The return code covers the call; the outcome of each model is in
 * status. */
int jaicov_simil_models(int32_t n_models, const int32_t *pt_begin, const double *src, const double *dst, const double *cof_src,
                        const double *cof_dst, const double *start, int32_t max_iterations, double reject_threshold, int32_t min_points,
                        double *out, int32_t *status, int32_t *iterations, int32_t *start_kind, uint8_t *pt_used, double *pt_q,
                        double *ms_out);

/* par[7 n_models]: the first seven values of each model's out.  pt_begin[n_models + 1] (may be NULL: no points) with xyz[3 n_pts] and
 * xyz_out[3 n_pts]; cof[6 n_pts] and cof_out[6 n_pts] are both given or both NULL.  img_begin[n_models + 1] (may be NULL: no
 * orientations) with eo[6 n_img] (X0 Y0 Z0 omega phi kappa) and eo_out[6 n_img].  An output may be its input.  The same return codes. */
int jaicov_simil_apply(int32_t n_models, const double *par, const int32_t *pt_begin, const double *xyz, const double *cof,
                       const int32_t *img_begin, const double *eo, double *xyz_out, double *cof_out, double *eo_out);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_SIMIL_H */
