/*
 * jaicov_calibration.h -- C ABI of the camera calibration in image space: the image correction of a camera at a place on the sensor
 * (the distortion field), how well the adjustment determines it there, and the comparison of two calibrations node by node with a
 * summary formed on the device.
 *
 * The parameters of a camera and their sigmas (jaicov_par_*) do not answer this: c, the A_i and the affinity terms are correlated at
 * 0.9 and above, and single Zernike coefficients have no meaning of their own.  The field is propagated here with the camera's
 * whole cofactor block.  Everything is a read-only consumer of the matrix an inverting solve left on the device
 * (bundle-adjustment_amd/csrc/calibration.hip).  Conventions are those of jaicov_predict.h: host pointers, jaicov_status return
 * codes, one engine externally synchronised; every refusal leaves the outputs, the engine and the cofactor matrix bit-identical.
 *
 * The quantity.  For camera k with its current parameters, a ray with the direction tangents t = (t_x, t_y) in the camera frame and
 * the depth N lands at
 *    g_k(t, N) = (x0 + xs + sum dX(xs, ys, N), y0 + ys + sum dY(xs, ys, N)),   xs = -c t_x, ys = -c t_y,
 * all distortion families included.  The RAY is held fixed, not the ideal image point: the trade-off between c and the A_i cancels
 * in J Q J' and in the difference of two parameter sets.
 *
 * A node is (xs, ys): ideal coordinates relative to the principal point at the camera's CURRENT c, with a depth N (depth == NULL:
 * N = -c, the depth at which the distance-dependent terms D_i are scaled by 1 / -c; refused where a camera of the call has a D_i
 * coefficient, as jaicov_lens.h refuses a missing depth).  Its ray is t = -(xs, ys) / c.
 *
 * The rows.  J and w of a node are computed by the kernel that computes the rows of the adjustment, on a synthetic problem: the node
 * is the object point (-xs N / c, -ys N / c, N) seen by an image of camera k whose six exterior orientation values are zero, and its
 * measurement is (x0 + xs, y0 + ys); -w is then the distortion displacement itself.  The camera's own columns of that row are the
 * local columns 3 .. 5 and 12 .. of jaicov_neq_get_rows:
 *    0 .. 2   x0, y0, c of camera k
 *    3 ..     the distortion coefficients cam_dist_begin[k] .. cam_dist_begin[k + 1] of camera k
 * K_k = 3 + n_dist(k) <= JAICOV_CALIB_MAX_COLUMNS columns.  No column of an exterior orientation is read, so the matrix of the
 * EO-reduced system (JAICOV_INVERT_REDUCED) serves as well as all of Qxx.  A fixed parameter (JAICOV_COL_FIXED) contributes no term.
 *
 * Refusals common to both calls, checked in this order
 *   NULL engine                                                              JAICOV_ERR_BAD_ARGUMENT
 *   sharded engine (image_begin / image_end, or apply_shared == 0)          JAICOV_ERR_UNSUPPORTED
 *   no cofactor matrix on the device (no inverting solve since the last accumulate)   JAICOV_ERR_BAD_STATE
 *   NULL, negative, non-finite or out-of-range arguments                     JAICOV_ERR_BAD_ARGUMENT
 *
 * Determinism.  Every entry of a node is one fixed-order sum over the camera's own columns, ascending: two runs give the same bits,
 * and a node's figures are the same bits whatever else is in the call and wherever it stands in it.  The summary is a fixed tree
 * over the nodes in the caller's order, without atomics: the same bits on every run.
 *
 * Not built: a joint test over all nodes.  The stacked covariance of n nodes has rank <= K_a + K_b, and [J_a, -J_b] is rank
 * deficient by construction (the two x0 columns coincide); the test in parameter space is jaicov_par_tests.
 */
#ifndef JAICOV_CALIBRATION_H
#define JAICOV_CALIBRATION_H

#include <stddef.h>
#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status bits of a node: the meanings of jaicov_predict.h */
#define JAICOV_CALIB_PARTIAL 1     /* a selected column of the camera is fixed: it contributes no term */
#define JAICOV_CALIB_NEGATIVE 2    /* the smaller eigenvalue of C (or C_d) is below -1e-12 times its trace */
#define JAICOV_CALIB_NOT_FINITE 4  /* a gathered entry, a row entry or a factor is not finite: the figures are NaN */
#define JAICOV_CALIB_SINGULAR 16   /* C_d has no positive determinant: q and the T values are NaN */

/* columns of one row of the outputs */
#define JAICOV_CALIB_FIELD_COLUMNS 14
#define JAICOV_CALIB_COMPARE_COLUMNS 8
#define JAICOV_CALIB_SUMMARY_COLUMNS 8
/* the camera's own columns at most: x0, y0, c and JAICOV_MAX_DIST_PER_CAMERA coefficients */
#define JAICOV_CALIB_MAX_COLUMNS 23

/* `columns` of jaicov_calib_field: which of the camera's columns enter the covariance.  Bit 0: x0, y0; bit 1: c; bit 2 + kind:
 * every coefficient of jaicov_dist_kind `kind`. */
#define JAICOV_CALIB_PRINCIPAL_POINT 1
#define JAICOV_CALIB_PRINCIPAL_DISTANCE 2
#define JAICOV_CALIB_KIND_SHIFT 2
#define JAICOV_CALIB_ALL 4095
/* `flags` of jaicov_calib_compare */
#define JAICOV_CALIB_RELATIVE 1    /* positions relative to each side's own principal point: x0, y0 leave d and the columns */

/* The distortion field of n nodes: node i is (xy[2 i], xy[2 i + 1]) of camera cams[i] at the depth depth[i].  Nodes may name
 * different cameras, repeat and come in any order; n == 0 is a valid empty call.  out[i][0 .. 13] =
 *   0, 1     dx, dy: the sum of all families at the node, -w of the rows.  Always the whole model, whatever `columns` selects
 *   2 .. 4   q_xx, q_xy, q_yy of C = J_s Q[s, s] J_s' over the selected columns s (not scaled by sigma2)
 *   5, 6     sigma_x, sigma_y = sqrt(sigma2 max(q, 0))
 *   7, 8     semi-axes A >= B = k2 sqrt(sigma2 max(L, 0)), L = (q_xx + q_yy) / 2 +- hypot((q_xx - q_yy) / 2, q_xy)
 *   9        direction of A in [0, pi), from +x towards +y: atan2(2 q_xy, q_xx - q_yy) / 2, plus pi when negative
 *   10, 11   dr = (xs dx + ys dy) / r, dt = (-ys dx + xs dy) / r: the radial and the tangential component, r = hypot(xs, ys)
 *   12, 13   sigma_dr, sigma_dt = sqrt(sigma2 max(q, 0)) of C rotated by the same angle:
 *            q_rr = (xs^2 q_xx + 2 xs ys q_xy + ys^2 q_yy) / r^2, q_tt = (ys^2 q_xx - 2 xs ys q_xy + xs^2 q_yy) / r^2
 * (7 .. 9 are the formulas of columns 7 .. 9 of jaicov_pred_points.)  At r == 0 columns 10 .. 13 are NaN and nothing else is
 * affected.  jac_out[i][2][JAICOV_CALIB_MAX_COLUMNS], if given, is the camera part of the node's row: x0, y0, c, then the
 * coefficients, zero behind K_k; it is the whole row whatever `columns` selects and whichever parameter is fixed: the design matrix
 * of the calibration in image space.  status[i]: JAICOV_CALIB_PARTIAL, _NEGATIVE, _NOT_FINITE (NaN in out[i]; the centre node of
 * a camera with Zernike terms is one, by m / r^2).
 * JAICOV_ERR_BAD_ARGUMENT: n < 0; with n > 0 a NULL cams, xy, out or status, or a camera outside the problem; sigma2 or k2 negative
 * or NaN; no bit of `columns` within JAICOV_CALIB_ALL, or a bit outside it; with n > 0 depth == NULL where a camera of the call has a
 * D_i coefficient. */
int jaicov_calib_field(jaicov_engine *e, double sigma2, double k2, uint32_t columns, const int32_t *cams, const double *xy, const double *depth,
                       int32_t n, double *out, double *jac_out, int32_t *status);

/* The difference field of two calibrations at n nodes (xy[2 i], xy[2 i + 1]): ideal coordinates at the CURRENT c of camera cam_a
 * of the engine, side A.  Side B is
 *   ref_values == NULL: camera cam_b != cam_a of the same engine (cam_b == cam_a is refused).  With J_a, J_b the two cameras' rows
 *       C_d = J_a Q_aa J_a' - J_a Q_ab J_b' - J_b Q_ba J_a' + J_b Q_bb J_b',
 *     every one of the four terms summed on its own with its indices ascending, then combined from left to right.
 *   ref_values[3 + n_dist(cam_b)] given: the coefficient table of camera cam_b (which may be cam_a) evaluated at these values,
 *     x0, y0, c first: a certificate, or the result of an earlier epoch.  C_d = J_a Q_aa J_a' comes from side A only; with ref_cov
 *     (K_b x K_b row-major, a covariance of ref_values in the units of sigma2 Q, the lower part read) J_b ref_cov J_b' / s0 is added
 *     in cofactor units, s0 the a-priori variance factor the engine recorded for the inverted build.
 * Both sides see the same ray t = -(xs, ys) / c_a, the same depth (depth == NULL: -c_a) and the same measurement
 * (x0_a + xs, y0_a + ys), so d = w_b - w_a = g_a - g_b.  flags & JAICOV_CALIB_RELATIVE: the position of each side is taken relative
 * to its own principal point, d = (w_b - w_a) + ((x0, y0)_b - (x0, y0)_a), and the columns of x0, y0 carry no term: the usual way to
 * compare two calibrations whose principal point was absorbed by the exterior orientations.  (Then the node on the principal point
 * has no column left, C_d = 0, and a camera with radially symmetric terms only has the rows (xs, ys) g(r): C_d has rank 1 at every
 * node, and JAICOV_CALIB_SINGULAR is left to the rounding.)  out[i][0 .. 7] =
 *   0, 1     d_x, d_y
 *   2 .. 4   m_xx, m_xy, m_yy of C_d
 *   5        q = d' C_d^-1 d = (m_yy d_x^2 - 2 m_xy d_x d_y + m_xx d_y^2) / (m_xx m_yy - m_xy^2); without a positive determinant
 *            JAICOV_CALIB_SINGULAR and NaN in 5 .. 7
 *   6        T_prio = q / (2 s0): F(2, inf) under the null hypothesis that both sets describe one camera
 *   7        T_post = q / (2 sigma2_post): F(2, f)
 * (the formulas of jaicov_pred_check; no quantile is evaluated).  status[i]: JAICOV_CALIB_PARTIAL, _NEGATIVE, _NOT_FINITE (NaN in
 * out[i]), _SINGULAR.  summary[0 .. 7], formed on the device by one workgroup (a fixed tree with compensated sums, no atomics) =
 *   0        n_f: the nodes without JAICOV_CALIB_NOT_FINITE
 *   1        rms = sqrt(sum |d|^2 / n_f) over these nodes
 *   2        rms_expected = sqrt(s0 sum tr C_d / n_f): what the difference field should amount to if both sets describe one camera
 *   3, 4     max |d| and its node
 *   5, 6     max T_prio and its node (over the nodes that have one)
 *   7        the nodes with JAICOV_CALIB_SINGULAR
 * Ties go to the smallest index; without a candidate the maximum is NaN and its node -1; with n_f == 0 columns 1 and 2 are NaN.
 * out and status may be NULL when only the summary is wanted (summary may be NULL as well); n == 0 is a valid empty call that
 * writes the summary of no nodes.
 * JAICOV_ERR_BAD_ARGUMENT: n < 0; with n > 0 a NULL xy; a camera outside the problem; ref_values == NULL with cam_b == cam_a, or
 * with ref_cov given; sigma2_post not positive or NaN; a bit of flags other than JAICOV_CALIB_RELATIVE; a ref_values or ref_cov
 * entry that is not finite; with n > 0 depth == NULL where cam_a or cam_b has a D_i coefficient. */
int jaicov_calib_compare(jaicov_engine *e, double sigma2_post, int32_t cam_a, int32_t cam_b, const double *ref_values, const double *ref_cov,
                         uint32_t flags, const double *xy, const double *depth, int32_t n, double *out, int32_t *status, double *summary);

/* Frees the work buffers that the two calls keep with the engine (they grow with n and are reused); the engine frees them with
 * itself otherwise.  JAICOV_ERR_BAD_ARGUMENT: NULL engine. */
int jaicov_calib_release(jaicov_engine *e);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_CALIBRATION_H */
