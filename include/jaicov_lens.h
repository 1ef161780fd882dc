/*
 * jaicov_lens.h -- C ABI of the lens-distortion correction of image points on the device: the measured image coordinates of many
 * points are reduced to those of the distortion-free pinhole camera (jaicov_lens_correct), their 2 x 2 dispersion is propagated, and
 * the inverse applies the camera's distortion model to ideal coordinates (jaicov_lens_distort), for simulation and for checking.
 *
 * It is the classical step in front of the start-value calls: jaicov_dlt_adjust, jaicov_isect_points, jaicov_resect_images and
 * jaicov_relorient_pairs take x0, y0, c of a calibrated camera and model no distortion.  The corrected coordinates and the (var_x,
 * var_y, rho) triplets have exactly the format those calls take.  Both calls are stand-alone, with no engine, like
 * jaicov_simil_models; every point is worked by one lane of one kernel launch (bundle-adjustment_amd/csrc/lens.hip).
 *
 * Model (the reference's; ASF = AffinityShearDistortionModelFactory.java, TDF = TangentialDistortionModelFactory.java,
 * RSF = RadiallySymmetricDistortionModelFactory.java, RDF = RadialDistanceDistortionModelFactory.java, ZDF =
 * ZernikeDistortionModelFactory.java, DMF = DistortionModelFactory.java, PDF = derivation/PartialDerivativeFactory.java):
 *     x = x0 + xs + sum dX(xs, ys, N),   y = y0 + ys + sum dY(xs, ys, N)
 *   with (xs, ys) the ideal coordinates relative to the principal point and every term evaluated at them.  The terms of a camera are
 *   its coefficients cam_dist_begin[cam] .. cam_dist_begin[cam + 1] - 1 of the tables dist_kind / dist_order / dist_value (the kinds
 *   are jaicov_dist_kind of jaicov_neq.h), summed in DistortionModel.Type order (PDF:417-442), as the adjustment's rows kernel
 *   applies them.  With r2 = xs^2 + ys^2, r02 = r0^2 and e the order of a coefficient:
 *     affinity and shear (ASF:37-81), only where Cx and Cy are both present:  dX = Cx xs + Cy ys, dY = 0;
 *     tangential (TDF:39-134), only where Bx and By are both present:  tX = Bx (r2 + 2 xs^2) + By 2 xs ys, tY = By (r2 + 2 ys^2) +
 *       Bx 2 xs ys, and (tX, tY) Bi r2^e more for every Bi of the camera;
 *     radial (RSF:39-90):  (xs, ys) Ai (r2^e - r02^e) for every Ai;
 *     distance-dependent (RDF:39-161):  (xs, ys) Di (r2^e - r02^e) / N for every Di, N the signed depth of PDF:151;
 *     Zernike X, Y, then Gradient (ZDF:153-227, ZDF:41-143), literally, the integer division of the radial exponents included
 *       (jaicov_neq.h, ZDF:107,176,178): n = ceil((-3 + sqrt(9 + 8 e)) / 2), m = 2 e - n (n + 2), and the sum over k = 0 .. (n - |m|) / 2
 *       of the terms with radial exponent p = n - 2 k on rn2 = r2 / r02 and azimuth phi = atan2(ys, xs).
 *   J = I + d(sum dX, sum dY) / d(xs, ys) is made of the six chain-rule factors the adjustment uses (dXxs, dXys, dYxs, dYys of DMF:33-101
 *   as every factory hands them over).  For Zernike X and Y coefficients of odd radial order n the integer division makes these
 *   factors something else than the derivatives of the value; they are kept as they are, since they are what the adjustment works
 *   with.  The Newton iteration of jaicov_lens_correct is then a quasi-Newton iteration with linear convergence; J is still what goes
 *   out.  (The factors of the Gradient kind are the derivatives of its value at every order.)
 *   At most JAICOV_MAX_DIST_PER_CAMERA coefficients per camera.  A Zernike order is at most JAICOV_LENS_MAX_ZERNIKE_ORDER (radial order
 *   n <= 36): up to there the products of binomials of every term (each below 3^n) are exact in 64-bit integers.
 *
 * Depth.  depth[k] is N of point k, as the engine forms it (PDF:151).  Only Di needs it.  depth == NULL while a camera that a point
 *   refers to has a Di coefficient is JAICOV_ERR_BAD_ARGUMENT: a caller who knows no object space strips the Di entries from the
 *   tables.  A depth that is 0 or not finite on a point whose camera has Di ends the point JAICOV_LENS_NOT_FINITE; where the camera has
 *   none, depth is not read.
 *
 * jaicov_lens_correct, per point k with camera cam = pt_camera[k]:
 *   Start at xs = x - x0, ys = y - y0.  At every iterate the model is evaluated: NaN or Inf in the terms or in J ends the point
 *   JAICOV_LENS_NOT_FINITE; det J <= sqrt(EPS), EPS = 2^-53, ends it JAICOV_LENS_SINGULAR (the mapping folds).  A step forms
 *   f = ((x - x0) - xs - sum dX, (y - y0) - ys - sum dY), solves J d = f by the 2 x 2 adjugate and adds d.  The point has converged when
 *   max |d| <= tol max(1, |xs|, |ys|) for the step just applied, (xs, ys) the new values; tol = tolerance, 0 selects sqrt(EPS).
 *   max_iterations steps without convergence: JAICOV_LENS_NOT_CONVERGED, the values are returned all the same.  The model is
 *   evaluated once more at the returned values, with the same two checks; J is that evaluation's.
 *   Output: xy_out = (x0 + xs, y0 + ys), again an image coordinate of the same camera; var_out = the triplet of Q' = J^-1 Q J^-T with
 *   Q = [var_x, rho sqrt(var_x var_y); ., var_y] (var == NULL: Q = I); jac_out = J row by row; iterations = the number of steps.
 *
 * jaicov_lens_distort, per point: one evaluation at xs = x - x0, ys = y - y0 with the same two checks; xy_out = (x0 + xs + sum dX,
 *   y0 + ys + sum dY), Q' = J Q J', J.
 *
 * JAICOV_LENS_SINGULAR and JAICOV_LENS_NOT_FINITE give NaN in all outputs of the point (iterations keeps its count).  A point's result
 * never depends on what else is in the batch, nor on the order of the batch: two runs give the same bits.
 *
 * Not modelled: the dispersion of the camera's own parameters in Q', and joint dispersions of several image points.
 */
#ifndef JAICOV_LENS_H
#define JAICOV_LENS_H

#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-point outcome in status[] */
enum {
    JAICOV_LENS_OK = 0,
    JAICOV_LENS_NOT_CONVERGED = 1, /* max_iterations steps; values are returned                 */
    JAICOV_LENS_SINGULAR = 2,      /* det J <= sqrt(EPS) at an iterate: the mapping folds       */
    JAICOV_LENS_NOT_FINITE = 3     /* NaN / Inf in the input or at an iterate; a depth of 0     */
};

#define JAICOV_LENS_MAX_ZERNIKE_ORDER 702 /* the last single index of radial order 36 */

/* n_points >= 0 points (0 is a valid call that touches nothing); pt_camera[n_points] in [0, n_cameras); xy[2 n_points] measured x, y;
 * var[3 n_points] (may be NULL: Q = I): var_x > 0, var_y > 0, |rho| < 1; depth[n_points] (may be NULL where no referenced camera has a
 * Di coefficient).  n_cameras >= 0 cameras: cam_io[3 n_cameras] x0, y0, c with c != 0; cam_r0[n_cameras], > 0 where the camera has a
 * radial, distance-dependent or Zernike coefficient; cam_dist_begin[n_cameras + 1]: CSR offsets into dist_kind / dist_order /
 * dist_value, cam_dist_begin[0] == 0, non-decreasing, at most JAICOV_MAX_DIST_PER_CAMERA per camera; kinds in [0, 9]; orders >= 1
 * for Bi, Ai, Di and the Zernike kinds, Zernike orders <= JAICOV_LENS_MAX_ZERNIKE_ORDER.  max_iterations >= 1; tolerance >= 0 (0: sqrt(EPS)).  xy_out[2 n_points], status[n_points];
 * var_out[3 n_points], jac_out[4 n_points], iterations[n_points], ms_out (kernel time) may each be NULL.  An output may be its input.
 * Bad arguments are JAICOV_ERR_BAD_ARGUMENT before any device is touched; without a gfx950 device JAICOV_ERR_NO_DEVICE (there is no CPU
 * fallback).  The return code covers the call; the outcome of each point is in status. */
int jaicov_lens_correct(int32_t n_points, const int32_t *pt_camera, const double *xy, const double *var, const double *depth,
                        int32_t n_cameras, const double *cam_io, const double *cam_r0, const int32_t *cam_dist_begin,
                        const int32_t *dist_kind, const int32_t *dist_order, const double *dist_value, int32_t max_iterations,
                        double tolerance, double *xy_out, double *var_out, double *jac_out, int32_t *status, int32_t *iterations,
                        double *ms_out);

/* the same tables; xy[2 n_points] ideal x, y -> xy_out as measured.  The same return codes. */
int jaicov_lens_distort(int32_t n_points, const int32_t *pt_camera, const double *xy, const double *var, const double *depth,
                        int32_t n_cameras, const double *cam_io, const double *cam_r0, const int32_t *cam_dist_begin,
                        const int32_t *dist_kind, const int32_t *dist_order, const double *dist_value, double *xy_out, double *var_out,
                        double *jac_out, int32_t *status, double *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_LENS_H */
