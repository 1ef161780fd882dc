/*
 * jaicov_dlt.h -- C ABI of the batched direct linear transformation (DLT) on the device: start values of the exterior and
 * interior orientation of many images in one call.
 *
 * Replaces DirectLinearTransformation.adjust(coefficients, objectCoordinates, restrictions...) of the reference
 * (JAICOV/src/org/applied_geodesy/adjustment/bundle/dlt/: DT = DirectLinearTransformation.java, DPF =
 * DLTPartialDerivativeFactory.java), which adjusts one image at a time on one thread.  Here every image of the call is adjusted
 * by one wave of one kernel launch (bundle-adjustment_amd/csrc/dlt.hip), the whole Gauss-Newton loop included.  It is a
 * stand-alone call with no engine (as jaicov_dense_spd_solve_packed): start values are needed before an engine means anything.
 * Lens distortion is not modelled; jaicov_lens_correct (jaicov_lens.h) reduces measured image points of a calibrated camera beforehand.
 *
 * Semantics, per image g (observations obs_begin[g] .. obs_begin[g+1]-1, the image's homologous points in the image's order:
 * the caller has already matched the image points with the control points, DT:73-94)
 *   Fewer than 6 observations: JAICOV_DLT_TOO_FEW_POINTS (DT:96-104).
 *   scale = sqrt(sum(X^2+Y^2+Z^2) / sum(x^2+y^2)), or 1 when the image sum is 0 (DT:106); object coordinates enter as X / scale.
 *   Unknowns b11..b14, b21..b24, b31..b33 (columns 0..10, DT:280-303), all starting at 0; x0, y0, c are the image's io values.
 *   Two rows per point (DPF:238-344): A = (X Y Z 1 0 0 0 0 -xX -xY -xZ), (0 0 0 0 X Y Z 1 -yX -yY -yZ), w = (x, y) - model(b),
 *   N += A'A, n += A'w with unit weights, summed in observation order (x row, then y row).
 *   Restrictions (DPF:86-236) are bordered rows 11, 12, ... with zero diagonal, in the caller's order after DT:269-278: a
 *   duplicated id is dropped (first-seen order kept), IDENTICAL_PRINCIPLE_DISTANCE is dropped when both FIXED_PRINCIPLE_DISTANCE_X
 *   and _Y are present.  Duplicates are therefore not an error.  The order of the bordered system is at most 16.
 *   Loop (DT:107-165): the first solve is unrestricted (order 11), every later one includes the restrictions.  Each solve is
 *   Jacobi-preconditioned (V = 1/sqrt(diag) when diag > EPS = 2^-53, else 1; DT:345-348, NES:82-91), factorised by Bunch-Kaufman
 *   (dsptrf, alpha = (1+sqrt(17))/8) and solved (dsptrs) as MathExtension.solve's dspsv (MX:338-366), un-preconditioned, and
 *   b += dx[0..10].  The step is max |dx| over the 11 b's.  runs starts at max_iterations - 1; the image has converged when
 *   max|dx| <= sqrt(EPS) while runs > 0, and `runs-- <= 1` ends it without convergence.  Without restrictions there is exactly one
 *   solve; with restrictions one more solve runs after convergence has been flagged.  This control is reproduced for every
 *   max_iterations >= 0 (0, 1 and 2 report JAICOV_DLT_NOT_CONVERGED even without restrictions, as the reference does).
 *   An exactly zero pivot (block) of dsptrf: JAICOV_DLT_SINGULAR.  NaN or Inf in dx: JAICOV_DLT_NOT_FINITE.
 *   Expansion (DT:185-267): every coefficient except b14, b24 is divided by scale; x0, y0, cx, cy, c = (cx + cy) / 2; R from the
 *   b's, flipped when det R < 0; omega = atan2(-r23, r33), phi = asin(r13), kappa = atan2(-r12, r11); the projection centre solves
 *   F t = (-b14, -b24, -1) by LU with partial pivoting (MTJ DenseMatrix.solve = dgesv).  A zero pivot there (the reference throws
 *   MatrixSingularException out of adjust) is JAICOV_DLT_SINGULAR.
 *
 * Output out[20 g + k]: b11 b12 b13 b14 b21 b22 b23 b24 b31 b32 b33 (expanded), x0, y0, c, X0, Y0, Z0, omega, phi, kappa -- the
 * order of DLTCoefficients.  JAICOV_DLT_NOT_CONVERGED images are expanded as the reference expands them.
 *
 * Reference quirks
 *   Q1  cx, cy are square roots: c > 0 always.  For a camera with c < 0 (the AICON convention) the result is the equivalent
 *       parametrisation (|c|, kappa + pi).  This ABI returns what the reference returns; a host that turns the result into start
 *       values for a camera with c < 0 adds pi to kappa (the C++ mirror's DirectLinearTransformation::applyExteriorOrientation).
 *   Q2  (deliberate deviation) a FIXED x0 / y0 / c is returned as the image's own io value.  The reference divides it by scale
 *       (DT:186-192) and never overwrites it (DT:253-258).
 *   Q3  (deliberate deviation) an image whose status is TOO_FEW_POINTS, SINGULAR or NOT_FINITE gets NaN in all 20 values; the
 *       reference leaves half-updated coefficients.
 */
#ifndef JAICOV_DLT_H
#define JAICOV_DLT_H

#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* DirectLinearTransformation.RestrictionType, DT:51-58 order */
typedef enum {
    JAICOV_DLT_IDENTICAL_PRINCIPLE_DISTANCE = 0,
    JAICOV_DLT_ROTATION_WITHOUT_SHEAR = 1,
    JAICOV_DLT_FIXED_PRINCIPLE_DISTANCE_X = 2,
    JAICOV_DLT_FIXED_PRINCIPLE_DISTANCE_Y = 3,
    JAICOV_DLT_FIXED_PRINCIPAL_POINT_X = 4,
    JAICOV_DLT_FIXED_PRINCIPAL_POINT_Y = 5
} jaicov_dlt_restriction;

/* per-image outcome in status[] */
enum {
    JAICOV_DLT_CONVERGED = 0,        /* adjust() returns true                                   */
    JAICOV_DLT_NOT_CONVERGED = 1,    /* adjust() returns false after expanding (isConverge)     */
    JAICOV_DLT_TOO_FEW_POINTS = 2,   /* fewer than 6 homologous points                          */
    JAICOV_DLT_SINGULAR = 3,         /* dspsv or the projection centre's dgesv hit a zero pivot */
    JAICOV_DLT_NOT_FINITE = 4        /* NaN / Inf in a step                                     */
};

#define JAICOV_DLT_OUT_PER_IMAGE 20

/* n_images >= 0 images; obs_begin[n_images + 1]: CSR offsets, obs_begin[0] == 0, non-decreasing; xy[2 n_obs]: x, y of every
 * observation; xyz[3 n_obs]: X, Y, Z of its control point; io[3 n_images]: x0, y0, c of each image's camera; io_fixed[3 n_images]
 * (may be NULL: all free): nonzero marks x0 / y0 / c as fixed; restrictions[n_restrictions]: jaicov_dlt_restriction ids, in the
 * caller's order (duplicates allowed); max_iterations >= 0 (the reference's default is 5000, DefaultValue:25).
 * out[20 n_images], status[n_images]; solves[n_images] (may be NULL): factorisations run per image; ms_out (may be NULL): kernel time.
 * Bad arguments are JAICOV_ERR_BAD_ARGUMENT before any device is touched; without a device JAICOV_ERR_NO_DEVICE.  The return code
 * covers the call; the outcome of each image is in status. */
int jaicov_dlt_adjust(int32_t n_images, const int32_t *obs_begin, const double *xy, const double *xyz, const double *io,
                      const uint8_t *io_fixed, const int32_t *restrictions, int32_t n_restrictions, int32_t max_iterations,
                      double *out, int32_t *status, int32_t *solves, double *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_DLT_H */
