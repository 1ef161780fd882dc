/*
 * jaicov_precision.h -- C ABI of the precision figures read from the cofactor matrix on the device: standard deviations, Helmert
 * point errors and confidence ellipsoids of object points and projection centres, standard deviations of lengths between adjusted
 * points, and the principal components (largest eigenpairs) of a principal sub-block of Qxx.
 *
 * The reference prints sigmas only; its hooks for a principal component analysis (EstimationStateType.PRINCIPAL_COMPONENT_ANALYSIS,
 * MathExtension.eig over dspevx, MX:448-494) are never connected to the bundle adjustment.  Everything here is a read-only
 * consumer of the matrix an inverting solve left on the device (bundle-adjustment_amd/csrc/precision.hip).  Conventions are those
 * of jaicov_datum.h: host pointers, jaicov_status return codes, one engine externally synchronised; every refusal leaves the engine
 * and the cofactor matrix bit-identical.
 *
 * What is read
 *   The cofactor matrix as the other consumers read it: lower part valid, order jaicov_neq_cofactor_order(), border rows 0 .. d-1;
 *   after jaicov_datum_transform the figures speak of the new datum.  Entry (i, j) is Q[max(i, j)][min(i, j)].  Columns come from
 *   the engine's slot table; a fixed coordinate has no column and counts as a zero row and column of its block.  Coordinates are
 *   the current slot vector on the device, as in jaicov_xform_run.
 *
 * Refusals common to all four calls, checked in this order
 *   sharded engine (image_begin / image_end, or apply_shared == 0)      JAICOV_ERR_UNSUPPORTED
 *   no cofactor matrix (no inverting solve since the last accumulate)   JAICOV_ERR_BAD_STATE
 *   NULL or out-of-range arguments                                      JAICOV_ERR_BAD_ARGUMENT
 *   (a NULL engine is JAICOV_ERR_BAD_ARGUMENT: there is nothing to ask.)
 *
 * The 3 x 3 eigen-decomposition (points, stations)
 *   C = the gathered block, m = its largest diagonal entry.  m == 0: eigenvalues 0, vectors the unit vectors.  Otherwise cyclic
 *   Jacobi in fp64 on A = C / m with V = I: sweeps of the rotations (p, q) = (0, 1), (0, 2), (1, 2); a rotation is skipped when
 *   |a_pq| <= EPS sqrt(|a_pp a_qq|), EPS = 2^-52; otherwise th = (a_qq - a_pp) / (2 a_pq), t = sign(th) / (|th| + sqrt(th^2 + 1))
 *   (sign(0) = +1), c = 1 / sqrt(t^2 + 1), s = t c; a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, and for the third index r
 *   (a_rp, a_rq) <- (c a_rp - s a_rq, s a_rp + c a_rq); the columns p, q of V likewise.  The iteration stops after a sweep without
 *   a rotation, or after 30 sweeps.  Eigenvalues l_i = m a_ii, sorted descending (equal values keep their order), the columns of V
 *   with them.  Sign rule: the component of largest magnitude of a vector is positive (the first among equals).
 *
 * Determinism.  Every figure is one fixed-order formula per item, every sum of the component iteration has a fixed order: two
 * runs give the same bits.
 */
#ifndef JAICOV_PRECISION_H
#define JAICOV_PRECISION_H

#include <stddef.h>
#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status bits of an item (point, station, pair) */
#define JAICOV_PREC_PARTIAL 1     /* a coordinate without a column (fixed): its row and column of the block are zero */
#define JAICOV_PREC_NEGATIVE 2    /* smallest eigenvalue < -1e-12 trace (rounding noise at a datum point of a free network); for a
                                     length: a negative variance of L or of a coordinate difference (its sigma is 0) */
#define JAICOV_PREC_NOT_FINITE 4  /* a gathered entry, a coordinate or sigma2 is not finite: the item's figures are NaN */
#define JAICOV_PREC_DEGENERATE 8  /* length: L == 0, sigma_L is NaN */

/* columns of one row of `out` */
#define JAICOV_PREC_POINT_COLUMNS 22
#define JAICOV_PREC_STATION_COLUMNS 25
#define JAICOV_PREC_LENGTH_COLUMNS 5

/* Precision of n object points (points[i], distinct or not; points == NULL: every object point in order, n = the problem's number).
 * With C = sigma2 Q3 (Q3 the point's 3 x 3 block) and l_0 >= l_1 >= l_2 the eigenvalues of Q3, out[i][0 .. 21] =
 *    0 ..  2  sigma_X, sigma_Y, sigma_Z = sqrt(sigma2 q_kk)
 *    3        Helmert point error sqrt(sigma2 trace Q3)
 *    4 ..  6  semi-axes a >= b >= c = k3 sqrt(sigma2 max(l_i, 0))
 *    7 .. 15  the unit vectors of a, b, c (three components each)
 *   16, 17    semi-axes A >= B = k2 sqrt(sigma2 max(L, 0)) of the horizontal ellipse from the X-Y block:
 *             L = (q_XX + q_YY) / 2 +- hypot((q_XX - q_YY) / 2, q_XY)
 *   18        direction of A in [0, pi), from +X towards +Y: atan2(2 q_XY, q_XX - q_YY) / 2, plus pi when negative
 *   19 .. 21  l_0, l_1, l_2 as computed (neither clamped nor scaled by sigma2)
 * k3 and k2 are the caller's expansion factors: 1 for the Helmert / standard figures, sqrt(3 F) or sqrt(chi^2) for a confidence
 * region; no quantile function is evaluated here.  status[i]: JAICOV_PREC_* bits.
 * JAICOV_ERR_BAD_ARGUMENT: out or status NULL, n < 0, points == NULL with n != the number of object points, an index outside
 * [0, n_points), sigma2, k3 or k2 negative or NaN.  After JAICOV_INVERT_REDUCED a point whose columns follow the exterior orientations (a point that
 * occurs in scale bars only, BA:724-745) is not in the matrix: JAICOV_ERR_BAD_STATE. */
int jaicov_prec_points(jaicov_engine *e, double sigma2, double k3, double k2, const int32_t *points, int32_t n, double *out, int32_t *status);

/* The same for the projection centres X0, Y0, Z0 of n images (images == NULL: every image), and beside them
 *   22 .. 24  sigma of omega, phi, kappa (0 for a fixed angle)
 * JAICOV_PREC_PARTIAL speaks of X0, Y0, Z0 only.  Needs the columns of the exterior orientations in the matrix (JAICOV_INVERT_FULL
 * or _FULL_EXPANDED): after JAICOV_INVERT_REDUCED JAICOV_ERR_BAD_STATE. */
int jaicov_prec_stations(jaicov_engine *e, double sigma2, double k3, double k2, const int32_t *images, int32_t n, double *out, int32_t *status);

/* Lengths between adjusted object points: pairs[2 i], pairs[2 i + 1] = A, B.  With X_A, X_B from the slot vector on the device,
 * D = X_B - X_A, L = sqrt(D.D), u = D / L, g = [-u, u] and Q6 the 6 x 6 block of (A, B) with its cross-covariances,
 * out[i][0 .. 4] = L, sigma_L = sqrt(sigma2 sum_i g_i (sum_j Q6_ij g_j)), then sigma of D_X, D_Y, D_Z =
 * sqrt(sigma2 (q_AkAk + q_BkBk - 2 q_AkBk)).  This is the one figure that needs the correlations between two points.
 * A pair naming the same point twice, or an index out of range: JAICOV_ERR_BAD_ARGUMENT.  REDUCED: as jaicov_prec_points. */
int jaicov_prec_lengths(jaicov_engine *e, double sigma2, const int32_t *pairs, int32_t n, double *out, int32_t *status);

/* The k <= 4 largest eigenpairs of the principal sub-block S = Q[first_col .. first_col + n_cols) (the weak forms of the network).
 * The range lies inside [d, order) and holds at least 8 columns.  The coordinates of the object points that images observe are
 * numbered first (BA:667-723), so their columns are one leading range of the matrix -- what the Python helper
 * Engine.point_column_range() returns; points that occur in scale bars only are numbered after the exterior orientations
 * (BA:724-745) and lie outside that range.
 *
 * Subspace iteration with a block of 8 vectors and Rayleigh-Ritz.  Start block: X0[i][a] = (z >> 11) 2^-53 - 0.5 for row i of the
 * sub-block and a = 0 .. 7, where z is splitmix64 of the counter c = 8 i + a in 64-bit unsigned arithmetic:
 *   z = (c + 1) 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) 0x94D049BB133111EB;  z = z ^ (z >> 31).
 * X = orth(X0).  Iteration: Y = S X on the device; H = X'Y (8 x 8) goes to the host and is symmetrised, its Jacobi eigen-decomposition
 * gives the Ritz values th_0 >= ... >= th_7 and Z; the residual norms |Y z_a - th_a X z_a| are formed on the device; converged when
 * the first k of them are <= tol th_0 (tol == 0: 1e-10).  Otherwise X = orth(Y).  orth(W): twice G = W'W on the device, its Cholesky
 * factor R'R = G on the host, W <- W R^-1 on the device (CholeskyQR2).  Only 8 x 8 matrices cross the bus per iteration.
 *
 * values[k]: the Ritz values; vectors[k][n_cols]: X z_a at unit norm with the sign rule above; *trace: the sum of the sub-block's
 * diagonal in a fixed order, so values[a] / *trace is the component's share; residuals[k]: the residual norms; *iterations: the
 * number of products Y = S X when converged, minus that number when max_iterations products did not converge
 * (NOT_CONVERGED: values, vectors and residuals are those of the last product, the return value is JAICOV_OK).
 * JAICOV_ERR_BAD_ARGUMENT: a NULL pointer, k outside 1 .. 4, n_cols < 8, a range that enters the border or leaves the order,
 * tol negative or NaN, max_iterations < 1.  JAICOV_ERR_SINGULAR: a Gram matrix without a Cholesky factor (the sub-block has rank < 8,
 * or is not finite). */
int jaicov_prec_components(jaicov_engine *e, int32_t first_col, int32_t n_cols, int32_t k, double tol, int32_t max_iterations,
                           double *values, double *vectors, double *trace, double *residuals, int32_t *iterations);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_PRECISION_H */
