/*
 * jaicov_forms.h -- C ABI of the forms through adjusted object points: planes, spheres, lines and circles fitted on the device to
 * the current coordinates of their member points, with the members' whole block of the cofactor matrix as the stochastic model.
 *
 * The reference has nothing of the kind.  The model is the Gauss-Helmert model of geodetic adjustment (conditions between
 * observations and unknowns).  Everything here is a read-only consumer of the matrix an inverting solve left on the device
 * (bundle-adjustment_amd/csrc/forms.hip).  Conventions are those of jaicov_precision.h: host pointers, jaicov_status return codes,
 * one engine externally synchronised; every call, refused or not, leaves the engine and the cofactor matrix bit-identical.
 *
 * What is read
 *   The coordinates X_i of the k members of a form: slots 3 p .. 3 p + 2 of point p in the current slot vector on the device.
 *   Q_ll, their 3k x 3k block of the cofactor matrix: entry (i, j) is Q[max(i, j)][min(i, j)] with the leading dimension of the
 *   matrix; a fixed coordinate has no column and counts as a zero row and column (JAICOV_FORM_PARTIAL), as in jaicov_precision.h.
 *   After jaicov_datum_transform the figures speak of the new datum.
 *
 * Refusals, checked in this order
 *   sharded engine                                                       JAICOV_ERR_UNSUPPORTED
 *   no cofactor matrix (no inverting solve since the last accumulate)    JAICOV_ERR_BAD_STATE
 *   a NULL pointer (form_type, form_begin, out, status; form_point with one member or more), n_forms < 0, an unknown form type,
 *   offsets that do not ascend from 0, a point outside [0, n_points), the same point twice in one form, sigma2 <= 0 or NaN,
 *   tol < 0 or NaN, max_iterations < 1                                   JAICOV_ERR_BAD_ARGUMENT
 *   after JAICOV_INVERT_REDUCED a member whose columns are not in the matrix   JAICOV_ERR_BAD_STATE (looked at after the arguments)
 *   (a NULL engine is JAICOV_ERR_BAD_ARGUMENT: there is nothing to ask.)
 *
 * The model, the same for all four forms
 *   c conditions per member, m = c k rows, m <= JAICOV_FORM_MAX_ROWS; u free parameters; f = m - u.
 *   G = (X_0 + X_1 + ... + X_{k-1}) / k in fp64 in member order; x_i = X_i - G; G is a constant.  extent = max |x_i|.
 *   All work is done on the x_i; the parameters are reported in the engine's frame.
 *
 *     form    reported (np)              free (u)                       c  conditions on xh = x + v                   least k
 *     plane   n, d            (4)        a, b, dd                (3)    1  n.xh - d_c = 0                             3
 *     sphere  c, r            (4)        dc (3), dr              (4)    1  |xh - c| - r = 0                           4
 *     line    x0, t           (6)        a0, b0, a, b            (4)    2  e1.(xh - x0) = 0, e2.(xh - x0) = 0         2
 *     circle  c, n, r         (7)        dc (3), a, b, dr        (6)    2  n.(xh - c) = 0, |xh - c| - r = 0           3
 *
 *   Tangent basis of a unit vector n (or t): e1 = (e_k x n) / |e_k x n| with k the index of the smallest |n_k| (the first among
 *   equals), e2 = n x e1.  A unit vector is updated as n <- (n + a e1 + b e2) / |n + a e1 + b e2|.  The line's foot point moves by
 *   a0 e1 + b0 e2 and is then brought back to the point of the line nearest G: x0 <- x0 - (t.x0) t with the new t.
 *   Rows of one member at (parameters, v), with dx = xh - c (or xh - x0), rho = |dx|, g = dx / rho, s = t.dx:
 *     plane   B = n;        A = [e1.xh, e2.xh, -1];                     f = n.xh - d_c
 *     sphere  B = g;        A = [-g, -1];                                f = rho - r
 *     line    B = e1, e2;   A = [-1, 0, -s, 0], [0, -1, 0, -s];          f = e1.dx, e2.dx
 *     circle  B = n, g;     A = [-n, e1.dx, e2.dx, 0], [-g, 0, 0, -1];   f = n.dx, rho - r
 *
 * Start values.  S = sum x_i x_i' (member order), its eigenvalues l0 >= l1 >= l2 and eigenvectors by cyclic Jacobi sweeps.
 *   plane, circle: n = the eigenvector of l2; l1 <= 1e-12 l0: DEGENERATE.  plane: d_c = 0.
 *   line: t = the eigenvector of l0, x0 = 0; l0 <= 0: DEGENERATE.
 *   sphere: |x|^2 - 2 c.x + q = 0 in (c, q) through its 4 x 4 normal equations, r = sqrt(|c|^2 - q).
 *   circle: the same in the coordinates (e1.x, e2.x) of the start plane (3 x 3), c = c1 e1 + c2 e2.
 *   Normal equations without a Cholesky factor (the solve below) or r^2 <= 0: DEGENERATE.
 *
 * One step at (parameters, v), v = 0 at the start
 *   w = f - B v (member by member).  M = B Q_ll B' (m x m): entry (r, s) of the members (i, j) is sum_a B_r[a] (sum_b Q_ij[a][b]
 *   B_s[b]), a and b ascending.  M is scaled as jaicov_par_tests scales Q_gg: W_r = 2^-floor(e_r / 2) with M_rr = m 2^e_r,
 *   1 <= m < 2, if M_rr > 0 and finite, else 1; then V_r = 1 / sqrt(a_rr) of the scaled diagonal if a_rr > 2^-53, else 1;
 *   U'U = (M_rs (W_r W_s)) (V_r V_s), S_r = W_r V_r:
 *     for j = 0 .. m-1: p = U_jj - sum_{r<j} U_rj U_rj (r ascending); p <= 2^-26.5: SINGULAR; U_jj = sqrt(p);
 *                       U_ji = (U_ji - sum_{r<j} U_ri U_rj) / U_jj for i > j.
 *   At = U^-T (S A), wt = U^-T (S w) by forward substitution: z_i = (b_i - sum_{r<i} U_ri z_r) / U_ii (r ascending).
 *   N = At' At, g = At' wt (rows ascending); parameters beyond u get N_aa = 1.  Delta = -N^-1 g by Jacobi scaling and Cholesky
 *   (csrc/wavealg.h, wave_solve); no factor: SINGULAR.  y = At Delta + wt.  Omega = y' y (= lambda' M lambda).
 *   lambda = -S U^-1 y by backward substitution: z_i = (y_i - sum_{r>i} U_ir z_r) / U_ii (r descending).
 *   v_i = sum_j Q_ij beta_j with beta_j = sum_q B_{cj+q} lambda_{cj+q} (j ascending).
 *   (This is N = A' M^-1 A, Delta = -N^-1 A' M^-1 w, lambda = -M^-1 (A Delta + w), v = Q_ll B' lambda.)
 *   The parameters take Delta.  The step count is iterations.  It stops when every position-like component of Delta (dd, dc, dr,
 *   a0, b0) divided by extent and every direction-like one (a, b) is <= tol in magnitude (tol == 0 means 1e-12); after
 *   max_iterations steps without that: NOT_CONVERGED, the last values are returned.
 *
 * Results of a form, out[g][0 .. JAICOV_FORM_COLUMNS)
 *   Sign rule: the component of largest magnitude of n or t is positive (the first among equals); d follows.
 *   [0 .. 7)   the parameters in the order of the table, in the engine's frame: d = d_c + n.G, c + G, x0 + G; NaN behind them
 *   [7 .. 14)  their sigma = sqrt(sigma2 q_pp), q_pp the diagonal of Q_pp; NaN behind them
 *   [14]       Omega     [15] f     [16] T = Omega / (f sigma2), NaN when f = 0 (no quantile is evaluated, as in jaicov_par_tests)
 *   [17], [18] the largest magnitude and the RMS of the orthogonal distances of the uncorrected members to the final form
 *   [19]       iterations
 *   Q_pp = J N^-1 J' of the last step, in the reported (redundant) parameter space, unscaled: qpp[g][0 .. 28) is the upper
 *   triangle of a 7 x 7 matrix row by row, zero outside the np x np part.  J maps the free parameters to the reported ones, with
 *   e1, e2 and x0 of the last step:
 *     plane   n: [e1 e2 0], d: [e1.G, e2.G, 1]          sphere  the unit matrix
 *     line    x0: [e1, e2, -(e1.x0) t, -(e2.x0) t], t: [0, 0, e1, e2]
 *     circle  c: [I 0 0 0], n: [0 e1 e2 0], r: [0 0 0 0 0 1]
 *   and the rows of a vector that the sign rule turned round are negated.
 *
 * Results of a member, member_out[i][0 .. JAICOV_FORM_MEMBER_COLUMNS), parallel to form_point
 *   [0 .. 3)  v_i     [3] the orthogonal distance of X_i to the final form: signed (n.x - d_c, |x - c| - r) where c = 1, the norm
 *   where c = 2 (circle: sqrt((n.dx)^2 + (|dx - (n.dx) n| - r)^2))
 *   [4], [5]  the estimated gross error of its c conditions, nabla_i = -(Q_kk,ii)^-1 lambda_i, with
 *             Q_kk = M^-1 - M^-1 A N^-1 A' M^-1 (the cofactors of lambda); [5] is NaN where c = 1.  Where the sign rule turned n
 *             or t round, the first component is negated with it.  The line's components refer to e1, e2 of the last step.
 *   [6]       T_i = lambda_i' (Q_kk,ii)^-1 lambda_i / (c sigma2)
 *   From the factor: Z = U^-1, (M^-1)_rs = S_r S_s sum_k Z_rk Z_sk, h_r = sum_k Z_rk At_k (k ascending),
 *   (Q_kk)_rs = S_r S_s (sum_k Z_rk Z_sk - h_r' N^-1 h_s).  With f = 0, or a block that is singular -- c = 1: q <= 1e-12 (M^-1)_rr;
 *   c = 2: q_11 <= 1e-12 (M^-1)_11 or q_22 - q_12^2 / q_11 <= 1e-12 (M^-1)_22 -- nabla_i and T_i are NaN and the member gets
 *   JAICOV_FORM_MEMBER_UNTESTED.
 *
 * With TOO_SMALL, TOO_LARGE, DEGENERATE, SINGULAR or NOT_FINITE every figure of the form and of its members is NaN, out[19] (the
 * steps begun) excepted, and qpp is NaN.
 *
 * Determinism.  Every sum has a fixed order that does not depend on the lane that forms it: two runs give the same bits.
 */
#ifndef JAICOV_FORMS_H
#define JAICOV_FORMS_H

#include <stddef.h>
#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define JAICOV_FORM_PLANE 0
#define JAICOV_FORM_SPHERE 1
#define JAICOV_FORM_LINE 2
#define JAICOV_FORM_CIRCLE 3

/* status bits of a form */
#define JAICOV_FORM_PARTIAL 1        /* a member has a fixed coordinate (a zero row and column of Q_ll) */
#define JAICOV_FORM_TOO_SMALL 2      /* fewer members than the form needs */
#define JAICOV_FORM_TOO_LARGE 4      /* more than JAICOV_FORM_MAX_ROWS rows */
#define JAICOV_FORM_DEGENERATE 8     /* members without the spread the start values need */
#define JAICOV_FORM_SINGULAR 16      /* M or N has no Cholesky factor (all members fixed, for example) */
#define JAICOV_FORM_NOT_FINITE 32
#define JAICOV_FORM_NOT_CONVERGED 64 /* the last values are returned */
/* status bit of a member */
#define JAICOV_FORM_MEMBER_UNTESTED 1

#define JAICOV_FORM_MAX_ROWS 64
#define JAICOV_FORM_MAX_PARAMS 7
#define JAICOV_FORM_COLUMNS 20
#define JAICOV_FORM_QPP_COLUMNS 28
#define JAICOV_FORM_MEMBER_COLUMNS 7

/* Fits n_forms forms.  Form g has the type form_type[g] and the member points form_point[form_begin[g] .. form_begin[g + 1])
 * (form_begin: n_forms + 1 ascending offsets from 0).  out [n_forms][20], status [n_forms]; qpp [n_forms][28], member_out
 * [n_members][7] and member_status [n_members] may each be NULL.  ms_out (may be NULL): the time of the kernel in milliseconds,
 * by events on the engine's stream.  One wave and one workgroup per form; an empty form is TOO_SMALL. */
int jaicov_form_fit(jaicov_engine *e, double sigma2, int32_t n_forms, const int32_t *form_type, const int32_t *form_begin,
                    const int32_t *form_point, int32_t max_iterations, double tol, double *out, double *qpp, double *member_out,
                    int32_t *status, int32_t *member_status, float *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_FORMS_H */
