/*
 * jaicov_parameters.h -- C ABI of the correlations and significance tests of the unknowns, read from the cofactor matrix on the
 * device: the worst-correlated partner of every column, the list of all pairs above a threshold, rectangular blocks of correlation
 * coefficients, and the test of the linear hypothesis x_g = x0_g on groups of parameters.
 *
 * The reference has nothing of the kind.  The definitions are the standard ones of geodetic adjustment: the third-party report
 * bundled with the tests prints a `Korrelation` matrix of the interior orientation, one `Korrelationen` table (exterior against
 * interior orientation) per image, and `fest` for the parameters it found not worth estimating.  Everything here is a read-only
 * consumer of the matrix an inverting solve left on the device (bundle-adjustment_amd/csrc/parameters.hip).  Conventions are those
 * of jaicov_precision.h: host pointers, jaicov_status return codes, one engine externally synchronised; every call, refused or not,
 * leaves the engine and the cofactor matrix bit-identical.
 *
 * What is read
 *   The cofactor matrix as the other consumers read it: lower part valid, order = jaicov_neq_cofactor_order(), border rows
 *   0 .. d-1, after JAICOV_INVERT_FULL, _FULL_EXPANDED or _REDUCED; after jaicov_datum_transform the figures speak of the new
 *   datum.  The columns that take part are [d, order); border rows and columns never do.  Entry (i, j) is Q[max(i, j)][min(i, j)].
 *
 * Refusals common to all four calls, checked in this order
 *   sharded engine (image_begin / image_end, or apply_shared == 0)      JAICOV_ERR_UNSUPPORTED
 *   no cofactor matrix (no inverting solve since the last accumulate)   JAICOV_ERR_BAD_STATE
 *   NULL or out-of-range arguments                                      JAICOV_ERR_BAD_ARGUMENT
 *   (a NULL engine is JAICOV_ERR_BAD_ARGUMENT: there is nothing to ask.)
 *   After JAICOV_INVERT_REDUCED a slot whose column is not in the matrix is JAICOV_ERR_BAD_STATE (jaicov_par_tests), as in
 *   jaicov_prec_points; it is looked at after the arguments.
 *
 * Scale and coefficient
 *   s_j = 1.0 / sqrt(q_jj) with q_jj = Q[j][j].  For i > j: rho_ij = (Q[i][j] * s_i) * s_j, two products rounded in this order
 *   (there are no sums, so contraction cannot change it).  rho_ji = rho_ij.  It is not clamped to [-1, 1].
 *
 * Bad columns
 *   A column whose q_jj is not finite (JAICOV_PAR_NOT_FINITE) or is <= 0 (JAICOV_PAR_NONPOSITIVE) is no partner of anything and has
 *   no partner: its own figures are NaN / -1.  An off-diagonal entry Q[i][j], d <= j < i < order, that is not finite is no candidate
 *   and no pair; in jaicov_par_maxima it sets JAICOV_PAR_NOT_FINITE on both of its columns, whatever the mask and the flags say.
 *
 * Class and item of a column, from the slot layout of jaicov_neq.h [3 n_points | 3 n_cameras | n_dist | 6 n_images]
 *   class 0 = object coordinate, 1 = interior orientation (x0, y0, c), 2 = distortion coefficient, 3 = exterior orientation.
 *   pair_mask (16 bits): bit 4 a + b set means that a column of class a considers partners of class b.  It need not be symmetric:
 *   "for every interior and distortion parameter its worst partner among the exterior orientations" is bits 4*1+3 and 4*2+3.
 *   Other bits of pair_mask are JAICOV_ERR_BAD_ARGUMENT.
 *   flags: JAICOV_PAR_SKIP_SAME_POINT -- two coordinates of one object point are no pair; JAICOV_PAR_SKIP_SAME_IMAGE -- two elements
 *   of one image's exterior orientation are no pair.  (Without them the worst partner of an X is almost always the Y or Z of the
 *   same point.)  Other bits are JAICOV_ERR_BAD_ARGUMENT.
 *
 * Determinism.  Every coefficient is one fixed-order formula, the maxima are reduced in a fixed order with the tie rule below, the
 * pair list is sorted on the host, every sum of the group tests has a fixed order: two runs give the same bits.
 */
#ifndef JAICOV_PARAMETERS_H
#define JAICOV_PARAMETERS_H

#include <stddef.h>
#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status bits of a column (maxima) or of a group (tests) */
#define JAICOV_PAR_NONPOSITIVE 1  /* column: q_jj <= 0 */
#define JAICOV_PAR_NOT_FINITE 2   /* column: q_jj or an off-diagonal entry of the column is not finite; group: a gathered entry, a
                                     value, x0 or sigma2 q_jj is not finite (figures NaN) */
#define JAICOV_PAR_PARTIAL 4      /* group: a fixed member (no column) was skipped */
#define JAICOV_PAR_EMPTY 8        /* group: no free member, figures NaN */
#define JAICOV_PAR_TOO_LARGE 16   /* group: more than JAICOV_PAR_MAX_GROUP free members, figures NaN */
#define JAICOV_PAR_SINGULAR 32    /* group: Q_gg has no Cholesky factor (a group that spans the datum defect), figures NaN */

#define JAICOV_PAR_SKIP_SAME_POINT 1
#define JAICOV_PAR_SKIP_SAME_IMAGE 2

#define JAICOV_PAR_CLASS_POINT 0
#define JAICOV_PAR_CLASS_INTERIOR 1
#define JAICOV_PAR_CLASS_DISTORTION 2
#define JAICOV_PAR_CLASS_EXTERIOR 3

#define JAICOV_PAR_MAX_GROUP 64
#define JAICOV_PAR_TEST_COLUMNS 4

/* The worst partner of every column.  n == order.  For every good column j in [d, order): among the columns k != j in [d, order)
 * that are good, whose entry with j is finite, whose class the mask admits (bit 4 class(j) + class(k)) and that the flags do not
 * exclude, the one of largest |rho_jk|; among equal values the lowest k.  rho[j] is that coefficient with its sign, partner[j] = k.
 * Without a candidate rho[j] is NaN and partner[j] is -1.  status[j]: JAICOV_PAR_NONPOSITIVE / _NOT_FINITE.  Entries j < d are
 * NaN / -1 / 0.
 * One pass over the lower triangle: every 128 x 128 tile is read once and serves its rows and, transposed, its columns; the
 * candidates of the tiles are reduced in ascending order of the partners' tile with a strict `>`.
 * JAICOV_ERR_BAD_ARGUMENT: a NULL output, n != order, bits of pair_mask above 15 or unknown flags. */
int jaicov_par_maxima(jaicov_engine *e, uint32_t pair_mask, uint32_t flags, double *rho, int32_t *partner, int32_t *status, int32_t n);

/* Every pair i > j of good columns in [d, order) with a finite entry, |rho_ij| >= threshold, not excluded by the flags and admitted
 * by the mask in either direction (bit 4 class(i) + class(j) or bit 4 class(j) + class(i)).  *count is always the exact number.
 * *count <= capacity: cols[2 m], cols[2 m + 1] = i, j and rho[m] = rho_ij of pair m, sorted by |rho| descending, then i ascending,
 * then j ascending.  *count > capacity: nothing is written to cols and rho, the return value is JAICOV_OK; the caller raises the
 * threshold or the capacity.
 * JAICOV_ERR_BAD_ARGUMENT: count NULL, cols or rho NULL with capacity > 0, capacity < 0, threshold outside (0, 1] or NaN, bad
 * pair_mask or flags. */
int jaicov_par_pairs(jaicov_engine *e, uint32_t pair_mask, uint32_t flags, double threshold, int64_t capacity, int32_t *cols, double *rho,
                     int64_t *count);

/* The rectangular block of correlation coefficients between two lists of columns: out[a n_c + b] = rho of (row_cols[a],
 * col_cols[b]) by the formula above with the larger column as i; exactly 1.0 where both are the same good column; NaN where one
 * of the two is a bad column.  With the 6 n_images columns of the exterior orientations as rows and the columns of one camera's
 * interior orientation and distortion as columns this is the whole `Korrelationen` section of the report in one call.
 * JAICOV_ERR_BAD_ARGUMENT: a NULL pointer, n_r < 1, n_c < 1, a column outside [d, order). */
int jaicov_par_block(jaicov_engine *e, const int32_t *row_cols, int32_t n_r, const int32_t *col_cols, int32_t n_c, double *out);

/* Test of the linear hypothesis x_g = x0_g on n_groups groups of parameters.  Group g has the slots
 * group_slot[group_begin[g] .. group_begin[g + 1]) (group_begin: n_groups + 1 ascending offsets, group_begin[0] == 0); x0 runs
 * parallel to group_slot, x0 == NULL means zeros.  Fixed members are skipped (JAICOV_PAR_PARTIAL); k = the number of free members.
 * delta_i = value_i - x0_i with the values of the current slot vector on the device.  Q_gg = the members' block of the cofactor
 * matrix.  q = delta' inv(Q_gg) delta from Q_gg y = delta, solved with Jacobi scaling and Cholesky in fp64, every product and sum
 * rounded on its own.  Powers of two first bring the diagonal into [1, 4), whatever its magnitude and without rounding (the cofactor
 * of a distortion coefficient lies far below the 2^-53 under which the solve below leaves a row unscaled and then finds its pivot
 * too small):
 *   W_i = 2^-floor(e_i / 2) with q_ii = m 2^e_i, 1 <= m < 2, if q_ii > 0 and finite, else 1;  A_ij = Q_gg,ij (W_i W_j), j >= i;
 *   b_i = W_i delta_i.
 * A z = b is solved as the start-value kernels solve their normal equations (csrc/wavealg.h, wave_solve_lds):
 *   V_i = 1 / sqrt(a_ii) if a_ii > 2^-53, else 1;  U_ij = A_ij (V_i V_j), j >= i;
 *   for j = 0 .. k-1: p = U_jj - sum_{r<j} U_rj U_rj (r ascending); p <= 2^-26.5: SINGULAR; U_jj = sqrt(p);
 *                     U_ji = (U_ji - sum_{r<j} U_ri U_rj) / U_jj for i > j;
 *   forward z_i = (V_i b_i - sum_{r<i} U_ri z_r) / U_ii, backward z_i = (z_i - sum_{r>i} U_ir z_r) / U_ii (r ascending),
 *   z_i = V_i z_i;  q = sum_i delta_i (W_i z_i) (i ascending).
 * out[g][0 .. 3] = q, T = q / (k sigma2), k, t; t = delta / sqrt(sigma2 q_jj) is the signed value of a single parameter when
 * k == 1 and NaN otherwise (then T == t^2 up to rounding).  No quantile is evaluated: the caller compares T with F(k, f), or k T
 * with chi^2(k) when sigma2 is the a-priori factor.  status[g]: JAICOV_PAR_PARTIAL, _EMPTY (k == 0), _TOO_LARGE (k > 64),
 * _SINGULAR, _NOT_FINITE; with any of the last four q, T and t are NaN, out[g][2] is k all the same.
 * The difference of two epochs is tested properly with the sum of both epochs' cofactor blocks; this call knows one matrix and
 * treats x0 as free of error.
 * JAICOV_ERR_BAD_ARGUMENT: a NULL pointer (x0 excepted), n_groups < 0, offsets that do not ascend from 0, sigma2 <= 0 or NaN, a
 * slot outside [0, jaicov_neq_num_slots()).  JAICOV_ERR_BAD_STATE: after JAICOV_INVERT_REDUCED a member whose column is not in the
 * matrix. */
int jaicov_par_tests(jaicov_engine *e, double sigma2, const int32_t *group_begin, const int32_t *group_slot, const double *x0,
                     int32_t n_groups, double *out, int32_t *status);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_PARAMETERS_H */
