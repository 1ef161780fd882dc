/*
 * jaicov_vce.h -- C ABI of the variance component estimation on the device: does the stochastic model of the adjustment fit?
 *
 * Every other analysis (jaicov_reliability.h, jaicov_precision.h, jaicov_parameters.h, ...) takes the dispersions of the problem as
 * given.  This one tests them: the observations are put into groups (the image points of a camera or of an image, the scale bars,
 * the control points, ...), and for every group the call returns the factor by which its a-priori dispersions should be multiplied
 * so that its residuals are as large as their redundancy says they should be.  The reference has no such call; the estimate is
 * Foerstner's form of the variance components, exact for groups that are unions of weight blocks.  Everything is a read-only
 * consumer of what an inverting solve and the reliability run leave on the device (bundle-adjustment_amd/csrc/vce.hip): the dense
 * weight matrices are read where they are, only the table leaves the device.  Conventions are those of jaicov_neq.h: host pointers,
 * jaicov_status return codes, one engine externally synchronised.
 *
 * Semantics
 *   Rows, weights, residuals, redundancy numbers.  Those of jaicov_reliability.h: P = sigma0^2 inv(D) with sigma0^2 the a-priori
 *   variance factor of the build whose system the cofactor matrix inverts, v = A dx - w, r = diag(Q_vv P).
 *   Weight blocks.  P is block diagonal.  A weight block is the 2 x 2 of an ordinary image point, the dense 2m x 2m of an image block,
 *   the scalar of a scale bar, or the diagonal or dense block of a directly observed group.
 *   Groups.  A group g is a union of weight blocks, named by the caller: ip_group[k] for image point k in the caller's order,
 *   sb_group[s] for scale bar s, dg_group[j] for directly observed group j.  A value is -1 (in no group) or 0 .. n_groups - 1.  All
 *   image points of one dense image block must name the same group: a group that cut through a block would need the off-diagonal
 *   part of P between its rows and the others', and the estimate below would not be exact.
 *   Per group.
 *     n_g      the number of rows of the group
 *     Omega_g  sum over the blocks b of g of v_b' P_b v_b
 *     r_g      sum over the rows i of g of r_i
 *     s2_g     Omega_g / r_g, the a-posteriori variance factor of the group
 *     k_g      s2_g / sigma0^2: multiply the group's dispersions by it
 *     sd(k_g)  k_g sqrt(2 / r_g), the standard deviation of k_g (that of chi^2_r / r, scaled)
 *   Totals.  Omega = sum of Omega_b and sum r over all weight blocks, grouped or not.  sum r = f = n - u + d whenever the build
 *   that Qxx inverts was undamped (jaicov_vce_summary reports the damping).
 *   Status.  JAICOV_VCE_EMPTY: the group has no rows.  Otherwise JAICOV_VCE_NOT_FINITE: Omega_g or r_g is NaN or Inf.  Otherwise
 *   JAICOV_VCE_UNCONTROLLED: r_g <= 1e-10 n_g, the group is not controlled by the others.  With any of the three, s2_g, k_g and
 *   sd(k_g) are NaN; n_g, Omega_g and r_g are what they are.
 *
 * The reliability result.  jaicov_vce_run first performs the run of jaicov_rel_run(e, sigma2_test, dx) through the same internal
 * routine, and therefore leaves a fresh v, qvv, r, t for jaicov_rel_get, as jaicov_rel_run_points does (without a table of the
 * image points).  sigma2_test enters the test values t only, not the components.
 *
 * Refusals, checked in this order; every one comes before the first write, so a refused call leaves the previous results (of this
 * header and of jaicov_reliability.h) in place
 *   NULL engine                                                              JAICOV_ERR_BAD_ARGUMENT
 *   sharded engine                                                           JAICOV_ERR_UNSUPPORTED
 *   not all of Qxx on the device (no inverting solve, or JAICOV_INVERT_REDUCED)
 *                                                                            JAICOV_ERR_BAD_STATE
 *   arguments: sigma2_test not positive and finite; n_groups <= 0; a group id < -1 or >= n_groups; a dense image block whose
 *   image points name different groups (jaicov_neq_last_error names the block)  JAICOV_ERR_BAD_ARGUMENT
 * A run that fails later (out of memory, device error) leaves no result.
 *
 * Determinism.  No atomic additions.  Omega_b and r of a dense block are the sums of one workgroup in a fixed order; a group's
 * figures are a fixed-order sum over its own blocks in ascending row order.  Two runs give the same bits, a group's figures are the
 * same bits whatever the other rows are grouped as, and renaming the groups permutes the table.
 *
 * The environment is not an interface: JAICOV_VCE_STAGE (a test hook, tests/test_gpu_vce.py) lowers the number of residuals of a
 * dense block that the kernel stages at a time, so that small blocks run the path of blocks too large to stage at once.
 *
 * Lifetime.  The result stays on the device with the engine until the next jaicov_vce_run, jaicov_vce_release or jaicov_neq_destroy.
 * A later jaicov_neq_build / jaicov_neq_solve does not touch it.
 */
#ifndef JAICOV_VCE_H
#define JAICOV_VCE_H

#include <stddef.h>
#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status bits of a group */
#define JAICOV_VCE_EMPTY 1          /* no rows */
#define JAICOV_VCE_UNCONTROLLED 2   /* r_g <= 1e-10 n_g */
#define JAICOV_VCE_NOT_FINITE 4     /* NaN / Inf in Omega_g or r_g */

#define JAICOV_VCE_COLUMNS 6

/* ip_group[n_image_points], sb_group[n_scale_bars], dg_group[n_direct_groups]: the group of every weight block (see above); a NULL
 * array puts all of its kind into no group.  dx: NULL (a zero step) or U doubles.  *n_rows (may be NULL) receives the number of
 * observation rows. */
int jaicov_vce_run(jaicov_engine *e, double sigma2_test, const double *dx, const int32_t *ip_group, const int32_t *sb_group,
                   const int32_t *dg_group, int32_t n_groups, int32_t *n_rows);
/* table[JAICOV_VCE_COLUMNS][n_groups]: the rows n_g, Omega_g, r_g, s2_g, k_g, sd(k_g); status[n_groups]: JAICOV_VCE_* bits.
 * n_groups must equal that of the last run.  Either pointer may be NULL. */
int jaicov_vce_get(jaicov_engine *e, double *table, int32_t *status, int32_t n_groups);
/* out[n], n = 5: [0] Omega over all rows  [1] sum r over all rows  [2] rows in a group  [3] rows in no group  [4] the damping value
 * of the build whose system the cofactor matrix inverts: sum r = f needs 0. */
int jaicov_vce_summary(jaicov_engine *e, double *out, int32_t n);
/* Frees the result (idempotent). */
int jaicov_vce_release(jaicov_engine *e);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_VCE_H */
