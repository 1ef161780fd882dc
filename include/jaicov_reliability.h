/*
 * jaicov_reliability.h -- C ABI of the device-side reliability analysis: residuals, redundancy numbers and outlier test values of
 * every observation.
 *
 * The reference computes the residuals in getOmega (BundleAdjustment.java:472-491, BA below) and discards them; the sum of the
 * redundancy numbers per observation is commented out (BA:435-441).  There is no reference semantics to restate: the definitions
 * below are the standard ones of geodetic adjustment, pinned by the bundled third-party report (JAICOV/example/example.htm:
 * "rx, ry", "Testwerte", "Gesamtredundanz").  Everything is formed next to the cofactor matrix Qxx
 * (bundle-adjustment_amd/csrc/reliability.hip); only the four vectors leave the device.  Conventions are those of jaicov_neq.h:
 * host pointers, jaicov_status return codes, one engine externally synchronised.
 *
 * Semantics
 *   Rows.  The reference's observation rows in its order (BA:670-771): image point k gives rows 2k (x) and 2k+1 (y), image-major in
 *   the caller's order of the problem description; then one row per scale bar; then one row per directly observed parameter,
 *   group by group.  n_rows = 2 n_image_points + n_scale_bars + n_direct_rows (BA:1056).
 *   Weights.  P = sigma0^2 inv(D), block diagonal with the blocks the engine assembles with: 2 x 2 (var_x, var_y, rho) per ordinary
 *   image point (PDF:296-319), the dense 2m x 2m of an image block, a scalar per scale bar, diagonal or dense per directly observed
 *   group (DOPG:71-86).  Q_ll = D / sigma0^2, its diagonal taken from the dispersions themselves (the diagonal of a dense block or
 *   group, the variances otherwise).  sigma0^2 is the a-priori variance factor of the build whose system the cofactor matrix
 *   inverts; the engine records it, and that build's damping value, at that build.
 *   Residuals.  v = A dx - w with the A and w of the engine's current parameter values (w = observed - computed, so dx = NULL, a
 *   zero step, gives v = computed - observed, the sign the report prints).  The step of an inverting solve passed before
 *   jaicov_neq_update gives the linearised residuals of that pass.  (BA:465 states this formula; BA:482-484 computes its negative.)
 *   Residual cofactors.  Q_vv = Q_ll - A Qxx A';  qvv_i = (Q_vv)_ii.
 *   Redundancy numbers.  r_i = (Q_vv P)_ii.  Their sum is f = n - u + d (BA:1080-1081) whenever Qxx inverts the undamped system
 *   built from the same A (jaicov_rel_summary reports the damping).  Where P is diagonal or 2 x 2 per point, 0 <= r_i <= 1; inside a
 *   dense block Q_vv P is an oblique projector and a single r_i may leave [0, 1].
 *   Test values.  t_i = (P v)_i / sqrt(sigma2_test (P Q_vv P)_ii): the one-dimensional w-test for correlated observations.  The
 *   a-priori sigma0^2 gives Baarda's w-test, the a-posteriori omega / f Pope's tau (the report's signed "Testwerte").  For an
 *   uncorrelated row it is v_i / sqrt(sigma2_test qvv_i).  An observation with (P Q_vv P)_ii <= 1e-10 P_ii is not controlled by the
 *   others: its t_i is NaN (the report prints "---").
 *   A directly observed FIXED parameter has a zero row of A: r = 1.
 *
 * Image points as a whole.  The joint test of both coordinates of an image point, its estimated gross error and what deleting it would
 * do to Omega and to its object point are in jaicov_reliability_points.h; that run fills the four vectors of this header as well.
 *
 * Determinism.  Every output entry is one fixed-order sum: two runs give the same bits.
 *
 * The environment is not an interface: JAICOV_REL_BATCH (a test hook, tests/test_gpu_reliability.py) caps the images per batch of the
 * dense-block products below what the 1 GB work-buffer bound allows, so that small problems run the multi-batch path.
 *
 * Lifetime.  The result stays on the device with the engine until the next jaicov_rel_run, jaicov_rel_release or jaicov_neq_destroy.
 * A later jaicov_neq_build / jaicov_neq_solve does not touch it.  A run that fails its argument or state checks leaves the previous
 * result in place; a run that fails later (out of memory, device error) leaves no result.
 */
#ifndef JAICOV_RELIABILITY_H
#define JAICOV_RELIABILITY_H

#include <stddef.h>
#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Requires an inverting solve that left all of Qxx: jaicov_neq_solve with JAICOV_INVERT_FULL or JAICOV_INVERT_FULL_EXPANDED
 * (jaicov_neq_cofactor_order() == U), else JAICOV_ERR_BAD_STATE.  A sharded engine (image_begin / image_end, or apply_shared == 0) is
 * JAICOV_ERR_UNSUPPORTED.  sigma2_test must be > 0 (else JAICOV_ERR_BAD_ARGUMENT).  dx: NULL (a zero step) or U doubles.
 * *n_rows (may be NULL) receives the number of observation rows. */
int jaicov_rel_run(jaicov_engine *e, double sigma2_test, const double *dx, int32_t *n_rows);
/* v, qvv, r, t of every row in row order; n must equal n_rows of the last run.  Any pointer may be NULL. */
int jaicov_rel_get(jaicov_engine *e, double *v, double *qvv, double *r, double *t, int32_t n);
/* out[n]: [0] sum of r  [1] max |t| over the controlled rows  [2] its row (the first of equals; -1 without one)  [3] rows with NaN t
 * [4] min r  [5] (n == 6) the damping value of the build whose system the cofactor matrix inverts: sum r = f needs 0.  n is 5 or 6. */
int jaicov_rel_summary(jaicov_engine *e, double *out, int32_t n);
/* Frees the result (idempotent). */
int jaicov_rel_release(jaicov_engine *e);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_RELIABILITY_H */
