/*
 * jaicov_datum.h -- C ABI of the device-side datum transformation (Baarda's S-transformation) of the cofactor matrix.
 *
 * In a free network (rank defect d > 0) the datum is the set of object points whose inner constraints fix the frame
 * (BundleAdjustment.java:493-635, BA below).  The datum changes Qxx and every point and station sigma; it changes neither the
 * residuals, the redundancy numbers, the test values nor the interior orientation and distortion.  The reference has no way to
 * re-express Qxx in another datum but a second adjustment with other datum flags; here the cofactor matrix that an inverting
 * solve left on the device is transformed in place (bundle-adjustment_amd/csrc/datum.hip).  Conventions are those of
 * jaicov_neq.h: host pointers, jaicov_status return codes, one engine externally synchronised.
 *
 * Semantics
 *   Null space.  The inverse of the bordered system [[0, B], [B', N]] that the engine holds has the unknowns x border block
 *   G^ = G (B G)^-1, where N G = 0 and B G is regular (G: the similarity null space of the free network, EO angles included).
 *   It is read from the cofactor matrix itself: no Jacobian of the similarity transformation is formed.
 *   New datum rows.  B' is built by the engine's own rule (BA:493-635: the same defect flags, the centroid of the datum points,
 *   the row normalisation) for the mask `point_datum` (the meaning of jaicov_problem_desc.point_datum) at the slot values of
 *   the inverting solve that produced the cofactor matrix (the engine records them; a later jaicov_neq_update does not move
 *   them).  B' touches point columns only.
 *   Transformation.  C = (B' G^)^-1 (d x d), Z = G^ C, S = I - Z B'.  On the unknowns block
 *     Q' = S Q S' = Q - Z Y~' - Y~ Z',   Y = Q B'',  W = B' Y,  Y~ = Y - Z W / 2,
 *   the unknowns x border block becomes Z and the border x border block 0 (its exact value).  Since B' touches point columns
 *   only, the same formula holds for the reduced cofactor matrix of JAICOV_INVERT_REDUCED (order jaicov_neq_cofactor_order()).
 *   Afterwards every consumer of the cofactor matrix sees the new datum: jaicov_neq_get_cofactor, _get_cofactor_sub,
 *   _get_dispersion_sub, the result writers and jaicov_xform_run.  A later inverting solve gives the adjustment's own datum
 *   (jaicov_problem_desc.point_datum) again.
 *
 * Determinism.  Y is one fixed-order sum per entry, the update an elementwise formula: two runs give the same bits.
 */
#ifndef JAICOV_DATUM_H
#define JAICOV_DATUM_H

#include <stddef.h>
#include <stdint.h>

#include "jaicov_neq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Replaces the engine's cofactor matrix, in place, by the one of the datum given by point_datum (n_points entries, nonzero = datum
 * point).  The defect flags stay the engine's.  Status, checked in this order:
 *   rank defect d == 0, or a sharded engine (image_begin / image_end, or apply_shared == 0)  JAICOV_ERR_UNSUPPORTED
 *   no cofactor matrix (no inverting solve since the last accumulate)                       JAICOV_ERR_BAD_STATE
 *   n_points != the problem's, point_datum NULL, or fewer than 3 datum points with free X, Y, Z (BA:515-516)
 *                                                                                            JAICOV_ERR_BAD_ARGUMENT
 *   B' G^ singular (e.g. collinear datum points)                                             JAICOV_ERR_SINGULAR
 * Every one of these leaves the cofactor matrix bit-identical. */
int jaicov_datum_transform(jaicov_engine *e, const uint8_t *point_datum, int32_t n_points);
/* out = S v with the S of the last jaicov_datum_transform; n = jaicov_neq_cofactor_order().  The border entries (0 .. d-1) of out
 * are 0, those of v are not read.  Brings a coordinate difference or a step into the same datum (deformation analysis).  Without a
 * transform since the last inverting solve: JAICOV_ERR_BAD_STATE.  v and out may be the same array. */
int jaicov_datum_apply(jaicov_engine *e, const double *v, double *out, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* JAICOV_DATUM_H */
