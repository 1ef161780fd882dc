"""ctypes binding of the C ABI in ``include/jaicov_neq.h`` / ``include/jaicov_dense.h`` / ``include/jaicov_transform.h`` /
``include/jaicov_dlt.h`` / ``include/jaicov_reliability.h`` / ``include/jaicov_reliability_points.h`` /
``include/jaicov_datum.h`` / ``include/jaicov_intersect.h`` / ``include/jaicov_resect.h`` /
``include/jaicov_relorient.h`` / ``include/jaicov_simil.h`` / ``include/jaicov_lens.h`` / ``include/jaicov_precision.h`` /
``include/jaicov_parameters.h`` / ``include/jaicov_forms.h`` / ``include/jaicov_predict.h`` /
``include/jaicov_newpoints.h`` / ``include/jaicov_vce.h`` / ``include/jaicov_calibration.h`` (``csrc/libjaicov_neq.so``).

This is the Python image of the stub a JNI shim would hold.  There is no CPU path: loading fails loudly when the HIP
library has not been built, and every call fails with ``EngineError`` when no gfx950 device is present.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from collections import namedtuple

import numpy as np

from .problem import DIST_DISTANCE_DI, FlatProblem, ProblemDesc

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libjaicov_neq.so")

STATUS = {0: "OK", -1: "BAD_ARGUMENT", -2: "BAD_STATE", -3: "UNSUPPORTED", -4: "OUT_OF_MEMORY", -5: "DEVICE",
          -6: "NO_DEVICE", 1: "SINGULAR", 2: "NOT_FINITE"}

EXPORTS = [
    "jaicov_neq_create", "jaicov_neq_destroy", "jaicov_neq_last_error", "jaicov_neq_abi_version",
    "jaicov_neq_num_slots", "jaicov_neq_packed_length", "jaicov_neq_set_parameters", "jaicov_neq_get_parameters",
    "jaicov_neq_build", "jaicov_neq_accumulate", "jaicov_neq_accumulate2", "jaicov_neq_prepare_inverse", "jaicov_neq_reduced_order", "jaicov_neq_cofactor_order",
    "jaicov_neq_finalize", "jaicov_neq_reduce_buffer", "jaicov_neq_reduce_buffer_async",
    "jaicov_neq_solve", "jaicov_neq_omega", "jaicov_neq_update", "jaicov_neq_get_normal", "jaicov_neq_get_cofactor",
    "jaicov_neq_get_cofactor_sub", "jaicov_neq_get_dispersion_sub", "jaicov_neq_get_rows", "jaicov_neq_estimate", "jaicov_neq_last_timings",
    "jaicov_neq_set_profiling", "jaicov_neq_kernel_stats", "jaicov_neq_cancel",
    "jaicov_dense_spd_solve_packed", "jaicov_dense_gemm", "jaicov_neq_eo_step_buffer",
    "jaicov_neq_create_timings", "jaicov_neq_get_block_weight", "jaicov_neq_expansion_buffer",
]

# include/jaicov_transform.h: CoordinateTransformationExteriorOrientation.transform on the device (its own list: EXPORTS is the
# declarations of jaicov_neq.h + jaicov_dense.h)
XFORM_EXPORTS = [
    "jaicov_xform_run", "jaicov_xform_get_coordinates", "jaicov_xform_get_covariance", "jaicov_xform_get_covariance_sub",
    "jaicov_xform_get_point_blocks", "jaicov_xform_release",
]

# include/jaicov_dlt.h: DirectLinearTransformation.adjust for a batch of images (stand-alone, no engine)
DLT_EXPORTS = ["jaicov_dlt_adjust"]
# include/jaicov_reliability.h: residuals, redundancy numbers and test values of every observation on the device
REL_EXPORTS = ["jaicov_rel_run", "jaicov_rel_get", "jaicov_rel_summary", "jaicov_rel_release"]
# include/jaicov_reliability_points.h: the leave-one-out table of every image point beside them
REL_POINT_EXPORTS = ["jaicov_rel_run_points", "jaicov_rel_get_points"]
# include/jaicov_datum.h: the cofactor matrix re-expressed in another datum (S-transformation) on the device
DATUM_EXPORTS = ["jaicov_datum_transform", "jaicov_datum_apply"]
# include/jaicov_precision.h: confidence ellipsoids, sigmas of lengths and principal components read from the cofactor matrix
PREC_EXPORTS = ["jaicov_prec_points", "jaicov_prec_stations", "jaicov_prec_lengths", "jaicov_prec_components"]
PREC_PARTIAL, PREC_NEGATIVE, PREC_NOT_FINITE, PREC_DEGENERATE = 1, 2, 4, 8     # status bits of a point, station or pair
PREC_POINT_COLUMNS, PREC_STATION_COLUMNS, PREC_LENGTH_COLUMNS = 22, 25, 5
# include/jaicov_parameters.h: correlations and significance tests of the unknowns read from the cofactor matrix
PARAM_EXPORTS = ["jaicov_par_maxima", "jaicov_par_pairs", "jaicov_par_block", "jaicov_par_tests"]
PAR_NONPOSITIVE, PAR_NOT_FINITE, PAR_PARTIAL, PAR_EMPTY, PAR_TOO_LARGE, PAR_SINGULAR = 1, 2, 4, 8, 16, 32   # status bits
PAR_SKIP_SAME_POINT, PAR_SKIP_SAME_IMAGE = 1, 2                                                           # flags
PAR_CLASS_POINT, PAR_CLASS_INTERIOR, PAR_CLASS_DISTORTION, PAR_CLASS_EXTERIOR = range(4)
PAR_CLASS_NAMES = ("point", "interior", "distortion", "exterior")
PAR_MAX_GROUP, PAR_TEST_COLUMNS = 64, 4
PAR_ALL_PAIRS = 0xFFFF
# include/jaicov_forms.h: planes, spheres, lines and circles through adjusted points with the members' whole cofactor block
FORM_EXPORTS = ["jaicov_form_fit"]
FORM_PLANE, FORM_SPHERE, FORM_LINE, FORM_CIRCLE = range(4)
FORM_KINDS = {"plane": FORM_PLANE, "sphere": FORM_SPHERE, "line": FORM_LINE, "circle": FORM_CIRCLE}
FORM_PARTIAL, FORM_TOO_SMALL, FORM_TOO_LARGE, FORM_DEGENERATE, FORM_SINGULAR, FORM_NOT_FINITE, FORM_NOT_CONVERGED = 1, 2, 4, 8, 16, 32, 64
FORM_MEMBER_UNTESTED = 1
FORM_MAX_ROWS, FORM_MAX_PARAMS, FORM_COLUMNS, FORM_QPP_COLUMNS, FORM_MEMBER_COLUMNS = 64, 7, 20, 28, 7
FORM_REPORTED = (4, 4, 6, 7)      # parameters reported per kind: n d | c r | x0 t | c n r
# include/jaicov_surfaces.h: cylinders and cones beside them, and start values from the caller for all six
SURF_EXPORTS = ["jaicov_surf_fit"]
SURF_CYLINDER, SURF_CONE = 4, 5
SURF_KINDS = dict(FORM_KINDS, cylinder=SURF_CYLINDER, cone=SURF_CONE)
SURF_REPORTED = FORM_REPORTED + (7, 7)      # x0 t r | apex t alpha
# include/jaicov_predict.h: predicted image points with their ellipses and the test of check measurements, read from the cofactor matrix
PRED_EXPORTS = ["jaicov_pred_points", "jaicov_pred_check"]
PRED_PARTIAL, PRED_NEGATIVE, PRED_NOT_FINITE, PRED_OBSERVED, PRED_SINGULAR = 1, 2, 4, 8, 16     # status bits of a pair or a group
PRED_POINT_COLUMNS, PRED_CHECK_COLUMNS, PRED_GROUP_COLUMNS, PRED_MAX_GROUP = 10, 8, 4, 32
# include/jaicov_newpoints.h: object points that were not part of the adjustment, intersected in the adjusted block with its full Qxx
NEWPT_EXPORTS = ["jaicov_newpt_intersect"]
NEWPT_PARTIAL, NEWPT_NOT_CONVERGED, NEWPT_TOO_FEW_RAYS, NEWPT_TOO_MANY, NEWPT_SINGULAR, NEWPT_NOT_FINITE = 1, 2, 4, 8, 16, 32   # bits of a point
NEWPT_FAILED = NEWPT_TOO_FEW_RAYS | NEWPT_TOO_MANY | NEWPT_SINGULAR | NEWPT_NOT_FINITE
NEWPT_PAIR_PARTIAL, NEWPT_PAIR_NEGATIVE, NEWPT_PAIR_NOT_FINITE, NEWPT_PAIR_DEGENERATE = 1, 2, 4, 8                             # bits of a pair
NEWPT_COLUMNS, NEWPT_PAIR_COLUMNS, NEWPT_MAX_RAYS, NEWPT_MAX_COLS = 20, 7, 64, 448
# include/jaicov_vce.h: variance components of observation groups from the residuals, redundancy numbers and weights on the device
VCE_EXPORTS = ["jaicov_vce_run", "jaicov_vce_get", "jaicov_vce_summary", "jaicov_vce_release"]
VCE_EMPTY, VCE_UNCONTROLLED, VCE_NOT_FINITE = 1, 2, 4                                                  # status bits of a group
VCE_COLUMNS = 6
# include/jaicov_calibration.h: the distortion field of a camera with its covariance, and the comparison of two calibrations
CALIB_EXPORTS = ["jaicov_calib_field", "jaicov_calib_compare", "jaicov_calib_release"]
CALIB_PARTIAL, CALIB_NEGATIVE, CALIB_NOT_FINITE, CALIB_SINGULAR = 1, 2, 4, 16                         # status bits of a node
CALIB_FIELD_COLUMNS, CALIB_COMPARE_COLUMNS, CALIB_SUMMARY_COLUMNS, CALIB_MAX_COLUMNS = 14, 8, 8, 23
CALIB_PRINCIPAL_POINT, CALIB_PRINCIPAL_DISTANCE, CALIB_KIND_SHIFT, CALIB_ALL = 1, 2, 2, 4095          # `columns` of calibration_field
CALIB_RELATIVE = 1                                                                                      # `flags` of calibration_compare
# jaicov_dlt_restriction (DirectLinearTransformation.RestrictionType, DT:51-58 order) and the per-image status values
DLT_IDENTICAL_PRINCIPLE_DISTANCE, DLT_ROTATION_WITHOUT_SHEAR, DLT_FIXED_PRINCIPLE_DISTANCE_X, DLT_FIXED_PRINCIPLE_DISTANCE_Y, \
    DLT_FIXED_PRINCIPAL_POINT_X, DLT_FIXED_PRINCIPAL_POINT_Y = range(6)
DLT_CONVERGED, DLT_NOT_CONVERGED, DLT_TOO_FEW_POINTS, DLT_SINGULAR, DLT_NOT_FINITE = range(5)
# include/jaicov_intersect.h: forward intersection of a batch of object points from oriented images (stand-alone, no engine)
ISECT_EXPORTS = ["jaicov_isect_points"]
ISECT_OK, ISECT_NOT_CONVERGED, ISECT_TOO_FEW_RAYS, ISECT_SINGULAR, ISECT_NOT_FINITE = range(5)
# include/jaicov_resect.h: spatial resection of a batch of images from known object points (stand-alone, no engine)
RESECT_EXPORTS = ["jaicov_resect_images"]
RESECT_OK, RESECT_NOT_CONVERGED, RESECT_TOO_FEW_POINTS, RESECT_SINGULAR, RESECT_NOT_FINITE = range(5)
RESECT_START_GIVEN, RESECT_START_SPACE, RESECT_START_PLANE = range(3)
# include/jaicov_relorient.h: relative orientation of a batch of image pairs from their common image points (stand-alone, no engine)
RELOR_EXPORTS = ["jaicov_relorient_pairs"]
RELOR_OK, RELOR_NOT_CONVERGED, RELOR_TOO_FEW_POINTS, RELOR_SINGULAR, RELOR_NOT_FINITE = range(5)
RELOR_START_GIVEN, RELOR_START_SPACE, RELOR_START_PLANE = range(3)
# include/jaicov_simil.h: absolute orientation (spatial similarity transformation) of a batch of models (stand-alone, no engine)
SIMIL_EXPORTS = ["jaicov_simil_models", "jaicov_simil_apply"]
SIMIL_OK, SIMIL_NOT_CONVERGED, SIMIL_TOO_FEW_POINTS, SIMIL_SINGULAR, SIMIL_NOT_FINITE = range(5)
SIMIL_START_GIVEN, SIMIL_START_CLOSED = range(2)
# include/jaicov_lens.h: lens-distortion correction of a batch of image points and its inverse (stand-alone, no engine)
LENS_EXPORTS = ["jaicov_lens_correct", "jaicov_lens_distort"]
LENS_OK, LENS_NOT_CONVERGED, LENS_SINGULAR, LENS_NOT_FINITE = range(4)

KROW = 32  # 12 + JAICOV_MAX_DIST_PER_CAMERA
INVERT_NONE, INVERT_FULL, INVERT_REDUCED = 0, 1, 2   # MatrixInversion (BundleAdjustment.java:65-70)
INVERT_FULL_EXPANDED = 3     # all of Qxx like FULL, computed from the EO-reduced system (jaicov_neq.h)

_pd = C.POINTER(C.c_double)
_pi = C.POINTER(C.c_int32)


class EngineError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        super().__init__(f"jaicov status {code} ({STATUS.get(code, '?')}): {msg}")


class EngineOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("image_begin", C.c_int32),
                ("image_end", C.c_int32), ("apply_shared", C.c_int32), ("assembly_mode", C.c_int32),
                ("block_size", C.c_int32), ("reduced_reference_quirk", C.c_int32), ("deterministic", C.c_int32), ("refinement", C.c_int32),
                ("ordinary_group_elimination", C.c_int32), ("dispersion_refinement", C.c_int32),
                ("expansion_exchange", C.c_int32), ("inverse_refinement", C.c_int32), ("reserved", C.c_int32 * 1)]


class EstimateOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_iterations", C.c_int32), ("invert", C.c_int32),
                ("simulation", C.c_int32), ("lambda0", C.c_double), ("sigma2apriori", C.c_double)]


class EstimateResult(C.Structure):
    _fields_ = [("state", C.c_int32), ("iterations", C.c_int32), ("omega", C.c_double), ("max_abs_dx", C.c_double),
                ("final_lambda", C.c_double), ("seconds_total", C.c_double), ("seconds_last_pass", C.c_double)]


_LIB = None


def build_library(force: bool = False) -> str:
    """Compiles csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    cmd = ["make", "-C", csrc, "-j4"] + (["-B"] if force else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return LIB_PATH


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                          "(hipcc --offload-arch=gfx950); this package has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.jaicov_neq_create.argtypes = [C.POINTER(ProblemDesc), C.POINTER(EngineOptions), C.POINTER(vp)]
    L.jaicov_neq_destroy.argtypes = [vp]
    L.jaicov_neq_destroy.restype = None
    L.jaicov_neq_last_error.argtypes = [vp]
    L.jaicov_neq_last_error.restype = C.c_char_p
    L.jaicov_neq_num_slots.argtypes = [vp]
    L.jaicov_neq_num_slots.restype = C.c_size_t
    L.jaicov_neq_packed_length.argtypes = [vp]
    L.jaicov_neq_packed_length.restype = C.c_size_t
    L.jaicov_neq_set_parameters.argtypes = [vp, _pd, C.c_size_t]
    L.jaicov_neq_get_parameters.argtypes = [vp, _pd, C.c_size_t]
    L.jaicov_neq_build.argtypes = [vp, C.c_double, C.c_double, C.c_int]
    L.jaicov_neq_accumulate.argtypes = [vp, C.c_double]
    L.jaicov_neq_accumulate2.argtypes = [vp, C.c_double, C.c_double]
    L.jaicov_neq_prepare_inverse.argtypes = [vp, C.c_int]
    L.jaicov_neq_reduced_order.argtypes = [vp]
    L.jaicov_neq_cofactor_order.argtypes = [vp]
    L.jaicov_neq_finalize.argtypes = [vp, C.c_double, C.c_double, C.c_int]
    L.jaicov_neq_reduce_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.jaicov_neq_reduce_buffer_async.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp)]
    L.jaicov_neq_solve.argtypes = [vp, C.c_int, _pd]
    L.jaicov_neq_eo_step_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.jaicov_neq_expansion_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.jaicov_neq_omega.argtypes = [vp, C.c_double, _pd, _pd]
    L.jaicov_neq_update.argtypes = [vp, _pd, _pd]
    L.jaicov_neq_get_normal.argtypes = [vp, _pd, C.c_size_t, _pd, C.c_size_t]
    L.jaicov_neq_get_cofactor.argtypes = [vp, _pd, C.c_size_t]
    L.jaicov_neq_get_cofactor_sub.argtypes = [vp, _pi, C.c_int32, _pd]
    L.jaicov_neq_get_dispersion_sub.argtypes = [vp, C.c_double, _pi, C.c_int32, _pd]
    L.jaicov_neq_get_rows.argtypes = [vp, C.c_int32, C.c_int32, _pd, _pd]
    L.jaicov_neq_estimate.argtypes = [vp, C.POINTER(EstimateOptions), C.POINTER(EstimateResult)]
    L.jaicov_neq_last_timings.argtypes = [vp, _pd, C.c_int32]
    L.jaicov_neq_set_profiling.argtypes = [vp, C.c_int]
    L.jaicov_neq_kernel_stats.argtypes = [vp, _pd, C.c_int32, C.c_int]
    L.jaicov_neq_cancel.argtypes = [vp]
    L.jaicov_neq_create_timings.argtypes = [vp, _pd, C.c_int32]
    L.jaicov_neq_get_block_weight.argtypes = [vp, C.c_int32, _pd, C.c_size_t]
    L.jaicov_dense_spd_solve_packed.argtypes = [C.c_int32, _pd, _pd, C.c_int32, C.c_int32, _pd]
    L.jaicov_dense_gemm.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, _pd, C.c_int64,
                                    _pd, C.c_int64, C.c_double, _pd, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _pd]
    L.jaicov_xform_run.argtypes = [vp, _pi, C.c_int32, _pi, _pi, C.c_int32, C.c_double, _pi]
    L.jaicov_xform_get_coordinates.argtypes = [vp, _pd, _pi, C.c_int32]
    L.jaicov_xform_get_covariance.argtypes = [vp, _pd, C.c_size_t]
    L.jaicov_xform_get_covariance_sub.argtypes = [vp, _pi, C.c_int32, _pd]
    L.jaicov_xform_get_point_blocks.argtypes = [vp, _pd, C.c_int32]
    L.jaicov_xform_release.argtypes = [vp]
    L.jaicov_rel_run.argtypes = [vp, C.c_double, _pd, _pi]
    L.jaicov_rel_get.argtypes = [vp, _pd, _pd, _pd, _pd, C.c_int32]
    L.jaicov_rel_summary.argtypes = [vp, _pd, C.c_int32]
    L.jaicov_rel_release.argtypes = [vp]
    L.jaicov_rel_run_points.argtypes = [vp, C.c_double, _pd, C.c_double, C.c_double, C.c_int32, _pi, _pi]
    L.jaicov_rel_get_points.argtypes = [vp, _pd, C.c_int32]
    L.jaicov_datum_transform.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int32]
    L.jaicov_datum_apply.argtypes = [vp, _pd, _pd, C.c_int32]
    L.jaicov_prec_points.argtypes = [vp, C.c_double, C.c_double, C.c_double, _pi, C.c_int32, _pd, _pi]
    L.jaicov_prec_stations.argtypes = [vp, C.c_double, C.c_double, C.c_double, _pi, C.c_int32, _pd, _pi]
    L.jaicov_prec_lengths.argtypes = [vp, C.c_double, _pi, C.c_int32, _pd, _pi]
    L.jaicov_prec_components.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, _pd, _pd, _pd, _pd, _pi]
    L.jaicov_par_maxima.argtypes = [vp, C.c_uint32, C.c_uint32, _pd, _pi, _pi, C.c_int32]
    L.jaicov_par_pairs.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_double, C.c_int64, _pi, _pd, C.POINTER(C.c_int64)]
    L.jaicov_par_block.argtypes = [vp, _pi, C.c_int32, _pi, C.c_int32, _pd]
    L.jaicov_par_tests.argtypes = [vp, C.c_double, _pi, _pi, _pd, C.c_int32, _pd, _pi]
    L.jaicov_form_fit.argtypes = [vp, C.c_double, C.c_int32, _pi, _pi, _pi, C.c_int32, C.c_double, _pd, _pd, _pd, _pi, _pi, C.POINTER(C.c_float)]
    L.jaicov_surf_fit.argtypes = [vp, C.c_double, C.c_int32, _pi, _pi, _pi, _pd, C.c_int32, C.c_double, _pd, _pd, _pd, _pi, _pi, C.POINTER(C.c_float)]
    L.jaicov_pred_points.argtypes = [vp, C.c_double, C.c_double, _pi, _pi, C.c_int32, _pd, _pi]
    L.jaicov_pred_check.argtypes = [vp, C.c_double, _pi, _pi, _pd, _pd, C.c_int32, _pi, C.c_int32, _pd, _pi, _pd, _pi]
    L.jaicov_newpt_intersect.argtypes = [vp, C.c_double, C.c_int32, _pi, _pi, _pd, _pd, _pd, C.c_int32, _pi, C.c_int32, _pd, _pi, _pi, _pd, _pd, _pi]
    L.jaicov_vce_run.argtypes = [vp, C.c_double, _pd, _pi, _pi, _pi, C.c_int32, _pi]
    L.jaicov_vce_get.argtypes = [vp, _pd, _pi, C.c_int32]
    L.jaicov_vce_summary.argtypes = [vp, _pd, C.c_int32]
    L.jaicov_vce_release.argtypes = [vp]
    L.jaicov_debug_vce_timing.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.jaicov_calib_field.argtypes = [vp, C.c_double, C.c_double, C.c_uint32, _pi, _pd, _pd, C.c_int32, _pd, _pd, _pi]
    L.jaicov_calib_compare.argtypes = [vp, C.c_double, C.c_int32, C.c_int32, _pd, _pd, C.c_uint32, _pd, _pd, C.c_int32, _pd, _pi, _pd]
    L.jaicov_calib_release.argtypes = [vp]
    L.jaicov_debug_calib_timing.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.jaicov_dlt_adjust.argtypes = [C.c_int32, _pi, _pd, _pd, _pd, C.POINTER(C.c_uint8), _pi, C.c_int32, C.c_int32, _pd, _pi, _pi, _pd]
    L.jaicov_isect_points.argtypes = [C.c_int32, _pi, _pi, _pd, _pd, C.c_int32, _pd, _pd, C.c_double, C.c_int32, C.c_double, C.c_int32,
                                      _pd, _pi, _pi, C.POINTER(C.c_uint8), _pd, _pd]
    L.jaicov_resect_images.argtypes = [C.c_int32, _pi, _pd, _pd, _pd, _pd, _pd, C.c_double, C.c_int32, C.c_double, C.c_int32,
                                       _pd, _pi, _pi, _pi, C.POINTER(C.c_uint8), _pd, _pd]
    L.jaicov_relorient_pairs.argtypes = [C.c_int32, _pi, _pd, _pd, _pd, _pd, _pd, _pd, C.c_double, C.c_int32, C.c_double, C.c_int32,
                                         _pd, _pi, _pi, _pi, C.POINTER(C.c_uint8), _pd, _pd]
    L.jaicov_simil_models.argtypes = [C.c_int32, _pi, _pd, _pd, _pd, _pd, _pd, C.c_int32, C.c_double, C.c_int32,
                                      _pd, _pi, _pi, _pi, C.POINTER(C.c_uint8), _pd, _pd]
    L.jaicov_simil_apply.argtypes = [C.c_int32, _pd, _pi, _pd, _pd, _pi, _pd, _pd, _pd, _pd]
    L.jaicov_lens_correct.argtypes = [C.c_int32, _pi, _pd, _pd, _pd, C.c_int32, _pd, _pd, _pi, _pi, _pi, _pd, C.c_int32, C.c_double,
                                      _pd, _pd, _pd, _pi, _pi, _pd]
    L.jaicov_lens_distort.argtypes = [C.c_int32, _pi, _pd, _pd, _pd, C.c_int32, _pd, _pd, _pi, _pi, _pi, _pd, _pd, _pd, _pd, _pi, _pd]
    _LIB = L
    return L


# Engine.reliability: one entry per observation row (include/jaicov_reliability.h)
Reliability = namedtuple("Reliability", ["v", "qvv", "r", "t"])
# Engine.reliability_points: one entry per image point, the columns of include/jaicov_reliability_points.h in their order
REL_POINT_COLUMNS = 14
PointReliability = namedtuple("PointReliability", ["q", "T_prio", "T_post", "nabla_x", "nabla_y", "Mxx", "Mxy", "Myy", "mdb_major",
                                                   "mdb_minor", "delta_ext", "dX", "dY", "dZ"])


# Engine.precision_points / precision_stations: one entry per item (include/jaicov_precision.h); axes[i, j] is the unit vector of
# semi-axis j; sigma_angles is None for points
PointPrecision = namedtuple("PointPrecision", ["sigma", "helmert", "semi_axes", "axes", "ellipse", "direction", "eigenvalues",
                                               "sigma_angles", "status"])
LengthPrecision = namedtuple("LengthPrecision", ["length", "sigma", "sigma_diff", "status"])
PrincipalComponents = namedtuple("PrincipalComponents", ["values", "vectors", "trace", "residuals", "iterations", "converged"])
# Engine.correlation_maxima: one entry per column of the cofactor matrix (include/jaicov_parameters.h)
CorrelationMaxima = namedtuple("CorrelationMaxima", ["rho", "partner", "status"])
# Engine.correlated_pairs: cols (m, 2) with i > j and rho (m,), sorted; both None when count exceeds the capacity
CorrelatedPairs = namedtuple("CorrelatedPairs", ["cols", "rho", "count"])
# Engine.parameter_tests: one entry per group; t is NaN unless k == 1
ParameterTests = namedtuple("ParameterTests", ["q", "T", "k", "t", "status"])
ColumnName = namedtuple("ColumnName", ["cls", "item", "component"])
# Engine.fit_forms: one entry per form (include/jaicov_forms.h).  params / sigma (n, 7), NaN behind the kind's parameters; qpp (n, 7, 7)
# symmetric; begin (n + 1,): the members of form g are rows begin[g] .. begin[g + 1] of v (M, 3), distance, nabla (M, 2), T_member and
# member_status; kernel_ms: the kernel's time by events
FormFits = namedtuple("FormFits", ["params", "sigma", "qpp", "omega", "dof", "T", "max_distance", "rms_distance", "iterations", "status",
                                   "begin", "v", "distance", "nabla", "T_member", "member_status", "kernel_ms"])
# Engine.predict_image_points: one entry per pair (include/jaicov_predict.h); cof (n, 3): q_xx, q_xy, q_yy of J Qxx J'; ellipse (n, 2): A >= B
ImagePrediction = namedtuple("ImagePrediction", ["xy", "cof", "sigma", "ellipse", "direction", "status"])
# Engine.check_image_points: one entry per pair (d (n, 2), M (n, 3): m_xx, m_xy, m_yy) and one per group (dof = 2 m)
ImageCheck = namedtuple("ImageCheck", ["d", "M", "q", "T_prio", "T_post", "status"])
GroupCheck = namedtuple("GroupCheck", ["q", "T_prio", "T_post", "dof", "status"])
# Engine.calibration_field: one entry per node (include/jaicov_calibration.h); delta (n, 2): the image correction; cof (n, 3): q_xx, q_xy,
# q_yy of J Q J' over the selected columns; radial (n, 2): dr, dt and sigma_radial (n, 2) their sigmas; jac (n, 2, 23) or None
CalibrationField = namedtuple("CalibrationField", ["delta", "cof", "sigma", "ellipse", "direction", "radial", "sigma_radial", "status", "jac"])
# Engine.calibration_compare: one entry per node (d (n, 2), M (n, 3): m_xx, m_xy, m_yy of C_d; all None with nodes=False) and the summary
CalibrationCompare = namedtuple("CalibrationCompare", ["d", "M", "q", "T_prio", "T_post", "status", "summary"])
CalibrationSummary = namedtuple("CalibrationSummary", ["n_finite", "rms", "rms_expected", "max_d", "max_d_node", "max_T_prio", "max_T_node",
                                                       "n_singular"])
# Engine.intersect_new_points: one entry per new point (cof_meas, cof (n, 6): xx xy xz yy yz zz of Q_meas and of Q_XX = Q_meas + Q_sys;
# ray_w (n_rays, 2)) and one per pair (lengths (n_pairs, 7): L, sigma_L, sigma of D_X, D_Y, D_Z, q_L, q_L without the cross block)
NewPoints = namedtuple("NewPoints", ["xyz", "cof_meas", "cof", "sigma", "omega", "dof", "status", "iterations", "ray_w", "lengths",
                                     "length_status"])


# Groups of weight blocks for Engine.variance_components (vce_groups builds them): ip / sb / dg hold the group of every image point,
# scale bar and directly observed group (-1: in none; None: none of that kind is in a group); names: one label per group
VceGroups = namedtuple("VceGroups", ["ip", "sb", "dg", "n_groups", "names"])
# the totals of Engine.variance_components over all rows, grouped or not
VceSummary = namedtuple("VceSummary", ["omega", "sum_r", "rows_grouped", "rows_ungrouped", "damping"])
# estimate_variance_components: factors (n_groups,) accumulated over the iterations, tables (one VarianceComponents per iteration),
# engine (the last one, open), problem (the FlatProblem that engine was built from), converged
VceEstimate = namedtuple("VceEstimate", ["factors", "tables", "engine", "problem", "converged"])


class VarianceComponents:
    """Engine.variance_components: one entry per group (include/jaicov_vce.h).  n rows, omega = sum v_b' P_b v_b, r = sum r_i,
    s2 = omega / r, k = s2 / sigma0^2 (the factor for the group's dispersions), sd = k sqrt(2 / r); s2, k, sd are NaN where status
    has VCE_EMPTY, VCE_UNCONTROLLED or VCE_NOT_FINITE.  table is the (VCE_COLUMNS, n_groups) array of them, summary a VceSummary."""

    def __init__(self, table, status, summary, names=None):
        self.table, self.status, self.summary, self.names = table, status, summary, names
        self.n, self.omega, self.r, self.s2, self.k, self.sd = table

    def __repr__(self):
        names = self.names if self.names is not None else [str(g) for g in range(self.status.size)]
        rows = [f"  {nm}: n={int(n)} omega={om:.6g} r={r:.6g} k={k:.4g} +- {sd:.2g} status={st}"
                for nm, n, om, r, k, sd, st in zip(names, self.n, self.omega, self.r, self.k, self.sd, self.status)]
        return "VarianceComponents(\n" + "\n".join(rows) + f"\n  {self.summary})"


def _p(a):
    return a.ctypes.data_as(_pd)


class Engine:
    """One engine per adjustment (``BundleAdjustment`` is single-shot: BundleAdjustment.java:203)."""

    def __init__(self, fp: FlatProblem, device: int = 0, image_range=None, apply_shared: bool = True, assembly_mode: int = 0,
                 reduced_reference_quirk: bool = False, deterministic=None, refinement: int = 0,
                 ordinary_group_elimination: int = 0, dispersion_refinement: int = 0, expansion_exchange: bool = False,
                 inverse_refinement: int = 0):
        self.L = load_library()
        self.fp = fp
        self.U = fp.n_unknowns
        self._desc, self._keep = fp.as_desc()
        opts = EngineOptions()
        opts.struct_size = C.sizeof(EngineOptions)
        opts.device = device
        opts.image_begin, opts.image_end = image_range if image_range is not None else (-1, -1)
        opts.apply_shared = int(apply_shared)
        opts.assembly_mode = int(assembly_mode)
        opts.reduced_reference_quirk = int(reduced_reference_quirk)
        # None: the engine's default (deterministic since round 4); True / False: on / off (arrival-order atomics, 0.3 ms faster at config 4)
        opts.deterministic = 0 if deterministic is None else (1 if deterministic else -1)
        opts.ordinary_group_elimination = int(ordinary_group_elimination)   # < 0: ordinary image groups stay outside the EO pre-elimination
        opts.dispersion_refinement = int(dispersion_refinement)             # < 0: inv(D) as the blocked Cholesky leaves it
        opts.expansion_exchange = int(expansion_exchange)                   # sharded engines: the caller all-reduces expansion_buffer()
        self.expansion_exchange = bool(expansion_exchange)
        opts.inverse_refinement = int(inverse_refinement)                   # < 0: no Newton-Schulz step on the inverse of orders <= 8192
        opts.refinement = int(refinement)      # 0 = default (one step of iterative refinement per solve), < 0 = none, k = k steps
        self._h = C.c_void_p()
        self.xform_count = 0
        rc = self.L.jaicov_neq_create(C.byref(self._desc), C.byref(opts), C.byref(self._h))
        if rc != 0:
            msg = self.L.jaicov_neq_last_error(self._h).decode() if self._h else ""
            if self._h:
                self.L.jaicov_neq_destroy(self._h)
                self._h = C.c_void_p()
            raise EngineError(rc, msg)

    def close(self):
        if getattr(self, "_h", None):
            self.L.jaicov_neq_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise EngineError(rc, self.L.jaicov_neq_last_error(self._h).decode())

    # parameters ---------------------------------------------------------------------------------------------
    def set_parameters(self, values):
        v = np.ascontiguousarray(values, np.float64)
        self._chk(self.L.jaicov_neq_set_parameters(self._h, _p(v), v.size))

    def get_parameters(self):
        v = np.zeros(self.fp.n_slots)
        self._chk(self.L.jaicov_neq_get_parameters(self._h, _p(v), v.size))
        return v

    # loop body ----------------------------------------------------------------------------------------------
    def build(self, sigma2, lam=0.0, simulation=False):
        self._sigma2_build = float(sigma2)      # reliability_points forms its default Omega with the weights of this build
        self._chk(self.L.jaicov_neq_build(self._h, sigma2, lam, int(simulation)))

    def accumulate(self, sigma2, lam=0.0):
        self._chk(self.L.jaicov_neq_accumulate2(self._h, sigma2, lam))

    def reduced_order(self):
        """Order of the system assembled by the last accumulate (U, or the first EO column with EO pre-elimination)."""
        return int(self.L.jaicov_neq_reduced_order(self._h))

    def prepare_inverse(self, inverse_follows=True):
        """Announce the `invert` value of the solve after the next build (final pass): INVERT_FULL (True) makes that
        build assemble the full system, INVERT_REDUCED keeps the EO pre-elimination."""
        self._chk(self.L.jaicov_neq_prepare_inverse(self._h, int(inverse_follows)))

    def cofactor_order(self):
        return int(self.L.jaicov_neq_cofactor_order(self._h))

    def finalize(self, sigma2, lam=0.0, simulation=False):
        self._sigma2_build = float(sigma2)
        self._chk(self.L.jaicov_neq_finalize(self._h, sigma2, lam, int(simulation)))

    def reduce_buffer(self):
        ptr = C.c_void_p(); cnt = C.c_size_t()
        self._chk(self.L.jaicov_neq_reduce_buffer(self._h, C.byref(ptr), C.byref(cnt)))
        return ptr.value, cnt.value

    def reduce_buffer_async(self):
        """(device pointer, count, hipStream_t) -- no host wait; the buffer is complete in the order of that stream."""
        ptr = C.c_void_p(); cnt = C.c_size_t(); st = C.c_void_p()
        self._chk(self.L.jaicov_neq_reduce_buffer_async(self._h, C.byref(ptr), C.byref(cnt), C.byref(st)))
        return ptr.value, cnt.value, st.value

    def eo_step_buffer(self):
        """(device pointer, count) of the EO steps this engine back-substituted in the last solve (6 per image, zeros elsewhere)."""
        ptr = C.c_void_p(); cnt = C.c_size_t()
        self._chk(self.L.jaicov_neq_eo_step_buffer(self._h, C.byref(ptr), C.byref(cnt)))
        return ptr.value, cnt.value

    def expansion_buffer(self):
        """(device pointer, count) of [F | L_E^-1] for a sharded FULL_EXPANDED final pass: sum over the ranks, then solve."""
        ptr = C.c_void_p(); cnt = C.c_size_t()
        self._chk(self.L.jaicov_neq_expansion_buffer(self._h, C.byref(ptr), C.byref(cnt)))
        return ptr.value, cnt.value

    def solve(self, invert=False):
        dx = np.zeros(max(self.U, 1))
        self._chk(self.L.jaicov_neq_solve(self._h, int(invert), _p(dx)))
        return dx[:self.U]

    def omega(self, sigma2, dx):
        dx = np.ascontiguousarray(dx, np.float64)
        om = np.zeros(1)
        self._chk(self.L.jaicov_neq_omega(self._h, sigma2, _p(dx), _p(om)))
        return float(om[0])

    def update(self, dx):
        dx = np.ascontiguousarray(dx, np.float64)
        mx = np.zeros(1)
        self._chk(self.L.jaicov_neq_update(self._h, _p(dx), _p(mx)))
        return float(mx[0])

    # results ------------------------------------------------------------------------------------------------
    def get_normal(self):
        N = np.zeros(self.fp.packed_length); n = np.zeros(self.U)
        self._chk(self.L.jaicov_neq_get_normal(self._h, _p(N), N.size, _p(n), n.size))
        return N, n

    def get_cofactor(self):
        """Packed 'U' cofactor matrix of order cofactor_order() (U after INVERT_FULL, reduced_order() after INVERT_REDUCED)."""
        k = self.cofactor_order()
        if k < 0:
            raise EngineError(-2, "no cofactor matrix: solve with invert != 0 first")
        Q = np.zeros(k * (k + 1) // 2)
        self._chk(self.L.jaicov_neq_get_cofactor(self._h, _p(Q), Q.size))
        return Q

    def get_cofactor_sub(self, idx):
        idx = np.ascontiguousarray(idx, np.int32)
        out = np.zeros((idx.size, idx.size))
        self._chk(self.L.jaicov_neq_get_cofactor_sub(self._h, idx.ctypes.data_as(_pi), idx.size, _p(out)))
        return out

    def get_dispersion_sub(self, sigma2_aposteriori, idx):
        """sigma2 * Qxx[idx, idx] gathered and scaled on the device (what the result writers print)."""
        idx = np.ascontiguousarray(idx, np.int32)
        out = np.zeros((idx.size, idx.size))
        self._chk(self.L.jaicov_neq_get_dispersion_sub(self._h, float(sigma2_aposteriori), idx.ctypes.data_as(_pi), idx.size, _p(out)))
        return out

    # coordinate transformation (include/jaicov_transform.h) -----------------------------------------------------------
    def transform(self, points, pairs, sigma2):
        """CoordinateTransformationExteriorOrientation.transform on the device: `points` (distinct object point indices, in order),
        `pairs` ((ref, src) image indices, the reference's Map<Image, List<Image>> flattened in iteration order).  Needs all of Qxx
        (an inverting solve with INVERT_FULL / INVERT_FULL_EXPANDED).  Returns (xyz (n, 3), ids (n, 3): point, src, ref); the
        covariance sigma2 J Qxx J' stays on the device (transform_covariance / transform_covariance_sub)."""
        pts = np.ascontiguousarray(points, np.int32).ravel()
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        ref = np.ascontiguousarray(pr[:, 0]); src = np.ascontiguousarray(pr[:, 1])
        n = C.c_int32(0)
        self._chk(self.L.jaicov_xform_run(self._h, pts.ctypes.data_as(_pi), pts.size, ref.ctypes.data_as(_pi), src.ctypes.data_as(_pi),
                                          ref.size, float(sigma2), C.byref(n)))
        self.xform_count = n.value
        xyz = np.zeros((n.value, 3)); ids = np.zeros((n.value, 3), np.int32)
        self._chk(self.L.jaicov_xform_get_coordinates(self._h, _p(xyz), ids.ctypes.data_as(_pi), n.value))
        return xyz, ids

    def transform_covariance(self):
        """The whole covariance of the last transform, packed 'U' of order R = 3 n."""
        R = 3 * self.xform_count
        ap = np.zeros(R * (R + 1) // 2)
        self._chk(self.L.jaicov_xform_get_covariance(self._h, _p(ap), ap.size))
        return ap

    def transform_covariance_sub(self, rows):
        """C[rows, rows] of the last transform, gathered on the device (row-major k x k)."""
        idx = np.ascontiguousarray(rows, np.int32)
        out = np.zeros((idx.size, idx.size))
        self._chk(self.L.jaicov_xform_get_covariance_sub(self._h, idx.ctypes.data_as(_pi), idx.size, _p(out)))
        return out

    def transform_point_blocks(self):
        """Every 3 x 3 diagonal block of the last transform's covariance in one call: (n, 3, 3)."""
        out = np.zeros((self.xform_count, 3, 3))
        self._chk(self.L.jaicov_xform_get_point_blocks(self._h, _p(out), self.xform_count))
        return out

    def transform_release(self):
        self._chk(self.L.jaicov_xform_release(self._h))
        self.xform_count = 0

    # reliability (include/jaicov_reliability.h) ---------------------------------------------------------------------------------
    def reliability(self, sigma2_test, dx=None):
        """Residuals v = A dx - w, their cofactors qvv = diag(Q_ll - A Qxx A'), redundancy numbers r = diag(Q_vv P) and test values
        t = (P v) / sqrt(sigma2_test diag(P Q_vv P)) (NaN: not controlled) of every observation row, in the reference's row order.
        Needs all of Qxx (an inverting solve with INVERT_FULL / INVERT_FULL_EXPANDED).  dx None = a zero step."""
        n = C.c_int32(0)
        d = None if dx is None else np.ascontiguousarray(dx, np.float64)
        if d is not None and d.size != self.fp.n_unknowns:
            raise ValueError("dx must have U entries")
        self._chk(self.L.jaicov_rel_run(self._h, float(sigma2_test), None if d is None else _p(d), C.byref(n)))
        out = [np.zeros(n.value) for _ in range(4)]
        self._chk(self.L.jaicov_rel_get(self._h, *[_p(a) for a in out], n.value))
        return Reliability(*out)

    def reliability_points(self, sigma2_test, dx=None, lambda0=17.075, omega=None, dof=None):
        """reliability() and, for every image point, what taking it out would do (include/jaicov_reliability_points.h): the drop q of
        Omega, the joint tests T_prio and T_post, the estimated gross error, M = (P Q_vv P)_SS, the minimal detectable bias, the
        external reliability and the shift of the point's own object coordinates.  omega None = Omega of dx (or of a zero step) with
        the variance factor of the last build (the problem's a-priori one after estimate()); dof None = n - u + d.  Returns (Reliability, PointReliability)."""
        d = None if dx is None else np.ascontiguousarray(dx, np.float64)
        if d is not None and d.size != self.fp.n_unknowns:
            raise ValueError("dx must have U entries")
        if omega is None:
            omega = self.omega(getattr(self, "_sigma2_build", self.fp.sigma2apriori), np.zeros(max(self.U, 1)) if d is None else d)
        if dof is None:
            dof = self.fp.degree_of_freedom      # n - u + d; the columns of a datum border are not parameters
        n = C.c_int32(0); k = C.c_int32(0)
        self._chk(self.L.jaicov_rel_run_points(self._h, float(sigma2_test), None if d is None else _p(d), float(lambda0), float(omega),
                                               int(dof), C.byref(n), C.byref(k)))
        out = [np.zeros(n.value) for _ in range(4)]
        self._chk(self.L.jaicov_rel_get(self._h, *[_p(a) for a in out], n.value))
        tab = np.zeros((REL_POINT_COLUMNS, k.value))
        self._chk(self.L.jaicov_rel_get_points(self._h, _p(tab), k.value))
        return Reliability(*out), PointReliability(*tab)

    def reliability_summary(self):
        """(sum r, max |t|, its row, rows with NaN t, min r, damping of the inverted build) of the last reliability run."""
        out = np.zeros(6)
        self._chk(self.L.jaicov_rel_summary(self._h, _p(out), 6))
        return out

    def reliability_release(self):
        self._chk(self.L.jaicov_rel_release(self._h))

    # variance components (include/jaicov_vce.h) -------------------------------------------------------------------------------
    def variance_components(self, groups, sigma2_test=None, dx=None):
        """Variance components of groups of observations (a VceGroups, see vce_groups): for every group the factor k by which its
        a-priori dispersions should be multiplied, from Omega_g = sum v' P v and r_g = sum r_i of its weight blocks.  Runs
        reliability(sigma2_test, dx) first, through the same routine, so that call's result is fresh afterwards.  sigma2_test None =
        the variance factor of the last build; it enters the test values of the reliability result only.  Needs all of Qxx."""
        d = None if dx is None else np.ascontiguousarray(dx, np.float64)
        if d is not None and d.size != self.fp.n_unknowns:
            raise ValueError("dx must have U entries")
        fp = self.fp

        def ids(a, n, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.int32).ravel()
            if a.size != n:
                raise ValueError(f"groups.{what} must have {n} entries")
            return a
        ip = ids(groups.ip, fp.n_image_points, "ip"); sb = ids(groups.sb, fp.n_scale_bars, "sb"); dg = ids(groups.dg, fp.n_direct_groups, "dg")
        if sigma2_test is None:
            sigma2_test = getattr(self, "_sigma2_build", fp.sigma2apriori)
        G = int(groups.n_groups)
        as_pi = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(_pi)
        self._chk(self.L.jaicov_vce_run(self._h, float(sigma2_test), None if d is None else _p(d), as_pi(ip), as_pi(sb), as_pi(dg), G, None))
        table = np.zeros((VCE_COLUMNS, G)); status = np.zeros(G, np.int32); summ = np.zeros(5)
        self._chk(self.L.jaicov_vce_get(self._h, _p(table), status.ctypes.data_as(_pi), G))
        self._chk(self.L.jaicov_vce_summary(self._h, _p(summ), 5))
        return VarianceComponents(table, status, VceSummary(*summ), groups.names)

    def variance_components_reliability(self, n_rows=None):
        """The Reliability (v, qvv, r, t) that the last variance_components left on the device."""
        n = self.fp.n_observations if n_rows is None else int(n_rows)
        out = [np.zeros(n) for _ in range(4)]
        self._chk(self.L.jaicov_rel_get(self._h, *[_p(a) for a in out], n))
        return Reliability(*out)

    def variance_components_release(self):
        self._chk(self.L.jaicov_vce_release(self._h))

    # datum transformation (include/jaicov_datum.h) --------------------------------------------------------------------------------
    def datum_transform(self, mask):
        """Replaces the cofactor matrix, in place, by the one of the datum whose points the mask flags (one entry per object point,
        the meaning of FlatProblem.point_datum; the defect flags stay the engine's).  Every consumer of the cofactor matrix sees the
        new datum until the next inverting solve."""
        m = np.ascontiguousarray(mask, np.uint8).ravel()
        self._chk(self.L.jaicov_datum_transform(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8)), m.size))

    def datum_apply(self, v):
        """S v with the S = I - Z B' of the last datum_transform (v of length cofactor_order(); border entries of the result 0)."""
        x = np.ascontiguousarray(v, np.float64).ravel()
        out = np.zeros(x.size)
        self._chk(self.L.jaicov_datum_apply(self._h, _p(x), _p(out), x.size))
        return out

    # precision (include/jaicov_precision.h) ---------------------------------------------------------------------------------------
    def _precision_blocks(self, fn, columns, total, sigma2, k3, k2, items):
        idx = None if items is None else np.ascontiguousarray(items, np.int32).ravel()
        n = total if idx is None else idx.size
        out = np.zeros((n, columns)); status = np.zeros(n, np.int32)
        self._chk(fn(self._h, float(sigma2), float(k3), float(k2), None if idx is None else idx.ctypes.data_as(_pi), n, _p(out),
                     status.ctypes.data_as(_pi)))
        return PointPrecision(out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 7:16].reshape(n, 3, 3), out[:, 16:18], out[:, 18], out[:, 19:22],
                              out[:, 22:25] if columns > PREC_POINT_COLUMNS else None, status)

    def precision_points(self, sigma2, k3=1.0, k2=1.0, points=None):
        """Standard deviations, Helmert point error, confidence ellipsoid (semi-axes k3 sqrt(sigma2 lambda) with their unit vectors as
        rows of `axes`), horizontal ellipse (k2) and raw eigenvalues of the 3 x 3 cofactor block of every object point (or of
        `points`), read on the device from the cofactor matrix of the last inverting solve.  Returns a PointPrecision."""
        return self._precision_blocks(self.L.jaicov_prec_points, PREC_POINT_COLUMNS, self.fp.n_points, sigma2, k3, k2, points)

    def precision_stations(self, sigma2, k3=1.0, k2=1.0, images=None):
        """precision_points for the projection centres X0, Y0, Z0 of every image (or of `images`), with the standard deviations of
        omega, phi, kappa in `sigma_angles`.  Needs INVERT_FULL or INVERT_FULL_EXPANDED."""
        return self._precision_blocks(self.L.jaicov_prec_stations, PREC_STATION_COLUMNS, self.fp.n_images, sigma2, k3, k2, images)

    def precision_lengths(self, sigma2, pairs):
        """Length L between the adjusted object points of every pair (A, B), its standard deviation from the 6 x 6 block with the
        cross-covariances, and the standard deviations of the three coordinate differences.  Returns a LengthPrecision."""
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        out = np.zeros((pr.shape[0], PREC_LENGTH_COLUMNS)); status = np.zeros(pr.shape[0], np.int32)
        self._chk(self.L.jaicov_prec_lengths(self._h, float(sigma2), pr.ctypes.data_as(_pi), pr.shape[0], _p(out), status.ctypes.data_as(_pi)))
        return LengthPrecision(out[:, 0], out[:, 1], out[:, 2:5], status)

    def point_column_range(self):
        """(first column, number of columns) of the coordinates of the object points that images observe: they are numbered first, so
        their free coordinates are one leading range of the cofactor matrix (points of scale bars only follow the exterior
        orientations and are not part of it)."""
        return point_column_range(self.fp)

    def principal_components(self, k=3, first_col=None, n_cols=None, tol=0.0, max_iterations=200):
        """The k <= 4 largest eigenpairs of the principal sub-block of the cofactor matrix over columns [first_col, first_col + n_cols)
        (default: point_column_range()) by subspace iteration on the device.  Returns a PrincipalComponents; `converged` is False
        when max_iterations products were not enough (the values are those of the last one)."""
        if first_col is None or n_cols is None:
            first_col, n_cols = self.point_column_range()
        kk = max(int(k), 0)
        values = np.zeros(kk); vectors = np.zeros((kk, max(int(n_cols), 0))); res = np.zeros(kk); tr = np.zeros(1)
        it = C.c_int32(0)
        self._chk(self.L.jaicov_prec_components(self._h, int(first_col), int(n_cols), int(k), float(tol), int(max_iterations), _p(values),
                                                _p(vectors), _p(tr), _p(res), C.byref(it)))
        return PrincipalComponents(values, vectors, float(tr[0]), res, abs(it.value), it.value > 0)

    # correlations and tests of the unknowns (include/jaicov_parameters.h) ----------------------------------------------------------
    def correlation_maxima(self, pair_mask=PAR_ALL_PAIRS, flags=0):
        """For every column of the cofactor matrix its admissible partner of largest |rho| (the lowest among equals), in one pass
        over the lower triangle on the device.  pair_mask bit 4 a + b: a column of class a considers partners of class b
        (PAR_CLASS_*); flags: PAR_SKIP_SAME_POINT / PAR_SKIP_SAME_IMAGE.  Returns a CorrelationMaxima."""
        n = self.cofactor_order()
        if n < 0:
            raise EngineError(-2, "no cofactor matrix: solve with invert != 0 first")
        rho = np.zeros(n); partner = np.zeros(n, np.int32); status = np.zeros(n, np.int32)
        self._chk(self.L.jaicov_par_maxima(self._h, int(pair_mask), int(flags), _p(rho), partner.ctypes.data_as(_pi),
                                           status.ctypes.data_as(_pi), n))
        return CorrelationMaxima(rho, partner, status)

    def correlated_pairs(self, threshold, pair_mask=PAR_ALL_PAIRS, flags=0, capacity=1 << 16):
        """Every pair of columns i > j with |rho| >= threshold that the mask admits in either direction, sorted by |rho| descending,
        then i, then j.  Returns a CorrelatedPairs; `count` is always exact, cols and rho are None when it exceeds `capacity`."""
        cap = int(capacity)
        cols = np.zeros((max(cap, 0), 2), np.int32); rho = np.zeros(max(cap, 0)); count = C.c_int64(-1)
        self._chk(self.L.jaicov_par_pairs(self._h, int(pair_mask), int(flags), float(threshold), cap, cols.ctypes.data_as(_pi), _p(rho),
                                          C.byref(count)))
        m = count.value
        if m > cap:
            return CorrelatedPairs(None, None, m)
        return CorrelatedPairs(cols[:m].copy(), rho[:m].copy(), m)

    def correlation_block(self, row_cols, col_cols):
        """rho between every column of `row_cols` and every column of `col_cols`: (n_r, n_c), 1.0 where both are the same column."""
        r = np.ascontiguousarray(row_cols, np.int32).ravel(); c = np.ascontiguousarray(col_cols, np.int32).ravel()
        out = np.zeros((r.size, c.size))
        self._chk(self.L.jaicov_par_block(self._h, r.ctypes.data_as(_pi), r.size, c.ctypes.data_as(_pi), c.size, _p(out)))
        return out

    def parameter_tests(self, sigma2, groups, x0=None):
        """Test of x_g = x0_g for every group of slots in `groups` (a list of slot lists; x0: None for zeros, or lists parallel to
        them): q = delta' inv(Q_gg) delta, T = q / (k sigma2), k free members, and the signed t of a single parameter.  No quantile
        is evaluated.  Returns a ParameterTests."""
        groups = [np.asarray(g, np.int32).ravel() for g in groups]
        begin = np.concatenate([[0], np.cumsum([g.size for g in groups])]).astype(np.int32)
        slots = np.ascontiguousarray(np.concatenate(groups) if groups else np.zeros(0), np.int32)
        xs = None
        if x0 is not None:
            xs = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float64).ravel() for x in x0]) if groups else np.zeros(0), np.float64)
            if xs.size != slots.size:
                raise ValueError("x0 must run parallel to the groups")
        n = len(groups)
        out = np.zeros((n, PAR_TEST_COLUMNS)); status = np.zeros(n, np.int32)
        self._chk(self.L.jaicov_par_tests(self._h, float(sigma2), begin.ctypes.data_as(_pi), slots.ctypes.data_as(_pi),
                                          None if xs is None else _p(xs), n, _p(out), status.ctypes.data_as(_pi)))
        return ParameterTests(out[:, 0], out[:, 1], out[:, 2].astype(np.int32), out[:, 3], status)

    # forms through adjusted points (include/jaicov_forms.h) ------------------------------------------------------------------------
    def fit_forms(self, sigma2, forms, max_iterations=20, tol=0.0):
        """Fits every form of `forms`, a list of (kind, point_indices) with kind "plane", "sphere", "line", "circle" or FORM_*, to
        the current coordinates of its points with their whole block of the cofactor matrix (Gauss-Helmert model).  Returns a
        FormFits: parameters with sigma and Q_pp, Omega, f, T = Omega / (f sigma2), the members' corrections, distances, estimated
        gross errors and tests.  No quantile is evaluated."""
        kinds = np.ascontiguousarray([FORM_KINDS.get(k, k) for k, _ in forms], np.int32)
        members = [np.asarray(pts, np.int32).ravel() for _, pts in forms]
        begin = np.concatenate([[0], np.cumsum([g.size for g in members])]).astype(np.int32)
        points = np.ascontiguousarray(np.concatenate(members) if members else np.zeros(0), np.int32)
        n, M = len(forms), int(points.size)
        out = np.zeros((n, FORM_COLUMNS)); qpp = np.zeros((n, FORM_QPP_COLUMNS)); mem = np.zeros((max(M, 1), FORM_MEMBER_COLUMNS))
        status = np.zeros(n, np.int32); mstatus = np.zeros(max(M, 1), np.int32)
        ms = C.c_float(0.0)
        self._chk(self.L.jaicov_form_fit(self._h, float(sigma2), n, kinds.ctypes.data_as(_pi), begin.ctypes.data_as(_pi),
                                         points.ctypes.data_as(_pi), int(max_iterations), float(tol), _p(out), _p(qpp), _p(mem),
                                         status.ctypes.data_as(_pi), mstatus.ctypes.data_as(_pi), C.byref(ms)))
        return form_fits(out, qpp, mem[:M], status, mstatus[:M], begin, ms.value)

    # cylinders, cones and start values from the caller (include/jaicov_surfaces.h) -------------------------------------------------
    def fit_surfaces(self, sigma2, forms, start=None, max_iterations=20, tol=0.0):
        """fit_forms with the kinds "cylinder" and "cone" (SURF_*) beside the four forms, and with start values: `start` is None or
        one row per form (seven values, the reported parameters in the reported order and the engine's frame, whatever behind
        them); None in the place of a row, or a row that begins with NaN, lets that form find its own.  Returns a FormFits; a cone's
        seventh parameter is its half angle alpha."""
        kinds = np.ascontiguousarray([SURF_KINDS.get(k, k) for k, _ in forms], np.int32)
        members = [np.asarray(pts, np.int32).ravel() for _, pts in forms]
        begin = np.concatenate([[0], np.cumsum([g.size for g in members])]).astype(np.int32)
        points = np.ascontiguousarray(np.concatenate(members) if members else np.zeros(0), np.int32)
        n, M = len(forms), int(points.size)
        rows = None
        if start is not None:
            if len(start) != n:
                raise ValueError("start must have one row per form")
            rows = np.full((max(n, 1), FORM_MAX_PARAMS), np.nan)
            for g, row in enumerate(start):
                if row is not None:
                    row = np.asarray(row, np.float64).ravel()
                    rows[g, :min(row.size, FORM_MAX_PARAMS)] = row[:FORM_MAX_PARAMS]
        out = np.zeros((n, FORM_COLUMNS)); qpp = np.zeros((n, FORM_QPP_COLUMNS)); mem = np.zeros((max(M, 1), FORM_MEMBER_COLUMNS))
        status = np.zeros(n, np.int32); mstatus = np.zeros(max(M, 1), np.int32)
        ms = C.c_float(0.0)
        self._chk(self.L.jaicov_surf_fit(self._h, float(sigma2), n, kinds.ctypes.data_as(_pi), begin.ctypes.data_as(_pi),
                                         points.ctypes.data_as(_pi), None if rows is None else _p(rows), int(max_iterations), float(tol),
                                         _p(out), _p(qpp), _p(mem), status.ctypes.data_as(_pi), mstatus.ctypes.data_as(_pi), C.byref(ms)))
        return form_fits(out, qpp, mem[:M], status, mstatus[:M], begin, ms.value)

    # image space (include/jaicov_predict.h) ------------------------------------------------------------------------------------------
    def predict_image_points(self, sigma2, images, points, k2=1.0):
        """Where the adjusted object point points[i] appears in image images[i] (any pair of the problem, observed or not): the model's
        image coordinates at the current parameters, the 2 x 2 cofactor block J Qxx J', sigma_x and sigma_y, and the confidence
        ellipse with the expansion factor k2.  Needs INVERT_FULL or INVERT_FULL_EXPANDED.  Returns an ImagePrediction."""
        im = np.ascontiguousarray(images, np.int32).ravel(); pt = np.ascontiguousarray(points, np.int32).ravel()
        if im.size != pt.size:
            raise ValueError("images and points must run parallel")
        n = im.size
        out = np.zeros((n, PRED_POINT_COLUMNS)); status = np.zeros(n, np.int32)
        self._chk(self.L.jaicov_pred_points(self._h, float(sigma2), float(k2), im.ctypes.data_as(_pi), pt.ctypes.data_as(_pi), n, _p(out),
                                            status.ctypes.data_as(_pi)))
        return ImagePrediction(out[:, 0:2], out[:, 2:5], out[:, 5:7], out[:, 7:9], out[:, 9], status)

    def check_image_points(self, images, points, xy, var_x, var_y, rho=None, sigma2_post=None, groups=None):
        """Tests measurements xy (n, 2) that were withheld from the adjustment: d = l - f(x), M = Q_ll + J Qxx J', q = d' inv(M) d,
        T_prio = q / (2 s0) and T_post = q / (2 sigma2_post) per pair (sigma2_post None: the a-priori factor), and the joint test
        of every group of `groups` (lists of 1 .. 32 pair indices that together run 0 .. n - 1 in order, or a CSR array).  No
        quantile is evaluated.  Returns (ImageCheck, GroupCheck or None)."""
        im = np.ascontiguousarray(images, np.int32).ravel(); pt = np.ascontiguousarray(points, np.int32).ravel()
        n = im.size
        l = np.ascontiguousarray(np.asarray(xy, np.float64).reshape(-1, 2))
        disp = np.empty((n, 3))
        disp[:, 0] = var_x; disp[:, 1] = var_y; disp[:, 2] = 0.0 if rho is None else rho
        if pt.size != n or l.shape[0] != n:
            raise ValueError("images, points and xy must run parallel")
        if sigma2_post is None:
            sigma2_post = getattr(self, "_sigma2_build", self.fp.sigma2apriori)
        begin = None
        if groups is not None:
            if len(groups) and np.ndim(groups[0]) > 0:
                if [int(i) for g in groups for i in g] != list(range(n)):
                    raise ValueError("the groups must hold the pairs 0 .. n - 1 in order")
                begin = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
            else:
                begin = np.ascontiguousarray(groups, np.int32).ravel()
        G = 0 if begin is None else begin.size - 1
        out = np.zeros((n, PRED_CHECK_COLUMNS)); status = np.zeros(n, np.int32)
        gout = np.zeros((max(G, 1), PRED_GROUP_COLUMNS)); gstatus = np.zeros(max(G, 1), np.int32)
        self._chk(self.L.jaicov_pred_check(self._h, float(sigma2_post), im.ctypes.data_as(_pi), pt.ctypes.data_as(_pi), _p(l), _p(disp), n,
                                           None if begin is None else begin.ctypes.data_as(_pi), G, _p(out), status.ctypes.data_as(_pi),
                                           _p(gout), gstatus.ctypes.data_as(_pi)))
        pairs = ImageCheck(out[:, 0:2], out[:, 2:5], out[:, 5], out[:, 6], out[:, 7], status)
        if begin is None:
            return pairs, None
        return pairs, GroupCheck(gout[:G, 0], gout[:G, 1], gout[:G, 2], gout[:G, 3].astype(np.int32), gstatus[:G])

    # the camera in image space (include/jaicov_calibration.h) ---------------------------------------------------------------------------
    def calibration_field(self, sigma2, cameras, xy, depth=None, k2=1.0, columns=CALIB_ALL, jacobian=False):
        """The image correction of camera cameras[i] (a scalar: one camera for all) at the node xy[i] = (xs, ys), ideal coordinates
        relative to the principal point at the current c, with its 2 x 2 cofactor block over the camera's selected columns (`columns`:
        CALIB_PRINCIPAL_POINT, CALIB_PRINCIPAL_DISTANCE, 1 << (CALIB_KIND_SHIFT + kind), CALIB_ALL), sigmas, the confidence ellipse and
        the radial and tangential components.  The ray is held fixed.  depth None: N = -c (refused for a camera with D_i terms).  Any
        cofactor matrix serves, that of INVERT_REDUCED included.  Returns a CalibrationField."""
        l = np.ascontiguousarray(np.asarray(xy, np.float64).reshape(-1, 2))
        n = l.shape[0]
        cam = np.ascontiguousarray(cameras, np.int32).ravel()
        if cam.size == 1:
            cam = np.full(n, cam[0], np.int32)
        dep = None if depth is None else np.ascontiguousarray(np.broadcast_to(np.asarray(depth, np.float64), (n,)))
        if cam.size != n or (dep is not None and dep.size != n):
            raise ValueError("cameras, xy and depth must run parallel")
        out = np.zeros((n, CALIB_FIELD_COLUMNS)); status = np.zeros(n, np.int32)
        jac = np.zeros((n, 2, CALIB_MAX_COLUMNS)) if jacobian else None
        self._chk(self.L.jaicov_calib_field(self._h, float(sigma2), float(k2), int(columns), cam.ctypes.data_as(_pi), _p(l),
                                            None if dep is None else _p(dep), n, _p(out), None if jac is None else _p(jac),
                                            status.ctypes.data_as(_pi)))
        return CalibrationField(out[:, 0:2], out[:, 2:5], out[:, 5:7], out[:, 7:9], out[:, 9], out[:, 10:12], out[:, 12:14], status, jac)

    def calibration_compare(self, cam_a, cam_b, xy, depth=None, ref_values=None, ref_cov=None, sigma2_post=None, relative=False, nodes=True):
        """The difference field d = g_a - g_b of two calibrations at the nodes xy (ideal coordinates at camera cam_a's current c, the
        same ray for both sides) with its cofactor block C_d, q = d' inv(C_d) d, T_prio and T_post.  Side B is camera cam_b of this
        engine, or with ref_values (x0, y0, c, then the coefficients of cam_b's table) a certificate or an earlier epoch, ref_cov its
        covariance.  relative: positions relative to each side's own principal point.  The summary (CalibrationSummary) is formed on
        the device; nodes=False returns it alone.  sigma2_post None: the a-priori factor.  Returns a CalibrationCompare."""
        l = np.ascontiguousarray(np.asarray(xy, np.float64).reshape(-1, 2))
        n = l.shape[0]
        dep = None if depth is None else np.ascontiguousarray(np.broadcast_to(np.asarray(depth, np.float64), (n,)))
        if dep is not None and dep.size != n:
            raise ValueError("xy and depth must run parallel")
        ref = None if ref_values is None else np.ascontiguousarray(ref_values, np.float64).ravel()
        cov = None if ref_cov is None else np.ascontiguousarray(ref_cov, np.float64)
        if ref is not None:
            K = 3 + int(self.fp.cam_dist_begin[cam_b + 1] - self.fp.cam_dist_begin[cam_b]) if 0 <= cam_b < self.fp.n_cameras else ref.size
            if ref.size != K or (cov is not None and cov.shape != (K, K)):
                raise ValueError("ref_values holds x0, y0, c and the coefficients of camera cam_b, ref_cov their covariance")
        if sigma2_post is None:
            sigma2_post = getattr(self, "_sigma2_build", self.fp.sigma2apriori)
        out = np.zeros((n, CALIB_COMPARE_COLUMNS)) if nodes else None
        status = np.zeros(n, np.int32) if nodes else None
        summ = np.zeros(CALIB_SUMMARY_COLUMNS)
        self._chk(self.L.jaicov_calib_compare(self._h, float(sigma2_post), int(cam_a), int(cam_b), None if ref is None else _p(ref),
                                              None if cov is None else _p(cov), CALIB_RELATIVE if relative else 0, _p(l),
                                              None if dep is None else _p(dep), n, None if out is None else _p(out),
                                              None if status is None else status.ctypes.data_as(_pi), _p(summ)))
        summary = CalibrationSummary(int(summ[0]), summ[1], summ[2], summ[3], int(summ[4]), summ[5], int(summ[6]), int(summ[7]))
        if not nodes:
            return CalibrationCompare(None, None, None, None, None, None, summary)
        return CalibrationCompare(out[:, 0:2], out[:, 2:5], out[:, 5], out[:, 6], out[:, 7], status, summary)

    def calibration_release(self):
        """Frees the work buffers of the calibration calls."""
        self._chk(self.L.jaicov_calib_release(self._h))

    # object space (include/jaicov_newpoints.h) -------------------------------------------------------------------------------------
    def new_point_start_values(self, ray_begin, ray_image, xy, disp):
        """Start values (n, 3) of new points for intersect_new_points: the measurements reduced to the distortion-free camera
        (lens_correct, the distance-dependent coefficients left out) and intersected with the current orientations
        (intersect_points).  NaN where that intersection fails."""
        fp = self.fp
        rb = np.ascontiguousarray(ray_begin, np.int32).ravel(); ri = np.ascontiguousarray(ray_image, np.int32).ravel()
        if rb.size < 2 or ri.size == 0:
            return np.full((max(rb.size - 1, 0), 3), np.nan)
        v = self.get_parameters()
        io = v[fp.slot_io(0):fp.slot_io(0) + 3 * fp.n_cameras].reshape(-1, 3)
        tables = lens_tables_without_distance(fp.cam_dist_begin, fp.dist_kind, fp.dist_order, v[fp.slot_dist(0):fp.slot_dist(0) + fp.n_dist])
        cam = np.asarray(fp.image_camera)[ri]
        l = np.asarray(xy, np.float64).reshape(-1, 2); dv = np.asarray(disp, np.float64).reshape(-1, 3)
        cxy, cvar, lst = lens_correct(l, cam, io, fp.cam_r0, *tables, var=dv)[:3]
        ok = lst <= LENS_NOT_CONVERGED
        cxy = np.where(ok[:, None], cxy, l); cvar = np.where(ok[:, None], cvar, dv)
        out, st = intersect_points(rb, ri, cxy, cvar, io[np.asarray(fp.image_camera)], v[fp.slot_eo(0):].reshape(-1, 6),
                                   sigma2apriori=getattr(self, "_sigma2_build", fp.sigma2apriori), min_rays=2)[:2]
        return np.where((st <= ISECT_NOT_CONVERGED)[:, None], out[:, :3], np.nan)

    def intersect_new_points(self, sigma2, ray_begin, ray_image, xy, disp, start=None, pairs=None, max_iterations=20):
        """Object points that were not part of the adjustment, from measurements xy (n_rays, 2) with the dispersions disp (n_rays, 3:
        var_x, var_y, rho) in the images ray_image of the adjusted block; ray_begin (n + 1,) is the CSR of the points' rays.  The model
        is the adjustment's own rows; the cofactors carry the share of the cameras and stations from Qxx (cof), beside the
        measurement noise alone (cof_meas).  start None: new_point_start_values.  pairs (n_pairs, 2): lengths between two new points
        (members >= 0) or a new point and object point P of the block (member -1 - P), with their correlations.  Needs INVERT_FULL or
        INVERT_FULL_EXPANDED.  Returns a NewPoints."""
        rb = np.ascontiguousarray(ray_begin, np.int32).ravel(); ri = np.ascontiguousarray(ray_image, np.int32).ravel()
        n = max(rb.size - 1, 0); R = ri.size
        l = np.ascontiguousarray(np.asarray(xy, np.float64).reshape(-1, 2)); dv = np.ascontiguousarray(np.asarray(disp, np.float64).reshape(-1, 3))
        if l.shape[0] != R or dv.shape[0] != R or (rb.size and rb[-1] != R):
            raise ValueError("ray_image, xy and disp must run parallel, and ray_begin must end at their number")
        x0 = self.new_point_start_values(rb, ri, l, dv) if start is None else np.asarray(start, np.float64).reshape(-1, 3)
        x0 = np.ascontiguousarray(x0)
        if x0.shape[0] != n:
            raise ValueError("one start value per point")
        pr = np.zeros((0, 2), np.int32) if pairs is None else np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        G = pr.shape[0]
        out = np.zeros((n, NEWPT_COLUMNS)); status = np.zeros(n, np.int32); iters = np.zeros(n, np.int32); rw = np.zeros((R, 2))
        pout = np.zeros((max(G, 1), NEWPT_PAIR_COLUMNS)); pst = np.zeros(max(G, 1), np.int32)
        self._chk(self.L.jaicov_newpt_intersect(self._h, float(sigma2), n, rb.ctypes.data_as(_pi), ri.ctypes.data_as(_pi), _p(l), _p(dv), _p(x0),
                                                int(max_iterations), pr.ctypes.data_as(_pi), G, _p(out), status.ctypes.data_as(_pi),
                                                iters.ctypes.data_as(_pi), _p(rw), _p(pout), pst.ctypes.data_as(_pi)))
        return NewPoints(out[:, 0:3], out[:, 3:9], out[:, 9:15], out[:, 17:20], out[:, 15], out[:, 16], status, iters, rw, pout[:G], pst[:G])

    def get_rows(self, ip_begin, ip_count):
        w = np.zeros((ip_count, 2)); A = np.zeros((ip_count, 2, KROW))
        self._chk(self.L.jaicov_neq_get_rows(self._h, ip_begin, ip_count, _p(w), _p(A)))
        return w, A

    def timings(self):
        ms = np.zeros(8)
        self._chk(self.L.jaicov_neq_last_timings(self._h, _p(ms), 8))
        return dict(zip(("rows", "assembly", "finalize", "factor", "solve", "inverse", "omega", "total"), ms))

    def create_timings(self):
        """What jaicov_neq_create spent, ms of host wall clock."""
        ms = np.zeros(8)
        self._chk(self.L.jaicov_neq_create_timings(self._h, _p(ms), 8))
        return {"create_ms": float(ms[0]), "dispersion_upload_host_ms": float(ms[1]), "dispersions_to_weights_ms": float(ms[2]),
                "tables_and_structure_upload_ms": float(ms[3]), "work_buffers_and_solver_ms": float(ms[4]), "elimination_buffers_and_reduced_solver_ms": float(ms[5])}

    def get_block_weight(self, block):
        """inv(D) of image block `block` as cached at create (DOPG:82-86 caches sigma0^2 times it), caller's observation order."""
        m = 2 * int(self.fp.blk_ip_begin[block + 1] - self.fp.blk_ip_begin[block])
        out = np.zeros((m, m))
        self._chk(self.L.jaicov_neq_get_block_weight(self._h, int(block), _p(out), out.size))
        return out

    def set_profiling(self, on=True):
        self._chk(self.L.jaicov_neq_set_profiling(self._h, int(on)))

    def kernel_stats(self, reset=False):
        st = np.zeros(13)
        self._chk(self.L.jaicov_neq_kernel_stats(self._h, _p(st), 13, int(reset)))
        return {"launches": st[0], "ms": st[1], "flops": st[2], "dense_passes": st[3], "dense_gemm_ms": st[4], "dense_flops": st[5],
                "flow_retries": int(st[6]), "flow_stale_events": int(st[7]), "flow_stale_confirmed": int(st[8]),
                "flow_rescued": int(st[9]), "last_refinement_correction": float(st[10]), "refine_steps": int(st[11]), "gather_strip_columns": int(st[12])}

    def cancel(self):
        """``BundleAdjustment.interrupt()`` (BundleAdjustment.java:1455): the running / next ``estimate`` ends with state -1."""
        self._chk(self.L.jaicov_neq_cancel(self._h))

    def estimate(self, values=None, sigma2=None, lam0=0.0, max_iter=5000, invert=True, simulation=False):
        """``BundleAdjustment.estimateModel()`` (BundleAdjustment.java:203-387) run natively on the engine."""
        self.set_parameters(self.fp.values if values is None else values)
        o = EstimateOptions()
        o.struct_size = C.sizeof(EstimateOptions)
        o.max_iterations = max_iter; o.invert = int(invert); o.simulation = int(simulation)
        o.lambda0 = lam0; o.sigma2apriori = self.fp.sigma2apriori if sigma2 is None else sigma2
        self._sigma2_build = float(o.sigma2apriori)
        res = EstimateResult()
        self._chk(self.L.jaicov_neq_estimate(self._h, C.byref(o), C.byref(res)))
        return self.get_parameters(), res


def sensor_grid(width, height, nx, ny):
    """nx x ny nodes (nx ny, 2) over a sensor of width x height about the principal point, row by row from (-width / 2, -height / 2):
    the nodes of Engine.calibration_field and calibration_compare"""
    gx, gy = np.meshgrid(np.linspace(-0.5 * width, 0.5 * width, int(nx)), np.linspace(-0.5 * height, 0.5 * height, int(ny)))
    return np.column_stack([gx.ravel(), gy.ravel()])


def radial_profile(rmax, n, azimuth=0.0):
    """n nodes (n, 2) at the radii rmax / n, 2 rmax / n, .., rmax along the direction `azimuth` (radians from +x towards +y)"""
    r = rmax * np.arange(1, int(n) + 1) / int(n)
    return np.column_stack([r * np.cos(azimuth), r * np.sin(azimuth)])


def vce_groups(fp: FlatProblem, by="kind") -> VceGroups:
    """Groups for Engine.variance_components.  by = "kind": image points / scale bars / directly observed rows (three groups, some
    perhaps empty); "camera": the image points of every camera; "image": the image points of every image; "direct_group": every
    directly observed group on its own."""
    n_ip, n_sb, n_dg = fp.n_image_points, fp.n_scale_bars, fp.n_direct_groups
    if by == "kind":
        return VceGroups(np.zeros(n_ip, np.int32), np.full(n_sb, 1, np.int32), np.full(n_dg, 2, np.int32), 3,
                         ["image points", "scale bars", "direct rows"])
    if by == "camera":
        return VceGroups(fp.image_camera[fp.ip_image].astype(np.int32), None, None, fp.n_cameras, [f"camera {c}" for c in range(fp.n_cameras)])
    if by == "image":
        return VceGroups(fp.ip_image.astype(np.int32), None, None, fp.n_images, [f"image {i}" for i in range(fp.n_images)])
    if by == "direct_group":
        if n_dg == 0:
            raise ValueError("the problem has no directly observed groups")
        return VceGroups(None, None, np.arange(n_dg, dtype=np.int32), n_dg, [f"direct group {g}" for g in range(n_dg)])
    raise ValueError(f"by must be 'kind', 'camera', 'image' or 'direct_group', not {by!r}")


def estimate_variance_components(fp: FlatProblem, groups, tol=0.05, max_iter=10, values=None, lam0=0.0, max_estimate_iter=5000,
                                 **engine_kw) -> VceEstimate:
    """Iterated variance component estimation.  Per iteration: a FRESH engine from the problem (the weights are cached when an
    engine is created, so scaled dispersions need a new one), estimate() from the last parameter values with the full inverse,
    variance_components(groups), and the dispersions of every group multiplied by its k (problem.scale_dispersions).  Stops when
    max |k_g - 1| <= tol over the groups with a finite k, or after max_iter iterations.  A group whose k is NaN (empty, not
    controlled) keeps its factor.  Returns a VceEstimate; its engine is the last one and stays open."""
    from .problem import scale_dispersions
    factors = np.ones(int(groups.n_groups))
    tables = []
    vals = fp.values if values is None else values
    eng, converged, k = None, False, None
    for _ in range(max_iter):
        if eng is not None:
            eng.close()
            fp = scale_dispersions(fp, groups, k)
        eng = Engine(fp, **engine_kw)
        vals, _res = eng.estimate(values=vals, lam0=lam0, max_iter=max_estimate_iter, invert=INVERT_FULL)
        vc = eng.variance_components(groups)
        tables.append(vc)
        k = np.where(np.isfinite(vc.k), vc.k, 1.0)
        factors = factors * k
        if np.max(np.abs(k - 1.0)) <= tol:
            converged = True
            break
    return VceEstimate(factors, tables, eng, fp, converged)


def point_column_range(fp: FlatProblem):
    """Engine.point_column_range for a problem (no device needed)."""
    seen = np.zeros(fp.n_points, bool)
    seen[np.asarray(fp.ip_point)] = True
    cols = np.asarray(fp.point_col).reshape(-1, 3)[seen].ravel()
    cols = np.sort(cols[cols >= 0])
    if cols.size == 0 or cols[-1] - cols[0] + 1 != cols.size:
        raise ValueError("the columns of the image-observed points are not one contiguous range")
    return int(cols[0]), int(cols.size)


def form_fits(out, qpp, mem, status, mstatus, begin, kernel_ms=0.0):
    """The tables of jaicov_form_fit as a FormFits"""
    n = out.shape[0]
    full = np.zeros((n, FORM_MAX_PARAMS, FORM_MAX_PARAMS))
    iu = np.triu_indices(FORM_MAX_PARAMS)
    full[:, iu[0], iu[1]] = qpp
    full[:, iu[1], iu[0]] = qpp
    return FormFits(out[:, 0:7], out[:, 7:14], full, out[:, 14], out[:, 15], out[:, 16], out[:, 17], out[:, 18], out[:, 19], status,
                    np.asarray(begin), mem[:, 0:3], mem[:, 3], mem[:, 4:6], mem[:, 6], mstatus, kernel_ms)


def column_names(fp: FlatProblem):
    """The ColumnName (class name, item, component) of every column of the full cofactor matrix from the flat problem (no device
    needed): ("point", p, "X"), ("interior", camera, "x0"), ("distortion", camera, index within the camera's coefficients),
    ("exterior", image, "omega"); a border column is ("border", row, "")."""
    names = [ColumnName("border", c, "") for c in range(fp.n_unknowns)]
    for p in range(fp.n_points):
        for k in range(3):
            if fp.point_col[p, k] >= 0:
                names[fp.point_col[p, k]] = ColumnName("point", p, "XYZ"[k])
    for c in range(fp.n_cameras):
        for k in range(3):
            if fp.io_col[c, k] >= 0:
                names[fp.io_col[c, k]] = ColumnName("interior", c, ("x0", "y0", "c")[k])
        for j in range(int(fp.cam_dist_begin[c]), int(fp.cam_dist_begin[c + 1])):
            if fp.dist_col[j] >= 0:
                names[fp.dist_col[j]] = ColumnName("distortion", c, j - int(fp.cam_dist_begin[c]))
    for i in range(fp.n_images):
        for k in range(6):
            if fp.eo_col[i, k] >= 0:
                names[fp.eo_col[i, k]] = ColumnName("exterior", i, ("X0", "Y0", "Z0", "omega", "phi", "kappa")[k])
    return names


def dense_spd_solve_packed(ap, b=None, invert=False):
    """MathExtension.solve(UpperSPDPackMatrix ...) / MathExtension.inv on the device.  Returns (x, ap_out, ms)."""
    L = load_library()
    ap = np.ascontiguousarray(ap, np.float64).copy()
    n = int(round((np.sqrt(8 * ap.size + 1) - 1) / 2))
    nrhs = 0
    if b is not None:
        b = np.ascontiguousarray(np.atleast_2d(b), np.float64).copy()
        nrhs = b.shape[0]
    ms = np.zeros(1)
    rc = L.jaicov_dense_spd_solve_packed(n, _p(ap), _p(b) if b is not None else C.cast(None, _pd), nrhs, int(invert), _p(ms))
    if rc != 0:
        raise EngineError(rc, "dense SPD solve")
    return b, ap, float(ms[0])


def dlt_adjust(obs_begin, xy, xyz, io, io_fixed=None, restrictions=(), max_iterations=5000, with_time=False):
    """DirectLinearTransformation.adjust for every image at once (include/jaicov_dlt.h).  obs_begin: (n + 1,) CSR offsets of the
    images' homologous points; xy: (n_obs, 2) image coordinates; xyz: (n_obs, 3) their control coordinates; io: (n, 3) x0, y0, c;
    io_fixed: (n, 3) bool or None; restrictions: jaicov_dlt_restriction ids in order (duplicates allowed).  Returns
    (out (n, 20): b11..b33, x0, y0, c, X0, Y0, Z0, omega, phi, kappa; status (n,); solves (n,)), plus the kernel time in ms with
    with_time."""
    L = load_library()
    ob = np.ascontiguousarray(obs_begin, np.int32).ravel()
    n = ob.size - 1
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1)
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1)
    io = np.ascontiguousarray(io, np.float64).reshape(-1)
    fx = None if io_fixed is None else np.ascontiguousarray(io_fixed, np.uint8).reshape(-1)
    rs = np.ascontiguousarray(restrictions, np.int32).ravel()
    out = np.zeros((max(n, 0), 20)); status = np.zeros(max(n, 0), np.int32); solves = np.zeros(max(n, 0), np.int32)
    ms = np.zeros(1)
    _pu8 = C.POINTER(C.c_uint8)
    rc = L.jaicov_dlt_adjust(n, ob.ctypes.data_as(_pi), _p(xy), _p(xyz), _p(io),
                             fx.ctypes.data_as(_pu8) if fx is not None else C.cast(None, _pu8),
                             rs.ctypes.data_as(_pi) if rs.size else C.cast(None, _pi), rs.size, int(max_iterations),
                             _p(out), status.ctypes.data_as(_pi), solves.ctypes.data_as(_pi), _p(ms))
    if rc != 0:
        raise EngineError(rc, "dlt adjust")
    return (out, status, solves, float(ms[0])) if with_time else (out, status, solves)


def intersect_points(ray_begin, ray_image, xy, var, image_io, image_eo, sigma2apriori=1.0, max_iterations=50, reject_threshold=0.0,
                     min_rays=3, with_time=False):
    """Forward intersection of every point of a batch from its image rays (include/jaicov_intersect.h).  ray_begin: (n + 1,) CSR
    offsets of the points' rays; ray_image: (n_rays,) image of each ray; xy: (n_rays, 2); var: (n_rays, 3) var_x, var_y, rho or None
    (unit weights); image_io: (n_images, 3) x0, y0, c of each image's camera; image_eo: (n_images, 6).  Returns (out (n, 11): X, Y, Z,
    qXX, qXY, qXZ, qYY, qYZ, qZZ, Omega, largest angle; status (n,); iterations (n,); ray_used (n_rays,); ray_q (n_rays,)), plus the
    kernel time in ms with with_time."""
    L = load_library()
    rb = np.ascontiguousarray(ray_begin, np.int32).ravel()
    n = rb.size - 1
    ri = np.ascontiguousarray(ray_image, np.int32).ravel()
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1)
    var = None if var is None else np.ascontiguousarray(var, np.float64).reshape(-1)
    io = np.ascontiguousarray(image_io, np.float64).reshape(-1)
    eo = np.ascontiguousarray(image_eo, np.float64).reshape(-1)
    if io.size % 3 or eo.size != 2 * io.size or 2 * ri.size != xy.size or (var is not None and 3 * ri.size != var.size) or \
            (n >= 0 and rb.size and rb[-1] != ri.size):
        raise EngineError(-1, "intersect points: array sizes do not agree")
    out = np.zeros((max(n, 0), 11)); status = np.zeros(max(n, 0), np.int32); iterations = np.zeros(max(n, 0), np.int32)
    used = np.zeros(ri.size, np.uint8); q = np.zeros(ri.size)
    ms = np.zeros(1)
    rc = L.jaicov_isect_points(n, rb.ctypes.data_as(_pi), ri.ctypes.data_as(_pi), _p(xy), _p(var) if var is not None else C.cast(None, _pd),
                               io.size // 3, _p(io), _p(eo), float(sigma2apriori), int(max_iterations), float(reject_threshold),
                               int(min_rays), _p(out), status.ctypes.data_as(_pi), iterations.ctypes.data_as(_pi),
                               used.ctypes.data_as(C.POINTER(C.c_uint8)), _p(q), _p(ms))
    if rc != 0:
        raise EngineError(rc, "intersect points")
    return (out, status, iterations, used, q) + ((float(ms[0]),) if with_time else ())


def intersect_problem(fp: FlatProblem, values=None, with_status=False, **kw):
    """Start values of a FlatProblem's object points by forward intersection: the rays of every point are its image points in the
    problem's order (a stable sort of ip_point) with their ip_var_x, ip_var_y, ip_rho; interior and exterior orientation come from
    the slot vector `values` (default fp.values).  Returns the slot vector with every intersected point replaced (a point whose status
    is TOO_FEW_RAYS, SINGULAR or NOT_FINITE keeps its value); with_status also (out, status).  kw: as intersect_points
    (sigma2apriori defaults to the problem's)."""
    v = np.array(fp.values if values is None else values, np.float64)
    order = np.argsort(fp.ip_point, kind="stable")
    begin = np.concatenate([[0], np.cumsum(np.bincount(fp.ip_point, minlength=fp.n_points))]).astype(np.int32)
    io = v[3 * fp.n_points:3 * fp.n_points + 3 * fp.n_cameras].reshape(-1, 3)[fp.image_camera]
    eo = v[fp.slot_eo(0):].reshape(-1, 6)
    var = np.stack([fp.ip_var_x, fp.ip_var_y, fp.ip_rho], 1)[order]
    kw.setdefault("sigma2apriori", fp.sigma2apriori)
    out, status, _, _, _ = intersect_points(begin, fp.ip_image[order], np.stack([fp.ip_x, fp.ip_y], 1)[order], var, io, eo, **kw)
    ok = status <= ISECT_NOT_CONVERGED
    v[:3 * fp.n_points].reshape(-1, 3)[ok] = out[ok, :3]
    return (v, out, status) if with_status else v


def resect_images(obs_begin, xy, xyz, var, image_io, eo_start=None, sigma2apriori=1.0, max_iterations=50, reject_threshold=0.0,
                  min_points=4, with_time=False):
    """Spatial resection of every image of a batch from its known object points (include/jaicov_resect.h).  obs_begin: (n + 1,) CSR
    offsets of the images' observations; xy: (n_obs, 2); xyz: (n_obs, 3) the object point of each observation; var: (n_obs, 3) var_x,
    var_y, rho or None (unit weights); image_io: (n, 3) x0, y0, c of each image's camera; eo_start: (n, 6) or None, an image whose six
    values are all finite starts from them, any other from the linear start.  Returns (out (n, 28): X0, Y0, Z0, omega, phi, kappa, the
    21 entries of the upper triangle of Q, Omega; status (n,); iterations (n,); start_kind (n,); obs_used (n_obs,); obs_q (n_obs,)),
    plus the kernel time in ms with with_time."""
    L = load_library()
    ob = np.ascontiguousarray(obs_begin, np.int32).ravel()
    n = ob.size - 1
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1)
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1)
    var = None if var is None else np.ascontiguousarray(var, np.float64).reshape(-1)
    io = np.ascontiguousarray(image_io, np.float64).reshape(-1)
    eo = None if eo_start is None else np.ascontiguousarray(eo_start, np.float64).reshape(-1)
    n_obs = xy.size // 2
    if xy.size % 2 or xyz.size != 3 * n_obs or (var is not None and var.size != 3 * n_obs) or io.size != 3 * max(n, 0) or \
            (eo is not None and eo.size != 6 * max(n, 0)) or (ob.size and ob[-1] != n_obs):
        raise EngineError(-1, "resect images: array sizes do not agree")
    out = np.zeros((max(n, 0), 28)); status = np.zeros(max(n, 0), np.int32); iterations = np.zeros(max(n, 0), np.int32)
    kind = np.zeros(max(n, 0), np.int32); used = np.zeros(n_obs, np.uint8); q = np.zeros(n_obs)
    ms = np.zeros(1)
    null = C.cast(None, _pd)
    rc = L.jaicov_resect_images(n, ob.ctypes.data_as(_pi), _p(xy), _p(xyz), _p(var) if var is not None else null, _p(io),
                                _p(eo) if eo is not None else null, float(sigma2apriori), int(max_iterations), float(reject_threshold),
                                int(min_points), _p(out), status.ctypes.data_as(_pi), iterations.ctypes.data_as(_pi),
                                kind.ctypes.data_as(_pi), used.ctypes.data_as(C.POINTER(C.c_uint8)), _p(q), _p(ms))
    if rc != 0:
        raise EngineError(rc, "resect images")
    return (out, status, iterations, kind, used, q) + ((float(ms[0]),) if with_time else ())


def resect_problem(fp: FlatProblem, values=None, with_status=False, **kw):
    """Start values of a FlatProblem's exterior orientations by spatial resection: the observations of every image are its image
    points in the problem's order (a stable sort of ip_image) with their ip_var_x, ip_var_y, ip_rho; the object points and the
    interior orientation come from the slot vector `values` (default fp.values).  Returns the slot vector with the orientation of
    every resected image replaced (an image whose status is TOO_FEW_POINTS, SINGULAR or NOT_FINITE keeps its values); with_status
    also (out, status).  kw: as resect_images (sigma2apriori defaults to the problem's)."""
    v = np.array(fp.values if values is None else values, np.float64)
    order = np.argsort(fp.ip_image, kind="stable")
    begin = np.concatenate([[0], np.cumsum(np.bincount(fp.ip_image, minlength=fp.n_images))]).astype(np.int32)
    io = v[3 * fp.n_points:3 * fp.n_points + 3 * fp.n_cameras].reshape(-1, 3)[fp.image_camera]
    xyz = v[:3 * fp.n_points].reshape(-1, 3)[np.asarray(fp.ip_point)[order]]
    var = np.stack([fp.ip_var_x, fp.ip_var_y, fp.ip_rho], 1)[order]
    kw.setdefault("sigma2apriori", fp.sigma2apriori)
    out, status = resect_images(begin, np.stack([fp.ip_x, fp.ip_y], 1)[order], xyz, var, io, **kw)[:2]
    ok = status <= RESECT_NOT_CONVERGED
    v[fp.slot_eo(0):].reshape(-1, 6)[ok] = out[ok, :6]
    return (v, out, status) if with_status else v


def relorient_pairs(obs_begin, xy_a, xy_b, var_a, var_b, pair_io, start=None, sigma2apriori=1.0, max_iterations=50, reject_threshold=0.0,
                    min_points=6, with_time=False):
    """Relative orientation of every image pair of a batch from its common image points (include/jaicov_relorient.h).  obs_begin:
    (n + 1,) CSR offsets of the pairs' observations; xy_a, xy_b: (n_obs, 2) the image point of observation k in image a and in image
    b; var_a, var_b: (n_obs, 3) var_x, var_y, rho or None; pair_io: (n, 6) x0, y0, c of image a's camera, then of image b's; start:
    (n, 6) or None, a pair whose six values are all finite starts from them, any other from the linear starts.  Returns (out (n, 28):
    X0, Y0, Z0 (unit length), omega, phi, kappa of image b in the frame of image a, the 21 entries of the upper triangle of their
    cofactor matrix, Omega; status (n,); iterations (n,); start_kind (n,); obs_used (n_obs,); obs_q (n_obs,)), plus the kernel time
    in ms with with_time."""
    L = load_library()
    ob = np.ascontiguousarray(obs_begin, np.int32).ravel()
    n = ob.size - 1
    xa = np.ascontiguousarray(xy_a, np.float64).reshape(-1)
    xb = np.ascontiguousarray(xy_b, np.float64).reshape(-1)
    va = None if var_a is None else np.ascontiguousarray(var_a, np.float64).reshape(-1)
    vb = None if var_b is None else np.ascontiguousarray(var_b, np.float64).reshape(-1)
    io = np.ascontiguousarray(pair_io, np.float64).reshape(-1)
    st = None if start is None else np.ascontiguousarray(start, np.float64).reshape(-1)
    n_obs = xa.size // 2
    if xa.size % 2 or xb.size != xa.size or (va is not None and va.size != 3 * n_obs) or (vb is not None and vb.size != 3 * n_obs) or \
            io.size != 6 * max(n, 0) or (st is not None and st.size != 6 * max(n, 0)) or (ob.size and ob[-1] != n_obs):
        raise EngineError(-1, "relorient pairs: array sizes do not agree")
    out = np.zeros((max(n, 0), 28)); status = np.zeros(max(n, 0), np.int32); iterations = np.zeros(max(n, 0), np.int32)
    kind = np.zeros(max(n, 0), np.int32); used = np.zeros(n_obs, np.uint8); q = np.zeros(n_obs)
    ms = np.zeros(1)
    null = C.cast(None, _pd)
    rc = L.jaicov_relorient_pairs(n, ob.ctypes.data_as(_pi), _p(xa), _p(xb), _p(va) if va is not None else null,
                                  _p(vb) if vb is not None else null, _p(io), _p(st) if st is not None else null, float(sigma2apriori),
                                  int(max_iterations), float(reject_threshold), int(min_points), _p(out), status.ctypes.data_as(_pi),
                                  iterations.ctypes.data_as(_pi), kind.ctypes.data_as(_pi), used.ctypes.data_as(C.POINTER(C.c_uint8)),
                                  _p(q), _p(ms))
    if rc != 0:
        raise EngineError(rc, "relorient pairs")
    return (out, status, iterations, kind, used, q) + ((float(ms[0]),) if with_time else ())


def relorient_problem(fp: FlatProblem, image_a, image_b, base_length=1.0, values=None, with_status=False, **kw):
    """Start values of two exterior orientations of a FlatProblem by relative orientation: the observations are the image points of the
    object points both images see, in rising point number, with their ip_var_x, ip_var_y, ip_rho; the interior orientations come from
    the slot vector `values` (default fp.values).  Returns the slot vector with image a at the origin with zero angles and image b at
    the result, its X0 times base_length (a pair whose status is TOO_FEW_POINTS, SINGULAR or NOT_FINITE keeps both images' values);
    with_status also (out (28,), status).  kw: as relorient_pairs (sigma2apriori defaults to the problem's)."""
    v = np.array(fp.values if values is None else values, np.float64)
    img, pt = np.asarray(fp.ip_image), np.asarray(fp.ip_point)
    ia, ib = np.flatnonzero(img == image_a), np.flatnonzero(img == image_b)
    _, ja, jb = np.intersect1d(pt[ia], pt[ib], return_indices=True)
    ia, ib = ia[ja], ib[jb]
    cam = v[3 * fp.n_points:3 * fp.n_points + 3 * fp.n_cameras].reshape(-1, 3)[fp.image_camera]
    xy = np.stack([fp.ip_x, fp.ip_y], 1)
    var = np.stack([fp.ip_var_x, fp.ip_var_y, fp.ip_rho], 1)
    kw.setdefault("sigma2apriori", fp.sigma2apriori)
    out, status = relorient_pairs([0, ia.size], xy[ia], xy[ib], var[ia], var[ib], np.concatenate([cam[image_a], cam[image_b]]), **kw)[:2]
    if status[0] <= RELOR_NOT_CONVERGED:
        eo = v[fp.slot_eo(0):].reshape(-1, 6)
        eo[image_a] = 0.0
        eo[image_b, :3] = base_length * out[0, :3]
        eo[image_b, 3:] = out[0, 3:6]
    return (v, out[0], int(status[0])) if with_status else v


def similarity_models(pt_begin, src, dst, cof_src=None, cof_dst=None, start=None, max_iterations=50, reject_threshold=0.0, min_points=3,
                      with_time=False):
    """Absolute orientation of every model of a batch: the similarity transformation dst = T + m R src between two sets of the same
    points (include/jaicov_simil.h).  pt_begin: (n + 1,) CSR offsets of the models' points; src, dst: (n_pts, 3) the point in the
    model's frame and in the target frame; cof_src, cof_dst: (n_pts, 6) qXX qXY qXZ qYY qYZ qZZ or None (0 and I); start: (n, 7) Tx Ty
    Tz m omega phi kappa or None, a model whose seven values are all finite starts from them, any other from the closed start.
    Returns (out (n, 36): Tx, Ty, Tz, m, omega, phi, kappa, the 28 entries of the upper triangle of their cofactor matrix, Omega;
    status (n,); iterations (n,); start_kind (n,); pt_used (n_pts,); pt_q (n_pts,)), plus the kernel time in ms with with_time."""
    L = load_library()
    pb = np.ascontiguousarray(pt_begin, np.int32).ravel()
    n = pb.size - 1
    s = np.ascontiguousarray(src, np.float64).reshape(-1)
    d = np.ascontiguousarray(dst, np.float64).reshape(-1)
    qs = None if cof_src is None else np.ascontiguousarray(cof_src, np.float64).reshape(-1)
    qd = None if cof_dst is None else np.ascontiguousarray(cof_dst, np.float64).reshape(-1)
    st = None if start is None else np.ascontiguousarray(start, np.float64).reshape(-1)
    n_pts = s.size // 3
    if s.size % 3 or d.size != s.size or (qs is not None and qs.size != 6 * n_pts) or (qd is not None and qd.size != 6 * n_pts) or \
            (st is not None and st.size != 7 * max(n, 0)) or (pb.size and pb[-1] != n_pts):
        raise EngineError(-1, "similarity models: array sizes do not agree")
    out = np.zeros((max(n, 0), 36)); status = np.zeros(max(n, 0), np.int32); iterations = np.zeros(max(n, 0), np.int32)
    kind = np.zeros(max(n, 0), np.int32); used = np.zeros(n_pts, np.uint8); q = np.zeros(n_pts)
    ms = np.zeros(1)
    null = C.cast(None, _pd)
    rc = L.jaicov_simil_models(n, pb.ctypes.data_as(_pi), _p(s), _p(d), _p(qs) if qs is not None else null,
                               _p(qd) if qd is not None else null, _p(st) if st is not None else null, int(max_iterations),
                               float(reject_threshold), int(min_points), _p(out), status.ctypes.data_as(_pi),
                               iterations.ctypes.data_as(_pi), kind.ctypes.data_as(_pi), used.ctypes.data_as(C.POINTER(C.c_uint8)),
                               _p(q), _p(ms))
    if rc != 0:
        raise EngineError(rc, "similarity models")
    return (out, status, iterations, kind, used, q) + ((float(ms[0]),) if with_time else ())


def similarity_apply(par, pt_begin, xyz, cof=None, img_begin=None, eo=None):
    """Carries the points and the image orientations of every model into the target frame (include/jaicov_simil.h).  par: (n, 7) or
    the (n, 36) output of similarity_models; pt_begin: (n + 1,) CSR offsets of the models' points or None, with xyz (n_pts, 3) and cof
    (n_pts, 6) or None; img_begin: (n + 1,) CSR offsets of the models' images or None, with eo (n_img, 6).  Returns (xyz, cof, eo) in
    the target frame, None where the input was.  The dispersion of the seven parameters is not propagated."""
    L = load_library()
    par = np.asarray(par, np.float64)
    par = np.ascontiguousarray(par.reshape(-1, par.shape[-1] if par.ndim > 1 else 7)[:, :7]).reshape(-1)
    n = par.size // 7
    null, nulli = C.cast(None, _pd), C.cast(None, _pi)

    def ranges(begin, values, width, what):
        if begin is None:
            if values is not None:
                raise EngineError(-1, f"similarity apply: {what} without their ranges")
            return None, None
        b = np.ascontiguousarray(begin, np.int32).ravel()
        v = np.ascontiguousarray(values, np.float64).reshape(-1)
        if b.size != n + 1 or v.size != width * b[-1]:
            raise EngineError(-1, f"similarity apply: the sizes of the {what} do not agree")
        return b, v
    pb, x = ranges(pt_begin, xyz, 3, "points")
    ib, e = ranges(img_begin, eo, 6, "orientations")
    q = None if cof is None else np.ascontiguousarray(cof, np.float64).reshape(-1)
    if q is not None and (x is None or q.size != 2 * x.size):
        raise EngineError(-1, "similarity apply: the sizes of the cofactors do not agree")
    xo = None if x is None else np.zeros_like(x)
    qo = None if q is None else np.zeros_like(q)
    eo_out = None if e is None else np.zeros_like(e)
    rc = L.jaicov_simil_apply(n, _p(par), pb.ctypes.data_as(_pi) if pb is not None else nulli, _p(x) if x is not None else null,
                              _p(q) if q is not None else null, ib.ctypes.data_as(_pi) if ib is not None else nulli,
                              _p(e) if e is not None else null, _p(xo) if xo is not None else null, _p(qo) if qo is not None else null,
                              _p(eo_out) if eo_out is not None else null)
    if rc != 0:
        raise EngineError(rc, "similarity apply")
    return (None if xo is None else xo.reshape(-1, 3), None if qo is None else qo.reshape(-1, 6),
            None if eo_out is None else eo_out.reshape(-1, 6))


def _lens_call(correct, xy, camera, cam_io, cam_r0, cam_dist_begin, dist_kind, dist_order, dist_value, var, depth, max_iterations,
               tolerance, with_jacobian, with_time):
    L = load_library()
    what = "lens correct" if correct else "lens distort"
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1)
    cam = np.ascontiguousarray(camera, np.int32).ravel()
    io = np.ascontiguousarray(cam_io, np.float64).reshape(-1)
    r0 = np.ascontiguousarray(cam_r0, np.float64).ravel()
    begin = np.ascontiguousarray(cam_dist_begin, np.int32).ravel()
    kind = np.ascontiguousarray(dist_kind, np.int32).ravel()
    order = np.ascontiguousarray(dist_order, np.int32).ravel()
    value = np.ascontiguousarray(dist_value, np.float64).ravel()
    var = None if var is None else np.ascontiguousarray(var, np.float64).reshape(-1)
    depth = None if depth is None else np.ascontiguousarray(depth, np.float64).ravel()
    n, nc = cam.size, r0.size
    if xy.size != 2 * n or io.size != 3 * nc or begin.size != nc + 1 or kind.size != order.size or kind.size != value.size or \
            (begin.size and begin[-1] != kind.size) or (var is not None and var.size != 3 * n) or (depth is not None and depth.size != n):
        raise EngineError(-1, f"{what}: array sizes do not agree")
    xy_out = np.zeros(2 * n); var_out = np.zeros(3 * n); status = np.zeros(n, np.int32); iterations = np.zeros(n, np.int32)
    jac = np.zeros(4 * n) if with_jacobian else None
    ms = np.zeros(1)
    null = C.cast(None, _pd)
    head = (n, cam.ctypes.data_as(_pi), _p(xy), _p(var) if var is not None else null, _p(depth) if depth is not None else null, nc, _p(io),
            _p(r0), begin.ctypes.data_as(_pi), kind.ctypes.data_as(_pi), order.ctypes.data_as(_pi), _p(value))
    tail = (_p(xy_out), _p(var_out), _p(jac) if jac is not None else null, status.ctypes.data_as(_pi))
    if correct:
        rc = L.jaicov_lens_correct(*head, int(max_iterations), float(tolerance), *tail, iterations.ctypes.data_as(_pi), _p(ms))
    else:
        rc = L.jaicov_lens_distort(*head, *tail, _p(ms))
    if rc != 0:
        raise EngineError(rc, what)
    out = (xy_out.reshape(-1, 2), var_out.reshape(-1, 3), status) + ((iterations,) if correct else ())
    return out + ((jac.reshape(-1, 2, 2),) if with_jacobian else ()) + ((float(ms[0]),) if with_time else ())


def lens_correct(xy, camera, cam_io, cam_r0, cam_dist_begin, dist_kind, dist_order, dist_value, var=None, depth=None, max_iterations=20,
                 tolerance=0.0, with_jacobian=False, with_time=False):
    """Reduces measured image coordinates to those of the distortion-free camera (include/jaicov_lens.h).  xy: (n, 2); camera: (n,)
    the camera of each point; cam_io: (C, 3) x0, y0, c; cam_r0: (C,); cam_dist_begin: (C + 1,) CSR offsets into dist_kind, dist_order,
    dist_value; var: (n, 3) var_x, var_y, rho or None (the unit matrix is propagated); depth: (n,) N of each point or None (needed
    only where a camera has a distance-dependent coefficient); tolerance 0: sqrt(EPS).  Returns (xy (n, 2), var (n, 3), status (n,),
    iterations (n,)), plus J (n, 2, 2) with with_jacobian and the kernel time in ms with with_time."""
    return _lens_call(True, xy, camera, cam_io, cam_r0, cam_dist_begin, dist_kind, dist_order, dist_value, var, depth, max_iterations,
                      tolerance, with_jacobian, with_time)


def lens_distort(xy, camera, cam_io, cam_r0, cam_dist_begin, dist_kind, dist_order, dist_value, var=None, depth=None, with_jacobian=False,
                 with_time=False):
    """Applies the cameras' distortion models to ideal image coordinates: the inverse of lens_correct, one evaluation per point
    (include/jaicov_lens.h).  The arguments are lens_correct's.  Returns (xy (n, 2), var (n, 3), status (n,)), plus J (n, 2, 2) with
    with_jacobian and the kernel time in ms with with_time."""
    return _lens_call(False, xy, camera, cam_io, cam_r0, cam_dist_begin, dist_kind, dist_order, dist_value, var, depth, 1, 0.0,
                      with_jacobian, with_time)


def lens_tables_without_distance(cam_dist_begin, dist_kind, dist_order, dist_value):
    """The coefficient tables without their distance-dependent (Di) entries, for a caller who knows no object space yet."""
    begin = np.asarray(cam_dist_begin, np.int64)
    kind = np.asarray(dist_kind, np.int32)
    keep = kind != DIST_DISTANCE_DI
    kept = np.concatenate([[0], np.cumsum(keep)])
    return kept[begin].astype(np.int32), kind[keep], np.asarray(dist_order, np.int32)[keep], np.asarray(dist_value, np.float64)[keep]


def lens_correct_problem(fp: FlatProblem, values=None, distance="ignore", with_status=False, **kw):
    """A copy of a FlatProblem whose image points are corrected for lens distortion, so that relorient_problem, intersect_problem,
    resect_problem and dlt_adjust take it unchanged: cameras and coefficients come from the slot vector `values` (default fp.values:
    slot_io, slot_dist, with the problem's cam_r0 and cam_dist_begin), and ip_x, ip_y, ip_var_x, ip_var_y, ip_rho of every image point
    are replaced by the corrected ones (a point whose status is SINGULAR or NOT_FINITE keeps its values).  distance="ignore" leaves the
    distance-dependent coefficients out; distance="values" forms N of every image point (PDF:151) from the object points and exterior
    orientations in `values`, for a second round once a model exists.  Joint dispersions of image blocks (blk_disp) are left as they
    are: only the 2 x 2 dispersion of a point is propagated.  with_status also returns (status, iterations).  kw: as lens_correct."""
    import copy
    if distance not in ("ignore", "values"):
        raise EngineError(-1, "lens correct problem: distance is 'ignore' or 'values'")
    v = np.array(fp.values if values is None else values, np.float64)
    io = v[fp.slot_io(0):fp.slot_io(0) + 3 * fp.n_cameras].reshape(-1, 3)
    tables = (fp.cam_dist_begin, fp.dist_kind, fp.dist_order, v[fp.slot_dist(0):fp.slot_dist(0) + fp.n_dist])
    img, pt = np.asarray(fp.ip_image), np.asarray(fp.ip_point)
    depth = None
    if distance == "ignore":
        tables = lens_tables_without_distance(*tables)
    else:
        eo = v[fp.slot_eo(0):].reshape(-1, 6)[img]
        so, co, sp, cp = np.sin(eo[:, 3]), np.cos(eo[:, 3]), np.sin(eo[:, 4]), np.cos(eo[:, 4])
        d = v[:3 * fp.n_points].reshape(-1, 3)[pt] - eo[:, :3]
        depth = sp * d[:, 0] + (-so * cp) * d[:, 1] + (co * cp) * d[:, 2]          # N = r13 dX + r23 dY + r33 dZ
    var = np.stack([fp.ip_var_x, fp.ip_var_y, fp.ip_rho], 1)
    xy, var_out, status, iterations = lens_correct(np.stack([fp.ip_x, fp.ip_y], 1), np.asarray(fp.image_camera)[img], io, fp.cam_r0,
                                                   *tables, var=var, depth=depth, **kw)[:4]
    ok = status <= LENS_NOT_CONVERGED
    out = copy.copy(fp)
    out.ip_x = np.where(ok, xy[:, 0], fp.ip_x); out.ip_y = np.where(ok, xy[:, 1], fp.ip_y)
    out.ip_var_x = np.where(ok, var_out[:, 0], fp.ip_var_x); out.ip_var_y = np.where(ok, var_out[:, 1], fp.ip_var_y)
    out.ip_rho = np.where(ok, var_out[:, 2], fp.ip_rho)
    return (out, status, iterations) if with_status else out


def dense_gemm(alay, blay, A, B, C_in, M, N, K, alpha=1.0, beta=0.0, lower_only=False, kmode=0, repeats=0):
    L = load_library()
    A = np.ascontiguousarray(A, np.float64); B = np.ascontiguousarray(B, np.float64)
    Cm = np.ascontiguousarray(C_in, np.float64).copy()
    ms = np.zeros(1)
    rc = L.jaicov_dense_gemm(alay, blay, M, N, K, alpha, _p(A), A.shape[1], _p(B), B.shape[1], beta, _p(Cm), Cm.shape[1],
                             int(lower_only), kmode, repeats, _p(ms))
    if rc != 0:
        raise EngineError(rc, "dense gemm")
    return Cm, float(ms[0])


class DebugGemmArgs(C.Structure):
    """jaicov_debug_gemm_args (csrc/debug.hip)"""
    _fields_ = [("struct_size", C.c_uint32), ("alay", C.c_int32), ("blay", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("alpha", C.c_double), ("beta", C.c_double), ("A", C.c_void_p), ("n_A", C.c_int64), ("B", C.c_void_p), ("n_B", C.c_int64),
                ("C", C.c_void_p), ("n_C", C.c_int64), ("lda", C.c_int64), ("ldb", C.c_int64), ("ldc", C.c_int64),
                ("c_alias", C.c_int32), ("lower_only", C.c_int32), ("kmode", C.c_int32), ("batch", C.c_int32), ("batch2", C.c_int32),
                ("strideA", C.c_int64), ("strideB", C.c_int64), ("strideC", C.c_int64),
                ("strideA2", C.c_int64), ("strideB2", C.c_int64), ("strideC2", C.c_int64),
                ("batch_sum_limit", C.c_int32), ("small_tiles", C.c_int32), ("tag", C.c_int32),
                ("tile_map", C.c_void_p), ("n_map", C.c_int32), ("plan_only", C.c_int32), ("plan_out", C.c_void_p)]


def debug_gemm(alay, blay, M, N, K, alpha, beta, A=None, B=None, C_in=None, lda=0, ldb=0, ldc=0, c_alias=0, lower_only=0, kmode=0,
               batch=1, batch2=1, strides=(0, 0, 0, 0, 0, 0), batch_sum_limit=0, small_tiles=-1, tag=0, tile_map=None, plan_only=False):
    """One launch of the fp64 GEMM launcher through jaicov_debug_gemm, every argument in the caller's hand.  A, B, C_in: flat float64
    buffers (B may be the same array as A: one device buffer then; with c_alias 1 / 2 C_in is ignored and C is A / B on the device).
    tile_map: (n, 2) int32.  Returns (status, plan, C): plan = (hipError_t, TM, TN, tag, grid x, y, z), C = the C buffer after the launch
    (a copy; None with plan_only).  The status is returned, not raised: the refusals are what the tests ask for."""
    L = load_library()
    a = DebugGemmArgs()
    a.struct_size = C.sizeof(DebugGemmArgs)
    a.alay, a.blay, a.M, a.N, a.K, a.alpha, a.beta = alay, blay, M, N, K, alpha, beta
    a.lda, a.ldb, a.ldc = lda, ldb, ldc
    a.c_alias, a.lower_only, a.kmode, a.batch, a.batch2 = c_alias, int(lower_only), kmode, batch, batch2
    a.strideA, a.strideB, a.strideC, a.strideA2, a.strideB2, a.strideC2 = strides
    a.batch_sum_limit, a.small_tiles, a.tag, a.plan_only = batch_sum_limit, small_tiles, tag, int(bool(plan_only))
    plan = np.full(7, -1, np.int32)
    a.plan_out = plan.ctypes.data
    keep = [plan]
    if tile_map is not None:
        tm = np.ascontiguousarray(tile_map, np.int32).reshape(-1, 2)
        keep.append(tm)
        a.tile_map, a.n_map = tm.ctypes.data, tm.shape[0]
    Cm = None
    if not plan_only:
        for x in (A, B):
            assert x.dtype == np.float64 and x.ndim == 1 and x.flags.c_contiguous
        a.A, a.n_A, a.B, a.n_B = A.ctypes.data, A.size, B.ctypes.data, B.size
        Cm = (A if c_alias == 1 else B if c_alias == 2 else np.ascontiguousarray(C_in, np.float64).reshape(-1)).copy()
        a.C, a.n_C = Cm.ctypes.data, Cm.size
    else:            # the plan looks at the aliasing alone: A == B is told by equal pointers and counts
        a.A, a.n_A, a.B, a.n_B = 1, 0, (1 if B is A and A is not None else 2), 0
    L.jaicov_debug_gemm.argtypes = [C.c_void_p]
    L.jaicov_debug_gemm.restype = C.c_int
    rc = L.jaicov_debug_gemm(C.addressof(a))
    return rc, tuple(int(v) for v in plan), Cm


def debug_xcd_tile_map(T):
    """xcd_tile_map(T) of csrc/gemm_f64.h as an (n, 2) int32 array; no device needed."""
    L = load_library()
    L.jaicov_debug_xcd_tile_map.argtypes = [C.c_int, C.c_void_p, C.c_int]
    L.jaicov_debug_xcd_tile_map.restype = C.c_int
    n = L.jaicov_debug_xcd_tile_map(T, None, 0)
    if n < 0:
        raise EngineError(n, "xcd tile map")
    out = np.zeros((n, 2), np.int32)
    assert L.jaicov_debug_xcd_tile_map(T, out.ctypes.data, n) == n
    return out
