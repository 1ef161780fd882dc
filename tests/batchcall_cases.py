"""The eight one-shot batched calls (csrc/batchcall.h: BatchCall) called through ctypes with nothing in between, so that every optional
input and output can be passed or left out: the wrappers of bundle_adjustment_amd/engine.py always pass the optional outputs.

A case is (function name, argument list).  An argument is ("n", int), ("d", float), or (kind, name, array or None, optional) with kind
"in" or "out"; invoke() replaces an optional argument by NULL when it is called with optional=False, fills every output with a
sentinel first, and returns (status, {name: output array}).

The optional inputs of a case hold what the call assumes without them (unit weights as var = (sigma2, sigma2, 0), start values of NaN,
cofactors 0 and I, no fixed interior orientation), so the outputs that both forms of the call write are the same to the bit."""
import ctypes as C

import numpy as np

import dlt_reference
import intersect_reference
import lens_reference
import relorient_reference
import resection_reference
import similarity_reference
from bundle_adjustment_amd import engine, scene

TOO_FEW = 2                                  # JAICOV_{DLT,RESECT,RELOR,SIMIL}_TOO_FEW_POINTS, JAICOV_ISECT_TOO_FEW_RAYS
BAD_ARGUMENT = -1
SENTINEL = {np.dtype(np.float64): -7.25, np.dtype(np.int32): -77, np.dtype(np.uint8): 77}


def library(path=None):
    """a handle of its own on the library, without the argument types that engine.load_library() sets on its handle"""
    lib = C.CDLL(path or engine.LIB_PATH)
    lib.jaicov_debug_device_census.argtypes = [C.POINTER(C.c_longlong)]
    lib.jaicov_debug_device_census.restype = None
    return lib


def census(lib):
    a = (C.c_longlong * 2)()                 # bytes, allocations held by the library right now
    lib.jaicov_debug_device_census(a)
    return int(a[0]), int(a[1])


def invoke(lib, case, optional=True):
    name, args = case
    cargs, outs, keep = [], {}, []
    for a in args:
        if a[0] == "n":
            cargs.append(C.c_int32(a[1]))
        elif a[0] == "d":
            cargs.append(C.c_double(a[1]))
        else:
            kind, label, arr, opt = a
            if arr is None or (opt and not optional):
                cargs.append(C.c_void_p(None))
                continue
            arr = np.ascontiguousarray(arr)
            if kind == "out":
                arr = np.full_like(arr, SENTINEL[arr.dtype])
                outs[label] = arr
            keep.append(arr)
            cargs.append(C.c_void_p(arr.ctypes.data))
    f = getattr(lib, name)
    f.restype = C.c_int
    return f(*cargs), outs


def _i(a):
    return np.ascontiguousarray(a, np.int32).ravel()


def _f(a):
    return np.ascontiguousarray(a, np.float64).ravel()


def _unit_var(n):
    return np.tile([1.0, 1.0, 0.0], n)


def _ms():
    return ("out", "ms", np.zeros(1), True)


# ---- the cases' arguments, from batches in the layout of the reference modules ------------------------------------------------------
def dlt_case(ob, xy, xyz, io, max_iterations=5000):
    n = len(ob) - 1
    return ("jaicov_dlt_adjust", [("n", n), ("in", "obs_begin", _i(ob), False), ("in", "xy", _f(xy), False), ("in", "xyz", _f(xyz), False),
                                  ("in", "io", _f(io), False), ("in", "io_fixed", np.zeros(3 * n, np.uint8), True),
                                  ("in", "restrictions", None, False), ("n", 0), ("n", max_iterations),
                                  ("out", "out", np.zeros(20 * n), False), ("out", "status", np.zeros(n, np.int32), False),
                                  ("out", "solves", np.zeros(n, np.int32), True), _ms()])


def isect_case(rb, ri, xy, io, eo, var=None, reject_threshold=0.0, min_rays=3):
    n, nr = len(rb) - 1, len(_i(ri))
    return ("jaicov_isect_points", [("n", n), ("in", "ray_begin", _i(rb), False), ("in", "ray_image", _i(ri), False), ("in", "xy", _f(xy), False),
                                    ("in", "var", _unit_var(nr) if var is None else _f(var), True), ("n", len(_f(io)) // 3),
                                    ("in", "io", _f(io), False), ("in", "eo", _f(eo), False), ("d", 1.0), ("n", 50), ("d", reject_threshold),
                                    ("n", min_rays), ("out", "out", np.zeros(11 * n), False), ("out", "status", np.zeros(n, np.int32), False),
                                    ("out", "iterations", np.zeros(n, np.int32), True), ("out", "used", np.zeros(nr, np.uint8), True),
                                    ("out", "q", np.zeros(nr), True), _ms()])


def resect_case(ob, xy, xyz, io, var=None, start=None, reject_threshold=0.0, min_points=4):
    n, no = len(ob) - 1, len(_f(xy)) // 2
    return ("jaicov_resect_images", [("n", n), ("in", "obs_begin", _i(ob), False), ("in", "xy", _f(xy), False), ("in", "xyz", _f(xyz), False),
                                     ("in", "var", _unit_var(no) if var is None else _f(var), True), ("in", "io", _f(io), False),
                                     ("in", "eo_start", np.full(6 * n, np.nan) if start is None else _f(start), True), ("d", 1.0), ("n", 50),
                                     ("d", reject_threshold), ("n", min_points), ("out", "out", np.zeros(28 * n), False),
                                     ("out", "status", np.zeros(n, np.int32), False), ("out", "iterations", np.zeros(n, np.int32), True),
                                     ("out", "start_kind", np.zeros(n, np.int32), True), ("out", "used", np.zeros(no, np.uint8), True),
                                     ("out", "q", np.zeros(no), True), _ms()])


def relor_case(ob, xa, xb, io, var_a=None, var_b=None, start=None, reject_threshold=0.0, min_points=6):
    n, no = len(ob) - 1, len(_f(xa)) // 2
    return ("jaicov_relorient_pairs", [("n", n), ("in", "obs_begin", _i(ob), False), ("in", "xy_a", _f(xa), False), ("in", "xy_b", _f(xb), False),
                                       ("in", "var_a", _unit_var(no) if var_a is None else _f(var_a), True),
                                       ("in", "var_b", _unit_var(no) if var_b is None else _f(var_b), True), ("in", "io", _f(io), False),
                                       ("in", "start", np.full(6 * n, np.nan) if start is None else _f(start), True), ("d", 1.0), ("n", 50),
                                       ("d", reject_threshold), ("n", min_points), ("out", "out", np.zeros(28 * n), False),
                                       ("out", "status", np.zeros(n, np.int32), False), ("out", "iterations", np.zeros(n, np.int32), True),
                                       ("out", "start_kind", np.zeros(n, np.int32), True), ("out", "used", np.zeros(no, np.uint8), True),
                                       ("out", "q", np.zeros(no), True), _ms()])


def simil_case(pb, src, dst, cof_src=None, cof_dst=None, start=None, reject_threshold=0.0, min_points=3):
    n, npt = len(pb) - 1, len(_f(src)) // 3
    return ("jaicov_simil_models", [("n", n), ("in", "pt_begin", _i(pb), False), ("in", "src", _f(src), False), ("in", "dst", _f(dst), False),
                                    ("in", "cof_src", np.zeros(6 * npt) if cof_src is None else _f(cof_src), True),
                                    ("in", "cof_dst", np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], npt) if cof_dst is None else _f(cof_dst), True),
                                    ("in", "start", np.full(7 * n, np.nan) if start is None else _f(start), True), ("n", 50),
                                    ("d", reject_threshold), ("n", min_points), ("out", "out", np.zeros(36 * n), False),
                                    ("out", "status", np.zeros(n, np.int32), False), ("out", "iterations", np.zeros(n, np.int32), True),
                                    ("out", "start_kind", np.zeros(n, np.int32), True), ("out", "used", np.zeros(npt, np.uint8), True),
                                    ("out", "q", np.zeros(npt), True), _ms()])


def apply_case(par, pb, xyz, cof, ib, eo):
    """cof and cof_out are the optional pair of this call"""
    n = len(_f(par)) // 7
    return ("jaicov_simil_apply", [("n", n), ("in", "par", _f(par), False), ("in", "pt_begin", None if pb is None else _i(pb), False),
                                   ("in", "xyz", None if xyz is None else _f(xyz), False), ("in", "cof", None if cof is None else _f(cof), True),
                                   ("in", "img_begin", None if ib is None else _i(ib), False), ("in", "eo", None if eo is None else _f(eo), False),
                                   ("out", "xyz_out", None if xyz is None else np.zeros(len(_f(xyz))), False),
                                   ("out", "cof_out", None if cof is None else np.zeros(len(_f(cof))), True),
                                   ("out", "eo_out", None if eo is None else np.zeros(len(_f(eo))), False)])


def lens_case(correct, xy, cam, tables, var=None, depth=None, max_iterations=20, tolerance=0.0):
    """tables: (cam_io, cam_r0, cam_dist_begin, dist_kind, dist_order, dist_value).  var, var_out, jac_out, iterations and ms_out are
    optional, and so is depth: the tables of a case that is also called without it hold no distance-dependent coefficient."""
    io, r0, begin, kind, order, value = tables
    n = len(_i(cam))
    head = [("n", n), ("in", "camera", _i(cam), False), ("in", "xy", _f(xy), False), ("in", "var", _unit_var(n) if var is None else _f(var), True),
            ("in", "depth", np.full(n, -1500.0) if depth is None else _f(depth), True), ("n", len(_f(r0))), ("in", "cam_io", _f(io), False),
            ("in", "cam_r0", _f(r0), False), ("in", "begin", _i(begin), False), ("in", "kind", _i(kind), False), ("in", "order", _i(order), False),
            ("in", "value", _f(value), False)]
    tail = [("out", "xy_out", np.zeros(2 * n), False), ("out", "var_out", np.zeros(3 * n), True), ("out", "jac", np.zeros(4 * n), True),
            ("out", "status", np.zeros(n, np.int32), False)]
    if correct:
        return ("jaicov_lens_correct", head + [("n", max_iterations), ("d", tolerance)] + tail + [("out", "iterations", np.zeros(n, np.int32), True), _ms()])
    return ("jaicov_lens_distort", head + tail + [_ms()])


# ---- batches of three items with 0, the minimum admissible and the minimum + 1 observations -------------------------------------------
def with_empty_first(begin, *per_item):
    """the ranges `begin` with an empty range in front; every per-item array gets its first row once more, for the empty item"""
    begin = np.concatenate([[0], np.asarray(begin)]).astype(np.int32)
    return (begin,) + tuple(np.concatenate([np.asarray(a)[:1], np.asarray(a)]) for a in per_item)


def _first(ob, counts):
    """the first counts[g] observations of item g of the ranges ob: (their indices, the new ranges)"""
    sel = np.concatenate([np.arange(ob[g], ob[g] + c) for g, c in enumerate(counts)])
    assert all(ob[g] + c <= ob[g + 1] for g, c in enumerate(counts))
    return sel, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def minimum_cases():
    """{call: (case of the two items with the minimum and the minimum + 1 observations, the same behind an empty item)}"""
    tiny = scene.config("tiny")
    cases = {}
    ob, xy, xyz, io, _ = dlt_reference.batch_from_scene(tiny)                   # fewer than 6 points: TOO_FEW_POINTS (jaicov_dlt.h)
    sel, ob = _first(ob, [6, 7])
    xy, xyz, io = np.asarray(xy)[sel], np.asarray(xyz)[sel], np.asarray(io)[:2]
    ob3, io3 = with_empty_first(ob, io)
    cases["dlt_adjust"] = (dlt_case(ob, xy, xyz, io), dlt_case(ob3, xy, xyz, io3))
    rb, ri, xy, _, io, eo, _ = intersect_reference.batch_from_scene(tiny)       # fewer than 2 rays
    sel, rb = _first(rb, [2, 3])
    ri, xy = np.asarray(ri)[sel], np.asarray(xy)[sel]
    cases["isect_points"] = (isect_case(rb, ri, xy, io, eo), isect_case(with_empty_first(rb)[0], ri, xy, io, eo))
    ob, xy, xyz, _, io, _ = resection_reference.plane_batch([4, 5])             # 4 points: the linear (plane) start is taken
    ob3, io3 = with_empty_first(ob, io)
    cases["resect_images"] = (resect_case(ob, xy, xyz, io), resect_case(ob3, xy, xyz, io3))
    (ob, xa, xb, _, _, io, _), _, _ = relorient_reference.plane_batch([6, 7], thickness=0.3)      # fewer than 6 without start values
    ob3, io3 = with_empty_first(ob, io)
    cases["relorient_pairs"] = (relor_case(ob, xa, xb, io), relor_case(ob3, xa, xb, io3))
    (pb, src, dst, _, _, _), _ = similarity_reference.models([3, 4])            # fewer than 3 points
    cases["simil_models"] = (simil_case(pb, src, dst), simil_case(with_empty_first(pb)[0], src, dst))
    return cases


PER_OBSERVATION = ("xy", "xyz", "var", "ray_image", "xy_a", "xy_b", "var_a", "var_b", "src", "dst", "cof_src", "cof_dst", "used", "q")


def all_empty(case):
    """the items of a case without their observations: every range empty, every array that holds one entry per observation NULL"""
    name, args = case
    n = args[0][1]

    def without(a):
        if a[0] in ("in", "out") and a[1].endswith("_begin"):
            return (a[0], a[1], np.zeros(n + 1, np.int32), a[3])
        return (a[0], a[1], None, a[3]) if a[0] in ("in", "out") and a[1] in PER_OBSERVATION else a
    return name, [without(a) for a in args]


def rangeless_cases(n):
    """{call: case} of the three calls without ranges per item, n points (and n images for the apply)"""
    rng = np.random.default_rng(n)
    par = np.concatenate([rng.uniform(-500, 500, 3), [1.7], rng.uniform(-1.0, 1.0, 3)])
    xyz = rng.uniform(-1000, 1000, (n, 3))
    cof = similarity_reference.random_cofactors(rng, n, 0.1)[0]
    eo = np.column_stack([rng.uniform(-1000, 1000, (n, 3)), rng.uniform(-1.0, 1.0, (n, 3))])
    xy, cam, t, _ = lens_reference.mixed_cameras(n)
    t = t[:2] + tuple(engine.lens_tables_without_distance(*t[2:]))
    return {"simil_apply": apply_case(par, [0, n], xyz, cof, [0, n], eo), "lens_correct": lens_case(True, xy, cam, t),
            "lens_distort": lens_case(False, xy, cam, t)}
