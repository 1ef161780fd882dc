"""Shared test helpers (host side only)."""
import dataclasses
import json
import os

import numpy as np

from bundle_adjustment_amd import numbering, scene
from bundle_adjustment_amd.problem import FlatProblem

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden_rows(name="jacobian_rows.json"):
    with open(os.path.join(GOLDEN, name)) as fh:
        return json.load(fh)["sets"]


def problem_from_cases(dist, cases, sigma=5e-4, rho=0.0):
    """One camera, one image and one object point PER case, everything free, d = 0 -- a carrier for row parity."""
    n = len(cases)
    nd = len(dist)
    P, I = n, n
    col = 0
    point_col = np.arange(3 * P).reshape(P, 3); col += 3 * P
    io_col = np.zeros((n, 3), np.int32); dist_col = np.zeros(n * nd, np.int32)
    for c in range(n):
        io_col[c] = col + np.arange(3); col += 3
        dist_col[c * nd:(c + 1) * nd] = col + np.arange(nd); col += nd
    eo_col = (col + np.arange(6 * I)).reshape(I, 6); col += 6 * I
    values = np.concatenate([np.array([c["point"] for c in cases]).ravel(),
                             np.array([c["io"] for c in cases]).ravel(),
                             np.array([c["dist_values"] for c in cases]).ravel() if nd else np.zeros(0),
                             np.array([c["eo"] for c in cases]).ravel()])
    return FlatProblem(
        n_unknowns=col, rank_defect=0, datum_flags=0, point_col=point_col, point_datum=np.ones(P, np.uint8),
        io_col=io_col, cam_r0=np.array([c["r0"] for c in cases]), cam_dist_begin=np.arange(n + 1) * nd,
        dist_kind=np.tile(np.array([k for k, _ in dist], np.int32), n),
        dist_order=np.tile(np.array([o for _, o in dist], np.int32), n), dist_col=dist_col,
        image_camera=np.arange(n), eo_col=eo_col, ip_image=np.arange(n), ip_point=np.arange(n),
        ip_x=np.array([c["obs"][0] for c in cases]), ip_y=np.array([c["obs"][1] for c in cases]),
        ip_var_x=np.full(n, sigma ** 2), ip_var_y=np.full(n, sigma ** 2), ip_rho=np.full(n, rho), values=values,
        sigma2apriori=sigma ** 2).validate()


def rel_err(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---- malformed problems (test_gpu_errors.py through jaicov_neq_create, test_create_plan.py through the plan alone) ----
def base_scene():
    return scene.make_scene(6, 40, 24, dist=scene.DIST_FULL, weights="block", n_control=4)


def corrupt(fp, what):
    """One malformed field per case; everything else stays the valid scene."""
    r = dataclasses.replace
    if what == "datum_flags":
        return r(fp, datum_flags=fp.datum_flags | 1), "datum_flags"                      # one flag, rank_defect 0
    if what == "dist_order_of_kinds":
        k = fp.dist_kind.copy(); k[[4, 5]] = k[[5, 4]]                                   # ... Bi, Ai -> Ai, Bi
        return r(fp, dist_kind=k), "Type order"
    if what == "unknown_kind":
        k = fp.dist_kind.copy(); k[-1] = 10
        return r(fp, dist_kind=k), "unknown distortion coefficient kind"
    if what == "zernike_order_0":
        k = fp.dist_kind.copy(); o = fp.dist_order.copy(); k[-1] = 9; o[-1] = 0
        return r(fp, dist_kind=k, dist_order=o), "1..119"
    if what == "zernike_order_120":
        k = fp.dist_kind.copy(); o = fp.dist_order.copy(); k[-1] = 7; o[-1] = 120
        return r(fp, dist_kind=k, dist_order=o), "1..119"
    if what == "not_image_major":
        im = fp.ip_image.copy(); im[0], im[-1] = im[-1], im[0]
        return r(fp, ip_image=im), "image-major"
    if what == "duplicate_column":
        pc = fp.point_col.copy(); free = np.argwhere(pc >= 0)
        pc[tuple(free[0])] = pc[tuple(free[1])]
        return r(fp, point_col=pc), "permutation"
    if what == "column_out_of_range":
        pc = fp.point_col.copy(); free = np.argwhere(pc >= 0)
        pc[tuple(free[0])] = fp.n_unknowns
        return r(fp, point_col=pc), "permutation"
    if what == "block_spans_images":
        b = fp.blk_ip_begin.copy(); b[1] += 1                                            # block 0 takes the first point of image 1
        return r(fp, blk_ip_begin=b), "span"
    if what == "blocks_descending":
        b = fp.blk_ip_begin.copy(); b[2] = b[1] - 1
        return r(fp, blk_ip_begin=b), "ascending"
    if what == "too_many_coefficients":
        n = 21                                                                           # JAICOV_MAX_DIST_PER_CAMERA = 20
        return r(fp, cam_dist_begin=np.array([0, n], np.int32), dist_kind=np.full(n, 5, np.int32), dist_order=np.arange(1, n + 1, dtype=np.int32),
                 dist_col=np.full(n, -1, np.int32)), "too many"
    raise KeyError(what)


# ---- irregular scenes (test_gpu_edge_cases.py against the oracle's full system, test_gpu_reduced_system.py against the reduced truth) ----
def renumber(fp, *, point_fixed=None, io_fixed=None, dist_fixed=None, eo_fixed=None, **changes):
    """Same scene, new index contract (BundleAdjustment.java:667-782) after fixing parameters / changing cameras."""
    image_camera = changes.get("image_camera", fp.image_camera)
    cam_dist_begin = changes.get("cam_dist_begin", fp.cam_dist_begin)
    n_cameras = len(cam_dist_begin) - 1
    num = numbering.number_unknowns(fp.n_points, n_cameras, image_camera, fp.ip_point, cam_dist_begin,
                                    point_fixed=point_fixed, io_fixed=io_fixed, dist_fixed=dist_fixed, eo_fixed=eo_fixed,
                                    sb_point_a=fp.sb_point_a, sb_point_b=fp.sb_point_b, dg_slot=changes.get("dg_slot", fp.dg_slot))
    return dataclasses.replace(fp, n_unknowns=num["n_unknowns"], rank_defect=num["rank_defect"], datum_flags=num["datum_flags"],
                               point_col=num["point_col"], io_col=num["io_col"], dist_col=num["dist_col"], eo_col=num["eo_col"],
                               n_observations=0, **changes).validate()


def two_camera_scene():
    """(two, base): the images of `base` shared out between two cameras, the second with affinity/shear and radial A1-A3 only."""
    base = scene.make_scene(8, 60, 36, dist=scene.DIST_FULL, weights="block", n_control=5, control_dense=True)
    P, I = base.n_points, base.n_images
    nd = base.dist_kind.size
    keep = (base.dist_kind <= 1) | (base.dist_kind == 5)   # camera 1: affinity/shear (Cx, Cy) + radial A1-A3 only
    nd1 = int(keep.sum())
    s_io = 3 * P
    v = base.values
    values = np.concatenate([v[:s_io], v[s_io:s_io + 3], v[s_io:s_io + 3], v[s_io + 3:s_io + 3 + nd],
                             v[s_io + 3:s_io + 3 + nd][keep], v[s_io + 3 + nd:]])
    image_camera = np.array([0] * (I // 2) + [1] * (I - I // 2), np.int32)
    two = renumber(base, image_camera=image_camera, cam_dist_begin=np.array([0, nd, nd + nd1], np.int32),
                   cam_r0=np.array([base.cam_r0[0], base.cam_r0[0]]),
                   dist_kind=np.concatenate([base.dist_kind, base.dist_kind[keep]]).astype(np.int32),
                   dist_order=np.concatenate([base.dist_order, base.dist_order[keep]]).astype(np.int32),
                   values=values, truth=None)
    assert two.n_unknowns == base.n_unknowns + 3 + nd1
    return two, base


def mixed_scene():
    """Jointly dispersed and ordinary images in one adjustment."""
    base = scene.make_scene(8, 60, 36, dist=scene.DIST_FULL, weights="block", n_control=5, control_dense=True)
    k = 5                                           # images 0..4 keep their joint dispersion, 5..7 fall back to sigma_x, sigma_y
    return dataclasses.replace(base, blk_ip_begin=base.blk_ip_begin[:k + 1].copy(), blk_disp_offset=base.blk_disp_offset[:k].copy(),
                               blk_disp=base.blk_disp[:int(base.blk_disp_offset[k])].copy(), n_observations=0).validate()


def ragged_scene():
    """Images with very different numbers of points (3 ... 45) in jointly dispersed groups."""
    base = scene.make_scene(9, 45, 45, dist=scene.DIST_RADIAL, weights="block", n_control=5, control_dense=True, min_rays=2)
    counts = np.diff(base.blk_ip_begin)
    want = np.minimum(counts, np.array([3, 45, 5, 17, 45, 9, 33, 4, 45])[:counts.size])
    keep = np.concatenate([np.arange(base.blk_ip_begin[i], base.blk_ip_begin[i] + want[i]) for i in range(counts.size)])
    disp, off = [], [0]
    for i in range(counts.size):
        m0, m1 = 2 * int(counts[i]), 2 * int(want[i])
        D = base.blk_disp[base.blk_disp_offset[i]:base.blk_disp_offset[i] + m0 * m0].reshape(m0, m0)[:m1, :m1]
        disp.append(D.ravel()); off.append(off[-1] + m1 * m1)
    rays = np.bincount(base.ip_point[keep], minlength=base.n_points)
    assert rays.min() >= 2, "scene too thin for this test: every point needs two rays"
    rag = dataclasses.replace(base, ip_image=base.ip_image[keep], ip_point=base.ip_point[keep], ip_x=base.ip_x[keep], ip_y=base.ip_y[keep],
                              ip_var_x=base.ip_var_x[keep], ip_var_y=base.ip_var_y[keep], ip_rho=base.ip_rho[keep],
                              blk_ip_begin=np.concatenate([[0], np.cumsum(want)]).astype(np.int32),
                              blk_disp_offset=np.array(off[:-1], np.int64), blk_disp=np.concatenate(disp), n_observations=0)
    return renumber(rag)
