"""The host stage of jaicov_neq_create (csrc/create_plan.h): what it refuses, what it decides and the tables it leaves for the device stage.
No device needed: jaicov_debug_create_plan runs the plan alone.  The rejections are the cases of test_gpu_errors.py (which sends them through
jaicov_neq_create on a GPU); the tables are held to what the kernels rely on:

  * the engine's order of the image points is the caller's outside dense blocks and a column-sorted rearrangement inside each (assemble.hip,
    blk_pp_gather_kernel streams the partners of a point as contiguous positions of the block);
  * the segments of launch_assemble_small cover exactly this engine's image points outside blocks, one image each, SEG points at most;
  * the gather's range table drops nothing of the lower triangle;
  * every rank of a sharded run reaches the same decisions (order of the reduced system, served-as-blocks or not).
"""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from bundle_adjustment_amd import engine, scene
from helpers import base_scene, corrupt

NOCOL = 1 << 30
SEG = 256                                # ba_kernels.h
FORM = {"default": 0, "t_vector": 1, "no_fork": 2, "materialise": 3}      # ba_kernels.h, ASSEMBLY_*
SUMMARY = ("n_blocks", "synthesized", "compact", "permuted", "n_seg", "n_blk_list", "n_blk_ip", "max_m", "w_total", "schur_ok", "e0", "cw",
           "n_chunks", "cmin", "cmax", "plain_ok")
TABLES = ("ip_old2new", "seg_b", "seg_e", "blk_list", "range", "recs", "blk_ip_begin")


def _call(fp, image_range=None, form="default", **options):
    lib = engine.load_library()
    desc, keep = fp.as_desc()
    opts = engine.EngineOptions()
    opts.struct_size = C.sizeof(engine.EngineOptions)
    opts.image_begin, opts.image_end = image_range if image_range is not None else (-1, -1)
    opts.apply_shared = 1
    for k, v in options.items():
        setattr(opts, k, v)
    return lib, desc, keep, opts, FORM[form]


def plan(fp, **kw):
    """(status, text, summary as a dict) of the plan for this problem and these engine options."""
    lib, desc, keep, opts, form = _call(fp, **kw)
    lib.jaicov_debug_create_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    out = np.zeros(len(SUMMARY), np.int32)
    err = C.create_string_buffer(256)
    rc = lib.jaicov_debug_create_plan(C.addressof(desc), C.addressof(opts), form, out.ctypes.data, out.size, err, 256)
    return rc, err.value.decode(), dict(zip(SUMMARY, (int(v) for v in out)))


def table(fp, name, **kw):
    lib, desc, keep, opts, form = _call(fp, **kw)
    lib.jaicov_debug_create_plan_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    args = (C.addressof(desc), C.addressof(opts), form, TABLES.index(name))
    n = lib.jaicov_debug_create_plan_table(*args, None, 0)
    assert n >= 0, n
    out = np.zeros(max(n, 1), np.int32)
    assert lib.jaicov_debug_create_plan_table(*args, out.ctypes.data, n) == n
    return out[:n]


# ---- rejections ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["datum_flags", "dist_order_of_kinds", "unknown_kind", "zernike_order_0", "zernike_order_120", "not_image_major",
                                  "duplicate_column", "column_out_of_range", "block_spans_images", "blocks_descending", "too_many_coefficients"])
def test_plan_rejects_a_malformed_problem(what):
    fp = base_scene()
    assert plan(fp)[:2] == (0, "")                                                       # the scene itself is fine
    bad, text = corrupt(fp, what)
    rc, msg, _ = plan(bad)
    assert rc == (-3 if what == "too_many_coefficients" else -1), msg
    assert text in msg, msg


@pytest.mark.parametrize("rng", [(3, 2), (5, 7), (0, 7)])
def test_plan_rejects_a_bad_image_range(rng):
    rc, msg, _ = plan(base_scene(), image_range=rng)
    assert rc == -1 and "image range" in msg


def test_plan_rejects_an_image_index_out_of_range_on_every_path():
    """The check used to sit inside the decision to serve ordinary images as blocks; a description that never got there was not looked at."""
    fp = base_scene()
    im = fp.ip_image.copy(); im[-1] = fp.n_images
    rc, msg, _ = plan(dataclasses.replace(fp, ip_image=im), ordinary_group_elimination=-1)
    assert rc == -1 and "image index out of range" in msg
    fp = scene.config("tiny")
    im = fp.ip_image.copy(); im[-1] = fp.n_images
    for oge in (-1, 0, 1):
        rc, msg, _ = plan(dataclasses.replace(fp, ip_image=im), ordinary_group_elimination=oge)
        assert rc == -1 and "image index out of range" in msg


def test_plan_rejects_an_unknown_assembly_mode():
    for mode in (-1, 3):
        rc, msg, _ = plan(base_scene(), assembly_mode=mode)
        assert rc == -1 and "assembly_mode must be" in msg
    for mode in (0, 1, 2):
        assert plan(base_scene(), assembly_mode=mode)[0] == 0


# ---- tables --------------------------------------------------------------------------------------------------------------------
def two_camera_scene():
    """The scene of test_gpu_ordinary_elimination.test_two_cameras_with_ordinary_images."""
    from bundle_adjustment_amd.problem import DIST_RADIAL_AI
    import test_gpu_edge_cases as ec
    base = scene.make_scene(8, 60, 36, dist=scene.DIST_FULL, weights="2x2", n_control=5)
    P, I, nd = base.n_points, base.n_images, base.dist_kind.size
    keep = (base.dist_kind <= 1) | (base.dist_kind == DIST_RADIAL_AI)
    s_io, v = 3 * P, base.values
    values = np.concatenate([v[:s_io], v[s_io:s_io + 3], v[s_io:s_io + 3], v[s_io + 3:s_io + 3 + nd], v[s_io + 3:s_io + 3 + nd][keep], v[s_io + 3 + nd:]])
    return ec.renumber(base, image_camera=np.array([0] * (I // 2) + [1] * (I - I // 2), np.int32),
                       cam_dist_begin=np.array([0, nd, nd + int(keep.sum())], np.int32), cam_r0=np.array([base.cam_r0[0], base.cam_r0[0]]),
                       dist_kind=np.concatenate([base.dist_kind, base.dist_kind[keep]]).astype(np.int32),
                       dist_order=np.concatenate([base.dist_order, base.dist_order[keep]]).astype(np.int32), values=values, truth=None)


def strips_scene(layout="strips"):
    return scene.make_scene(40, 600, 150, layout=layout, dist=scene.DIST_FULL, weights="block", n_control=8, control_dense=True)


SCENES = {"tiny": lambda: scene.config("tiny"), "tiny_block": lambda: scene.config("tiny_block"), "tiny_free": lambda: scene.config("tiny_free"),
          "cfg2": lambda: scene.config("cfg2"), "cfg3": lambda: scene.config("cfg3"), "two_cameras": two_camera_scene,
          "strips": strips_scene, "sphere": lambda: strips_scene("sphere")}
_cache = {}


def get_scene(name):
    if name not in _cache:
        _cache[name] = SCENES[name]()
    return _cache[name]


def ranges_of(fp):
    I = fp.n_images
    return [None, (0, I // 2), (I // 2, I)]


def options_of(fp):
    """Ordinary scenes: the elimination of ordinary image groups off / by the size rule / forced."""
    return [{}] if fp.n_image_blocks else [{"ordinary_group_elimination": o} for o in (-1, 0, 1)]


def check_tables(fp, image_range, **options):
    rc, msg, S = plan(fp, image_range=image_range, **options)
    assert rc == 0, msg
    T = {name: table(fp, name, image_range=image_range, **options) for name in TABLES}
    n = fp.n_image_points
    bb = T["blk_ip_begin"]
    assert bb.size == S["n_blocks"] + 1 and S["n_seg"] == T["seg_b"].size == T["seg_e"].size and S["n_blk_list"] == T["blk_list"].size
    in_block = np.zeros(n, bool)
    for g in range(S["n_blocks"]):
        in_block[bb[g]:bb[g + 1]] = True
    # -- the engine's order of the image points
    o2n = T["ip_old2new"] if S["permuted"] else np.arange(n, dtype=np.int32)
    assert o2n.size == n and np.array_equal(np.sort(o2n), np.arange(n))
    assert np.array_equal(o2n[~in_block], np.arange(n)[~in_block])
    for g in range(S["n_blocks"]):
        assert np.array_equal(np.sort(o2n[bb[g]:bb[g + 1]]), np.arange(bb[g], bb[g + 1])), g
    new2old = np.argsort(o2n)
    image, point = fp.ip_image[new2old], fp.ip_point[new2old]
    assert np.array_equal(image, fp.ip_image)
    col = fp.point_col[point]                                                            # (n, 3), engine order
    lo = np.where(col >= 0, col, NOCOL).min(1)
    hi = col.max(1)
    for g in T["blk_list"]:
        assert np.all(np.diff(lo[bb[g]:bb[g + 1]]) >= 0), g
    assert S["n_blk_ip"] == sum(bb[g + 1] - bb[g] for g in T["blk_list"])
    assert S["max_m"] == max([2 * (bb[g + 1] - bb[g]) for g in T["blk_list"]], default=0)
    # -- segments
    ib, ie = image_range if image_range is not None else (0, fp.n_images)
    ip0, ip1 = np.searchsorted(fp.ip_image, ib), np.searchsorted(fp.ip_image, ie)
    covered = np.zeros(n, int)
    for b, e in zip(T["seg_b"], T["seg_e"]):
        assert ip0 <= b < e <= ip1 and e - b <= SEG and np.all(image[b:e] == image[b])
        covered[b:e] += 1
    want = ~in_block
    want[:ip0] = False; want[ip1:] = False
    assert np.array_equal(covered, want.astype(int))
    assert all(ib <= image[bb[g]] < ie for g in T["blk_list"])
    # -- the gather's ranges
    recs = T["recs"].reshape(-1, 3)
    if recs.size:
        assert S["n_chunks"] > 0 and S["cmin"] <= S["cmax"] and S["cw"] >= 64 and S["cw"] % 4 == 0
        assert S["n_chunks"] == (S["cmax"] - S["cmin"]) // S["cw"] + 1
        rng = T["range"].reshape(recs.shape[0], S["n_chunks"], 2)
        assert recs.shape[0] == S["n_blk_ip"]
        for (ipb, mp, lp), r in zip(recs, rng):
            assert np.all((0 <= r[:, 0]) & (r[:, 0] <= r[:, 1]) & (r[:, 1] <= mp))
            seen = np.zeros(mp, bool)
            for a, b in r:
                seen[a:b] = True
            need = lo[ipb:ipb + mp] <= hi[ipb + lp]                                      # the partners of the lower triangle
            assert np.all(seen[need]), (ipb, lp)
    else:
        assert T["range"].size == 0
    return S


@pytest.mark.parametrize("name", sorted(SCENES))
def test_tables_hold_their_invariants(name):
    fp = get_scene(name)
    for options in options_of(fp):
        for image_range in ranges_of(fp):
            check_tables(fp, image_range, **options)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_rank_decides_alike(name):
    fp = get_scene(name)
    for options in options_of(fp):
        whole, *shards = [plan(fp, image_range=r, **options)[2] for r in ranges_of(fp)]
        for s in shards:
            assert (s["schur_ok"], s["e0"], s["synthesized"], s["n_blocks"]) == (whole["schur_ok"], whole["e0"], whole["synthesized"], whole["n_blocks"])


def test_default_serves_ordinary_images_as_blocks_only_where_it_saves_block_columns():
    """What test_gpu_ordinary_elimination.test_default_eliminates_ordinary_images_only_where_it_saves_block_columns reads off reduced_order()."""
    s2, s3 = plan(get_scene("cfg2"))[2], plan(get_scene("cfg3"))[2]
    assert (s2["synthesized"], s2["schur_ok"], s2["n_blocks"]) == (0, 0, 0)
    fp = get_scene("cfg3")
    assert (s3["synthesized"], s3["compact"], s3["schur_ok"], s3["n_blocks"]) == (1, 1, 1, fp.n_images)
    assert s3["e0"] == fp.n_unknowns - 6 * fp.n_images and s3["w_total"] == 0
    forced, off = plan(get_scene("cfg2"), ordinary_group_elimination=1)[2], plan(fp, ordinary_group_elimination=-1)[2]
    assert forced["synthesized"] == 1 and off["synthesized"] == 0 and off["schur_ok"] == 0
    # the alternative assembly forms read m x m weights: dense, not compact
    dense = plan(get_scene("tiny"), form="t_vector", ordinary_group_elimination=1)[2]
    assert dense["synthesized"] == 1 and dense["compact"] == 0 and dense["w_total"] > 0
    # assembly_mode 1 / 2 (densemode.hip) replaces the elimination
    assert plan(get_scene("tiny_block"))[2]["schur_ok"] == 1 and plan(get_scene("tiny_block"), assembly_mode=1)[2]["schur_ok"] == 0


# What the one-piece create_impl of the commit before the plan was split off (883a9a7) chooses for these scenes and reports as
# Engine.kernel_stats()["gather_strip_columns"]: the plan must choose the same.  (Literals obtained by running that commit's table code
# unchanged on the host.)  The strips scene and
# config 3 (400 of 1 000 points per image, every image served as a block) narrow the strip, the sphere twin of the strips scene keeps
# the default.
STRIP_WIDTH = {"strips": 768, "sphere": 1664, "cfg3": 448}


@pytest.mark.parametrize("name", sorted(STRIP_WIDTH))
def test_strip_width_follows_the_scene(name):
    assert plan(get_scene(name))[2]["cw"] == STRIP_WIDTH[name]


def test_the_plan_touches_no_device():
    """create_plan.h is host logic: no HIP runtime call, no launch (the style of test_abi.test_engine_frees_none_of_its_members_by_hand)."""
    src = open(os.path.join(os.path.dirname(engine.LIB_PATH), "create_plan.h")).read()
    assert not re.search(r"hip[A-Z]\w*\(", src)
    assert "<<<" not in src and "hipLaunchKernelGGL" not in src
