#!/usr/bin/env python3
"""The calls of include/jaicov_parameters.h at config 4 after one FULL_EXPANDED pass: the maxima pass with all mask bits, the two
pair passes at threshold 0.9, a 3 000 x 14 block and 5 000 point groups.

Whole calls are timed as scripts/precision_bench.py times them: HIP events on the null stream around the call (the calls
synchronise, so the events bracket uploads, kernels and downloads) and the host's wall clock, medians of `--repeats` runs after a
warm-up that also allocates the work buffers.

The kernels alone are timed inside the library (jaicov_debug_par_kernel_ms): events on the engine's stream around `--kernel-repeats`
launches each, interleaved, after the tables are ready.  The yardstick is not a fixed number: it is one product Y = S X of
sym_y_tile_kernel<8> + sym_y_reduce_kernel<8> (csrc/symtile.h) over [d, order) of the same matrix in the same process, which reads
exactly the bytes the maxima pass reads.  Reported: the medians, the run-to-run spread of each ((p90 - p10) / median), the ratio of
the maxima pass to the product, and both as a share of the time HBM needs for the lower triangle at 8 TB/s.
One JSON object on stdout (and in --out)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bundle_adjustment_amd  # noqa: E402,F401
from bundle_adjustment_amd import engine, scene  # noqa: E402
from precision_bench import Events, timed  # noqa: E402

HBM_BYTES_PER_S = 8e12
KERNELS = ("maxima_pass", "pairs_count_pass", "yardstick_product", "maxima_tile_kernel", "yardstick_tile_kernel")


def spread(x):
    x = np.sort(np.asarray(x))
    return float((np.percentile(x, 90) - np.percentile(x, 10)) / np.median(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-repeats", type=int, default=30)
    ap.add_argument("--small", action="store_true", help="a small scene (8 x 60) instead of config 4: a quick check")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    fp = scene.make_scene(8, 60, 40, dist=scene.DIST_FULL, weights="block", n_control=4) if a.small else scene.config("cfg4")
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(engine.INVERT_FULL_EXPANDED)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(engine.INVERT_FULL_EXPANDED)
    U, d, P = eng.cofactor_order(), fp.rank_defect, fp.n_points
    s2 = fp.sigma2apriori
    ev = Events()
    mx, mx_ms, mx_wall = timed(ev, lambda: eng.correlation_maxima(), a.repeats)
    pr, pr_ms, pr_wall = timed(ev, lambda: eng.correlated_pairs(0.9, capacity=1 << 24), a.repeats)
    eo = np.asarray(fp.eo_col).ravel()
    rows = eo[eo >= 0][:3000].astype(np.int32)
    inner = np.r_[np.asarray(fp.io_col).ravel(), np.asarray(fp.dist_col).ravel()]
    inner = inner[inner >= 0]
    cols = np.r_[inner, np.asarray(fp.point_col).ravel()[:14]][:14].astype(np.int32)
    blk, blk_ms, blk_wall = timed(ev, lambda: eng.correlation_block(rows, cols), a.repeats)
    n_groups = min(5000, P)
    groups = [[3 * p, 3 * p + 1, 3 * p + 2] for p in range(n_groups)]
    vals = eng.get_parameters()
    x0 = [list(vals[3 * p:3 * p + 3] + 1e-3) for p in range(n_groups)]
    gt, gt_ms, gt_wall = timed(ev, lambda: eng.parameter_tests(s2, groups, x0), a.repeats)

    L = engine.load_library()
    L.jaicov_debug_par_kernel_ms.argtypes = [C.c_void_p, C.c_uint32, C.c_double, C.c_int32, C.POINTER(C.c_double)]
    k = a.kernel_repeats
    ms = np.zeros((len(KERNELS), k + 3))
    rc = L.jaicov_debug_par_kernel_ms(eng._h, 0xFFFF, 0.9, k + 3, ms.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, rc
    ms = ms[:, 3:]                                               # the first three rounds are warm-up
    eng.close()
    n = U - d
    tri = n * (n + 1) // 2 * 8
    hbm_ms = 1e3 * tri / HBM_BYTES_PER_S
    med = {name: float(np.median(ms[i])) for i, name in enumerate(KERNELS)}
    res = {
        "scene": "small" if a.small else "cfg4", "order": U, "d": d, "repeats": a.repeats, "kernel_repeats": k,
        "maxima_event_ms": mx_ms, "maxima_wall_ms": mx_wall, "maxima_columns_with_partner": int((mx.partner >= 0).sum()),
        "maxima_status_nonzero": int((mx.status != 0).sum()), "maxima_largest_abs_rho": float(np.nanmax(np.abs(mx.rho))),
        "pairs_threshold": 0.9, "pairs_count": int(pr.count), "pairs_event_ms": pr_ms, "pairs_wall_ms": pr_wall,
        "block_shape": [int(rows.size), int(cols.size)], "block_event_ms": blk_ms, "block_wall_ms": blk_wall,
        "groups": n_groups, "groups_event_ms": gt_ms, "groups_wall_ms": gt_wall, "groups_status_nonzero": int((gt.status != 0).sum()),
        "kernel_median_ms": {name: round(v, 4) for name, v in med.items()},
        "kernel_min_ms": {name: round(float(ms[i].min()), 4) for i, name in enumerate(KERNELS)},
        "kernel_spread": {name: round(spread(ms[i]), 4) for i, name in enumerate(KERNELS)},
        "lower_triangle_bytes": tri, "hbm_ms_at_8TBps": round(hbm_ms, 4),
        "maxima_pass_over_yardstick": round(med["maxima_pass"] / med["yardstick_product"], 4),
        "maxima_tile_over_yardstick_tile": round(med["maxima_tile_kernel"] / med["yardstick_tile_kernel"], 4),
        "maxima_pass_hbm_share": round(hbm_ms / med["maxima_pass"], 4),
        "yardstick_hbm_share": round(hbm_ms / med["yardstick_product"], 4),
        "candidate_table_bytes": 16 * 128 * ((U + 127) // 128) ** 2,
    }
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
