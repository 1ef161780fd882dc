#!/usr/bin/env python3
"""jaicov_vce_run (include/jaicov_vce.h) against the host path it replaces.

At config 2, and at config 4 after one FULL_EXPANDED pass, with the groups "by image" and the control group: the synchronous
call's wall time (the reliability run it begins with included; that run alone is reported beside it), medians of `--repeats` calls
after two warm-up calls, with the run-to-run spread ((p90 - p10) / median), and the device time of vce_block_kernel,
vce_small_kernel and vce_group_kernel by HIP events on the engine's stream (jaicov_debug_vce_timing).  For vce_block_kernel the
bytes of the lower triangles it reads give a bandwidth.

The host path: get_block_weight of every dense image block plus numpy's v_b' P_b v_b on the residuals of a reliability run that is
already on the host -- what a caller had to do before, the export of every weight matrix included.  The device's Omega_g is held
against the host figures.  One JSON object on stdout (and in --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bundle_adjustment_amd  # noqa: E402,F401
from bundle_adjustment_amd import engine, scene  # noqa: E402


def spread(x):
    x = np.sort(np.asarray(x))
    return float((np.percentile(x, 90) - np.percentile(x, 10)) / np.median(x))


def inverting_pass(fp):
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(engine.INVERT_FULL_EXPANDED)
    eng.build(fp.sigma2apriori, 0.0)
    dx = eng.solve(engine.INVERT_FULL_EXPANDED)
    return eng, dx


def timing(eng, on):
    ms = (C.c_float * 3)()
    assert eng.L.jaicov_debug_vce_timing(eng._h, int(on), ms) == 0
    return [float(x) for x in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="config 2 only: a quick check")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {"repeats": a.repeats, "workloads": {}}
    for name in ("cfg2",) if a.small else ("cfg2", "cfg4"):
        fp = scene.config(name)
        eng, dx = inverting_pass(fp)
        s0 = fp.sigma2apriori
        I = fp.n_images
        groups = engine.VceGroups(fp.ip_image.astype(np.int32), None, np.full(fp.n_direct_groups, I, np.int32), I + 1, None)
        for _ in range(2):
            eng.variance_components(groups, dx=dx)
        timing(eng, True)
        wall, parts, rel_wall = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            vc = eng.variance_components(groups, dx=dx)
            wall.append(1e3 * (time.perf_counter() - t0))
            parts.append(timing(eng, True))
            t0 = time.perf_counter()
            rel = eng.reliability(s0, dx)
            rel_wall.append(1e3 * (time.perf_counter() - t0))
        timing(eng, False)
        parts = np.array(parts)
        # the host path: every dense weight matrix exported, the quadratic forms in numpy
        host = []
        omega_host = np.zeros(fp.n_image_blocks)
        for _ in range(a.repeats if fp.n_image_blocks else 0):
            t0 = time.perf_counter()
            for b in range(fp.n_image_blocks):
                lo, hi = 2 * int(fp.blk_ip_begin[b]), 2 * int(fp.blk_ip_begin[b + 1])
                vb = rel.v[lo:hi]
                omega_host[b] = s0 * (vb @ (eng.get_block_weight(b) @ vb))
            host.append(1e3 * (time.perf_counter() - t0))
        tri_bytes = 8 * sum((2 * int(m)) * (2 * int(m) + 1) // 2 for m in np.diff(fp.blk_ip_begin))
        r = {"order": int(fp.n_unknowns), "rows": int(fp.n_observations), "groups": int(groups.n_groups), "dense_image_blocks": int(fp.n_image_blocks),
             "call_wall_ms": round(float(np.median(wall)), 3), "call_wall_spread": round(spread(wall), 4),
             "reliability_run_alone_wall_ms": round(float(np.median(rel_wall)), 3),
             "block_kernel_ms": round(float(np.median(parts[:, 0])), 4), "block_kernel_spread": round(spread(parts[:, 0]), 4),
             "small_kernel_ms": round(float(np.median(parts[:, 1])), 4), "small_kernel_spread": round(spread(parts[:, 1]), 4),
             "group_kernel_ms": round(float(np.median(parts[:, 2])), 4), "group_kernel_spread": round(spread(parts[:, 2]), 4),
             "lower_triangle_bytes": int(tri_bytes)}
        if fp.n_image_blocks:
            r["block_kernel_GB_per_s"] = round(tri_bytes / (1e6 * float(np.median(parts[:, 0]))), 1)
            r["host_path_ms"] = round(float(np.median(host)), 1)
            r["host_path_spread"] = round(spread(host), 4)
            # images are the groups 0 .. I - 1 and, with a dense dispersion per image, the blocks
            r["device_omega_vs_host_max_rel"] = float(np.max(np.abs(vc.omega[:fp.n_image_blocks] - omega_host) / np.abs(omega_host)))
        res["workloads"][name] = r
        eng.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
