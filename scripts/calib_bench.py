#!/usr/bin/env python3
"""jaicov_calib_field / jaicov_calib_compare (include/jaicov_calibration.h) on sensor grids.

Two scenes after one inverting pass: config 2 (one camera, 11 coefficients, EO-reduced matrix) and the two-camera scene of the tests
(11 and 5 coefficients).  Per scene and grid (64 x 64 and 1 024 x 1 024 nodes over 36 x 24 mm): the field of camera 0, the
comparison of camera 0 with its own values shifted by 1e-5 as a certificate (per-node output and summary, and the summary alone),
and on the two-camera scene the comparison of its two cameras.  Reported per call: the synchronous call's wall time (host sort, upload,
rows, kernels, download, scatter), medians of `--repeats` calls after two warm-up calls, with the run-to-run spread
((p90 - p10) / median), and the three device parts by HIP events on the engine's stream (jaicov_debug_calib_timing: the node and rows
kernels, calib_cov_kernel, calib_summary_kernel).  One JSON object on stdout (and in --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import bundle_adjustment_amd  # noqa: E402,F401
from bundle_adjustment_amd import engine, scene  # noqa: E402
import helpers  # noqa: E402


def spread(x):
    x = np.sort(np.asarray(x))
    return float((np.percentile(x, 90) - np.percentile(x, 10)) / np.median(x))


def inverting_pass(fp, mode):
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(mode)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(mode)
    return eng


def timing(eng, on):
    ms = (C.c_float * 3)()
    assert eng.L.jaicov_debug_calib_timing(eng._h, int(on), ms) == 0
    return [float(x) for x in ms]


def measured(eng, call, repeats):
    call(); call()                                               # warm-up: allocates the work buffers, reads the camera tables once
    timing(eng, True)
    wall, parts = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        wall.append(1e3 * (time.perf_counter() - t0))
        parts.append(timing(eng, True))
    timing(eng, False)
    parts = np.array(parts)
    return {"call_wall_ms": round(float(np.median(wall)), 3), "call_wall_spread": round(spread(wall), 4),
            "rows_ms": round(float(np.median(parts[:, 0])), 4), "cov_kernel_ms": round(float(np.median(parts[:, 1])), 4),
            "cov_kernel_spread": round(spread(parts[:, 1]), 4), "summary_kernel_ms": round(float(np.median(parts[:, 2])), 4)}


def camera_values(fp, values, k):
    j0, j1 = int(fp.cam_dist_begin[k]), int(fp.cam_dist_begin[k + 1])
    return np.concatenate([values[fp.slot_io(k):fp.slot_io(k) + 3], values[fp.slot_dist(j0):fp.slot_dist(j0) + j1 - j0]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="the 64 x 64 grid only: a quick check")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res = {"repeats": a.repeats, "workloads": {}}
    scenes = {"cfg2": (scene.config("cfg2"), engine.INVERT_REDUCED), "two_camera": (helpers.two_camera_scene()[0], engine.INVERT_FULL_EXPANDED)}
    for name, (fp, mode) in scenes.items():
        eng = inverting_pass(fp, mode)
        s2 = fp.sigma2apriori
        ref = camera_values(fp, eng.get_parameters(), 0) * (1.0 + 1e-5)
        for side in (64,) if a.small else (64, 1024):
            xy = engine.sensor_grid(36.0, 24.0, side, side)
            depth = np.full(xy.shape[0], -1500.0)
            cam = np.zeros(xy.shape[0], np.int32)
            calls = {"field": lambda: eng.calibration_field(s2, cam, xy, depth),
                     "compare_certificate": lambda: eng.calibration_compare(0, 0, xy, depth, ref_values=ref),
                     "compare_certificate_summary_only": lambda: eng.calibration_compare(0, 0, xy, depth, ref_values=ref, nodes=False)}
            if fp.n_cameras > 1:
                calls["compare_cameras"] = lambda: eng.calibration_compare(0, 1, xy, depth)
                calls["compare_cameras_summary_only"] = lambda: eng.calibration_compare(0, 1, xy, depth, nodes=False)
            for what, call in calls.items():
                r = measured(eng, call, a.repeats)
                r.update({"nodes": int(xy.shape[0]), "order": int(eng.cofactor_order()), "columns": [int(3 + fp.cam_dist_begin[k + 1] - fp.cam_dist_begin[k])
                                                                                                      for k in range(fp.n_cameras)]})
                if what.startswith("compare"):
                    s = call().summary
                    r.update({"rms": float(s.rms), "rms_expected": float(s.rms_expected), "max_T_prio": float(s.max_T_prio), "n_finite": int(s.n_finite)})
                res["workloads"][f"{name}_{side}x{side}_{what}"] = r
        eng.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
