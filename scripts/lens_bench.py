#!/usr/bin/env python3
"""Lens-distortion correction (include/jaicov_lens.h) of 1 000 000 image points of one camera, correct and distort, for the bundled
camera's coefficients (example.ior: C1 C2 B1 B2 A1 A2 A3), scene.DIST_FULL with depth and the Zernike set of tests/lens_reference.py,
and of 19 945 points (the bundled block's size) for the bundled camera.  The points are the images of ideal points spread over the
sensor, so that correct has the iteration a real measurement needs; dispersions go in and out in every case.

Reports per case: the call's wall time (host clock around engine.lens_correct / lens_distort, which synchronise; copies and
allocation included; median of --repeats after one warm-up), the kernel time by HIP events (ms_out), the statuses, the mean number of
solves, and the kernel's effective memory rate: the bytes it has to read and write per point (16 of xy, 4 of the camera index, 24 of
the dispersion and 8 of the depth where given in; 16 + 24 + 4 out, 4 more for the iteration count) over the kernel time.  There is no
parent and no reference implementation to compare a time with.  One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bundle_adjustment_amd  # noqa: E402,F401
from bundle_adjustment_amd import engine, scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import lens_reference as R
    bundled = [t for t in scene.DIST_FULL if t[0] in (R.CX, R.CY, R.BX, R.BY)] + \
        [(R.AI, 1, -1.09607e-4), (R.AI, 2, 1.49566e-7), (R.AI, 3, 0.0)]
    sets = {"bundled": (bundled, False), "full_with_depth": (scene.DIST_FULL, True), "zernike": (R.DIST_ZERNIKE, False)}
    cases = [(f"{name}_{a.points}", dist, depth, a.points) for name, (dist, depth) in sets.items()] + [("bundled_19945", bundled, False, 19945)]
    res = {"what": "jaicov_lens_correct / jaicov_lens_distort", "cases": {}}
    for name, dist, with_depth, n in cases:
        t = R.tables([dist])
        ideal = R.sensor_points(n, 41) + [scene.X0_EX, scene.Y0_EX]
        cam = np.zeros(n, np.int32)
        var = R.dispersions(n, 42)
        depth = np.random.default_rng(43).uniform(-3000.0, -400.0, n) if with_depth else None
        measured = engine.lens_distort(ideal, cam, *t, depth=depth)[0]
        for direction, f, xy in (("correct", engine.lens_correct, measured), ("distort", engine.lens_distort, ideal)):
            f(xy, cam, *t, var=var, depth=depth)                                # warm-up (code object load)
            walls, kms = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                out = f(xy, cam, *t, var=var, depth=depth, with_time=True)
                walls.append((time.perf_counter() - t0) * 1e3)
                kms.append(out[-1])
            bytes_per_point = 16 + 4 + 24 + (8 if with_depth else 0) + 16 + 24 + 4 + (4 if direction == "correct" else 0)
            k = float(np.median(kms))
            r = {"points": n, "coefficients": len(dist), "wall_ms_median": float(np.median(walls)), "wall_ms_all": walls,
                 "kernel_ms_median_hip_events": k, "kernel_ms_all": kms, "kernel_ns_per_point": k * 1e6 / n,
                 "bytes_per_point": bytes_per_point, "kernel_effective_GB_per_s": bytes_per_point * n / (k * 1e-3) / 1e9,
                 "status_counts": np.bincount(out[2], minlength=4).tolist()}
            if direction == "correct":
                r["solves_min_max_mean"] = [int(out[3].min()), int(out[3].max()), float(out[3].mean())]
                r["max_error_mm_against_the_ideal_points"] = float(np.abs(out[0] - ideal).max())
            res["cases"][f"{name}_{direction}"] = r
            print(name, direction, json.dumps({k_: w for k_, w in r.items() if not k_.endswith("_all")}), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
