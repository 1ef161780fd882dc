#!/usr/bin/env python3
"""Spatial resection (include/jaicov_resect.h) at config 4's geometry (500 images x 500 points, scene.make_scene with config 4's
arguments and diagonal noise, object points = truth, linear start) and at a 50 000-image batch of 12 points (every image of that scene
a hundred times over, each copy with its own 12 of the image's points).  Each size runs without rejection on the scene's own
observations (noise and distortion), and with rejection (threshold 5, sigma2apriori 1, min_points 6) on noise-free observations +
N(0, sigma) noise + one gross error of 50 sigma per image, where every image takes exactly one more round.

Reports per case: the call's wall time (host clock around engine.resect_images, which synchronises; copies and allocation included;
median of --repeats after one warm-up), the kernel time by HIP events (ms_out), the statuses, iterations, start kinds and withdrawn
observations, and the time per image of the single-threaded numpy restatement (tests/resection_reference.py, one image at a time) on
the first --cpu-images images of the same input, with the largest difference to it.  The restatement's time is a rough scale, not the
reference: the reference has no resection.  One JSON object on stdout (and in --out)."""
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


def small_images(batch, times, points, rng):
    """every image `times` times over, each copy with `points` of the image's observations drawn without replacement"""
    ob, xy, xyz, var, io = batch
    pick = np.concatenate([ob[g] + np.sort(rng.choice(ob[g + 1] - ob[g], points, replace=False))
                           for _ in range(times) for g in range(ob.size - 1)])
    begin = (np.arange(times * (ob.size - 1) + 1) * points).astype(np.int32)
    return begin, xy[pick], xyz[pick], var[pick], np.tile(io, (times, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-images", type=int, default=100, help="images given to the numpy restatement (0: skip it)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import resection_reference as X
    fp = scene.make_scene(500, 5000, 500, dist=scene.DIST_FULL, weights="diag", n_control=15)
    ob, xy, xyz, var, io, _ = X.batch_from_scene(fp)
    gb, gxy, gxyz, gvar, gio, _, planted = X.gross_error_batch(fp)
    rng = np.random.default_rng(20261018)
    small = small_images((ob, xy, xyz, var, io), 100, 12, rng)
    gsmall = list(small_images((gb, gxy, gxyz, gvar, gio), 100, 12, rng))
    bad = gsmall[0][:-1] + rng.integers(0, 12, gsmall[0].size - 1)              # one gross error of 50 sigma per small image
    gsmall[1] = gsmall[1].copy()
    gsmall[1][bad] += rng.choice([-1.0, 1.0], (bad.size, 2)) * 50.0 * np.sqrt(gsmall[3][bad, :2])
    rej = dict(reject_threshold=5.0, min_points=6)
    cases = {
        "cfg4_500x500": ((ob, xy, xyz, var, io), {}),
        "cfg4_500x500_rejection": ((gb, gxy, gxyz, gvar, gio), rej),
        "batch_50000x12": (small, {}),
        "batch_50000x12_rejection": (tuple(gsmall), rej),
    }
    res = {"what": "jaicov_resect_images", "cases": {}}
    for name, ((b, x, p, v, i), kw) in cases.items():
        engine.resect_images(b, x, p, v, i, **kw)                               # warm-up (code object load)
        walls, kms = [], []
        for _ in range(a.repeats):
            t = time.perf_counter()
            out, st, it, kind, used, q, ms = engine.resect_images(b, x, p, v, i, with_time=True, **kw)
            walls.append((time.perf_counter() - t) * 1e3)
            kms.append(ms)
        n_img = int(b.size - 1)
        r = {"images": n_img, "observations": int(b[-1]), "points_per_image": float(b[-1] / n_img), "options": kw,
             "wall_ms_median": float(np.median(walls)), "wall_ms_all": walls, "kernel_ms_median_hip_events": float(np.median(kms)),
             "kernel_us_per_image": float(np.median(kms)) * 1e3 / n_img,
             "status_counts": np.bincount(st, minlength=5).tolist(), "start_kind_counts": np.bincount(kind, minlength=3).tolist(),
             "iterations_min_max_mean": [int(it.min()), int(it.max()), float(it.mean())], "observations_withdrawn": int((used == 0).sum())}
        if a.cpu_images > 0:
            n = min(a.cpu_images, n_img)
            e = b[n]
            t = time.perf_counter()
            ref = X.resect(b[:n + 1], x[:e], p[:e], v[:e], i[:n], **kw)
            secs = time.perf_counter() - t
            r["cpu_restatement_images"] = n
            r["cpu_restatement_ms_per_image"] = secs * 1e3 / n
            r["status_equal"] = bool(np.array_equal(st[:n], ref[1]) and np.array_equal(it[:n], ref[2]) and np.array_equal(kind[:n], ref[3]) and
                                     np.array_equal(used[:e], ref[4]))
            ok = ~np.isnan(ref[0])
            col = np.nanmax(np.abs(np.where(ok, ref[0], np.nan)), axis=0)
            r["max_rel_diff_to_restatement"] = float((np.abs(np.where(ok, out[:n] - ref[0], 0.0)) / np.where(col > 0, col, 1.0)).max())
        res["cases"][name] = r
        print(name, json.dumps({k: w for k, w in r.items() if k != "wall_ms_all"}), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
