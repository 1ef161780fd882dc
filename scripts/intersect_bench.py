#!/usr/bin/env python3
"""Forward intersection (include/jaicov_intersect.h) at config 4's geometry (500 images, 5 000 points x ~50 rays, scene.make_scene with
config 4's arguments and diagonal noise, orientations = truth) and at a 50 000-point batch (the same rays ten times over, each copy with
its own noise).  Each size runs without rejection on the scene's own observations (noise and distortion), and with rejection
(threshold 5, sigma2apriori 1, min_rays 3) on noise-free rays + N(0, 0.0005) noise + one gross error of 1 mm per point, where every point
takes exactly one more round.

Reports per case: the call's wall time (host clock around engine.intersect_points, which synchronises; copies and allocation
included; median of --repeats after one warm-up), the kernel time by HIP events (ms_out: the per-image prologue and the per-point
kernel), the statuses, iterations and withdrawn rays, and the time of the single-threaded numpy restatement
(tests/intersect_reference.py, one point at a time) on the first --cpu-points points of the same input, scaled to the batch, with the
largest difference to it.  The restatement's time is a rough scale, not the reference: the reference has no forward intersection.
One JSON object on stdout (and in --out)."""
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


def tiled(batch, times, rng):
    rb, ri, xy, var = batch
    n = rb[-1]
    begin = np.concatenate([[0]] + [rb[1:] + k * n for k in range(times)]).astype(np.int32)
    noise = np.concatenate([np.zeros_like(xy)] + [rng.normal(0, scene.SIGMA_IMG, xy.shape) for _ in range(times - 1)])
    return begin, np.tile(ri, times), np.tile(xy, (times, 1)) + noise, np.tile(var, (times, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-points", type=int, default=1000, help="points given to the numpy restatement (0: skip it)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import intersect_reference as X
    fp = scene.make_scene(500, 5000, 500, dist=scene.DIST_FULL, weights="diag", n_control=15)
    rb, ri, xy, var, io, eo, _ = X.batch_from_scene(fp)
    gb, gi, gxy, gvar, _, _, planted = X.gross_error_batch(fp)
    rng = np.random.default_rng(20261017)
    cases = {
        "cfg4_5000": ((rb, ri, xy, var), {}),
        "cfg4_5000_rejection": ((gb, gi, gxy, gvar), dict(reject_threshold=5.0, min_rays=3)),
        "batch_50000": (tiled((rb, ri, xy, var), 10, rng), {}),
        "batch_50000_rejection": (tiled((gb, gi, gxy, gvar), 10, rng), dict(reject_threshold=5.0, min_rays=3)),
    }
    res = {"what": "jaicov_isect_points", "cases": {}}
    for name, ((b, i, x, v), kw) in cases.items():
        engine.intersect_points(b, i, x, v, io, eo, **kw)                       # warm-up (code object load)
        walls, kms = [], []
        for _ in range(a.repeats):
            t = time.perf_counter()
            out, st, it, used, q, ms = engine.intersect_points(b, i, x, v, io, eo, with_time=True, **kw)
            walls.append((time.perf_counter() - t) * 1e3)
            kms.append(ms)
        r = {"points": int(b.size - 1), "rays": int(b[-1]), "rays_per_point_mean": float(b[-1] / (b.size - 1)), "options": kw,
             "wall_ms_median": float(np.median(walls)), "wall_ms_all": walls, "kernel_ms_median_hip_events": float(np.median(kms)),
             "status_counts": np.bincount(st, minlength=5).tolist(), "iterations_min_max_mean": [int(it.min()), int(it.max()), float(it.mean())],
             "rays_withdrawn": int((used == 0).sum())}
        if a.cpu_points > 0:
            n = min(a.cpu_points, b.size - 1)
            e = b[n]
            t = time.perf_counter()
            ro, rst, rit, rused, rq = X.intersect(b[:n + 1], i[:e], x[:e], v[:e], io, eo, **kw)
            secs = time.perf_counter() - t
            r["cpu_restatement_points"] = n
            r["cpu_restatement_s_scaled_to_batch"] = secs * (b.size - 1) / n
            r["status_equal"] = bool(np.array_equal(st[:n], rst) and np.array_equal(it[:n], rit) and np.array_equal(used[:e], rused))
            col = np.abs(ro).max(0)
            col[10] = 1.0
            r["max_rel_diff_to_restatement"] = float((np.abs(out[:n] - ro) / np.where(col > 0, col, 1.0)).max())
        res["cases"][name] = r
        print(name, json.dumps({k: w for k, w in r.items() if k != "wall_ms_all"}), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
