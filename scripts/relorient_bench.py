#!/usr/bin/env python3
"""Relative orientation (include/jaicov_relorient.h) on 500 pairs of 500 common points and on a 50 000-pair batch of 12 points (500
different pairs a hundred times over).  The pairs are relorient_reference.plane_batch with a thickness of half the extent: a spatial
field of points seen by two cameras at oblique angles, noise-free pinhole observations + N(0, sigma) noise.  Each size runs without
rejection, and with rejection (threshold 5, sigma2apriori 1, min_points 8) after one gross error of 50 sigma in image b of every pair,
where every pair takes exactly one more round.

Reports per case: the call's wall time (host clock around engine.relorient_pairs, which synchronises; copies and allocation included;
median of --repeats after one warm-up), the kernel time by HIP events (ms_out), the statuses, Gauss-Newton steps, start kinds and
withdrawn observations, and the time per pair of the single-threaded numpy restatement (tests/relorient_reference.py) on the first
--cpu-pairs pairs of the same input, with the largest difference to it.  The restatement's time is a rough scale, not the reference:
the reference has no relative orientation, and there is no parent to compare with.  One JSON object on stdout (and in --out)."""
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


def with_gross_errors(batch, rng):
    ob = batch[0]
    bad = ob[:-1] + rng.integers(0, np.diff(ob))
    xb = batch[2].copy()
    xb[bad] += rng.choice([-1.0, 1.0], (bad.size, 2)) * 50.0 * scene.SIGMA_IMG
    return batch[:2] + (xb,) + batch[3:]


def tiled(batch, times):
    ob = batch[0]
    n = ob.size - 1
    begin = np.concatenate([[0], np.cumsum(np.tile(np.diff(ob), times))]).astype(np.int32)
    assert begin.size - 1 == n * times
    return (begin,) + tuple(np.tile(a, (times, 1)) for a in batch[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-pairs", type=int, default=8, help="pairs given to the numpy restatement (0: skip it)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import relorient_reference as R
    rng = np.random.default_rng(20261019)
    big = R.plane_batch([500] * 500, thickness=0.5, seed=21, noise=scene.SIGMA_IMG)[0]
    small = R.plane_batch([12] * 500, thickness=0.5, seed=22, noise=scene.SIGMA_IMG)[0]
    rej = dict(reject_threshold=5.0, min_points=8)
    cases = {
        "pairs_500x500": (big, {}),
        "pairs_500x500_rejection": (with_gross_errors(big, rng), rej),
        "pairs_50000x12": (tiled(small, 100), {}),
        "pairs_50000x12_rejection": (tiled(with_gross_errors(small, rng), 100), rej),
    }
    res = {"what": "jaicov_relorient_pairs", "cases": {}}
    for name, (b, kw) in cases.items():
        engine.relorient_pairs(*b, **kw)                                        # warm-up (code object load)
        walls, kms = [], []
        for _ in range(a.repeats):
            t = time.perf_counter()
            out, st, it, kind, used, q, ms = engine.relorient_pairs(*b, with_time=True, **kw)
            walls.append((time.perf_counter() - t) * 1e3)
            kms.append(ms)
        n_pairs = int(b[0].size - 1)
        r = {"pairs": n_pairs, "observations": int(b[0][-1]), "points_per_pair": float(b[0][-1] / n_pairs), "options": kw,
             "wall_ms_median": float(np.median(walls)), "wall_ms_all": walls, "kernel_ms_median_hip_events": float(np.median(kms)),
             "kernel_us_per_pair": float(np.median(kms)) * 1e3 / n_pairs,
             "status_counts": np.bincount(st, minlength=5).tolist(), "start_kind_counts": np.bincount(kind, minlength=3).tolist(),
             "steps_min_max_mean": [int(it.min()), int(it.max()), float(it.mean())], "observations_withdrawn": int((used == 0).sum())}
        if a.cpu_pairs > 0:
            n = min(a.cpu_pairs, n_pairs)
            e = b[0][n]
            t = time.perf_counter()
            ref = R.relorient(b[0][:n + 1], b[1][:e], b[2][:e], b[3][:e], b[4][:e], b[5][:n], b[6][:n], **kw)
            secs = time.perf_counter() - t
            r["cpu_restatement_pairs"] = n
            r["cpu_restatement_ms_per_pair"] = secs * 1e3 / n
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
