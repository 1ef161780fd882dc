#!/usr/bin/env python3
"""Absolute orientation (include/jaicov_simil.h) on 500 models of 500 points and on a 50 000-model batch of 12 points (500 different
models a hundred times over).  The models are similarity_reference.models: random transformations of spatial point fields, every point
with its own fully populated cofactor matrices on both sides and noise drawn from them.  Each size runs without rejection, and with
rejection (threshold 6, min_points 5) after one gross error of 100 sigma on one point of every model, where every model takes exactly
one more round.

Reports per case: the call's wall time (host clock around engine.similarity_models, which synchronises; copies and allocation
included; median of --repeats after one warm-up), the kernel time by HIP events (ms_out), the statuses, Gauss-Newton steps per model
and withdrawn points, and the time per model of the single-threaded numpy restatement (tests/similarity_reference.py) on the first
--cpu-models models of the same input, with the largest difference to it.  The restatement's time is a rough scale, not the
reference: the reference has no absolute orientation, and there is no parent to compare with.  jaicov_simil_apply is timed on the
larger input's points (wall time only: the call has no ms_out).  One JSON object on stdout (and in --out)."""
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
from bundle_adjustment_amd import engine  # noqa: E402


def with_gross_errors(batch, rng, sigma):
    pb = batch[0]
    bad = pb[:-1] + rng.integers(0, np.diff(pb))
    dst = batch[2].copy()
    dst[bad] += rng.choice([-1.0, 1.0], (bad.size, 3)) * 100.0 * sigma
    return batch[:2] + (dst,) + batch[3:]


def tiled(batch, times):
    pb = batch[0]
    begin = np.concatenate([[0], np.cumsum(np.tile(np.diff(pb), times))]).astype(np.int32)
    return (begin,) + tuple(np.tile(a, (times, 1)) for a in batch[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-models", type=int, default=8, help="models given to the numpy restatement (0: skip it)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import similarity_reference as S
    rng = np.random.default_rng(20261019)
    big = S.models([500] * 500, seed=31, sigma=S.SIGMA)[0]
    small = S.models([12] * 500, seed=32, sigma=S.SIGMA)[0]
    rej = dict(reject_threshold=6.0, min_points=5)
    cases = {
        "models_500x500": (big, {}),
        "models_500x500_rejection": (with_gross_errors(big, rng, S.SIGMA), rej),
        "models_50000x12": (tiled(small, 100), {}),
        "models_50000x12_rejection": (tiled(with_gross_errors(small, rng, S.SIGMA), 100), rej),
    }
    res = {"what": "jaicov_simil_models", "cases": {}}
    for name, (b, kw) in cases.items():
        engine.similarity_models(*b, **kw)                                      # warm-up (code object load)
        walls, kms = [], []
        for _ in range(a.repeats):
            t = time.perf_counter()
            out, st, it, kind, used, q, ms = engine.similarity_models(*b, with_time=True, **kw)
            walls.append((time.perf_counter() - t) * 1e3)
            kms.append(ms)
        n_models = int(b[0].size - 1)
        r = {"models": n_models, "points": int(b[0][-1]), "points_per_model": float(b[0][-1] / n_models), "options": kw,
             "wall_ms_median": float(np.median(walls)), "wall_ms_all": walls, "kernel_ms_median_hip_events": float(np.median(kms)),
             "kernel_us_per_model": float(np.median(kms)) * 1e3 / n_models,
             "status_counts": np.bincount(st, minlength=5).tolist(), "start_kind_counts": np.bincount(kind, minlength=2).tolist(),
             "steps_min_max_mean": [int(it.min()), int(it.max()), float(it.mean())], "points_withdrawn": int((used == 0).sum())}
        if a.cpu_models > 0:
            n = min(a.cpu_models, n_models)
            e = b[0][n]
            t = time.perf_counter()
            ref = S.similarity(b[0][:n + 1], b[1][:e], b[2][:e], b[3][:e], b[4][:e], b[5][:n], **kw)
            secs = time.perf_counter() - t
            r["cpu_restatement_models"] = n
            r["cpu_restatement_ms_per_model"] = secs * 1e3 / n
            r["status_equal"] = bool(np.array_equal(st[:n], ref[1]) and np.array_equal(it[:n], ref[2]) and np.array_equal(kind[:n], ref[3]) and
                                     np.array_equal(used[:e], ref[4]))
            ok = ~np.isnan(ref[0])
            col = np.nanmax(np.abs(np.where(ok, ref[0], np.nan)), axis=0)
            r["max_rel_diff_to_restatement"] = float((np.abs(np.where(ok, out[:n] - ref[0], 0.0)) / np.where(col > 0, col, 1.0)).max())
        res["cases"][name] = r
        print(name, json.dumps({k: w for k, w in r.items() if k != "wall_ms_all"}), file=sys.stderr)
    out = engine.similarity_models(*big)[0]
    engine.similarity_apply(out, big[0], big[1], big[3])
    walls = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        engine.similarity_apply(out, big[0], big[1], big[3])
        walls.append((time.perf_counter() - t) * 1e3)
    res["apply_500x500_points_with_cofactors"] = {"points": int(big[0][-1]), "wall_ms_median": float(np.median(walls)), "wall_ms_all": walls}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
