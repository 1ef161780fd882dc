#!/usr/bin/env python3
"""Device-side datum transformation at config 4's size (include/jaicov_datum.h): the free-network variant of config 4 (no control
points, a scale bar, d = 6), FULL_EXPANDED, datum all points -> every second point.

Reports the time of jaicov_datum_transform (host wall clock around the call, which synchronises; the host algebra and the copies
of G^, Y and (Z, Y~) included; the first call also allocates its work buffers), the compulsory bytes (two reads and one write of
the lower triangle) and their fraction of 8 TB/s at that wall time, the time of jaicov_datum_apply, and the baseline: an
inverting FULL_EXPANDED build and solve in datum B, i.e. what it takes today to get Qxx in that datum (an engine whose problem
has datum B, after one non-inverting pass; the same build and solve in datum A is reported too).  One JSON object on stdout (and
in --out)."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bundle_adjustment_amd  # noqa: E402,F401
from bundle_adjustment_amd import engine, scene  # noqa: E402


def inverting_pass_ms(eng, fp):
    """one non-inverting pass (first touch of the pass's buffers), then the timed inverting FULL_EXPANDED build + solve"""
    eng.set_parameters(fp.values)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(engine.INVERT_NONE)
    eng.prepare_inverse(engine.INVERT_FULL_EXPANDED)
    t0 = time.perf_counter()
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(engine.INVERT_FULL_EXPANDED)
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a small scene (8 x 60) instead of config 4's size: a quick check")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.small:
        fp = scene.make_scene(8, 60, 40, dist=scene.DIST_FULL, weights="block", n_control=0, scale_bar=True)
    else:
        fp = scene.make_scene(500, 5000, 500, dist=scene.DIST_FULL, weights="block", n_control=0, scale_bar=True)
    P, U, d = fp.point_datum.size, fp.n_unknowns, fp.rank_defect
    mask_a = np.ones(P, np.uint8)
    mask_b = np.zeros(P, np.uint8); mask_b[::2] = 1
    eng = engine.Engine(dataclasses.replace(fp, point_datum=mask_a), device=0)
    pass_a_ms = inverting_pass_ms(eng, fp)
    n = eng.cofactor_order()
    assert n == U
    run_ms = []
    for k in range(a.repeats + 1):                         # A -> B, B -> A, ...: the same work each time
        t0 = time.perf_counter()
        eng.datum_transform(mask_b if k % 2 == 0 else mask_a)
        run_ms.append(1e3 * (time.perf_counter() - t0))
    v = np.random.default_rng(1).normal(size=n)
    t0 = time.perf_counter()
    eng.datum_apply(v)
    apply_ms = 1e3 * (time.perf_counter() - t0)
    eng.close()
    engb = engine.Engine(dataclasses.replace(fp, point_datum=mask_b), device=0)
    pass_b_ms = inverting_pass_ms(engb, fp)
    engb.close()
    tri = n * (n + 1) // 2 * 8
    nbk = -(-n // 128)
    table = nbk * nbk * 128 * d * 8
    best = min(run_ms[1:])
    res = {
        "scene": "small" if a.small else "cfg4_free", "U": U, "d": d, "points": P, "datum_a_points": int(mask_a.sum()),
        "datum_b_points": int(mask_b.sum()),
        "transform_ms": [round(x, 3) for x in run_ms], "transform_ms_best": round(best, 3), "apply_ms": round(apply_ms, 3),
        "baseline_full_expanded_pass_datum_b_ms": round(pass_b_ms, 3), "full_expanded_pass_datum_a_ms": round(pass_a_ms, 3),
        "transform_over_baseline": round(best / pass_b_ms, 4),
        "compulsory_bytes": 3 * tri, "partial_table_bytes": 2 * table, "host_copy_bytes": 8 * d * 5 * n,
        "fraction_of_8TBps_at_wall_time": round(3 * tri / (best * 1e-3) / 8e12, 4),
    }
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
