#!/usr/bin/env python3
"""jaicov_newpt_intersect (include/jaicov_newpoints.h) against the host path it replaces.

At config 2, and at config 4 after one FULL_EXPANDED pass: `--points` new points with 4, 8 and 32 rays each (distinct images while
the block has them) and the lengths between consecutive points.  Reported per workload: the synchronous call's wall time (host
column lists, upload, the Gauss-Newton loop, kernels, download), medians of `--repeats` calls after four warm-up calls (the first allocates
the work buffers), with the run-to-run spread ((p90 - p10) / median), the device parts by HIP events on the engine's stream
(jaicov_debug_newpt_timing: the Gauss-Newton loop of rows and steps, newpt_gain_kernel, newpt_pair_kernel) and the steps enqueued.

The host path: per point the export of its |S| x |S| sub-block through get_cofactor_sub, the oracle's rows through the auxiliary
problem of tests/newpoint_reference.py at the device's X and the reference's numpy evaluation -- one evaluation, no iteration, on
`--sample` points, extrapolated to all of them; per pair the export of the union's sub-block and the reference's pair figures.  The
device's Q_XX and q_L are held against those host figures in units of the reference's bounds.  One JSON object on stdout (and in
--out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import bundle_adjustment_amd  # noqa: E402,F401
from bundle_adjustment_amd import engine, scene  # noqa: E402
import oracle as oracle_mod  # noqa: E402
import newpoint_reference as R  # noqa: E402


def spread(x):
    x = np.sort(np.asarray(x))
    return float((np.percentile(x, 90) - np.percentile(x, 10)) / np.median(x))


def inverting_pass(fp):
    eng = engine.Engine(fp, device=0)
    eng.L.jaicov_debug_newpt_timing.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    eng.set_parameters(fp.values)
    eng.prepare_inverse(engine.INVERT_FULL_EXPANDED)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(engine.INVERT_FULL_EXPANDED)
    return eng


def timing(eng, on):
    ms = (C.c_float * 3)(); steps = C.c_int32()
    assert eng.L.jaicov_debug_newpt_timing(eng._h, int(on), ms, C.byref(steps)) == 0
    return [float(x) for x in ms] + [float(steps.value)]


def measured(eng, call, repeats):
    for _ in range(4):                                           # warm-up: allocates the work buffers, reads the tables once; single calls
        call()                                                   # among the first three after the buffers have grown take up to 25 ms
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
            "gauss_newton_loop_ms": round(float(np.median(parts[:, 0])), 4), "steps_enqueued": int(parts[0, 3]),
            "gain_kernel_ms": round(float(np.median(parts[:, 1])), 4), "gain_kernel_spread": round(spread(parts[:, 1]), 4),
            "pair_kernel_ms": round(float(np.median(parts[:, 2])), 4)}


class SubMatrix:
    """a sub-block of the cofactor matrix that answers Q[np.ix_(cols, cols)] in the matrix's own column numbers"""

    def __init__(self, cols, block):
        self.cols, self.block = np.asarray(cols), block

    def __getitem__(self, key):
        r = np.searchsorted(self.cols, np.asarray(key[0]).ravel()); c = np.searchsorted(self.cols, np.asarray(key[1]).ravel())
        return self.block[np.ix_(r, c)]


def columns_of(fp, images):
    c = np.unique(np.concatenate([R.shared_columns(fp, im) for im in images]))
    return c[c >= 0].astype(np.int32)


def host_path(eng, fp, got, rb, ri, xy, disp, pairs, sample):
    """(ms per point, ms per pair, worst Q_XX and q_L of the device in units of the reference's bounds) on `sample` points and pairs"""
    s0 = fp.sigma2apriori
    pick = np.linspace(0, len(rb) - 2, sample).astype(int)
    worst_x = worst_p = 0.0
    t0 = time.perf_counter()
    members = {}
    for i in pick:
        k = slice(rb[i], rb[i + 1])
        cols = columns_of(fp, ri[k])
        Q = SubMatrix(cols, eng.get_cofactor_sub(cols))
        w, J = R.rows(oracle_mod, fp, fp.values, got.xyz[i:i + 1], np.array([0, rb[i + 1] - rb[i]], np.int32), ri[k], xy[k])
        e = R.evaluate(fp, Q, w, J, ri[k], disp[k], s0)
        members[int(i)] = e
        worst_x = max(worst_x, float((np.abs(got.cof[i] - R.sym6(e["Q_XX"])) / R.sym6(e["E_XX"])).max()))
    per_point = 1e3 * (time.perf_counter() - t0) / pick.size
    t0 = time.perf_counter()
    n_pairs = 0
    for j, (a, b) in enumerate(pairs):
        if int(a) not in members or int(b) not in members:
            continue
        cols = np.union1d(members[int(a)]["cols"], members[int(b)]["cols"]).astype(np.int32)
        Q = SubMatrix(cols, eng.get_cofactor_sub(cols))
        ref, _, bound, _ = R.pair_figures(Q, R.new_member(got.xyz[a], members[int(a)]), R.new_member(got.xyz[b], members[int(b)]), 1.0)
        worst_p = max(worst_p, abs(got.lengths[j, 5] - ref[5]) / bound[0])
        n_pairs += 1
    per_pair = 1e3 * (time.perf_counter() - t0) / max(n_pairs, 1)
    return per_point, per_pair, worst_x, worst_p, int(pick.size), n_pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--sample", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="config 2 only: a quick check")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    oracle_mod.build()
    res = {"repeats": a.repeats, "points": a.points, "workloads": {}}
    for name in ("cfg2",) if a.small else ("cfg2", "cfg4"):
        fp = scene.config(name)
        eng = inverting_pass(fp)
        for m in (4, 8, 32):
            X = R.new_points(fp, a.points)
            rb, ri = R.rays_of(fp, np.full(a.points, m))
            xy = R.measure(fp, fp.values, X, rb, ri, sigma=0.0005)
            disp = R.dispersions(fp, ri.size)
            start = X + 2.0
            pairs = np.stack([np.arange(a.points - 1), np.arange(1, a.points)], 1).astype(np.int32)
            r = measured(eng, lambda: eng.intersect_new_points(1.0, rb, ri, xy, disp, start=start, pairs=pairs), a.repeats)
            got = eng.intersect_new_points(1.0, rb, ri, xy, disp, start=start, pairs=pairs)
            # the first `sample` points, so that the pairs between neighbours are sampled too
            ns = min(a.sample, a.points)
            per_point, per_pair, wx, wp, n_s, n_p = host_path(eng, fp, got, rb[:ns + 1], ri[:rb[ns]], xy[:rb[ns]], disp[:rb[ns]], pairs[:ns - 1], ns)
            r.update({"rays_per_point": m, "pairs": int(len(pairs)), "order": int(fp.n_unknowns),
                      "columns_per_point_mean": round(float(np.mean([columns_of(fp, ri[rb[i]:rb[i + 1]]).size for i in range(min(a.points, 50))])), 1),
                      "status_nonzero": int((got.status != 0).sum()), "iterations_max": int(got.iterations.max()),
                      "pair_status_nonzero": int((got.length_status != 0).sum()),
                      "host_ms_per_point": round(per_point, 3), "host_ms_per_pair": round(per_pair, 3), "host_points_sampled": n_s,
                      "host_pairs_sampled": n_p, "host_extrapolated_ms": round(per_point * a.points + per_pair * len(pairs), 1),
                      "device_Q_XX_of_bound": wx, "device_q_L_of_bound": wp,
                      "sigma_ratio_Q_XX_over_Q_meas_median": round(float(np.median(np.sqrt(got.cof[:, [0, 3, 5]] / got.cof_meas[:, [0, 3, 5]]))), 3),
                      "q_L_without_correlations_over_q_L_median": round(float(np.nanmedian(got.lengths[:, 6] / got.lengths[:, 5])), 3)})
            res["workloads"][f"{name}_{m}_rays"] = r
        eng.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
