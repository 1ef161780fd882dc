#!/usr/bin/env python3
"""The leave-one-out table of every image point at config 4 (include/jaicov_reliability_points.h): one FULL_EXPANDED pass, then
jaicov_rel_run and jaicov_rel_run_points with the pass's step, each timed as the best of --repeats (host wall clock around the
call, which synchronises; work-buffer allocations included; one untimed run of each first).

With --trace DIR the script starts itself once more under `rocprofv3 --kernel-trace --stats` (a fresh process, --repeats 1) and
turns the kernel trace into the per-kernel table of the last jaicov_rel_run_points (--stats-out, CSV).  One JSON object on stdout
(and in --out)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bundle_adjustment_amd  # noqa: E402,F401
from bundle_adjustment_amd import engine, scene  # noqa: E402

LAMBDA0 = 17.075


def kernel_table(trace_dir, out_csv):
    """Per-kernel totals of the dispatches from the last rel_v_kernel on (the last run is a jaicov_rel_run_points)."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + trace_dir
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(fh)]
    rows.sort(key=lambda r: r[1])
    first = max(i for i, r in enumerate(rows) if "rel_v_kernel" in r[0])
    last = max(i for i, r in enumerate(rows) if "rel_summary_kernel" in r[0])
    run = rows[first:last + 1]
    span = (run[-1][2] - run[0][1]) * 1e-6
    tot = {}
    for name, t0, t1 in run:
        name = name.split("(")[0]
        c = tot.setdefault(name, [0, 0.0])
        c[0] += 1; c[1] += (t1 - t0) * 1e-6
    table = [(k, c[0], round(c[1], 4), round(c[1] / c[0], 4), round(c[1] / span, 3)) for k, c in tot.items()]
    with open(out_csv, "w", newline="") as fh:
        wr = csv.writer(fh)
        wr.writerow(["kernel", "calls", "total_ms", "average_ms", "share_of_span"])
        wr.writerows(table)
        wr.writerow(["span of one jaicov_rel_run_points (first to last kernel)", 1, round(span, 4), round(span, 4), 1.0])
    return {"span_ms": round(span, 4), "kernels": {k: t for k, _, t, _, _ in table}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace", default="", help="directory for a rocprofv3 kernel trace of a second process")
    ap.add_argument("--stats-out", default="")
    a = ap.parse_args()
    fp = scene.config(a.config)
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(engine.INVERT_FULL_EXPANDED)
    eng.build(fp.sigma2apriori, 0.0)
    dx = eng.solve(engine.INVERT_FULL_EXPANDED)
    assert eng.cofactor_order() == fp.n_unknowns
    s0 = float(fp.sigma2apriori)
    omega = eng.omega(s0, dx)
    f = fp.degree_of_freedom
    L = eng.L
    n = engine.C.c_int32(0); k = engine.C.c_int32(0)
    pd = engine.C.POINTER(engine.C.c_double)
    pdx = dx.ctypes.data_as(pd)
    plain_ms, points_ms = [], []
    for i in range(a.repeats + 1):                       # the first run of each includes the first touch of the allocations
        t0 = time.perf_counter()
        assert L.jaicov_rel_run(eng._h, s0, pdx, engine.C.byref(n)) == 0
        plain_ms.append(1e3 * (time.perf_counter() - t0))
    plain = [np.zeros(n.value) for _ in range(4)]
    assert L.jaicov_rel_get(eng._h, *[o.ctypes.data_as(pd) for o in plain], n.value) == 0
    for i in range(a.repeats + 1):
        t0 = time.perf_counter()
        assert L.jaicov_rel_run_points(eng._h, s0, pdx, LAMBDA0, omega, f, engine.C.byref(n), engine.C.byref(k)) == 0
        points_ms.append(1e3 * (time.perf_counter() - t0))
    four = [np.zeros(n.value) for _ in range(4)]
    assert L.jaicov_rel_get(eng._h, *[o.ctypes.data_as(pd) for o in four], n.value) == 0
    tab = np.zeros((14, k.value))
    t0 = time.perf_counter()
    assert L.jaicov_rel_get_points(eng._h, tab.ctypes.data_as(pd), k.value) == 0
    get_ms = 1e3 * (time.perf_counter() - t0)
    eng.close()
    m = 2 * np.diff(fp.blk_ip_begin.astype(np.int64))
    nd = int(np.sum(m > 0))
    mpad = int(-(-int(m.max(initial=0)) // 128) * 128)
    per_image = (3 * mpad * mpad + 2 * mpad * 64 + mpad + (mpad // 2) * (mpad // 32) * 3) * 8
    t2 = np.fmax(four[3][0:2 * k.value:2] ** 2, four[3][1:2 * k.value:2] ** 2)
    res = {
        "config": a.config, "rows": n.value, "image_points": k.value, "U": fp.n_unknowns, "f": f, "omega": omega, "dense_blocks": nd,
        "mpad": mpad, "batch": max(1, min(nd, (1 << 30) // per_image)) if nd else 0,
        "rel_run_ms": [round(x, 3) for x in plain_ms], "rel_run_ms_best": round(min(plain_ms[1:]), 3),
        "rel_run_ms_spread": round(max(plain_ms[1:]) - min(plain_ms[1:]), 3),
        "rel_run_points_ms": [round(x, 3) for x in points_ms], "rel_run_points_ms_best": round(min(points_ms[1:]), 3),
        "ratio": round(min(points_ms[1:]) / min(plain_ms[1:]), 3), "get_points_ms": round(get_ms, 3),
        "four_vectors_bit_identical": bool(all(np.array_equal(x, y, equal_nan=True) for x, y in zip(plain, four))),
        "points_not_controlled": int(np.isnan(tab[0]).sum()), "max_T_prio": float(np.nanmax(tab[1])),
        "T_prio_at_least_half_t2": bool(np.all(tab[1] >= 0.5 * t2 * (1 - 1e-9))),
        "max_abs_shift": float(np.nanmax(np.abs(tab[11:14]))), "table_bytes": 8 * 14 * k.value,
    }
    if a.trace:
        os.makedirs(a.trace, exist_ok=True)
        subprocess.check_call(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.trace, "--", sys.executable,
                               os.path.abspath(__file__), "--config", a.config, "--repeats", "1"], stdout=subprocess.DEVNULL)
        res["kernel_trace"] = kernel_table(a.trace, a.stats_out or os.path.join(a.trace, "point_reliability_kernel_stats.csv"))
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
