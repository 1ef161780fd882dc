#!/usr/bin/env python3
"""Device-side reliability analysis at config 4 (include/jaicov_reliability.h): one FULL_EXPANDED pass, then jaicov_rel_run with the
pass's step.

Reports the time of jaicov_rel_run (host wall clock around the call, which synchronises; work-buffer allocations included), the
time of copying the four vectors back, the sum of the redundancy numbers against f, the range of r, the summary, the flops of the
two batched GEMMs (G = H P and the shared-column product) and the time of the FULL_EXPANDED pass it follows.  One JSON object on
stdout (and in --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bundle_adjustment_amd  # noqa: E402,F401
from bundle_adjustment_amd import engine, scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    fp = scene.config(a.config)
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(engine.INVERT_FULL_EXPANDED)
    t0 = time.perf_counter()
    eng.build(fp.sigma2apriori, 0.0)
    dx = eng.solve(engine.INVERT_FULL_EXPANDED)
    pass_ms = 1e3 * (time.perf_counter() - t0)
    assert eng.cofactor_order() == fp.n_unknowns
    L = eng.L
    n = engine.C.c_int32(0)
    pd = engine.C.POINTER(engine.C.c_double)
    run_ms = []
    for _ in range(a.repeats + 1):                       # the first run includes the first touch of the allocations
        t0 = time.perf_counter()
        assert L.jaicov_rel_run(eng._h, float(fp.sigma2apriori), dx.ctypes.data_as(pd), engine.C.byref(n)) == 0
        run_ms.append(1e3 * (time.perf_counter() - t0))
    rows = n.value
    out = [np.zeros(rows) for _ in range(4)]
    t0 = time.perf_counter()
    assert L.jaicov_rel_get(eng._h, *[o.ctypes.data_as(pd) for o in out], rows) == 0
    get_ms = 1e3 * (time.perf_counter() - t0)
    v, qvv, r, t = out
    summ = eng.reliability_summary()
    # the dense image blocks and the GEMM sizes the run chose (csrc/reliability.hip)
    m = 2 * np.diff(fp.blk_ip_begin.astype(np.int64))
    nd = int(np.sum(m > 0))
    mpad = int(-(-int(m.max(initial=0)) // 128) * 128)
    gemm_hp_flop = 2.0 * nd * mpad ** 3
    gemm_shared_flop = 2.0 * nd * mpad ** 2 * 64
    per_image = (3 * mpad * mpad + 2 * mpad * 64) * 8
    batch = max(1, min(nd, (1 << 30) // per_image)) if nd else 0
    f = fp.degree_of_freedom
    res = {
        "config": a.config, "rows": rows, "U": fp.n_unknowns, "f": f, "dense_blocks": nd, "mpad": mpad, "batch": batch,
        "run_ms": [round(x, 3) for x in run_ms], "run_ms_best": round(min(run_ms[1:]), 3), "get_ms": round(get_ms, 3),
        "full_expanded_pass_ms": round(pass_ms, 3),
        "sum_r": float(r.sum()), "sum_r_rel_err": float(abs(r.sum() - f) / f), "r_min": float(r.min()), "r_max": float(r.max()),
        "t_finite": bool(np.all(np.isfinite(t))), "max_abs_t": float(np.nanmax(np.abs(t))), "summary": [float(x) for x in summ],
        "gemm_hp_flop": gemm_hp_flop, "gemm_shared_flop": gemm_shared_flop,
        "work_buffer_bytes_per_batch": per_image * batch, "output_bytes": 8 * 4 * rows,
    }
    eng.close()
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
