#!/usr/bin/env python3
"""Device-side coordinate transformation at config 4 (include/jaicov_transform.h): one FULL_EXPANDED pass, then
CoordinateTransformationExteriorOrientation.transform of all 5 000 points from 20 source images into image 0 plus (0, 0).

Reports the time of jaicov_xform_run (host wall clock around the call, which synchronises; allocations and the host-side row
enumeration included), the compulsory bytes (packed output + one read of Q[S, S]) and their fraction of 8 TB/s, the time of
reading all 3 x 3 diagonal blocks (one jaicov_xform_get_covariance_sub call per point, and jaicov_xform_get_point_blocks once), the
time of jaicov_neq_get_cofactor alone on the same engine, |S| and the size of every work buffer.  One JSON object
on stdout (and in --out)."""
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
    ap.add_argument("--sources", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    fp = scene.config(a.config)
    P = fp.point_col.shape[0]
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(engine.INVERT_FULL_EXPANDED)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(engine.INVERT_FULL_EXPANDED)
    assert eng.cofactor_order() == fp.n_unknowns
    pairs = [(0, s) for s in range(1, a.sources + 1)] + [(0, 0)]
    points = list(range(P))
    run_ms = []
    for _ in range(a.repeats + 1):                       # the first run includes the allocations' first touch
        t0 = time.perf_counter()
        xyz, ids = eng.transform(points, pairs, fp.sigma2apriori)
        run_ms.append(1e3 * (time.perf_counter() - t0))
    n = len(ids)
    R = 3 * n
    diag = (3 * np.arange(n)[:, None] + np.arange(3)).astype(np.int32)
    sub_ms = []
    L = eng.L
    out = np.zeros(9)
    pi, pd = engine.C.POINTER(engine.C.c_int32), engine.C.POINTER(engine.C.c_double)
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for t in range(n):
            rc = L.jaicov_xform_get_covariance_sub(eng._h, diag[t].ctypes.data_as(pi), 3, out.ctypes.data_as(pd))
            assert rc == 0
        sub_ms.append(1e3 * (time.perf_counter() - t0))
    blk_ms = []                                          # the same blocks in one call (jaicov_xform_get_point_blocks)
    blocks = np.zeros(9 * n)
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        assert L.jaicov_xform_get_point_blocks(eng._h, blocks.ctypes.data_as(pd), n) == 0
        blk_ms.append(1e3 * (time.perf_counter() - t0))
    cof_ms = []
    U = fp.n_unknowns
    Qp = np.zeros(U * (U + 1) // 2)
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        rc = L.jaicov_neq_get_cofactor(eng._h, Qp.ctypes.data_as(pd), Qp.size)
        assert rc == 0
        cof_ms.append(1e3 * (time.perf_counter() - t0))
    # involved columns S (the point columns of the transformed points + the exterior orientations of the images involved)
    cols = set()
    for p, s, r in ids:
        cols.update(int(c) for c in fp.point_col[p] if c >= 0)
        if s != r:
            cols.update(int(c) for c in fp.eo_col[s] if c >= 0)
            cols.update(int(c) for c in fp.eo_col[r] if c >= 0)
    S = len(cols)
    out_bytes = 8 * R * (R + 1) // 2
    q_bytes = 8 * S * (S + 1) // 2
    run_best = min(run_ms[1:])
    chunks = sum(-(-int(np.sum((ids[:, 1] == s) & (ids[:, 2] == 0))) // 16) for s in range(0, a.sources + 1))
    res = {
        "config": a.config, "sources": a.sources, "transformed_points": n, "R": R, "S": S, "U": U,
        "run_ms": [round(x, 3) for x in run_ms], "run_ms_best": round(run_best, 3),
        "compulsory_bytes": out_bytes + q_bytes, "packed_output_bytes": out_bytes, "q_ss_read_bytes": q_bytes,
        "achieved_TBps": round((out_bytes + q_bytes) / (run_best * 1e-3) / 1e12, 3),
        "fraction_of_8TBps": round((out_bytes + q_bytes) / (run_best * 1e-3) / 8e12, 3),
        "diag_blocks_sub_ms": [round(x, 3) for x in sub_ms], "diag_blocks_sub_calls": n,
        "diag_blocks_one_call_ms": [round(x, 3) for x in blk_ms],
        "get_cofactor_ms": [round(x, 3) for x in cof_ms],
        "run_plus_diag_one_call_ms": round(run_best + min(blk_ms), 3), "run_plus_diag_sub_calls_ms": round(run_best + min(sub_ms), 3),
        "get_cofactor_ms_best": round(min(cof_ms), 3),
        "acceptance_run_plus_diag_below_get_cofactor": bool(run_best + min(blk_ms) < min(cof_ms)),
        "work_buffers_bytes": {"packed_output": out_bytes, "jacobian_values": 8 * 45 * n, "jacobian_columns": 4 * 15 * n,
                               "coordinates": 8 * 3 * n, "row_ids": 4 * 3 * n, "chunks": 8 * chunks},
        "chunks": chunks, "tiles": chunks * (chunks + 1) // 2,
    }
    eng.close()
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
