#!/usr/bin/env python3
"""Batched DLT (include/jaicov_dlt.h) at two sizes: config 4's geometry (500 images x 500 observations, scene.make_scene with
config 4's arguments and diagonal noise) and a wider synthetic block (5 000 images x 1 000 observations, stations on a sphere round
a 2 000 mm box, radial distortion and 0.5 um noise).  Restriction sets: none, and all six (five after DT:269-278).

Reports per size and set: the call's wall time (host clock around engine.dlt_adjust, which synchronises; copies and allocation
included; median of --repeats after one warm-up), the kernel time by HIP events (ms_out), the statuses and solves, and the time of
the single-threaded CPU restatement (tests/dlt_reference.py, one image at a time, numpy + the oracle's dspsv) on the same input,
with the largest difference to it.  One JSON object on stdout (and in --out).  The kernel time of rocprofv3 comes from a separate
run: rocprofv3 --kernel-trace --stats -- python scripts/dlt_bench.py --repeats 1 --no-cpu."""
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


def wide_block(n_images, n_obs, seed=20261016):
    rng = np.random.default_rng(seed)
    P = 20000
    pts = np.stack([rng.uniform(-1000, 1000, P), rng.uniform(-150, 150, P), rng.uniform(-1000, 1000, P)], 1)
    xy, xyz = [], []
    for i in range(n_images):
        while True:
            az, el = rng.uniform(0, 2 * np.pi), rng.uniform(np.deg2rad(30), np.deg2rad(85))
            st = 3500 * np.array([np.cos(el) * np.cos(az), -np.sin(el), np.cos(el) * np.sin(az)])
            r3 = st / np.linalg.norm(st)
            up = np.array([0.0, 0.0, 1.0]) if abs(r3[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
            r1 = np.cross(up, r3); r1 /= np.linalg.norm(r1)
            r2 = np.cross(r3, r1)
            om, ph, ka = scene.angles_from_rotation(np.stack([r1, r2, r3], 1))
            eo = np.array([st[0], st[1], st[2], om, ph, ka])
            x, y, N = scene.project(scene.C_EX, scene.X0_EX, scene.Y0_EX, eo, pts, scene.R0_EX, scene.DIST_RADIAL)
            vis = np.flatnonzero((N < 0) & (np.abs(x) < scene.SENSOR_W / 2) & (np.abs(y) < scene.SENSOR_H / 2))
            if vis.size >= n_obs:
                break
        sel = np.sort(rng.choice(vis, n_obs, replace=False))
        xy.append(np.stack([x[sel], y[sel]], 1) + rng.normal(0, scene.SIGMA_IMG, (n_obs, 2)))
        xyz.append(pts[sel])
    ob = (np.arange(n_images + 1) * n_obs).astype(np.int32)
    io = np.tile([scene.X0_EX, scene.Y0_EX, scene.C_EX], (n_images, 1))
    return ob, np.concatenate(xy), np.concatenate(xyz), io


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement (profiler runs)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import dlt_reference as R
    sizes = {}
    fp = scene.make_scene(500, 5000, 500, dist=scene.DIST_FULL, weights="diag", n_control=15)
    ob, xy, xyz, io, _ = R.batch_from_scene(fp)
    sizes["cfg4_500x500"] = (ob, xy, xyz, io)
    sizes["wide_5000x1000"] = wide_block(5000, 1000)
    res = {"what": "jaicov_dlt_adjust", "sizes": {}}
    for name, (ob, xy, xyz, io) in sizes.items():
        for rs in ((), (0, 1, 2, 3, 4, 5)):
            engine.dlt_adjust(ob, xy, xyz, io, restrictions=rs)                     # warm-up (code object load)
            walls, kms = [], []
            for _ in range(a.repeats):
                t = time.perf_counter()
                out, st, sv, ms = engine.dlt_adjust(ob, xy, xyz, io, restrictions=rs, with_time=True)
                walls.append((time.perf_counter() - t) * 1e3)
                kms.append(ms)
            r = {"images": int(ob.size - 1), "observations": int(ob[-1]), "restrictions": list(rs),
                 "wall_ms_median": float(np.median(walls)), "wall_ms_all": walls, "kernel_ms_median_hip_events": float(np.median(kms)),
                 "status_counts": np.bincount(st, minlength=5).tolist(), "solves_min_max_mean": [int(sv.min()), int(sv.max()), float(sv.mean())]}
            if not a.no_cpu:
                t = time.perf_counter()
                ro, rst, rsv = R.adjust(ob, xy, xyz, io, restrictions=rs)
                r["cpu_restatement_s"] = time.perf_counter() - t
                r["status_equal"] = bool(np.array_equal(st, rst)) and bool(np.array_equal(sv, rsv))
                ok = ~np.isnan(ro)
                col = np.nanmax(np.abs(np.where(ok, ro, np.nan)), axis=0)
                d = np.abs(np.where(ok, out - ro, 0.0))
                d[:, 17:20] = np.abs(R.wrap(np.where(ok[:, 17:20], out[:, 17:20] - ro[:, 17:20], 0.0)))
                r["max_rel_diff_to_restatement"] = float(np.nanmax(d / np.where(col > 0, col, 1.0)))
            res["sizes"][f"{name}{'_all6' if rs else ''}"] = r
            print(name, rs, json.dumps({k: v for k, v in r.items() if k != "wall_ms_all"}), file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
