#!/usr/bin/env python3
"""The precision calls of include/jaicov_precision.h at config 4 after one FULL_EXPANDED pass: all 5 000 object points, all 500
stations, 100 000 point pairs, and the k = 3 largest principal components of the block of the point coordinates.

Each call is timed by HIP events recorded on the null stream around it (the calls synchronise, so the events bracket the upload of
the index table, the kernels, the download and, for the components, the host's 8 x 8 algebra) and by the host's wall clock: medians
of `--repeats` runs after one warm-up, which also allocates the work buffers.  For the components the time of one more product is
taken from two runs with a fixed number of products (tol so small that neither converges); it holds the 8-wide product Y = S X over
the lower triangle of the sub-block, the n x 8 kernels and the four host hops of an iteration.  The kernel's own time comes from
`rocprofv3 --kernel-trace --stats -- python scripts/precision_bench.py --repeats 1`.  One JSON object on stdout (and in --out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bundle_adjustment_amd  # noqa: E402,F401
from bundle_adjustment_amd import engine, scene  # noqa: E402


class Events:
    """hipEvent pairs on the null stream, from the runtime the engine library is linked against."""

    def __init__(self):
        engine.load_library()
        with open("/proc/self/maps") as fh:              # the copy that is already loaded, whatever its version suffix
            path = next(line.split()[-1] for line in fh if "libamdhip64" in line)
        self.hip = C.CDLL(path)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for ev in (self.a, self.b):
            assert self.hip.hipEventCreate(C.byref(ev)) == 0

    def time(self, fn):
        assert self.hip.hipEventRecord(self.a, None) == 0
        t0 = time.perf_counter()
        out = fn()
        wall = 1e3 * (time.perf_counter() - t0)
        assert self.hip.hipEventRecord(self.b, None) == 0 and self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float(0)
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return out, float(ms.value), wall


def timed(ev, fn, repeats):
    fn()
    runs = [ev.time(fn) for _ in range(repeats)]
    return runs[-1][0], round(statistics.median(r[1] for r in runs), 4), round(statistics.median(r[2] for r in runs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a small scene (8 x 60) instead of config 4: a quick check")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    fp = scene.make_scene(8, 60, 40, dist=scene.DIST_FULL, weights="block", n_control=4) if a.small else scene.config("cfg4")
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(engine.INVERT_FULL_EXPANDED)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(engine.INVERT_FULL_EXPANDED)
    U, P, I = eng.cofactor_order(), fp.n_points, fp.n_images
    s2 = fp.sigma2apriori
    rng = np.random.default_rng(1)
    n_pairs = 1000 if a.small else 100000
    pa = rng.integers(0, P, n_pairs)
    pairs = np.stack([pa, (pa + 1 + rng.integers(0, P - 1, n_pairs)) % P], 1).astype(np.int32)
    ev = Events()
    pts, pts_ms, pts_wall = timed(ev, lambda: eng.precision_points(s2), a.repeats)
    sta, sta_ms, sta_wall = timed(ev, lambda: eng.precision_stations(s2), a.repeats)
    ln, ln_ms, ln_wall = timed(ev, lambda: eng.precision_lengths(s2, pairs), a.repeats)
    first, n = eng.point_column_range()
    pc, pc_ms, pc_wall = timed(ev, lambda: eng.principal_components(3), a.repeats)
    _, few_ms, _ = timed(ev, lambda: eng.principal_components(3, tol=1e-300, max_iterations=2), a.repeats)
    _, many_ms, _ = timed(ev, lambda: eng.principal_components(3, tol=1e-300, max_iterations=12), a.repeats)
    per_product = (many_ms - few_ms) / 10.0
    eng.close()
    tri = n * (n + 1) // 2 * 8
    res = {
        "scene": "small" if a.small else "cfg4", "U": U, "points": P, "stations": I, "pairs": n_pairs, "repeats": a.repeats,
        "points_event_ms": pts_ms, "points_wall_ms": pts_wall, "stations_event_ms": sta_ms, "stations_wall_ms": sta_wall,
        "lengths_event_ms": ln_ms, "lengths_wall_ms": ln_wall,
        "status_points_nonzero": int((pts.status != 0).sum()), "status_stations_nonzero": int((sta.status != 0).sum()),
        "status_pairs_nonzero": int((ln.status != 0).sum()),
        "largest_helmert": float(pts.helmert.max()), "median_sigma_length": float(np.median(ln.sigma)),
        "components_k": 3, "components_first_col": first, "components_n_cols": n, "components_converged": bool(pc.converged),
        "components_products": pc.iterations, "components_event_ms": pc_ms, "components_wall_ms": pc_wall,
        "components_share_of_trace": [float(x) for x in pc.values / pc.trace], "components_residuals_over_theta1": [float(x) for x in pc.residuals / pc.values[0]],
        "event_ms_2_products": few_ms, "event_ms_12_products": many_ms, "ms_per_iteration": round(per_product, 4),
        "sub_block_lower_triangle_bytes": tri,
        "iteration_bytes_per_second": round(tri / (per_product * 1e-3), 1),
        "iteration_fraction_of_8TBps": round(tri / (per_product * 1e-3) / 8e12, 4),
    }
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
