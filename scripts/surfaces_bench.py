#!/usr/bin/env python3
"""jaicov_surf_fit (include/jaicov_surfaces.h) at config 4 after a FULL_EXPANDED pass: cylinders of 12 and of 64 points and cones of 12
and of 64 points, one call per class, every form from start values of its own (the search over candidate axes runs in every call).
Config 4 has 5 000 object points, so there are two passes: one whose object-point start values lie on 78 cylinders of 64 points (the
cylinders of 12 are windows of these, spread over the group), one with 78 cones.  A group is a run of points neighbouring in X; it
is replaced by points on a random surface of 0.7 of its extent around its centroid (an arc of 120 degrees and more) with noise of
about three sigma (sigma from a pass of the unchanged scene unless --sigma is given), as tests/test_gpu_surfaces.py plants them.

Reported, as scripts/forms_bench.py reports it: the kernels' time by HIP events on the engine's stream (the library records them
around the search and the fit: ms_out), the synchronous call's wall time, medians of `--repeats` calls after a warm-up that also
allocates the work buffers, with their run-to-run spread ((p90 - p10) / median); the same call with the converged figures given as
the start (no search); and the numpy restatement's time per form, its get_cofactor_sub gathers included, over `--numpy-forms` forms
of every class.  One JSON object on stdout (and in --out)."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bundle_adjustment_amd  # noqa: E402,F401
from bundle_adjustment_amd import engine, scene  # noqa: E402
import surface_reference as R  # noqa: E402
from forms_bench import inverting_pass, spread  # noqa: E402


def planted(fp, kind, groups, sig, rng):
    vals = np.array(fp.values, float)
    X = vals[:3 * fp.n_points].reshape(-1, 3)
    for idx in groups:
        c0 = X[idx].mean(0)
        pts, _ = R.surface_points(kind, len(idx), rng, size=0.7 * np.linalg.norm(X[idx] - c0, axis=1).max(), centre=c0)
        X[idx] = pts + 3.0 * sig * rng.normal(size=pts.shape)
    return dataclasses.replace(fp, values=vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--numpy-forms", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.0, help="the noise's sigma; 0: from a first pass of the unchanged scene")
    ap.add_argument("--small", action="store_true", help="config 2 with 3 groups of 64: a quick check")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    fp = scene.config("cfg2" if a.small else "cfg4")
    n_big, k_big, k_small = (3 if a.small else 78), 64, 12
    P = fp.n_points
    pcol = np.asarray(fp.point_col).reshape(-1, 3)
    sig = a.sigma
    if sig == 0.0:
        eng = inverting_pass(fp)
        rows = pcol[pcol[:, 0] >= 0][:256, 0].astype(np.int32)
        sig = float(np.sqrt(fp.sigma2apriori * np.median(np.diag(eng.get_cofactor_sub(rows)))))
        eng.close()
    rng = np.random.default_rng(7)
    order = np.argsort(np.asarray(fp.values, float)[:3 * P].reshape(P, 3)[:, 0], kind="stable").astype(np.int32)
    assert n_big * k_big <= P
    big = [order[g * k_big:(g + 1) * k_big] for g in range(n_big)]           # member order = the order along the planted arc
    small = [grp[w::k_big // k_small][:k_small] for grp in big for w in range(k_big // k_small)]
    s2 = fp.sigma2apriori
    per_class, numpy_ms, bad, most = {}, {}, {}, 0

    def run(eng, fs, start=None):
        eng.fit_surfaces(s2, fs, start=start)                                # warm-up: allocates the work buffers
        ms, wall = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            f = eng.fit_surfaces(s2, fs, start=start)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms.append(f.kernel_ms)
        return f, ms, wall

    def measure(eng, name, kind, groups):
        nonlocal most
        fs = [(kind, g.astype(np.int32)) for g in groups]
        fits, ms, wall = run(eng, fs)
        bad[name] = int((fits.status != 0).sum()); most = max(most, int(np.nanmax(fits.iterations)))
        good = fits.status == 0
        rows = [fits.params[g] if good[g] else None for g in range(len(fs))]
        _, ms_given, _ = run(eng, fs, start=rows)
        per_class[name] = {"forms": len(fs), "members": len(groups[0]), "kernel_ms": round(float(np.median(ms)), 4),
                           "kernel_min_ms": round(float(np.min(ms)), 4), "kernel_spread": round(spread(ms), 4),
                           "call_wall_ms": round(float(np.median(wall)), 4), "call_wall_spread": round(spread(wall), 4),
                           "kernel_us_per_form": round(1e3 * float(np.median(ms)) / len(fs), 3),
                           "kernel_ms_start_given": round(float(np.median(ms_given)), 4), "iterations_median": float(np.nanmedian(fits.iterations))}
        X = eng.get_parameters()[:3 * P].reshape(P, 3)                      # the numpy restatement, its gathers included
        ts = []
        for g in range(min(a.numpy_forms, len(fs))):
            idx = fs[g][1]
            t0 = time.perf_counter()
            Qll = eng.get_cofactor_sub(pcol[idx].ravel().astype(np.int32))
            ref = R.fit_surface(kind, X[idx], Qll, s2)
            ts.append(1e3 * (time.perf_counter() - t0))
            assert ref["status"] == fits.status[g], (name, g, ref["status"], fits.status[g])
        numpy_ms[name] = round(float(np.median(ts)), 3)

    for kind, label in ((R.CYLINDER, "cylinder"), (R.CONE, "cone")):
        eng = inverting_pass(planted(fp, kind, big, sig, rng))
        measure(eng, label + "12", kind, small)
        measure(eng, label + "64", kind, big)
        eng.close()
    res = {"scene": "cfg2" if a.small else "cfg4", "noise_sigma": sig, "repeats": a.repeats, "status_nonzero": bad, "iterations_max": most,
           "per_class": per_class, "numpy_ms_per_form": numpy_ms}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
