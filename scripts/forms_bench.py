#!/usr/bin/env python3
"""jaicov_form_fit (include/jaicov_forms.h) at config 4 after a FULL_EXPANDED pass: 500 planes of 10 points, 156 spheres of 32
points and 78 planes of 64 points, one call per class.  Config 4 has 5 000 object points and every class takes nearly all of them,
so there are two passes: one whose object-point start values lie on 78 planes of 64 points (the planes of 10 are windows of these),
one whose start values lie on 156 spheres of 32 points.  A group is a run of points neighbouring in X; its points are moved the
shortest way onto the plane or sphere that fits them best and get noise of about three sigma (sigma from a pass of the unchanged
scene unless --sigma is given).

Reported: the kernel's time by HIP events on the engine's stream (the library records them around the launch: ms_out), the
synchronous call's wall time (upload, kernel, download), medians of `--repeats` calls after a warm-up that also allocates the work
buffers, with their run-to-run spread ((p90 - p10) / median); the numpy restatement's time per form, its get_cofactor_sub gathers
included, over `--numpy-forms` forms of every class; and, measured once beside it, the same call with M factorised by
wave_solve_lds in the place of wave_chol_lds (jaicov_debug_form_fit_serial) on the 78 planes of m = 64 and on the planes of 10.
One JSON object on stdout (and in --out)."""
import argparse
import ctypes as C
import dataclasses
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
import form_reference as R  # noqa: E402

CLASSES = {"plane10": (R.PLANE, 500, 10), "sphere32": (R.SPHERE, 156, 32), "plane64": (R.PLANE, 78, 64)}


def spread(x):
    x = np.sort(np.asarray(x))
    return float((np.percentile(x, 90) - np.percentile(x, 10)) / np.median(x))


def inverting_pass(fp):
    eng = engine.Engine(fp, device=0)
    eng.set_parameters(fp.values)
    eng.prepare_inverse(engine.INVERT_FULL_EXPANDED)
    eng.build(fp.sigma2apriori, 0.0)
    eng.solve(engine.INVERT_FULL_EXPANDED)
    return eng


def planted(fp, kind, groups, sig, rng):
    """fp with the points of every group moved onto the plane or sphere that fits them best (the shortest way, so that the block's
    geometry stays what it was), with noise of 3 sig"""
    vals = np.array(fp.values, float)
    X = vals[:3 * fp.n_points].reshape(-1, 3)
    for idx in groups:
        x = X[idx]
        c0 = x.mean(0)
        if kind == R.PLANE:
            n = np.linalg.svd(x - c0)[2][2]
            x = x - np.outer((x - c0) @ n, n)
        else:
            th = np.linalg.lstsq(np.c_[-2.0 * (x - c0), np.ones(len(x))], -((x - c0) ** 2).sum(1), rcond=None)[0]
            c, r = c0 + th[:3], np.sqrt(th[:3] @ th[:3] - th[3])
            d = x - c
            x = c + r * d / np.linalg.norm(d, axis=1)[:, None]
        X[idx] = x + 3.0 * sig * rng.normal(size=x.shape)
    return dataclasses.replace(fp, values=vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--numpy-forms", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.0, help="the noise's sigma; 0: from a first pass of the unchanged scene")
    ap.add_argument("--small", action="store_true", help="config 2 with forms of 5, 8 and 16 points: a quick check")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    fp = scene.config("cfg2" if a.small else "cfg4")
    classes = {"plane10": (R.PLANE, 30, 5), "sphere32": (R.SPHERE, 25, 8), "plane64": (R.PLANE, 12, 16)} if a.small else dict(CLASSES)
    P = fp.n_points
    pcol = np.asarray(fp.point_col).reshape(-1, 3)
    sig = a.sigma
    if sig == 0.0:
        eng = inverting_pass(fp)
        rows = pcol[pcol[:, 0] >= 0][:256, 0].astype(np.int32)
        sig = float(np.sqrt(fp.sigma2apriori * np.median(np.diag(eng.get_cofactor_sub(rows)))))
        eng.close()
    rng = np.random.default_rng(7)
    order = np.argsort(np.asarray(fp.values, float)[:3 * P].reshape(P, 3)[:, 0], kind="stable").astype(np.int32)   # neighbours in X: short ways
    _, n_big, k_big = classes["plane64"]
    _, n_small, k_small = classes["plane10"]
    _, n_sph, k_sph = classes["sphere32"]
    assert n_big * k_big <= P and n_sph * k_sph <= P
    big = [np.sort(order[g * k_big:(g + 1) * k_big]) for g in range(n_big)]
    small = [grp[w * k_small:(w + 1) * k_small] for grp in big for w in range(k_big // k_small)]
    small += [grp[-k_small:] for grp in big]                               # more windows of the same planes
    small = small[:n_small]
    assert len(small) == n_small
    sph = [np.sort(order[g * k_sph:(g + 1) * k_sph]) for g in range(n_sph)]
    s2 = fp.sigma2apriori
    L = engine.load_library()
    pi, pd = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    L.jaicov_debug_form_fit_serial.argtypes = [C.c_void_p, C.c_double, C.c_int32, pi, pi, pi, C.c_int32, C.c_double, pd, pi, C.POINTER(C.c_float)]
    per_class, numpy_ms, serial_ms, same, bad, most = {}, {}, {}, {}, 0, 0

    def run(eng, fs):
        eng.fit_forms(s2, fs)                                               # warm-up: allocates the work buffers
        ms, wall = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            f = eng.fit_forms(s2, fs)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms.append(f.kernel_ms)
        return f, ms, wall

    def serial(eng, fs):
        kinds = np.ascontiguousarray([k for k, _ in fs], np.int32)
        begin = np.concatenate([[0], np.cumsum([len(p) for _, p in fs])]).astype(np.int32)
        pts = np.ascontiguousarray(np.concatenate([p for _, p in fs]), np.int32)
        out = np.zeros((len(fs), engine.FORM_COLUMNS)); st = np.zeros(len(fs), np.int32); t = C.c_float(0.0)
        res = []
        for _ in range(a.repeats + 1):
            rc = L.jaicov_debug_form_fit_serial(eng._h, s2, len(fs), kinds.ctypes.data_as(pi), begin.ctypes.data_as(pi), pts.ctypes.data_as(pi), 20, 0.0,
                                                out.ctypes.data_as(pd), st.ctypes.data_as(pi), C.byref(t))
            assert rc == 0, rc
            res.append(t.value)
        return out, res[1:]

    def measure(eng, name, kind, groups, with_serial):
        nonlocal bad, most
        fs = [(kind, g.astype(np.int32)) for g in groups]
        fits, ms, wall = run(eng, fs)
        bad += int((fits.status != 0).sum()); most = max(most, int(np.nanmax(fits.iterations)))
        per_class[name] = {"forms": len(fs), "members": len(groups[0]), "kernel_ms": round(float(np.median(ms)), 4),
                           "kernel_min_ms": round(float(np.min(ms)), 4), "kernel_spread": round(spread(ms), 4),
                           "call_wall_ms": round(float(np.median(wall)), 4), "call_wall_spread": round(spread(wall), 4),
                           "kernel_us_per_form": round(1e3 * float(np.median(ms)) / len(fs), 3)}
        if with_serial:
            so, sms = serial(eng, fs)
            serial_ms[name] = {"kernel_ms": round(float(np.median(sms)), 4), "gain": round(float(np.median(sms) / np.median(ms)), 3)}
            ours = np.c_[fits.params, fits.sigma, fits.omega, fits.dof, fits.T, fits.max_distance, fits.rms_distance, fits.iterations]
            same[name] = float(np.nanmax(np.abs(so[:, :4] - ours[:, :4])) / np.nanmax(np.abs(ours[:, :4])))
        X = eng.get_parameters()[:3 * P].reshape(P, 3)                      # the numpy restatement, its gathers included
        ts = []
        for g in range(min(a.numpy_forms, len(fs))):
            idx = fs[g][1]
            t0 = time.perf_counter()
            Qll = eng.get_cofactor_sub(pcol[idx].ravel().astype(np.int32))
            ref = R.fit_form(kind, X[idx], Qll, s2)
            ts.append(1e3 * (time.perf_counter() - t0))
            assert ref["status"] == fits.status[g], (name, g, ref["status"], fits.status[g])
        numpy_ms[name] = round(float(np.median(ts)), 3)

    eng = inverting_pass(planted(fp, R.PLANE, big, sig, rng))
    measure(eng, "plane10", R.PLANE, small, True)
    measure(eng, "plane64", R.PLANE, big, True)
    eng.close()
    eng = inverting_pass(planted(fp, R.SPHERE, sph, sig, rng))
    measure(eng, "sphere32", R.SPHERE, sph, False)
    eng.close()
    res = {
        "scene": "cfg2" if a.small else "cfg4", "noise_sigma": sig, "repeats": a.repeats, "status_nonzero": bad, "iterations_max": most,
        "per_class": per_class, "kernel_ms_sum": round(sum(v["kernel_ms"] for v in per_class.values()), 4),
        "call_wall_ms_sum": round(sum(v["call_wall_ms"] for v in per_class.values()), 4),
        "numpy_ms_per_form": numpy_ms, "serial_factorisation": serial_ms, "serial_parameter_difference": same,
    }
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
