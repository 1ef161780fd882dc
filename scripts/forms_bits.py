#!/usr/bin/env python3
"""Does jaicov_form_fit (include/jaicov_forms.h) return the same bits in two builds?  The cases are those of tests/test_gpu_forms.py
(DESIGN 6m): three scenes x three inversion modes, every form of cases_of.

    forms_bits.py --tree <checkout with a built library> --dump a.npz --values v.npz     one dump per build (default tree: this checkout)
    forms_bits.py --compare a.npz b.npz                                    one JSON object on stdout (and in --out)

A dump holds, per case, every table that fit_forms returns and a SHA-256 of what the kernel read: the coordinates and the cofactor
matrix that the engine exports.  Two inverting passes need not leave the same bits in the matrix (their sums are not all in a fixed
order), so the comparison says for every case whether the inputs were the same bits; where they were, the results must be, and where
they were not, the largest relative difference of the results is reported beside that of the matrices and proves nothing either way.
The planted coordinates depend on a sigma taken from a pass, so the first dump writes them to --values and the second reads them there.
--repeat N dumps every case N times (a fresh engine each), so that two dumps have a better chance of a pair with the same inputs:
the comparison pairs every repeat of one dump with every repeat of the other."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

FIELDS = ("params", "sigma", "qpp", "omega", "dof", "T", "max_distance", "rms_distance", "iterations", "status", "v", "distance", "nabla",
          "T_member", "member_status")


def dump(tree, path, repeat, values_path):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import bundle_adjustment_amd  # noqa: F401
    import test_gpu_forms as T
    import dataclasses
    out = {}
    values = dict(np.load(values_path)) if values_path and os.path.exists(values_path) else {}
    for name in T.SCENES:
        fp, groups = T.planted(name)
        if name in values:
            fp = dataclasses.replace(fp, values=values[name])
        values[name] = np.asarray(fp.values, float)
        forms = T.cases_of(name, groups)
        for mode in T.MODES:
            for r in range(repeat):
                eng = T.inverting_pass(fp, T.MODES[mode])
                Q = T.exported(eng)
                X = eng.get_parameters()[:3 * fp.n_points]
                fits = eng.fit_forms(T.S2, forms)
                eng.close()
                key = f"{name}|{mode}|{r}"
                out[key + "|input"] = np.frombuffer(hashlib.sha256(Q.tobytes() + X.tobytes()).digest(), np.uint8)
                out[key + "|Qnorm"] = np.array([np.abs(Q).max()])
                out[key + "|Q"] = Q if Q.shape[0] <= 200 else np.diag(Q).copy()
                for f in FIELDS:
                    out[key + "|" + f] = np.ascontiguousarray(getattr(fits, f))
    np.savez_compressed(path, **out)
    if values_path:
        np.savez_compressed(values_path, **values)
    print(json.dumps({"dumped": path, "cases": len(out) // (len(FIELDS) + 3)}))


def reldiff(a, b):
    ok = ~(np.isnan(a) & np.isnan(b))
    if not ok.any():
        return 0.0
    return float(np.abs(a[ok].astype(float) - b[ok].astype(float)).max() / max(np.abs(b[ok].astype(float)).max(), 1e-300))


def compare(pa, pb, out_path):
    A, B = np.load(pa), np.load(pb)
    cases = sorted({k.rsplit("|", 2)[0] for k in A.files})
    reps_a = sorted({k.split("|")[2] for k in A.files}); reps_b = sorted({k.split("|")[2] for k in B.files})
    res = {"cases": len(cases), "same_input_pairs": 0, "same_input_same_bits": 0, "cases_with_a_same_input_pair": 0, "per_case": {}}
    for c in cases:
        same_in = same_out = 0
        worst_q = worst_f = 0.0
        for ra in reps_a:
            for rb in reps_b:
                ka, kb = f"{c}|{ra}|", f"{c}|{rb}|"
                if A[ka + "input"].tobytes() == B[kb + "input"].tobytes():
                    same_in += 1
                    same_out += all(A[ka + f].tobytes() == B[kb + f].tobytes() for f in FIELDS)
                else:
                    worst_q = max(worst_q, reldiff(A[ka + "Q"].ravel(), B[kb + "Q"].ravel()))
                    worst_f = max(worst_f, max(reldiff(A[ka + f].ravel(), B[kb + f].ravel()) for f in ("params", "sigma", "qpp", "omega", "v")))
        res["same_input_pairs"] += same_in; res["same_input_same_bits"] += same_out
        res["cases_with_a_same_input_pair"] += same_in > 0
        res["per_case"][c] = {"same_input_pairs": same_in, "of_them_same_bits": same_out, "other_pairs_matrix_difference": worst_q,
                              "other_pairs_result_difference": worst_f}
    res["verdict"] = ("no pair of runs had the same inputs: nothing is shown" if res["same_input_pairs"] == 0 else
                      "the same bits wherever the inputs were the same bits" if res["same_input_pairs"] == res["same_input_same_bits"] else
                      "DIFFERENT BITS from the same inputs")
    print(json.dumps({k: v for k, v in res.items() if k != "per_case"}))
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0 if res["same_input_pairs"] == res["same_input_same_bits"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--dump", default="")
    ap.add_argument("--values", default="", help="the planted coordinates: written by the first dump, read by the next")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--compare", nargs=2, default=None)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.out))
    dump(os.path.abspath(a.tree), a.dump, a.repeat, a.values)


if __name__ == "__main__":
    main()
