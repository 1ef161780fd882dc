"""The host shell of the one-shot batched calls (csrc/batchcall.h: BatchCall), where no test of the six families looks: empty items
beside items of the minimum size, every optional input and output passed and then left out, and the device's memory census around
every such call.  The calls go through ctypes directly (tests/batchcall_cases.py); the families' own tests (test_gpu_dlt.py,
test_gpu_intersect.py, test_gpu_resection.py, test_gpu_relorient.py, test_gpu_similarity.py, test_gpu_lens.py) hold the values.

Already asserted elsewhere and not repeated here: the census after calls with every optional output passed
(test_gpu_ownership.py::test_one_shot_entry_holds_nothing_after_it_returns for dlt_adjust and intersect_points,
test_device_memory_returns_to_its_census of test_gpu_resection.py, test_gpu_relorient.py, test_gpu_similarity.py and test_gpu_lens.py,
the last two with refused calls); item counts at the lane and chunk boundaries (the families' *_at_the_lane_boundaries tests)."""
import numpy as np
import pytest

import batchcall_cases as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return B.library()


@pytest.fixture(scope="module")
def minimum():
    return B.minimum_cases()


def same_census(lib, case, optional):
    """the call once as warm-up (code objects, the runtime's own first allocations), then between two readings of the census"""
    B.invoke(lib, case, optional)
    before = B.census(lib)
    rc, outs = B.invoke(lib, case, optional)
    assert B.census(lib) == before, (case[0], optional, before, B.census(lib))
    return rc, outs


def written(outs):
    """no output still holds the sentinel everywhere it was to be written"""
    for name, a in outs.items():
        assert a.size == 0 or not (a == B.SENTINEL[a.dtype]).all(), name


@pytest.mark.parametrize("call", ["dlt_adjust", "isect_points", "resect_images", "relorient_pairs", "simil_models"])
def test_an_empty_item_beside_items_of_the_minimum_size(lib, minimum, call):
    """Items of 0, the minimum and the minimum + 1 observations.  The empty item reports TOO_FEW; the other two give, bit for bit, what
    they give in a batch of their own; and the call with every optional argument left out writes the same bits into what is left."""
    pair, triple = minimum[call]
    rc2, alone = same_census(lib, pair, True)
    rc3, full = same_census(lib, triple, True)
    rc0, bare = same_census(lib, triple, False)
    assert rc2 == 0 and rc3 == 0 and rc0 == 0, (rc2, rc3, rc0)
    written(alone); written(full); written(bare)
    assert set(bare) == {"out", "status"} and set(full) > set(bare)
    for name in bare:
        assert bare[name].tobytes() == full[name].tobytes(), name
    status = full["status"]
    assert status[0] == B.TOO_FEW and (status[1:] != B.TOO_FEW).all(), status
    width = full["out"].size // 3
    assert np.isnan(full["out"][:width]).all()
    for name, a in alone.items():                       # per item or per observation: the empty item has no observations
        if name == "ms":
            continue
        per_item = a.size // 2 if name in ("out", "status", "iterations", "start_kind", "solves") else 0
        assert full[name][per_item:].tobytes() == a.tobytes(), name
    if "iterations" in full:
        assert full["iterations"][0] == 0
    if "start_kind" in full:
        assert full["start_kind"][0] == 0
    print(f"{call}: status {status}, ms {full['ms'][0]:.3f}")


@pytest.mark.parametrize("call", ["dlt_adjust", "isect_points", "resect_images", "relorient_pairs", "simil_models"])
def test_a_batch_of_empty_items_without_its_observation_arrays(lib, minimum, call):
    """Two items, no observation at all, and NULL for every array that holds one entry per observation: the kernel gets null
    pointers for them (BatchCall::in), reports TOO_FEW for both items and reads none of them."""
    rc, outs = same_census(lib, B.all_empty(minimum[call][0]), True)
    assert rc == 0, rc
    assert (outs["status"] == B.TOO_FEW).all() and outs["status"].size == 2, outs["status"]
    assert np.isnan(outs["out"]).all()
    for name in ("iterations", "start_kind", "solves"):
        assert name not in outs or (outs[name] == 0).all(), (name, outs[name])
    assert outs["ms"][0] >= 0.0


@pytest.mark.parametrize("n", [1, 65])                  # one point, and one past a wave
@pytest.mark.parametrize("call", ["simil_apply", "lens_correct", "lens_distort"])
def test_calls_without_ranges_with_and_without_their_optional_arguments(lib, call, n):
    case = B.rangeless_cases(n)[call]
    rc1, full = same_census(lib, case, True)
    rc0, bare = same_census(lib, case, False)
    assert rc1 == 0 and rc0 == 0, (rc1, rc0)
    written(full); written(bare)
    assert bare and set(full) > set(bare)
    for name in bare:
        assert bare[name].tobytes() == full[name].tobytes(), name
    if "status" in full:
        assert (full["status"] == 0).all(), full["status"]
    assert np.isfinite(full["xy_out" if "xy_out" in full else "xyz_out"]).all()


def refused(case, name, value):
    """the case with one of its arguments replaced"""
    fn, args = case
    return fn, [(a[0], a[1], value, a[3]) if a[0] in ("in", "out") and a[1] == name else a for a in args]


def test_a_refused_call_touches_no_device_memory(lib, minimum):
    """JAICOV_ERR_BAD_ARGUMENT is an ordinary return before the call object exists: no output is written, the census stays."""
    bad = {call: refused(minimum[call][1], *what) for call, what in
           {"dlt_adjust": ("io", None), "isect_points": ("ray_image", np.full(5, 9, np.int32)), "resect_images": ("xyz", None),
            "relorient_pairs": ("var_a", np.zeros(3 * 13)), "simil_models": ("cof_dst", np.zeros(6 * 7))}.items()}
    rangeless = B.rangeless_cases(65)
    bad["simil_apply"] = refused(rangeless["simil_apply"], "cof", None)           # cof_out without cof
    bad["lens_correct"] = refused(rangeless["lens_correct"], "var", np.zeros(3 * 65))
    bad["lens_distort"] = refused(rangeless["lens_distort"], "camera", np.full(65, 3, np.int32))
    assert len(bad) == 8
    for call, case in bad.items():
        before = B.census(lib)
        rc, outs = B.invoke(lib, case, True)
        assert rc == B.BAD_ARGUMENT, (call, rc)
        assert B.census(lib) == before, call
        for name, a in outs.items():
            assert (a == B.SENTINEL[a.dtype]).all(), (call, name)
