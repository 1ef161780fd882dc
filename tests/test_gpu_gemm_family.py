"""GPU: every instance the fp64 GEMM launcher (csrc/gemm_f64.h) can choose, through jaicov_debug_gemm -- one launch with every argument
of the launcher in the test's hand -- against tests/gemm_reference.py.

Integer operands, equality instead of a tolerance: A and B hold integers in [-1023, 1023], C0 integers below 2^20, (alpha, beta) one of
(-1, 1), (1, 0), (0.5, -2), (-4, 1) so that beta / alpha is a power of two, K <= 4096.  A product needs 10 + 10 bits, a sum of 4096 of them
12 more, the start (beta/alpha) C0 stays below 2^22: every partial sum is an integer below 2^33 and every order of accumulation gives the
same double, so np.array_equal with the int64 reference is the assertion.  (Signed zeros are not told apart: alpha (+0) is -0 for a
negative alpha.)

What is NaN and what is a pattern (gemm_family_cases.build): every entry of A and B that no tile may read -- the padding of the leading
dimensions, the operand outside each tile's k range, batches that do not exist -- is NaN, so a kernel that read it would show it; with
beta == 0 all of C0 that is written is NaN too (C must not be read); every entry of C outside the write mask, padding included, holds a
quiet NaN with its own payload and has to come back bit for bit.

Every case asserts the returned plan first: a rule change that reroutes a case fails instead of passing on another instance.  The same
table is held without a device by tests/test_gemm_plan.py.

Real operands, a derived bound: normal variates, rows of A and columns of B scaled by powers of two over 2^+-20, alpha 0.75, beta -0.5,
against the longdouble reference: |got - ref| <= (k_len + 8) 2^-53 S elementwise, S = |alpha| sum |a||b| + |beta| |c0| -- the bound of a
recursive sum of k_len fused products, 8 for the roundings of beta/alpha, of its product with C0 and of the final scaling."""
import ctypes as C

import numpy as np
import pytest

import gemm_family_cases as gc
from bundle_adjustment_amd import engine

pytestmark = pytest.mark.gpu


def launch(case, real=False):
    d = gc.build(case, real)
    rc, plan, got = engine.debug_gemm(A=d["A"], B=d["B"], C_in=d["C0"], tile_map=d["tile_map"], **gc.hook_kwargs(case, d["layout"]))
    assert plan == (gc.HIP_SUCCESS,) + tuple(case["plan"]) + (case["batch"], case["batch2"]), "the launcher chose another instance or grid"
    assert rc == 0
    return d, got


def check_exact(case):
    d, got = launch(case)
    ref, m = d["ref"], d["ref"]["mask"]
    assert m.any()
    untouched = got.view(np.int64)[~m] == d["start"].view(np.int64)[~m]
    assert untouched.all(), f"{(~untouched).sum()} entries outside the write mask changed"
    assert np.isfinite(got[m]).all(), "NaN or Inf: the kernel used an entry it may not read"
    assert np.array_equal(got[m], ref["C"][m])
    empty = m & (ref["klen"] == 0)
    if empty.any():                    # a tile with an empty k range becomes exactly beta C0
        assert np.array_equal(got[empty], case["ab"][1] * d["start"][empty])
    return d, got


@pytest.mark.parametrize("case", gc.instance_cases(), ids=lambda c: c["id"])
def test_every_instance_exact(case):
    check_exact(case)


@pytest.mark.parametrize("case", gc.krange_cases(), ids=lambda c: c["id"])
def test_k_ranges_exact(case):
    assert case["plan"][:2] == (128, 128)          # the ranges are counted in 128-tiles and hold on the 128-tile instances only
    d, _ = check_exact(case)
    assert np.isnan(d["A"]).any() or np.isnan(d["B"]).any()
    if "empty" in case["id"]:
        m = d["ref"]["mask"]
        assert (d["ref"]["klen"][m] == 0).sum() == 2 * 128 * 128


@pytest.mark.parametrize("case", gc.batch_cases(), ids=lambda c: c["id"])
def test_batches_exact(case):
    d, _ = check_exact(case)
    if case["batch_sum_limit"]:
        exist = sum(y + z < case["batch_sum_limit"] for y in range(case["batch"]) for z in range(case["batch2"]))
        assert 0 < exist < case["batch"] * case["batch2"] and d["ref"]["mask"].sum() == exist * case["M"] * case["N"]


@pytest.mark.parametrize("case", gc.map_cases(), ids=lambda c: c["id"])
def test_tile_maps_exact(case):
    d, _ = check_exact(case)
    assert len(d["tile_map"]) == case["plan"][3]


@pytest.mark.parametrize("case,status", [pytest.param(c, s, id=c["id"]) for c, s in gc.refusal_cases()])
def test_refusals_leave_c_alone(case, status):
    L = gc.layout(case)
    A = np.ones(L["n_A"]); B = np.ones(L["n_B"]); C0 = gc.pattern(L["n_C"])
    if case["c_alias"] == 1:
        A = gc.pattern(L["n_A"])
    if case["c_alias"] == 2:
        B = gc.pattern(L["n_B"])
    start = (A if case["c_alias"] == 1 else B if case["c_alias"] == 2 else C0).copy()
    rc, plan, got = engine.debug_gemm(A=A, B=B, C_in=C0, **gc.hook_kwargs(case, L))
    assert rc == gc.BAD_ARGUMENT
    assert plan[0] == (status if status is not None else -1)
    assert np.array_equal(got.view(np.int64), start.view(np.int64))


def test_accesses_that_would_leave_the_buffers_are_refused():
    """The hook decides on the host that every access stays inside what it uploads; nothing here reaches the device."""
    case = gc._case("bounds", "kckc", 128, 256, 48, None, ab=0, batch=3, batch2=2, small_tiles=0)
    L = gc.layout(case)
    A = np.ones(L["n_A"]); B = np.ones(L["n_B"]); C0 = gc.pattern(L["n_C"])
    kw = gc.hook_kwargs(case, L)
    assert engine.debug_gemm(A=A, B=B, C_in=C0, **kw)[0] == 0
    s = list(L["strides"])
    bad = [dict(A=A[:-4]), dict(B=B[:-6]), dict(C_in=C0[:-8]), dict(lda=L["lda"] + 2), dict(ldb=46), dict(ldc=L["ldc"] + 2), dict(ldc=254),
           dict(lda=L["lda"] - 1), dict(batch=4), dict(batch2=3), dict(M=256), dict(K=64), dict(M=100), dict(K=40), dict(kmode=4), dict(alay=2)]
    for i in range(6):
        t = list(s); t[i] += 16
        bad.append(dict(strides=tuple(t)))
        t = list(s); t[i] = -t[i]
        bad.append(dict(strides=tuple(t)))
    for tmap in ([(0, 0), (1, 0)], [(0, 2), (0, 0)], [(0, -1), (0, 0)]):           # tile row 1, tile column 2 and column -1 do not exist
        bad.append(dict(tile_map=np.array(tmap, np.int32)))
    for over in bad:
        args = dict(dict(A=A, B=B, C_in=C0, **kw), **over)
        rc, _, got = engine.debug_gemm(**args)
        assert rc == gc.BAD_ARGUMENT, over
        assert np.array_equal(got.view(np.int64), args["C_in"].view(np.int64))
    for tmap in ([(0, 1), (0, 0)], [(0, 1)], [(-1, 7), (0, 0), (-3, -3)]):         # a map may leave tiles out; a negative row is no tile
        assert engine.debug_gemm(A=A, B=B, C_in=C0, tile_map=np.array(tmap, np.int32), **kw)[0] == 0


def test_the_hook_frees_what_it_allocates():
    lib = engine.load_library()
    lib.jaicov_debug_device_census.argtypes = [C.POINTER(C.c_longlong)]
    lib.jaicov_debug_device_census.restype = None
    def census():
        a = (C.c_longlong * 2)()
        lib.jaicov_debug_device_census(a)
        return tuple(a)
    case = next(c for c in gc.map_cases() if c["id"] == "map-holes")
    launch(case)
    before = census()
    launch(case)
    bad = gc.refusal_cases()[2][0]
    L = gc.layout(bad)
    A = np.ones(L["n_A"])
    assert engine.debug_gemm(A=A, B=np.ones(L["n_B"]), C_in=None, **gc.hook_kwargs(bad, L))[0] == gc.BAD_ARGUMENT
    assert census() == before


@pytest.mark.parametrize("case", gc.real_cases(), ids=lambda c: c["id"])
def test_real_operands_within_the_derived_bound(case):
    d, got = launch(case, real=True)
    ref, m = d["ref"], d["ref"]["mask"]
    assert np.array_equal(got.view(np.int64)[~m], d["start"].view(np.int64)[~m])
    assert np.isfinite(got[m]).all()
    assert (ref["klen"][m] == case["K"]).all() and float(ref["S"][m].min()) > 0.0
    err = np.abs(got[m].astype(np.longdouble) - ref["C"][m])
    bound = (ref["klen"][m] + 8) * np.longdouble(2.0) ** -53 * ref["S"][m]
    ratio = err / bound
    spread = float(np.log2(ref["S"][m].max() / ref["S"][m].min()))
    print(f"{case['id']}: worst |got - ref| / bound = {float(ratio.max()):.4f}, magnitudes spread over 2^{spread:.0f}")
    assert spread > 30                      # small rows exist beside large ones: an absolute tolerance could not hold both
    assert (err <= bound).all(), float(ratio.max())
