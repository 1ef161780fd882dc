"""CPU: tests/gemm_reference.py against itself and against brute force.  Its two arithmetic modes (int64 sums, longdouble sums) must give
the same numbers on integer operands, where both are exact; its write mask, k-range lengths and operand-use masks must be what an
entry-by-entry loop over the header's rules gives, at one small shape per kmode (and for the lower grids in both tile units, a tile map
with holes and a triangular batch set)."""
import numpy as np
import pytest

import gemm_family_cases as gc
import gemm_reference as gr

BOTH_MODES = [c for c in gc.instance_cases() + gc.krange_cases() + gc.batch_cases() + gc.map_cases()
              if c["id"] in ("kckc128-tag0-256x384-K272", "xcxc128-256x384-K48", "rect64-128x256-K272", "inplace64x128-c_is_a-M384",
                             "lower64-tag1-384", "lower128-384-map", "le_row-kcxc-K272", "ge_row-xcxc-lower-K384", "ge_col-kckc-empty-N384-K128",
                             "batch3x2-kcxc-broadcast-b2", "batch3x3-sum-limit-3", "map-holes")]


def test_the_selection_found_its_cases():
    assert len(BOTH_MODES) == 12


@pytest.mark.parametrize("case", BOTH_MODES, ids=lambda c: c["id"])
def test_int64_and_longdouble_modes_agree_on_integers(case):
    d = gc.build(case)
    L, ref = d["layout"], d["ref"]
    other = gr.gemm_reference(case["alay"], case["blay"], case["M"], case["N"], case["K"], *case["ab"], d["A"], d["B"], d["C0"], L["lda"], L["ldb"],
                              L["ldc"], tile=case["plan"][:2], c_alias=case["c_alias"], lower_only=case["lower_only"], kmode=case["kmode"],
                              batch=case["batch"], batch2=case["batch2"], strides=L["strides"], batch_sum_limit=case["batch_sum_limit"],
                              tile_map=d["tile_map"], mode="longdouble")
    m = ref["mask"]
    assert m.any() and np.array_equal(m, other["mask"]) and np.array_equal(ref["klen"], other["klen"])
    assert np.isfinite(ref["C"][m]).all()
    assert np.array_equal(ref["C"][m].astype(np.longdouble), other["C"][m])
    assert np.array_equal(ref["S"], other["S"])
    assert np.array_equal(ref["C"].view(np.int64)[~m], d["start"].view(np.int64)[~m])          # what is not written is not touched
    # a product that is not trivially zero, and the exactness budget of the integer tests: every magnitude far below 2^53
    assert np.abs(ref["C"][m]).max() > 1e3 and float(ref["S"].max()) < 2.0 ** 36


def brute_force(M, N, K, TM, TN, lower_only, kmode, tiles, alay, blay, lda, ldb, ldc):
    """Entry by entry, for one batch at offset 0: (mask, klen) over C and the use masks over A and B."""
    def k_lo_hi(r, c):
        lo, hi = 0, K
        if kmode == 1:
            hi = min(K, (r + 1) * 128)
        elif kmode == 2:
            lo = min(K, r * 128)
        elif kmode == 3:
            lo = min(K, c * 128)
        return lo, hi
    mask = np.zeros(M * ldc, bool); klen = np.zeros(M * ldc, np.int64)
    uA = np.zeros((M if alay == 0 else K) * lda, bool); uB = np.zeros((N if blay == 0 else K) * ldb, bool)
    for i in range(M):
        for j in range(N):
            if (i // TM, j // TN) in tiles:
                lo, hi = k_lo_hi(i // TM, j // TN)
                mask[i * ldc + j] = True
                klen[i * ldc + j] = hi - lo
    for k in range(K):                     # an operand entry is read if some tile of its row (column) strip has k in its range
        for i in range(M):
            if any(r == i // TM and k_lo_hi(r, c)[0] <= k < k_lo_hi(r, c)[1] for r, c in tiles):
                uA[i * lda + k if alay == 0 else k * lda + i] = True
        for j in range(N):
            if any(c == j // TN and k_lo_hi(r, c)[0] <= k < k_lo_hi(r, c)[1] for r, c in tiles):
                uB[j * ldb + k if blay == 0 else k * ldb + j] = True
    return mask, klen, uA, uB


@pytest.mark.parametrize("kmode,alay,blay,M,N,K,TM,lower,use_map", [
    (0, 0, 0, 128, 256, 32, 128, 0, False), (1, 0, 1, 256, 128, 208, 128, 0, False), (2, 1, 1, 256, 256, 256, 128, 1, False),
    (3, 0, 1, 128, 256, 208, 128, 0, False), (2, 0, 0, 256, 128, 128, 128, 0, False), (3, 1, 0, 128, 256, 128, 128, 0, False),
    (0, 0, 0, 256, 256, 16, 64, 1, False), (0, 0, 0, 256, 256, 16, 128, 1, False), (0, 0, 0, 128, 128, 16, 32, 0, False),
    (1, 0, 0, 256, 256, 256, 128, 1, True), (3, 1, 1, 256, 256, 144, 128, 0, True)])
def test_masks_against_brute_force(kmode, alay, blay, M, N, K, TM, lower, use_map):
    TN = TM
    lda, ldb, ldc = (K if alay == 0 else M) + 2, (K if blay == 0 else N) + 4, N + 6
    tmap = None
    if use_map:
        tmap = np.array([(-1, -1), (1, 0), (-1, 5), (0, 0), (1, 1), (-1, -1)], np.int32)       # (0, 1) is missing; a negative row is no tile
        tiles = {(1, 0), (0, 0), (1, 1)}
    else:
        tiles = {(r, c) for r in range(M // TM) for c in range(N // TN) if not lower or c <= r}
    if TM == 64 and lower:
        assert (0, 1) not in tiles and (1, 0) in tiles and (2, 3) not in tiles and (3, 2) in tiles      # 64-tile units: (3, 2) lies inside a diagonal 128-tile
    want = brute_force(M, N, K, TM, TN, lower, kmode, tiles, alay, blay, lda, ldb, ldc)
    n_A, n_B = want[2].size, want[3].size
    got = gr.gemm_reference(alay, blay, M, N, K, 1.0, 1.0, np.zeros(n_A), np.zeros(n_B), np.zeros(M * ldc), lda, ldb, ldc, tile=(TM, TN),
                            lower_only=lower, kmode=kmode, tile_map=tmap, values=False)
    for name, w in zip(("mask", "klen", "used_A", "used_B"), want):
        assert np.array_equal(got[name], w), name
    assert got["mask"].sum() == len(tiles) * TM * TN


def test_batches_that_do_not_exist_are_left_out():
    M = N = 128; K = 16
    sA, sB, sC = 128 * 16 + 2, 128 * 16 + 4, 128 * 128 + 6
    strides = (sA, sB, sC, 3 * sA, 0, 3 * sC)
    n_A, n_B, n_C = 9 * sA, 3 * sB, 9 * sC
    got = gr.gemm_reference(0, 0, M, N, K, 1.0, 0.0, np.zeros(n_A), np.zeros(n_B), np.zeros(n_C), K, K, N, tile=(128, 128), batch=3, batch2=3,
                            strides=strides, batch_sum_limit=3, values=False)
    for y in range(3):
        for z in range(3):
            o = y * sC + z * 3 * sC
            assert got["mask"][o:o + M * N].all() == (y + z < 3) and got["mask"][o:o + M * N].any() == (y + z < 3)
            assert not got["mask"][o + M * N:o + sC].any()
    assert got["used_B"].sum() == 3 * 128 * 16 and got["used_A"].sum() == 6 * 128 * 16


def test_values_against_a_plain_product():
    rng = np.random.default_rng(3)
    M, N, K = 128, 256, 48
    Aop = rng.integers(-9, 10, size=(M, K)).astype(np.float64); Bop = rng.integers(-9, 10, size=(K, N)).astype(np.float64)
    C0 = rng.integers(-99, 100, size=(M, N)).astype(np.float64)
    want = -4.0 * (Aop @ Bop) + C0
    for alay in (0, 1):
        for blay in (0, 1):
            A = Aop if alay == 0 else Aop.T
            B = Bop.T if blay == 0 else Bop
            for mode in ("int64", "longdouble"):
                got = gr.gemm_reference(alay, blay, M, N, K, -4.0, 1.0, np.ascontiguousarray(A).ravel(), np.ascontiguousarray(B).ravel(), C0.ravel(),
                                        A.shape[1], B.shape[1], N, tile=(64, 64), mode=mode)
                assert np.array_equal(got["C"].reshape(M, N), want) and got["mask"].all()
