"""Plain numpy restatement of one launch of the fp64 GEMM family (csrc/gemm_f64.h), written from the header's comments and using none
of the project's code.  It takes the arguments of the debug hook jaicov_debug_gemm plus the instance's tile (TM, TN), which decides the
units of lower_only and of the tile map, and returns what the launch has to leave in C.

Semantics restated:
  layouts   A: KC  A(i,k) = A[i*lda + k]     XC  A(i,k) = A[k*lda + i]
            B: KC  B(k,j) = B[j*ldb + k]     XC  B(k,j) = B[k*ldb + j]          C(i,j) = C[i*ldc + j]
  tiles     the grid is cut into TM x TN tiles.  lower_only keeps the tiles with tile_col <= tile_row -- in 128-tiles on the 128-tile
            instances, in 64-tiles on the lower 64 x 64 instance (which therefore also writes the upper 64-tile inside a diagonal
            128-tile when tile_col <= tile_row in 64-tile units).  A tile map (128-tile instances only) replaces the grid: its entries
            with row >= 0 are the tiles that are computed, whatever lower_only says; entries with a negative row are no tile.
  k range   of the tile (tile_row, tile_col), clamped to K:  FULL [0, K);  LE_ROW [0, (tile_row+1) TM);  GE_ROW [tile_row TM, K);
            GE_COL [tile_col TN, K).  An empty range leaves beta C.
  batches   batch (y, z) of batch x batch2 exists unless batch_sum_limit > 0 and y + z >= batch_sum_limit; its operands start at
            y stride + z stride2.
  value     C = alpha sum_k A(i,k) B(k,j) + beta C0; with beta == 0, C0 is not read.
Two arithmetic modes: "int64" (integer operands: the sums are exact integers, the scaling by alpha and beta is exact in double as long
as alpha, beta are small powers of two or their negatives and the sums stay far below 2^53) and "longdouble" (real operands)."""
import numpy as np
from numpy.lib.stride_tricks import as_strided

KC, XC = 0, 1
FULL, LE_ROW, GE_ROW, GE_COL = 0, 1, 2, 3


def tile_list(M, N, TM, TN, lower_only, tile_map, lower64=False):
    """(tile_row, tile_col) of every tile one batch computes, in units of the instance's tile."""
    if tile_map is not None and not lower64 and TM == 128 and TN == 128:
        return [(int(r), int(c)) for r, c in np.asarray(tile_map).reshape(-1, 2) if r >= 0]
    return [(r, c) for r in range(M // TM) for c in range(N // TN) if not lower_only or c <= r]


def k_range(kmode, r, c, TM, TN, K):
    if kmode == LE_ROW:
        return 0, min(K, (r + 1) * TM)
    if kmode == GE_ROW:
        return min(K, r * TM), K
    if kmode == GE_COL:
        return min(K, c * TN), K
    return 0, K


def _view(buf, off, rows, cols, ld):
    assert off >= 0 and rows > 0 and cols > 0 and off + (rows - 1) * ld + cols <= buf.size, "the reference would leave the buffer"
    return as_strided(buf[off:], shape=(rows, cols), strides=(ld * buf.itemsize, buf.itemsize), writeable=buf.flags.writeable)


def gemm_reference(alay, blay, M, N, K, alpha, beta, A, B, C0, lda, ldb, ldc, tile, c_alias=0, lower_only=0, kmode=FULL, batch=1, batch2=1,
                   strides=(0, 0, 0, 0, 0, 0), batch_sum_limit=0, tile_map=None, mode="int64", values=True):
    """A, B, C0: flat float64 buffers (with c_alias 1 / 2, C0 is ignored and C starts as a copy of A / B).  tile = (TM, TN) of the
    instance.  Returns a dict of flat arrays over the C buffer -- C (expected contents), mask (entries the launch writes), S (the
    magnitude |alpha| sum |A||B| + |beta| |C0|), klen (length of the entry's k range) -- and used_A, used_B over the operand buffers
    (entries some tile reads).  In "longdouble" mode C is a longdouble array (the reference is not rounded to double).  values=False: the
    masks and klen alone, without reading the operands."""
    TM, TN = tile
    lower64 = bool(lower_only) and TM == 64 and TN == 64
    assert mode in ("int64", "longdouble")
    A = np.asarray(A, np.float64).reshape(-1); B = np.asarray(B, np.float64).reshape(-1)
    start = A if c_alias == 1 else B if c_alias == 2 else np.asarray(C0, np.float64).reshape(-1)
    out = start.copy() if mode == "int64" else start.astype(np.longdouble)
    mask = np.zeros(out.size, bool)
    S = np.zeros(out.size, np.longdouble)
    klen = np.zeros(out.size, np.int64)
    used_A = np.zeros(A.size, bool); used_B = np.zeros(B.size, bool)
    sA, sB, sC, sA2, sB2, sC2 = strides
    wide = np.int64 if mode == "int64" else np.longdouble
    tiles = tile_list(M, N, TM, TN, lower_only, tile_map, lower64)
    for y in range(batch):
        for z in range(batch2):
            if batch_sum_limit > 0 and y + z >= batch_sum_limit:
                continue
            oA, oB, oC = y * sA + z * sA2, y * sB + z * sB2, y * sC + z * sC2
            a_rows, a_cols = (M, K) if alay == KC else (K, M)
            b_rows, b_cols = (N, K) if blay == KC else (K, N)
            Av, uA = _view(A, oA, a_rows, a_cols, lda), _view(used_A, oA, a_rows, a_cols, lda)
            Bv, uB = _view(B, oB, b_rows, b_cols, ldb), _view(used_B, oB, b_rows, b_cols, ldb)
            if alay == XC:
                Av, uA = Av.T, uA.T            # now (i, k)
            if blay == KC:
                Bv, uB = Bv.T, uB.T            # now (k, j)
            Cs, Co = _view(start, oC, M, N, ldc), _view(out, oC, M, N, ldc)
            Cm, CS, Ck = _view(mask, oC, M, N, ldc), _view(S, oC, M, N, ldc), _view(klen, oC, M, N, ldc)
            for r, c in tiles:
                i0, j0 = r * TM, c * TN
                k0, k1 = k_range(kmode, r, c, TM, TN, K)
                rows, cols = slice(i0, i0 + TM), slice(j0, j0 + TN)
                assert not Cm[rows, cols].any(), "two tiles of one launch write the same entries"
                Cm[rows, cols] = True; Ck[rows, cols] = k1 - k0
                uA[rows, k0:k1] = True; uB[k0:k1, cols] = True
                if not values:
                    continue
                if k1 > k0:
                    a = Av[rows, k0:k1]; b = Bv[k0:k1, cols]
                    assert np.isfinite(a).all() and np.isfinite(b).all(), "an operand entry inside a k range is not finite"
                    if mode == "int64":
                        assert (a == np.rint(a)).all() and (b == np.rint(b)).all()
                    acc = a.astype(wide) @ b.astype(wide)
                    if mode == "int64":
                        mag = (np.abs(a) @ np.abs(b)).astype(np.longdouble)      # integers below 2^53: exact in double
                    else:
                        mag = np.abs(a).astype(np.longdouble) @ np.abs(b).astype(np.longdouble)
                else:
                    acc = np.zeros((TM, TN), wide); mag = np.zeros((TM, TN), np.longdouble)
                if mode == "int64":
                    val = alpha * acc.astype(np.float64)      # exact: |acc| < 2^53
                    if beta != 0.0:
                        val = val + beta * Cs[rows, cols]
                else:
                    val = np.longdouble(alpha) * acc
                    if beta != 0.0:
                        val = val + np.longdouble(beta) * Cs[rows, cols].astype(np.longdouble)
                if beta != 0.0:
                    mag = abs(alpha) * mag + abs(beta) * np.abs(Cs[rows, cols]).astype(np.longdouble)
                else:
                    mag = abs(alpha) * mag
                Co[rows, cols] = val; CS[rows, cols] = mag
    return {"C": out, "mask": mask, "S": S, "klen": klen, "used_A": used_A, "used_B": used_B}
