"""The call shapes that pin the fp64 GEMM family (csrc/gemm_f64.h): one table for tests/test_gemm_plan.py (no device: the instance and
grid every shape must be given) and tests/test_gpu_gemm_family.py (the products themselves), and the builder of their operands.

A case is a dict: the launcher's arguments, the expected plan (TM, TN, tag, grid x) and how the buffers are laid out.
  pad        extra doubles on lda, ldb, ldc (even; 0 = leading dimension equals the extent)
  bcast_b2   strideB2 = 0 (one B for all of the second batch dimension, as SolveChains::premultiply passes W_k)
  same_ab    B is A: one buffer, one pointer (the trailing updates)
  map        None or a function (tile rows, tile cols, lower_only, rng) -> (n, 2) int32 tile map
"""
import numpy as np

import gemm_reference as gr

PAIRS = [(-1.0, 1.0), (1.0, 0.0), (0.5, -2.0), (-4.0, 1.0)]          # beta / alpha is a power of two
HIP_SUCCESS, HIP_INVALID_VALUE, BAD_ARGUMENT = 0, 1, -1
LAYOUTS = {"kckc": (0, 0), "kcxc": (0, 1), "xcxc": (1, 1), "xckc": (1, 0)}


def lower_tiles(T):
    return [(r, c) for r in range(T) for c in range(r + 1)]


def map_permutation(tm, tn, lower, rng):
    t = lower_tiles(tm) if lower else [(r, c) for r in range(tm) for c in range(tn)]
    return np.array(t, np.int32)[rng.permutation(len(t))]


def map_with_holes(tm, tn, lower, rng):
    m = map_permutation(tm, tn, lower, rng)
    out = np.full((len(m) + 5, 2), -1, np.int32)
    out[np.sort(rng.permutation(len(out))[:len(m)])] = m
    return out


def map_column_major(tm, tn, lower, rng):        # the orders of trtri_tile_order (dense.hip)
    return np.array([(r, c) for c in range(tn) for r in range(tm)], np.int32)


def map_reverse_row_major(tm, tn, lower, rng):
    return np.array([(r, c) for r in reversed(range(tm)) for c in range(tn)], np.int32)


def map_xcd(tm, tn, lower, rng):
    from bundle_adjustment_amd import engine
    return engine.debug_xcd_tile_map(tm)


def _case(id, lay, M, N, K, plan, ab=0, **kw):
    alay, blay = LAYOUTS[lay]
    c = dict(id=id, alay=alay, blay=blay, M=M, N=N, K=K, ab=PAIRS[ab % 4] if isinstance(ab, int) else ab, plan=plan, pad=(2, 4, 6), c_alias=0,
             lower_only=0, kmode=0, batch=1, batch2=1, batch_sum_limit=0, small_tiles=-1, tag=0, map=None, bcast_b2=False, same_ab=False)
    c.update(kw)
    return c


def instance_cases():
    """Every instance the launcher can choose, at the smallest shapes that still have one stage, two stages, odd and even stage counts,
    one tile and several."""
    out = []
    n = 0
    for tag in (0, 1):
        for M, N in ((128, 128), (256, 384)):
            for K in (16, 32, 48, 272):
                out.append(_case(f"kckc128-tag{tag}-{M}x{N}-K{K}", "kckc", M, N, K, (128, 128, tag, (M // 128) * (N // 128)), ab=n,
                                 small_tiles=0, tag=tag, pad=(0, 0, 0) if K == 32 else (2, 4, 6)))
                n += 1
    for lay in ("kcxc", "xcxc", "xckc"):
        for K in (16, 32, 48, 272):
            out.append(_case(f"{lay}128-256x384-K{K}", lay, 256, 384, K, (128, 128, 0, 6), ab=n, pad=(0, 0, 0) if K == 32 else (6, 2, 4)))
            n += 1
    for M, N in ((128, 256), (256, 128)):
        for K in (48, 272):
            out.append(_case(f"rect64-{M}x{N}-K{K}", "kckc", M, N, K, (64, 64, 0, 8), ab=n, small_tiles=1))
            n += 1
    for M, N in ((128, 128), (256, 384)):
        for K in (16, 272):
            out.append(_case(f"rect32-{M}x{N}-K{K}", "kckc", M, N, K, (32, 32, 0, (M // 128) * (N // 128) * 16), ab=n))
            n += 1
    for M in (128, 384):           # in place, C is A: one column tile, beta = 0
        t = M // 128
        out.append(_case(f"inplace64x128-c_is_a-M{M}", "kckc", M, 128, 128, (64, 128, 0, 2 * t), ab=1, c_alias=1, small_tiles=1))
        out.append(_case(f"inplace32x128-c_is_a-M{M}", "kckc", M, 128, 128, (32, 128, 0, 4 * t), ab=1, c_alias=1))
        out.append(_case(f"inplace128-c_is_a-M{M}", "kckc", M, 128, 128, (128, 128, 0, t), ab=1, c_alias=1, small_tiles=0))
    # C is B: every workgroup reads all of B, so only the launch with ONE workgroup is in place; the others are refused (refusal_cases)
    out.append(_case("inplace128-c_is_b-M128", "kckc", 128, 128, 128, (128, 128, 0, 1), ab=1, c_alias=2, small_tiles=0))
    for tag in (0, 1):
        for M in (128, 384):
            t64 = M // 64
            out.append(_case(f"lower64-tag{tag}-{M}", "kckc", M, M, 48, (64, 64, tag, t64 * (t64 + 1) // 2), ab=n, lower_only=1, small_tiles=1,
                             tag=tag, same_ab=(M == 384 and tag == 1), pad=(2, 2, 6)))
            n += 1
    out.append(_case("lower128-384", "kckc", 384, 384, 48, (128, 128, 0, 6), ab=0, lower_only=1))
    out.append(_case("lower128-384-map", "kckc", 384, 384, 48, (128, 128, 0, 6), ab=2, lower_only=1, small_tiles=0, map=map_permutation))
    return out


def krange_cases():
    """kmode 1, 2, 3 on every layout pair, K a multiple of 128 and not, and the shapes where some tiles have an empty range."""
    out = []
    n = 0
    for kmode, name in ((1, "le_row"), (2, "ge_row"), (3, "ge_col")):
        for lay in LAYOUTS:
            for K in (384, 272):
                M, N = (256, 384) if kmode == 3 else (384, 256)
                out.append(_case(f"{name}-{lay}-K{K}", lay, M, N, K, (128, 128, 0, 6), ab=n, kmode=kmode, small_tiles=(0, -1, 1)[n % 3]))
                n += 1
    for lay in ("kckc", "xcxc"):
        out.append(_case(f"ge_row-{lay}-empty-M384-K128", lay, 384, 128, 128, (128, 128, 0, 3), ab=(0.5, -2.0), kmode=2))
        out.append(_case(f"ge_col-{lay}-empty-N384-K128", lay, 128, 384, 128, (128, 128, 0, 3), ab=(-4.0, 1.0), kmode=3))
    out.append(_case("ge_row-xcxc-lower-K384", "xcxc", 384, 384, 384, (128, 128, 0, 6), ab=1, kmode=2, lower_only=1))     # W'W
    return out


def batch_cases():
    out = []
    for name, small, plan in (("128", 0, (128, 128, 0, 2)), ("64", 1, (64, 64, 0, 8)), ("32", -1, (32, 32, 0, 32))):
        out.append(_case(f"batch3x2-{name}", "kckc", 128, 256, 48, plan, ab=0, batch=3, batch2=2, small_tiles=small))
    out.append(_case("batch3x2-kcxc-broadcast-b2", "kcxc", 128, 256, 48, (128, 128, 0, 2), ab=2, batch=3, batch2=2, bcast_b2=True))
    out.append(_case("batch3x2-64-broadcast-b2", "kckc", 128, 256, 48, (64, 64, 0, 8), ab=3, batch=3, batch2=2, bcast_b2=True, small_tiles=1))
    out.append(_case("batch2-lower-same-ab", "kckc", 256, 256, 48, (128, 128, 0, 3), ab=0, batch2=2, lower_only=1, same_ab=True, pad=(2, 2, 6)))
    out.append(_case("batch3-lower64-same-ab", "kckc", 256, 256, 48, (64, 64, 0, 10), ab=3, batch=3, lower_only=1, small_tiles=1, same_ab=True,
                     pad=(2, 2, 6)))
    out.append(_case("batch3x3-sum-limit-3", "kckc", 128, 256, 48, (128, 128, 0, 2), ab=0, batch=3, batch2=3, batch_sum_limit=3, small_tiles=0))
    out.append(_case("batch3x3-sum-limit-2-xckc", "xckc", 128, 256, 48, (128, 128, 0, 2), ab=1, batch=3, batch2=3, batch_sum_limit=2))
    out.append(_case("batch3x3-sum-limit-3-rect64", "kckc", 128, 128, 48, (64, 64, 0, 4), ab=2, batch=3, batch2=3, batch_sum_limit=3, small_tiles=1))
    return out


def map_cases():
    out = [
        _case("map-permutation", "kckc", 256, 384, 48, (128, 128, 0, 6), ab=0, small_tiles=0, map=map_permutation),
        _case("map-holes", "kcxc", 256, 384, 48, (128, 128, 0, 11), ab=1, map=map_with_holes),
        _case("map-holes-lower-tag1", "kckc", 384, 384, 48, (128, 128, 1, 11), ab=3, lower_only=1, tag=1, small_tiles=0, map=map_with_holes),
        _case("map-xcd-T3", "kckc", 384, 384, 48, (128, 128, 1, 8), ab=0, lower_only=1, tag=1, same_ab=True, pad=(2, 2, 6), map=map_xcd),
        # the first size the solver uses the map at: 24 tile rows, 300 tiles in 8 lists of 37 or 38
        _case("map-xcd-T24", "kckc", 3072, 3072, 16, (128, 128, 1, 304), ab=0, lower_only=1, tag=1, same_ab=True, pad=(2, 2, 2), map=map_xcd),
        _case("map-column-major-ge_col-batch2", "kcxc", 256, 384, 384, (128, 128, 0, 6), ab=1, kmode=3, batch=2, map=map_column_major),
        _case("map-reverse-rows-le_row-batch2", "kcxc", 384, 256, 384, (128, 128, 0, 6), ab=1, kmode=1, batch=2, map=map_reverse_row_major),
    ]
    return out


def refusal_cases():
    """(case, expected status of the plan or None when the hook refuses before it plans).  All are answered BAD_ARGUMENT and leave C alone."""
    two = dict(c_alias=1, ab=1)
    return [
        (_case("alpha-zero", "kckc", 128, 128, 48, None, ab=(0.0, 1.0)), HIP_INVALID_VALUE),
        (_case("alpha-zero-beta-zero-xcxc", "xcxc", 128, 128, 48, None, ab=(0.0, 0.0)), HIP_INVALID_VALUE),
        (_case("inplace-two-columns-small-branch", "kckc", 128, 256, 256, None, small_tiles=1, **two), HIP_INVALID_VALUE),
        (_case("inplace-two-columns-tiny-rule", "kckc", 128, 256, 256, None, small_tiles=-1, **two), HIP_INVALID_VALUE),
        (_case("inplace-two-columns-small-tiles-0", "kckc", 128, 256, 256, None, small_tiles=0, **two), HIP_INVALID_VALUE),
        (_case("inplace-two-columns-480-tiles", "kckc", 128, 256, 256, None, small_tiles=-1, batch=240, **two), HIP_INVALID_VALUE),
        (_case("inplace-two-columns-kcxc", "kcxc", 128, 256, 256, None, **two), HIP_INVALID_VALUE),
        (_case("inplace-two-columns-lower-grid", "kckc", 256, 256, 256, None, lower_only=1, **two), HIP_INVALID_VALUE),
        (_case("inplace-lower64", "kckc", 128, 128, 128, None, lower_only=1, small_tiles=1, **two), HIP_INVALID_VALUE),
        (_case("inplace-c_is_b-two-columns", "kckc", 256, 256, 256, None, small_tiles=0, c_alias=2, ab=1), HIP_INVALID_VALUE),
        (_case("inplace64x128-c_is_b-M128", "kckc", 128, 128, 128, None, small_tiles=1, c_alias=2, ab=1), HIP_INVALID_VALUE),
        (_case("inplace32x128-c_is_b-M128", "kckc", 128, 128, 128, None, small_tiles=-1, c_alias=2, ab=1), HIP_INVALID_VALUE),
        (_case("inplace64x128-c_is_b-M384", "kckc", 384, 128, 128, None, small_tiles=1, c_alias=2, ab=1), HIP_INVALID_VALUE),
        (_case("inplace32x128-c_is_b-M384", "kckc", 384, 128, 128, None, small_tiles=-1, c_alias=2, ab=1), HIP_INVALID_VALUE),
        (_case("inplace128-c_is_b-M384", "kckc", 384, 128, 128, None, small_tiles=0, c_alias=2, ab=1), HIP_INVALID_VALUE),
        (_case("tag-2", "kckc", 128, 128, 48, None, small_tiles=0, tag=2), None),
        (_case("tag-3", "kckc", 128, 128, 48, None, small_tiles=0, tag=3), None),
    ]


def real_cases():
    """alpha = 0.75, beta = -0.5, one case per layout pair and per tile size, K = 48 and 1024."""
    out = []
    for K in (48, 1024):
        M, N = (256, 384) if K == 48 else (128, 256)
        t = (M // 128) * (N // 128)
        for lay in LAYOUTS:
            out.append(_case(f"real-{lay}128-K{K}", lay, M, N, K, (128, 128, 0, t), ab=(0.75, -0.5), small_tiles=0))
        out.append(_case(f"real-rect64-K{K}", "kckc", M, N, K, (64, 64, 0, 4 * t), ab=(0.75, -0.5), small_tiles=1))
        out.append(_case(f"real-rect32-K{K}", "kckc", M, N, K, (32, 32, 0, 16 * t), ab=(0.75, -0.5)))
        out.append(_case(f"real-inplace64x128-K{K}", "kckc", 256, 128, K, (64, 128, 0, 4), ab=(0.75, -0.5), c_alias=1, small_tiles=1))
        out.append(_case(f"real-inplace32x128-K{K}", "kckc", 256, 128, K, (32, 128, 0, 8), ab=(0.75, -0.5), c_alias=1))
        out.append(_case(f"real-lower64-K{K}", "kckc", 256, 256, K, (64, 64, 0, 10), ab=(0.75, -0.5), lower_only=1, small_tiles=1))
        out.append(_case(f"real-lower128-tag1-K{K}", "kckc", 256, 256, K, (128, 128, 1, 3), ab=(0.75, -0.5), lower_only=1, tag=1))
    return out


def hook_kwargs(c, L):
    """The arguments of engine.debug_gemm that do not depend on the data (L = layout(c))."""
    return dict(alay=c["alay"], blay=c["blay"], M=c["M"], N=c["N"], K=c["K"], alpha=c["ab"][0], beta=c["ab"][1], lda=L["lda"], ldb=L["ldb"],
                ldc=L["ldc"], c_alias=c["c_alias"], lower_only=c["lower_only"], kmode=c["kmode"], batch=c["batch"], batch2=c["batch2"],
                strides=L["strides"], batch_sum_limit=c["batch_sum_limit"], small_tiles=c["small_tiles"], tag=c["tag"])


def layout(c):
    """Leading dimensions, strides and element counts: the full batch rectangle of every operand, distinct strides with gaps."""
    M, N, K = c["M"], c["N"], c["K"]
    a_rows, a_cols = (M, K) if c["alay"] == 0 else (K, M)
    b_rows, b_cols = (N, K) if c["blay"] == 0 else (K, N)
    lda, ldb, ldc = a_cols + c["pad"][0], b_cols + c["pad"][1], N + c["pad"][2]
    if c["c_alias"] == 1:
        lda = ldc = max(lda, ldc)
    if c["c_alias"] == 2:
        ldb = ldc = max(ldb, ldc)
    by, bz = c["batch"], c["batch2"]
    sA, sB, sC = a_rows * lda + 10, b_rows * ldb + 6, M * ldc + 14
    sA2, sB2, sC2 = by * sA + 2, by * sB + 4, by * sC + 8
    if c["bcast_b2"]:
        sB2 = 0
    if c["same_ab"]:
        assert (a_rows, a_cols, lda) == (b_rows, b_cols, ldb)
        sB, sB2 = sA, sA2
    if by == 1:
        sA = sB = sC = 0
    if bz == 1:
        sA2 = sB2 = sC2 = 0
    size = lambda rows, ld, s1, s2: (by - 1) * s1 + (bz - 1) * s2 + rows * ld      # noqa: E731  (the last row keeps its padding)
    n_A, n_B, n_C = size(a_rows, lda, sA, sA2), size(b_rows, ldb, sB, sB2), size(M, ldc, sC, sC2)
    if c["c_alias"] == 1:
        n_A = n_C = max(n_A, n_C)
    if c["c_alias"] == 2:
        n_B = n_C = max(n_B, n_C)
    return dict(lda=lda, ldb=ldb, ldc=ldc, strides=(sA, sB, sC, sA2, sB2, sC2), n_A=n_A, n_B=n_B, n_C=n_C)


def pattern(n):
    """n distinct quiet NaNs with a recognisable payload: what C holds wherever the launch must not write."""
    return (np.int64(0x7FF8C0DE00000000) + np.arange(n, dtype=np.int64)).view(np.float64)


def build(c, real=False):
    """Operands of a case and the reference's answer.  Integer mode: A, B in [-1023, 1023], C0 below 2^20.  Real mode: normal variates, the
    rows of op(A) and the columns of op(B) scaled by powers of two spread over 2^+-20.  Everything no tile reads -- padding, the operand
    outside the tiles' k ranges, batches that do not exist -- is NaN in A and B; everything the launch must not write holds pattern() in
    C; with beta == 0 the rest of C is NaN too."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    L = layout(c)
    M, N, K = c["M"], c["N"], c["K"]
    TM, TN = c["plan"][:2]
    tmap = c["map"](M // 128, N // 128, c["lower_only"], rng) if c["map"] else None
    alpha, beta = c["ab"]
    if real:                   # (one batch: the flat index of an entry gives its row and column)
        ea = np.exp2(rng.integers(-20, 21, size=M).astype(np.float64)); eb = np.exp2(rng.integers(-20, 21, size=N).astype(np.float64))
        ia, ib, ic = np.arange(L["n_A"]), np.arange(L["n_B"]), np.arange(L["n_C"])
        A = rng.normal(size=L["n_A"]) * ea[(ia // L["lda"] if c["alay"] == 0 else ia % L["lda"]) % M]
        B = A if c["same_ab"] else rng.normal(size=L["n_B"]) * eb[(ib // L["ldb"] if c["blay"] == 0 else ib % L["ldb"]) % N]
        C0 = rng.normal(size=L["n_C"]) * ea[(ic // L["ldc"]) % M] * eb[(ic % L["ldc"]) % N] * np.sqrt(K)      # the size of the product beside it
    else:
        A = rng.integers(-1023, 1024, size=L["n_A"]).astype(np.float64)
        B = A if c["same_ab"] else rng.integers(-1023, 1024, size=L["n_B"]).astype(np.float64)
        C0 = rng.integers(-(1 << 20) + 1, 1 << 20, size=L["n_C"]).astype(np.float64)
    args = dict(alay=c["alay"], blay=c["blay"], M=M, N=N, K=K, alpha=alpha, beta=beta, lda=L["lda"], ldb=L["ldb"], ldc=L["ldc"], tile=(TM, TN),
                c_alias=c["c_alias"], lower_only=c["lower_only"], kmode=c["kmode"], batch=c["batch"], batch2=c["batch2"], strides=L["strides"],
                batch_sum_limit=c["batch_sum_limit"], tile_map=tmap, mode="longdouble" if real else "int64")
    sets = gr.gemm_reference(A=A, B=B, C0=C0, values=False, **args)
    mask = sets["mask"]
    used_A, used_B = sets["used_A"], sets["used_B"]
    if c["same_ab"]:
        used_A = used_B = used_A | used_B
    if c["c_alias"] == 1:
        used_A = used_A | (mask if beta != 0.0 else False)     # C0 is A's buffer: what beta reads stays finite
    if c["c_alias"] == 2:
        used_B = used_B | (mask if beta != 0.0 else False)
    A[~used_A] = np.nan
    if not c["same_ab"]:
        B[~used_B] = np.nan
    if c["c_alias"] == 0:
        C0[~mask] = pattern(C0.size)[~mask]
        if beta == 0.0:
            C0[mask] = np.nan
    ref = gr.gemm_reference(A=A, B=B, C0=C0, **args)
    start = A if c["c_alias"] == 1 else B if c["c_alias"] == 2 else C0
    return dict(A=A, B=B, C0=C0, start=start.copy(), tile_map=tmap, ref=ref, layout=L)
