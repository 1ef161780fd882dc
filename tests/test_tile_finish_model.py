"""The register-level finish of an off-diagonal Cholesky tile (csrc/cholflow.hip, chol_tile_kernel with REG_FINISH), restated in numpy.

The kernel forms Y' = inv(L_jj) X with X = C' held in the accumulators: 8 x 8 blocks of 16 x 16, wave (wr, wc) = (wave >> 1, wave & 1)
owns block rows 4 wr .. 4 wr + 3 and block columns 4 wc .. 4 wc + 3.  The top waves leave their blocks for the bottom waves, then
every wave multiplies IN PLACE, bottom block row first, only the block pairs kb <= mb.  What can go wrong there is index work, so the
model keeps every index of the kernel: who owns what, what is read from whom, in which order, and which register is which operand.
"""
import numpy as np

NB, BS = 8, 16            # blocks per side, block size
WAVES = [(w >> 1, w & 1) for w in range(4)]


def finish_model(M, X, log=None):
    """Steps 2-3 as the kernel runs them.  Returns M X.  log: list of (wave, 'r' | 'w', (block row, block column)) in program order,
    reads of the published top half as (wave, 'p', ...)."""
    blk = lambda A, i, j: A[BS * i:BS * (i + 1), BS * j:BS * (j + 1)]
    own = {w: {(mb, nb): blk(X, mb, nb).copy() for mb in range(4 * wr, 4 * wr + 4) for nb in range(4 * wc, 4 * wc + 4)}
           for w, (wr, wc) in enumerate(WAVES)}
    # step 2: the waves with wr == 0 publish their 16 blocks (before anybody multiplies: one barrier in the kernel)
    published = {wc: {key: b.copy() for key, b in own[w].items()} for w, (wr, wc) in enumerate(WAVES) if wr == 0}
    # step 3, each wave on its own
    for w, (wr, wc) in enumerate(WAVES):
        for x in (3, 2, 1, 0):
            mb = 4 * wr + x
            tmp = {nb: np.zeros((BS, BS)) for nb in range(4 * wc, 4 * wc + 4)}
            if wr != 0:
                for kb in range(4):
                    for r in range(4):             # register r of X[kb][nb] is the B operand of the k-block {4 r .. 4 r + 3}
                        for nb in tmp:
                            if log is not None:
                                log.append((w, "p", (kb, nb)))
                            tmp[nb] += blk(M, mb, kb)[:, 4 * r:4 * r + 4] @ published[wc][(kb, nb)][4 * r:4 * r + 4, :]
            for kb in range(4 * wr, mb + 1):
                for r in range(4):
                    for nb in tmp:
                        if log is not None:
                            log.append((w, "r", (kb, nb)))
                        tmp[nb] += blk(M, mb, kb)[:, 4 * r:4 * r + 4] @ own[w][(kb, nb)][4 * r:4 * r + 4, :]
            for nb in tmp:
                if log is not None:
                    log.append((w, "w", (mb, nb)))
                own[w][(mb, nb)] = tmp[nb]
    Y = np.zeros_like(X)
    for w in range(4):
        for (mb, nb), b in own[w].items():
            blk(Y, mb, nb)[:] = b
    return Y


def test_in_place_product_is_the_product():
    rng = np.random.default_rng(1)
    for _ in range(3):
        # entries of |M| |X| stay below one (128 terms of mean 0.64 / 128), so 1e-14 absolute is 90 rounding errors of such a sum: the
        # sums have 128 terms, in blocks of four
        M = np.tril(rng.normal(size=(128, 128))) / 128
        X = rng.normal(size=(128, 128))
        assert float((np.abs(M) @ np.abs(X)).max()) < 1.0
        Y = finish_model(M, X)
        ref = M.astype(np.longdouble) @ X.astype(np.longdouble)
        assert float(np.abs(Y - ref).max()) <= 1e-14


def test_no_block_is_read_after_it_was_overwritten():
    log = []
    M = np.tril(np.ones((128, 128)))
    finish_model(M, np.ones((128, 128)), log)
    for w, (wr, wc) in enumerate(WAVES):
        written = set()
        n_mult = 0
        for who, what, key in log:
            if who != w:
                continue
            if what == "w":
                assert key not in written
                written.add(key)
            elif what == "r":
                assert key not in written, (w, key)
                assert 4 * wr <= key[0] < 4 * wr + 4 and 4 * wc <= key[1] < 4 * wc + 4        # its own registers only
                n_mult += 1
            else:
                assert wr == 1 and key[0] < 4 and 4 * wc <= key[1] < 4 * wc + 4                # the top half, same block columns
                n_mult += 1
        assert len(written) == 16
        assert n_mult == (26 if wr else 10) * 4 * 4            # block pairs kb <= mb of its four block rows x four nb x four registers
    # 36 of the 64 block pairs are multiplied, each for every one of the 8 block columns and 4 registers
    assert sum(1 for who, what, key in log if what != "w") == 36 * 8 * 4


def test_published_top_half_is_the_original():
    """The top waves overwrite their own blocks while the bottom waves may still be reading: the bottom waves must see X, not Y'."""
    rng = np.random.default_rng(2)
    M = np.tril(rng.normal(size=(128, 128)))
    X = rng.normal(size=(128, 128))
    Y = finish_model(M, X)
    np.testing.assert_allclose(Y[64:], M[64:] @ X, rtol=0, atol=1e-12)


def test_accumulator_register_is_the_b_operand_of_its_k_block():
    """v_mfma_f64_16x16x4_f64: accumulator register r holds D[(lane >> 4) + 4 r][lane & 15]; the B operand is B[k = lane >> 4][n = lane & 15];
    the A operand is A[m = lane & 15][k = lane >> 4].  Register r of a block of X is therefore the B operand of rows 4 r .. 4 r + 3,
    and the A fragment that goes with it is inv[16 mb + (lane & 15)][16 kb + 4 r + (lane >> 4)].  One 16 x 16 product, lane by lane."""
    rng = np.random.default_rng(3)
    A = rng.normal(size=(16, 16))
    Xb = rng.normal(size=(16, 16))
    lanes = np.arange(64)
    acc = [Xb[(lanes >> 4) + 4 * r, lanes & 15] for r in range(4)]        # the block as the accumulators hold it
    D = np.zeros((16, 16))
    for r in range(4):
        a_frag = A[lanes & 15, 4 * r + (lanes >> 4)]                       # what the kernel loads from the inverse
        Aop = np.zeros((16, 4)); Bop = np.zeros((4, 16))
        Aop[lanes & 15, lanes >> 4] = a_frag
        Bop[lanes >> 4, lanes & 15] = acc[r]                               # register r, as it stands
        D += Aop @ Bop
    np.testing.assert_allclose(D, A @ Xb, rtol=0, atol=1e-13)
    # the kernel's own table: the four lane groups carry rows 4 r + {0, 1, 3, 2} (the order in which the pipelined loop's staging feeds
    # them, so that the sums stay the ones of that loop); A fragment and B operand are permuted alike, the product is the same
    perm = (lanes >> 4) ^ (lanes >> 5)
    assert [int(perm[16 * g]) for g in range(4)] == [0, 1, 3, 2]
    D = np.zeros((16, 16))
    for r in range(4):
        Aop = np.zeros((16, 4)); Bop = np.zeros((4, 16))
        Aop[lanes & 15, lanes >> 4] = A[lanes & 15, 4 * r + perm]
        Bop[lanes >> 4, lanes & 15] = Xb[4 * r + perm, lanes & 15]
        D += Aop @ Bop
    np.testing.assert_allclose(D, A @ Xb, rtol=0, atol=1e-13)
    # the index table itself: register r <-> k-block r
    for r in range(4):
        assert sorted(set((lanes >> 4) + 4 * r)) == list(range(4 * r, 4 * r + 4))


def test_transposition_halves_are_their_own_mirror_image():
    """transpose_acc: block (x, y) of a wave goes out in half 0 when (x < 2) == (y < 2), else in half 1; the wave reads block (y, x) of
    the wave across the diagonal into the registers of (x, y).  Each half must hold the mirror image of each of its blocks (the
    registers read are the ones just written), 8 blocks with 8 different slots, and fit the staging array with a row stride of 17.
    Both forms: rows as they stand (the way back), and rows 4 r + {0, 1, 3, 2} in the four lane groups (the way in)."""
    slot = lambda x, y: 4 * (x >> 1) + 2 * (x & 1) + (y & 1)
    for half in (0, 1):
        S = [(x, y) for x in range(4) for y in range(4) if ((x >> 1) == (y >> 1)) == (half == 0)]
        assert len(S) == 8 and {(y, x) for x, y in S} == set(S)
        assert sorted(slot(x, y) for x, y in S) == list(range(8))
    assert 4 * 8 * 16 * 17 <= 2 * 16 * 2 * 144 and 2 * 64 * 64 <= 2 * 16 * 2 * 144
    # the whole transposition, element by element, with the kernel's addresses
    rng = np.random.default_rng(4)
    C = rng.normal(size=(128, 128))
    lanes = np.arange(64)
    for kk in (lanes >> 4, (lanes >> 4) ^ (lanes >> 5)):
        _transposition(C, lanes, kk, slot)


def _transposition(C, lanes, kk, slot):
    regs = {w: {(x, y, r): C[64 * wr + 16 * x + 4 * r + (lanes >> 4), 64 * wc + 16 * y + (lanes & 15)]
                for x in range(4) for y in range(4) for r in range(4)} for w, (wr, wc) in enumerate(WAVES)}
    TS, TB, TW = 17, 16 * 17, 8 * 16 * 17
    for half in (0, 1):
        lds = np.full(4 * TW, np.nan)
        S = [(x, y) for x in range(4) for y in range(4) if ((x >> 1) == (y >> 1)) == (half == 0)]
        for w in range(4):
            for x, y in S:
                for r in range(4):
                    lds[w * TW + (lanes >> 4) * TS + (lanes & 15) + slot(x, y) * TB + 4 * r * TS] = regs[w][(x, y, r)]
        for w in range(4):
            src = 2 * (w & 1) + (w >> 1)
            for x, y in S:
                for r in range(4):
                    regs[w][(x, y, r)] = lds[src * TW + (lanes & 15) * TS + kk + slot(y, x) * TB + 4 * r]
    for w, (wr, wc) in enumerate(WAVES):
        for (x, y, r), v in regs[w].items():
            np.testing.assert_array_equal(v, C.T[64 * wr + 16 * x + 4 * r + kk, 64 * wc + 16 * y + (lanes & 15)])
