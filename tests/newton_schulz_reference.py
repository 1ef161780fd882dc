"""numpy restatement of the Newton-Schulz step with an error-free residual (csrc/batchinv.hip), for the tests.

The device refines an inverse X of a symmetric D by X <- X + sym(X R), R = I - D X, and forms R from slices: D = D1 + D2 by
rows, X = X1 + X2 by rows (X is symmetric: its row slices, transposed, are its column slices), D1 and X1 holding the leading
20 bits relative to their row's largest entry.  Every product D1[i][k] X1[k][j] is then a multiple of one unit per (i, j) and
a sum of n <= 8192 of them stays below 2^53 units: D1 X1 is exact in fp64 in ANY summation order, so the BLAS product below
is the same number the matrix cores give.  The two small products are ordinary fp64 here as there.

Also here: the test matrices (prescribed spectrum, rows of different scale, a permuted block-diagonal form whose exact
inverse costs one small inversion), the error measure, and the helper that puts such matrices into a FlatProblem."""
import dataclasses

import numpy as np

SLICE_BITS = 20


def slice_rows(A, bits=SLICE_BITS):
    """(hi, lo): hi = the leading `bits` bits of every entry relative to its row's largest, lo = A - hi (exact)."""
    A = np.asarray(A, dtype=np.float64)
    mx = np.abs(A).max(axis=1)
    _, ex = np.frexp(mx)                                   # mx = f 2^ex, f in [0.5, 1)
    unit = np.ldexp(1.0, ex - bits)[:, None]
    hi = np.rint(A / unit) * unit                          # (a power of two: the division and the product are exact)
    hi[mx == 0.0] = 0.0
    return hi, A - hi


def step(D, X):
    """One step from X: returns (X + (Y + Y') / 2, R) with Y = X R, R = I - D1 X1 - D1 X2 - D2 X."""
    D = np.asarray(D, dtype=np.float64); X = np.asarray(X, dtype=np.float64)
    D1, D2 = slice_rows(D)
    X1r, X2r = slice_rows(X)
    R = np.eye(D.shape[0]) - D1 @ X1r.T                    # exact
    R -= D1 @ X2r.T
    R -= D2 @ X
    Y = X @ R
    return X + 0.5 * (Y + Y.T), R


def corr_err(W, P):
    """max |W_ij - P_ij| / sqrt(P_ii P_jj): the error of an inverse against truth P, free of the scale of its rows."""
    s = np.sqrt(np.abs(np.diag(P)).astype(np.float64))
    return float((np.abs(np.asarray(W, np.float64) - P) / np.outer(s, s)).max())


def newton_ld(K, X0, max_iter=4, tol=1e-13):
    """The inverse of K by Newton steps in extended precision from X0, to convergence (cond(K) 2^-64 of its largest entries)."""
    Kl, X = np.asarray(K).astype(np.longdouble), np.asarray(X0).astype(np.longdouble)
    I2 = 2 * np.eye(K.shape[0], dtype=np.longdouble)
    for _ in range(max_iter):
        Xn = X @ (I2 - Kl @ X)
        Xn = 0.5 * (Xn + Xn.T)
        last = corr_err(X.astype(np.float64), Xn.astype(np.float64))
        X = Xn
        if last < tol:
            return X
    raise ArithmeticError(f"extended-precision Newton iteration did not converge: {last:.2e}")


# ---- test matrices ---------------------------------------------------------------------------------------------------------
def spectrum_matrix(m, decades, seed, scaled=False):
    """Q diag(logspace(0, -decades)) Q', symmetrised; scaled: rows and columns times s, log-uniform over three decades."""
    rng = np.random.Generator(np.random.Philox(seed))
    Q, _ = np.linalg.qr(rng.normal(size=(m, m)))
    C = (Q * np.logspace(0.0, -float(decades), m)) @ Q.T
    C = 0.5 * (C + C.T)
    if scaled:
        s = 10.0 ** rng.uniform(-1.5, 1.5, m)
        C = np.outer(s, s) * C                             # s_i s_j = s_j s_i in fp64: still symmetric to the bit
    return np.ascontiguousarray(C)


def permuted_blocks(B, n, seed, max_shift=4):
    """A symmetric random permutation of blockdiag(B 2^e_0, B 2^e_1, ...), order n (a multiple of B's), and the function that
    arranges inv(B) -- whatever form it is known in -- into the inverse: arrange(Binv)[i][j] = Binv 2^-e_k in the same places.
    Powers of two scale exactly, so truth at order n is as good as truth for B."""
    k = B.shape[0]
    assert n % k == 0
    rng = np.random.Generator(np.random.Philox(seed))
    shift = rng.integers(-max_shift, max_shift + 1, n // k)
    perm = rng.permutation(n)

    def arrange(blk, sign=-1):
        A = np.zeros((n, n), dtype=np.asarray(blk).dtype)
        for b in range(n // k):
            A[b * k:(b + 1) * k, b * k:(b + 1) * k] = np.ldexp(blk, sign * int(shift[b]))
        return np.ascontiguousarray(A[np.ix_(perm, perm)])

    return arrange(B, +1), arrange


def signed_integers(n, seed, symmetric=False, bits=SLICE_BITS):
    """n x n random integers of magnitude below 2^bits, as int64."""
    rng = np.random.Generator(np.random.Philox(seed))
    A = rng.integers(-(2 ** bits) + 1, 2 ** bits, (n, n), dtype=np.int64)
    if symmetric:
        A = np.tril(A) + np.tril(A, -1).T
    return A


# ---- dispersions of a FlatProblem -------------------------------------------------------------------------------------------
def carrier(m, n_images=3):
    """A small scene whose every image is one jointly dispersed block of order m (every image sees all m / 2 points)."""
    from bundle_adjustment_amd import scene
    return scene.make_scene(n_images, m // 2, m // 2, dist=scene.DIST_RADIAL, weights="block", n_control=4, min_rays=min(3, n_images))


def with_dispersions(fp, mats):
    """fp (every image one jointly dispersed block) with mats[i] as the dispersion of image i.  A matrix smaller than the
    image's block keeps the image's first points only; var_x, var_y are the diagonals, as scene.make_scene leaves them."""
    assert len(mats) == fp.n_image_blocks == fp.n_images
    counts = np.diff(fp.blk_ip_begin)
    want = np.array([M.shape[0] // 2 for M in mats])
    assert all(M.shape[0] % 2 == 0 for M in mats) and (want <= counts).all() and (want > 0).all()
    keep = np.concatenate([np.arange(fp.blk_ip_begin[i], fp.blk_ip_begin[i] + want[i]) for i in range(counts.size)])
    assert np.array_equal(np.unique(fp.ip_point[keep]), np.unique(fp.ip_point)), "a point would lose all its observations"
    sizes = np.array([M.size for M in mats], np.int64)
    diag = np.concatenate([np.diag(M) for M in mats])
    return dataclasses.replace(
        fp, ip_image=fp.ip_image[keep], ip_point=fp.ip_point[keep], ip_x=fp.ip_x[keep], ip_y=fp.ip_y[keep], ip_rho=fp.ip_rho[keep],
        ip_var_x=np.ascontiguousarray(diag[0::2]), ip_var_y=np.ascontiguousarray(diag[1::2]),
        blk_ip_begin=np.concatenate([[0], np.cumsum(want)]).astype(np.int32),
        blk_disp_offset=np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64),
        blk_disp=np.concatenate([np.asarray(M, np.float64).ravel() for M in mats]), n_observations=0).validate()
