// Precision figures read from the cofactor matrix on the device (include/jaicov_precision.h).
//
//   prec_block_kernel   points and stations: one lane per item gathers its 3 x 3 block (and, for a station, the three diagonal
//                       entries of the angles), runs the cyclic Jacobi of the header and writes one row of figures.
//   prec_length_kernel  lengths: one lane per pair gathers the 6 x 6 block with its cross-covariances.
//   components          subspace iteration with a block of 8 vectors.  The product Y = S X is the pair of symtile.h that the datum
//                       transformation uses (D = 8, bounds of the sub-block); prec_gram_*, prec_apply_kernel and
//                       prec_resid_kernel are n x 8 operations with fixed-order sums.  The 8 x 8 algebra (Jacobi of the Ritz matrix,
//                       Cholesky factor of the Gram matrix) stays on the host, as datum.hip keeps its d x d algebra there.
// Nothing here writes to the cofactor matrix or to any other state of the engine but the work buffers of PrecisionState.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/jaicov_precision.h"
#include "precision.h"
#include "qview.h"
#include "status.h"
#include "symtile.h"

namespace jaicov {

constexpr double PREC_EPS = 2.220446049250313e-16;     // 2^-52
constexpr int PREC_SWEEPS = 30;
constexpr int PREC_TAB = 8;                            // int32 per item of the column table

// one Jacobi rotation (P, Q) of the symmetric a with third index R; false: skipped
template <int P, int Q_, int R>
__device__ __forceinline__ bool prec_rot(double (&a)[3][3], double (&v)[3][3]) {
    const double apq = a[P][Q_];
    if (fabs(apq) <= PREC_EPS * sqrt(fabs(a[P][P] * a[Q_][Q_]))) return false;
    const double th = (a[Q_][Q_] - a[P][P]) / (2.0 * apq);
    const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    a[P][P] -= t * apq;
    a[Q_][Q_] += t * apq;
    a[P][Q_] = a[Q_][P] = 0.0;
    const double arp = a[R][P], arq = a[R][Q_];
    a[R][P] = a[P][R] = c * arp - s * arq;
    a[R][Q_] = a[Q_][R] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double vp = v[k][P], vq = v[k][Q_];
        v[k][P] = c * vp - s * vq;
        v[k][Q_] = s * vp + c * vq;
    }
    return true;
}

template <int I, int J>
__device__ __forceinline__ void prec_order(double (&l)[3], double (&v)[3][3]) {      // descending, equal values keep their order
    if (l[J] > l[I]) {
        const double x = l[I]; l[I] = l[J]; l[J] = x;
#pragma unroll
        for (int k = 0; k < 3; k++) { const double y = v[k][I]; v[k][I] = v[k][J]; v[k][J] = y; }
    }
}

// tab[8 i + 0 .. 2]: columns of X, Y, Z; [3 .. 5]: columns of omega, phi, kappa (ncol == 25)
__global__ __launch_bounds__(256) void prec_block_kernel(const double *__restrict__ Q, long ld, const int32_t *__restrict__ tab, int n,
                                                         double sigma2, double k3, double k2, int ncol, double *__restrict__ out,
                                                         int32_t *__restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t *tb = tab + (size_t)PREC_TAB * i;
    const int c0 = tb[0], c1 = tb[1], c2 = tb[2];
    double C[3][3];
    C[0][0] = q_at(Q, ld, c0, c0); C[1][1] = q_at(Q, ld, c1, c1); C[2][2] = q_at(Q, ld, c2, c2);
    C[0][1] = C[1][0] = q_at(Q, ld, c0, c1);
    C[0][2] = C[2][0] = q_at(Q, ld, c0, c2);
    C[1][2] = C[2][1] = q_at(Q, ld, c1, c2);
    double ang[3] = {0.0, 0.0, 0.0};
    if (ncol > JAICOV_PREC_POINT_COLUMNS)
#pragma unroll
        for (int k = 0; k < 3; k++) ang[k] = q_at(Q, ld, tb[3 + k], tb[3 + k]);
    int st = (c0 < 0 || c1 < 0 || c2 < 0) ? JAICOV_PREC_PARTIAL : 0;
    double *o = out + (size_t)ncol * i;
    const double sum = ((C[0][0] + C[1][1]) + C[2][2]) + (C[0][1] + C[0][2] + C[1][2]) + (ang[0] + ang[1] + ang[2]) + sigma2 + k3 + k2;
    if (!isfinite(sum)) {
        for (int k = 0; k < ncol; k++) o[k] = NAN;
        status[i] = st | JAICOV_PREC_NOT_FINITE;
        return;
    }
    const double tr = (C[0][0] + C[1][1]) + C[2][2];
    const double m = fmax(C[0][0], fmax(C[1][1], C[2][2]));
    double l[3] = {0.0, 0.0, 0.0};
    double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    if (m != 0.0) {
        double a[3][3];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) a[r][c] = C[r][c] / m;
#pragma unroll 1
        for (int sweep = 0; sweep < PREC_SWEEPS; sweep++) {
            bool any = prec_rot<0, 1, 2>(a, v);
            any |= prec_rot<0, 2, 1>(a, v);
            any |= prec_rot<1, 2, 0>(a, v);
            if (!any) break;
        }
#pragma unroll
        for (int k = 0; k < 3; k++) l[k] = m * a[k][k];
    }
    prec_order<0, 1>(l, v);
    prec_order<1, 2>(l, v);
    prec_order<0, 1>(l, v);
#pragma unroll
    for (int c = 0; c < 3; c++) {                  // sign rule: the component of largest magnitude is positive
        double big = v[0][c];
        if (fabs(v[1][c]) > fabs(big)) big = v[1][c];
        if (fabs(v[2][c]) > fabs(big)) big = v[2][c];
        if (big < 0.0)
#pragma unroll
            for (int k = 0; k < 3; k++) v[k][c] = -v[k][c];
    }
    if (l[2] < -1e-12 * tr) st |= JAICOV_PREC_NEGATIVE;
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = sqrt(sigma2 * fmax(C[k][k], 0.0));
    o[3] = sqrt(sigma2 * fmax(tr, 0.0));
#pragma unroll
    for (int c = 0; c < 3; c++) {
        o[4 + c] = k3 * sqrt(sigma2 * fmax(l[c], 0.0));
#pragma unroll
        for (int k = 0; k < 3; k++) o[7 + 3 * c + k] = v[k][c];
        o[19 + c] = l[c];
    }
    const double hm = 0.5 * (C[0][0] + C[1][1]), hd = 0.5 * (C[0][0] - C[1][1]), hw = hypot(hd, C[0][1]);
    o[16] = k2 * sqrt(sigma2 * fmax(hm + hw, 0.0));
    o[17] = k2 * sqrt(sigma2 * fmax(hm - hw, 0.0));
    double dir = 0.5 * atan2(2.0 * C[0][1], C[0][0] - C[1][1]);
    if (dir < 0.0) dir += M_PI;
    if (dir >= M_PI) dir = 0.0;
    o[18] = dir;
    if (ncol > JAICOV_PREC_POINT_COLUMNS)
#pragma unroll
        for (int k = 0; k < 3; k++) o[22 + k] = sqrt(sigma2 * fmax(ang[k], 0.0));
    status[i] = st;
}

// tab[8 i + 0 .. 5]: columns of X, Y, Z of A and of B; [6], [7]: first slot of A and of B
__global__ __launch_bounds__(256) void prec_length_kernel(const double *__restrict__ Q, long ld, const double *__restrict__ vals,
                                                          const int32_t *__restrict__ tab, int n, double sigma2, double *__restrict__ out,
                                                          int32_t *__restrict__ status) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t *tb = tab + (size_t)PREC_TAB * i;
    int col[6];
    int st = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        col[k] = tb[k];
        if (col[k] < 0) st = JAICOV_PREC_PARTIAL;
    }
    const int sa = tb[6], sb = tb[7];
    double D[3], g[6];
#pragma unroll
    for (int k = 0; k < 3; k++) D[k] = vals[sb + k] - vals[sa + k];
    const double L = sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) { g[3 + k] = D[k] / L; g[k] = -g[3 + k]; }
    double var = 0.0, chk = sigma2 + L;
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            const double q = q_at(Q, ld, col[r], col[c]);
            chk += q;
            s += q * g[c];
        }
        var += g[r] * s;
    }
    double *o = out + (size_t)JAICOV_PREC_LENGTH_COLUMNS * i;
    if (!isfinite(chk)) {
#pragma unroll
        for (int k = 0; k < JAICOV_PREC_LENGTH_COLUMNS; k++) o[k] = NAN;
        status[i] = st | JAICOV_PREC_NOT_FINITE;
        return;
    }
    o[0] = L;
    if (L == 0.0) {
        st |= JAICOV_PREC_DEGENERATE;
        o[1] = NAN;
    } else {
        if (var < 0.0) st |= JAICOV_PREC_NEGATIVE;
        o[1] = sqrt(sigma2 * fmax(var, 0.0));
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double dv = (q_at(Q, ld, col[k], col[k]) + q_at(Q, ld, col[3 + k], col[3 + k])) - 2.0 * q_at(Q, ld, col[3 + k], col[k]);
        if (dv < 0.0) st |= JAICOV_PREC_NEGATIVE;
        o[2 + k] = sqrt(sigma2 * fmax(dv, 0.0));
    }
    status[i] = st;
}

// ---- the n x 8 operations of the component iteration.  Every array is [np][8] (rows outside the sub-block are zero), np a multiple of 128.

// partial[blk][8 a + b] = sum over the 256 rows of the workgroup of A[i][a] B[i][b]: thread (quarter, entry) adds every fourth row in
// order, the quarters are combined in order
__global__ __launch_bounds__(256) void prec_gram_partial_kernel(const double *__restrict__ A, const double *__restrict__ B, int np,
                                                                double *__restrict__ partial) {
    __shared__ double sa[256][8], sb[256][8];
    __shared__ double part[4][64];
    const int tid = threadIdx.x, row0 = blockIdx.x * 256;
    for (int k = tid; k < 256 * 8; k += 256) {
        const int r = k >> 3, c = k & 7;
        const bool ok = row0 + r < np;
        sa[r][c] = ok ? A[(size_t)(row0 + r) * 8 + c] : 0.0;
        sb[r][c] = ok ? B[(size_t)(row0 + r) * 8 + c] : 0.0;
    }
    __syncthreads();
    const int e = tid & 63, q = tid >> 6, a = e >> 3, b = e & 7;
    double acc = 0.0;
    for (int r = q; r < 256; r += 4) acc = fma(sa[r][a], sb[r][b], acc);
    part[q][e] = acc;
    __syncthreads();
    if (tid < 64) partial[(size_t)blockIdx.x * 64 + tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

// G[e] = the partial sums added in workgroup order
__global__ __launch_bounds__(64) void prec_gram_final_kernel(const double *__restrict__ partial, int nblk, double *__restrict__ G) {
    double acc = 0.0;
    for (int k = 0; k < nblk; k++) acc += partial[(size_t)k * 64 + threadIdx.x];
    G[threadIdx.x] = acc;
}

// out[i][b] = sum_a in[i][a] M[a][b]; written row-wise (out_r, [np][8]) and, when out_t is given, column-wise ([8][np])
__global__ __launch_bounds__(256) void prec_apply_kernel(const double *__restrict__ in, const double *__restrict__ M, int np,
                                                         double *__restrict__ out_r, double *__restrict__ out_t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    double x[8];
#pragma unroll
    for (int a = 0; a < 8; a++) x[a] = in[(size_t)i * 8 + a];
#pragma unroll
    for (int b = 0; b < 8; b++) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 8; a++) s = fma(x[a], M[8 * a + b], s);
        out_r[(size_t)i * 8 + b] = s;
        if (out_t) out_t[(size_t)b * np + i] = s;
    }
}

// R[i][a] = sum_b Y[i][b] Z[b][a] - theta[a] sum_b X[i][b] Z[b][a];  ZT: Z (64, row-major) | theta (8)
__global__ __launch_bounds__(256) void prec_resid_kernel(const double *__restrict__ X, const double *__restrict__ Y, const double *__restrict__ ZT,
                                                         int np, double *__restrict__ R) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    double x[8], y[8];
#pragma unroll
    for (int b = 0; b < 8; b++) { x[b] = X[(size_t)i * 8 + b]; y[b] = Y[(size_t)i * 8 + b]; }
#pragma unroll
    for (int a = 0; a < 8; a++) {
        double sy = 0.0, sx = 0.0;
#pragma unroll
        for (int b = 0; b < 8; b++) {
            sy = fma(y[b], ZT[8 * b + a], sy);
            sx = fma(x[b], ZT[8 * b + a], sx);
        }
        R[(size_t)i * 8 + a] = sy - ZT[64 + a] * sx;
    }
}

// the sum of Q[i][i], lo <= i < hi: thread t adds every 256th entry in order, thread 0 adds the 256 sums in order
__global__ __launch_bounds__(256) void prec_trace_kernel(const double *__restrict__ Q, long ld, int lo, int hi, double *__restrict__ out) {
    __shared__ double part[256];
    double acc = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) acc += Q[(long)i * ld + i];
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < 256; k++) s += part[k];
        *out = s;
    }
}

// ---- the 8 x 8 algebra on the host

// eigen-decomposition of the symmetric H (8 x 8, row-major) by cyclic Jacobi: th descending, the columns of Z with them
static void prec_jacobi8(const double *H, double *th, double *Z) {
    double a[8][8], v[8][8];
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++) { a[i][j] = 0.5 * (H[8 * i + j] + H[8 * j + i]); v[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; sweep++) {
        bool any = false;
        for (int p = 0; p < 7; p++)
            for (int q = p + 1; q < 8; q++) {
                const double apq = a[p][q];
                if (!(fabs(apq) > PREC_EPS * sqrt(fabs(a[p][p] * a[q][q])))) continue;
                any = true;
                const double t0 = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (t0 >= 0.0 ? 1.0 : -1.0) / (fabs(t0) + sqrt(t0 * t0 + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                a[p][p] -= t * apq;
                a[q][q] += t * apq;
                a[p][q] = a[q][p] = 0.0;
                for (int r = 0; r < 8; r++) {
                    if (r != p && r != q) {
                        const double arp = a[r][p], arq = a[r][q];
                        a[r][p] = a[p][r] = c * arp - s * arq;
                        a[r][q] = a[q][r] = s * arp + c * arq;
                    }
                    const double vp = v[r][p], vq = v[r][q];
                    v[r][p] = c * vp - s * vq;
                    v[r][q] = s * vp + c * vq;
                }
            }
        if (!any) break;
    }
    int idx[8];
    for (int i = 0; i < 8; i++) idx[i] = i;
    std::stable_sort(idx, idx + 8, [&](int x, int y) { return a[x][x] > a[y][y]; });
    for (int c = 0; c < 8; c++) {
        th[c] = a[idx[c]][idx[c]];
        for (int r = 0; r < 8; r++) Z[8 * r + c] = v[r][idx[c]];
    }
}

// G = R'R (R upper), Rinv = R^-1 (upper, row-major); false: no factor
static bool prec_chol_inverse8(const double *G, double *Rinv) {
    double R[8][8] = {};
    for (int j = 0; j < 8; j++) {
        double s = G[8 * j + j];
        for (int k = 0; k < j; k++) s -= R[k][j] * R[k][j];
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        R[j][j] = sqrt(s);
        for (int c = j + 1; c < 8; c++) {
            double u = 0.5 * (G[8 * j + c] + G[8 * c + j]);
            for (int k = 0; k < j; k++) u -= R[k][j] * R[k][c];
            R[j][c] = u / R[j][j];
        }
    }
    for (int i = 0; i < 64; i++) Rinv[i] = 0.0;
    for (int c = 0; c < 8; c++) {                       // column c of R^-1 by back substitution of R x = e_c
        for (int r = c; r >= 0; r--) {
            double s = r == c ? 1.0 : 0.0;
            for (int k = r + 1; k <= c; k++) s -= R[r][k] * Rinv[8 * k + c];
            Rinv[8 * r + c] = s / R[r][r];
        }
    }
    return true;
}

static inline uint64_t prec_splitmix(uint64_t c) {
    uint64_t z = (c + 1) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

static const char PREC_SHARDED[] = "precision figures on a sharded engine";

// points (station == false) or projection centres: the column table, the launch, the download
static int prec_blocks(jaicov_engine *e, bool station, double sigma2, double k3, double k2, const int32_t *items, int32_t n, double *out,
                       int32_t *status) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    TRY(q_guard(v, PREC_SHARDED));
    const DevProblem &p = *v.p;
    if (station && v.reduced) FAIL(*v.err, JAICOV_ERR_BAD_STATE, "station precision needs the exterior orientations' columns: invert FULL or FULL_EXPANDED");
    const int total = station ? p.n_images : p.n_points;
    if (!out || !status || n < 0 || (!items && n != total)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "precision: NULL output or a wrong count");
    if (!(sigma2 >= 0.0) || !(k3 >= 0.0) || !(k2 >= 0.0)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "precision: sigma2, k3 and k2 must not be negative");
    const int eo0 = 3 * p.n_points + 3 * p.n_cameras + p.n_dist;
    std::vector<int32_t> tab((size_t)PREC_TAB * std::max(n, 1), -1);
    for (int i = 0; i < n; i++) {
        const int it = items ? items[i] : i;
        if (it < 0 || it >= total) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "precision: index out of range");
        const int slot = station ? eo0 + 6 * it : 3 * it;
        for (int k = 0; k < (station ? 6 : 3); k++) {
            TRY(q_column(v, slot + k, "precision: the item's columns are not in the reduced cofactor matrix", &tab[(size_t)PREC_TAB * i + k]));
        }
    }
    if (n == 0) return JAICOV_OK;
    const int ncol = station ? JAICOV_PREC_STATION_COLUMNS : JAICOV_PREC_POINT_COLUMNS;
    HIPE(*v.err, hipSetDevice(v.device));
    PrecisionState *st = q_state(v.slot->prec);
    HIPE(*v.err, st->tab.reserve((size_t)(PREC_TAB + 1) * n));
    HIPE(*v.err, st->out.reserve((size_t)ncol * n));
    int32_t *d_tab = st->tab.get(), *d_status = d_tab + (size_t)PREC_TAB * n;
    HIPE(*v.err, hipMemcpyAsync(d_tab, tab.data(), (size_t)PREC_TAB * n * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(prec_block_kernel, dim3((n + 255) / 256), dim3(256), 0, v.stream, v.Q, v.ld, d_tab, n, sigma2, k3, k2, ncol,
                       st->out.get(), d_status);
    HIPE(*v.err, hipGetLastError());
    return q_download(v, {{out, st->out.get(), (size_t)ncol * n * sizeof(double)}, {status, d_status, (size_t)n * sizeof(int32_t)}});
}

}  // namespace jaicov

using namespace jaicov;

extern "C" int jaicov_prec_points(jaicov_engine *e, double sigma2, double k3, double k2, const int32_t *points, int32_t n, double *out,
                                  int32_t *status) {
    return prec_blocks(e, false, sigma2, k3, k2, points, n, out, status);
}

extern "C" int jaicov_prec_stations(jaicov_engine *e, double sigma2, double k3, double k2, const int32_t *images, int32_t n, double *out,
                                    int32_t *status) {
    return prec_blocks(e, true, sigma2, k3, k2, images, n, out, status);
}

extern "C" int jaicov_prec_lengths(jaicov_engine *e, double sigma2, const int32_t *pairs, int32_t n, double *out, int32_t *status) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    TRY(q_guard(v, PREC_SHARDED));
    const DevProblem &p = *v.p;
    if (!pairs || !out || !status || n < 0) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "length precision: NULL argument or a negative count");
    if (!(sigma2 >= 0.0)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "length precision: sigma2 must not be negative");
    std::vector<int32_t> tab((size_t)PREC_TAB * std::max(n, 1), -1);
    for (int i = 0; i < n; i++) {
        const int a = pairs[2 * i], b = pairs[2 * i + 1];
        if (a < 0 || a >= p.n_points || b < 0 || b >= p.n_points) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "length precision: point index out of range");
        if (a == b) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "length precision: a pair names the same point twice");
        for (int k = 0; k < 6; k++) {
            TRY(q_column(v, 3 * (k < 3 ? a : b) + k % 3, "length precision: a point's columns are not in the reduced cofactor matrix",
                         &tab[(size_t)PREC_TAB * i + k]));
        }
        tab[(size_t)PREC_TAB * i + 6] = 3 * a;
        tab[(size_t)PREC_TAB * i + 7] = 3 * b;
    }
    if (n == 0) return JAICOV_OK;
    HIPE(*v.err, hipSetDevice(v.device));
    PrecisionState *st = q_state(v.slot->prec);
    HIPE(*v.err, st->tab.reserve((size_t)(PREC_TAB + 1) * n));
    HIPE(*v.err, st->out.reserve((size_t)JAICOV_PREC_LENGTH_COLUMNS * n));
    int32_t *d_tab = st->tab.get(), *d_status = d_tab + (size_t)PREC_TAB * n;
    HIPE(*v.err, hipMemcpyAsync(d_tab, tab.data(), (size_t)PREC_TAB * n * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(prec_length_kernel, dim3((n + 255) / 256), dim3(256), 0, v.stream, v.Q, v.ld, v.d_vals, d_tab, n, sigma2, st->out.get(),
                       d_status);
    HIPE(*v.err, hipGetLastError());
    return q_download(v, {{out, st->out.get(), (size_t)JAICOV_PREC_LENGTH_COLUMNS * n * sizeof(double)},
                          {status, d_status, (size_t)n * sizeof(int32_t)}});
}

extern "C" int jaicov_prec_components(jaicov_engine *e, int32_t first_col, int32_t n_cols, int32_t k, double tol, int32_t max_iterations,
                                      double *values, double *vectors, double *trace, double *residuals, int32_t *iterations) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    TRY(q_guard(v, PREC_SHARDED));
    if (!values || !vectors || !trace || !residuals || !iterations) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "principal components: NULL output");
    if (k < 1 || k > 4) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "principal components: k must be 1 .. 4");
    if (n_cols < 8 || first_col < v.d || first_col > v.order || n_cols > v.order - first_col)
        FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "principal components: the range must hold 8 columns or more inside [d, order)");
    if (!(tol >= 0.0) || max_iterations < 1) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "principal components: tol must not be negative, max_iterations at least 1");
    if (tol == 0.0) tol = 1e-10;
    const int lo = first_col, hi = first_col + n_cols;
    const int nbk = (hi + 127) / 128, np = nbk * 128, nblk = (np + 255) / 256;
    const size_t n8 = (size_t)np * 8;
    HIPE(*v.err, hipSetDevice(v.device));
    PrecisionState *st = q_state(v.slot->prec);
    HIPE(*v.err, st->work.reserve(4 * n8 + 256 + (size_t)nblk * 64 + (size_t)nbk * nbk * 128 * 8));
    double *dXt = st->work.get(), *dXr = dXt + n8, *dY = dXr + n8, *dW = dY + n8, *dM = dW + n8, *dG = dM + 128, *dPart = dM + 256,
           *dP = dPart + (size_t)nblk * 64;
    hipStream_t s = v.stream;
    double M[72], G[64], th[8], Z[64], res[8];

    // G = A'B to the host
    auto gram = [&](const double *A, const double *B) -> hipError_t {
        hipLaunchKernelGGL(prec_gram_partial_kernel, dim3(nblk), dim3(256), 0, s, A, B, np, dPart);
        hipLaunchKernelGGL(prec_gram_final_kernel, dim3(1), dim3(64), 0, s, dPart, nblk, dG);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(G, dG, sizeof(G), hipMemcpyDeviceToHost, s));
        return hipStreamSynchronize(s);
    };
    // out = in M (M: 64 doubles of the host, or 72 with theta behind them for the residual kernel)
    auto upload = [&](int count) -> hipError_t { return hipMemcpyAsync(dM, M, count * sizeof(double), hipMemcpyHostToDevice, s); };
    auto apply = [&](const double *in, double *out_r, double *out_t) -> hipError_t {
        HIPCHK(upload(64));
        hipLaunchKernelGGL(prec_apply_kernel, dim3((np + 255) / 256), dim3(256), 0, s, in, dM, np, out_r, out_t);
        HIPCHK(hipGetLastError());
        return hipStreamSynchronize(s);      // M is free again
    };
    // X = orth(W0) by CholeskyQR2; 1: no Cholesky factor
    auto orth = [&](const double *W0, int *singular) -> hipError_t {
        *singular = 0;
        HIPCHK(gram(W0, W0));
        if (!prec_chol_inverse8(G, M)) { *singular = 1; return hipSuccess; }
        HIPCHK(apply(W0, dW, nullptr));
        HIPCHK(gram(dW, dW));
        if (!prec_chol_inverse8(G, M)) { *singular = 1; return hipSuccess; }
        return apply(dW, dXr, dXt);
    };

    // trace of the sub-block
    hipLaunchKernelGGL(prec_trace_kernel, dim3(1), dim3(256), 0, s, v.Q, v.ld, lo, hi, dG);
    HIPE(*v.err, hipGetLastError());
    double tr = 0.0;
    HIPE(*v.err, hipMemcpyAsync(&tr, dG, sizeof(double), hipMemcpyDeviceToHost, s));
    // start block
    std::vector<double> X0(n8, 0.0);
    for (int i = 0; i < n_cols; i++)
        for (int a = 0; a < 8; a++)
            X0[(size_t)(lo + i) * 8 + a] = (double)(prec_splitmix((uint64_t)8 * i + a) >> 11) * 0x1.0p-53 - 0.5;
    HIPE(*v.err, hipMemcpyAsync(dY, X0.data(), n8 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPE(*v.err, hipStreamSynchronize(s));
    int singular = 0;
    HIPE(*v.err, orth(dY, &singular));
    if (singular) FAIL(*v.err, JAICOV_ERR_SINGULAR, "principal components: the start block has no Cholesky factor");

    int it = 0;
    bool converged = false;
    for (;;) {
        HIPE(*v.err, launch_sym_y<8>(s, v.Q, v.ld, hi, lo, dXt, np, nbk, dP, dY));
        ++it;
        HIPE(*v.err, gram(dXr, dY));                          // H = X'Y
        prec_jacobi8(G, th, Z);
        for (int i = 0; i < 64; i++) M[i] = Z[i];
        for (int a = 0; a < 8; a++) M[64 + a] = th[a];
        HIPE(*v.err, upload(72));
        hipLaunchKernelGGL(prec_resid_kernel, dim3((np + 255) / 256), dim3(256), 0, s, dXr, dY, dM, np, dW);
        HIPE(*v.err, hipGetLastError());
        HIPE(*v.err, gram(dW, dW));
        for (int a = 0; a < 8; a++) res[a] = sqrt(std::max(G[9 * a], 0.0));
        converged = true;
        for (int a = 0; a < k; a++)
            if (!(res[a] <= tol * th[0])) converged = false;
        if (converged || it >= max_iterations) break;
        HIPE(*v.err, orth(dY, &singular));
        if (singular) FAIL(*v.err, JAICOV_ERR_SINGULAR, "principal components: the Gram matrix of S X has no Cholesky factor (rank of the sub-block < 8?)");
    }
    // the Ritz vectors X Z, column-wise into the operand buffer that the iteration needs no more
    for (int i = 0; i < 64; i++) M[i] = Z[i];
    HIPE(*v.err, apply(dXr, dW, dXt));
    HIPE(*v.err, hipMemcpy2DAsync(vectors, (size_t)n_cols * sizeof(double), dXt + lo, (size_t)np * sizeof(double), (size_t)n_cols * sizeof(double), k,
                                  hipMemcpyDeviceToHost, s));
    HIPE(*v.err, hipStreamSynchronize(s));
    for (int a = 0; a < k; a++) {
        double *x = vectors + (size_t)a * n_cols, nrm = 0.0, big = 0.0;
        for (int i = 0; i < n_cols; i++) {
            nrm += x[i] * x[i];
            if (fabs(x[i]) > fabs(big)) big = x[i];
        }
        const double f = (big < 0.0 ? -1.0 : 1.0) / sqrt(nrm);
        for (int i = 0; i < n_cols; i++) x[i] *= f;
        values[a] = th[a];
        residuals[a] = res[a];
    }
    *trace = tr;
    *iterations = converged ? it : -it;
    return JAICOV_OK;
}
