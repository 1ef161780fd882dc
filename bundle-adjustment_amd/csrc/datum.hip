// Baarda's S-transformation of the cofactor matrix on the device (include/jaicov_datum.h).
//
// The cofactor matrix Q (order n, border rows 0 .. d-1, lower part of a row-major square) is read twice and written once:
//   1. datum_y_tile_kernel + datum_y_reduce_kernel: Y = Q B'' over the lower triangle.  Each 128 x 128 tile serves its rows and,
//      transposed, its columns; the partial sums go to a [block row][slot] table and are added in slot order (as the refinement's
//      symv_dd_tile_kernel does in refine.hip), so two runs give the same bits.
//   2. the d x d algebra on the host: G^ (the unknowns x border block, n d doubles), C = (B' G^)^-1, Z = G^ C, W = B' Y,
//      Y~ = Y - Z W / 2.
//   3. datum_update_kernel: Q' = Q - Z Y~' - Y~ Z' on the unknowns block, Z in the border block, 0 in the border x border block,
//      one read and one write of the lower triangle.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/jaicov_datum.h"
#include "datum.h"
#include "status.h"

namespace jaicov {

void datum_state_invalidate(DatumState *s) {
    if (s) s->valid = false;
}

// One workgroup per lower tile (I, J), J <= I, in four slabs of 32 rows.  Row part: thread (rr, seg) holds row rr of the slab,
// columns 16 q + 2 seg + {0, 1}; the 8 lanes of a row are summed by butterfly.  Column part: thread (h, c) adds rows
// 16 h .. 16 h + 15 of every slab for column c from LDS.  Entries outside rows / columns [d, n) count as zero; on a diagonal tile
// the strict upper part is not Q and the diagonal is counted once (row part).
// P[((I nbk + slot) 128 + i) D + a] = contribution of block column `slot` to Y[128 I + i][a].
template <int D>
__global__ __launch_bounds__(256) void datum_y_tile_kernel(const double *__restrict__ Q, long ld, int n, int d,
                                                           const double *__restrict__ Bt, int np, int nbk, double *__restrict__ P) {
    __shared__ double slab[32 * 128];        // one slab of the tile; afterwards the column partial sums [2][128][D]
    __shared__ double bJ[D][128], bI[D][128];
    __shared__ double rowres[128][D];
    const int t = blockIdx.x;
    int I = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((long)(I + 1) * (I + 2) / 2 <= t) ++I;
    while ((long)I * (I + 1) / 2 > t) --I;
    const int J = t - I * (I + 1) / 2;
    const int tid = threadIdx.x;
    const bool diag = I == J;
    for (int k = tid; k < D * 128; k += 256) {
        const int a = k >> 7, c = k & 127;
        bJ[a][c] = Bt[(long)a * np + J * 128 + c];
        bI[a][c] = Bt[(long)a * np + I * 128 + c];
    }
    __syncthreads();
    const int rr = tid >> 3, seg = tid & 7;      // row role
    const int cc = tid & 127, h = tid >> 7;      // column role
    double cacc[D];
#pragma unroll
    for (int a = 0; a < D; a++) cacc[a] = 0.0;
#pragma unroll 1
    for (int s = 0; s < 4; s++) {
        const int r = 32 * s + rr, gr = I * 128 + r;
        const bool rowok = gr >= d && gr < n;
        const double *qrow = Q + (long)gr * ld;
        double v[16];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int c0 = 16 * q + 2 * seg, gc = J * 128 + c0;
            if (rowok && gc >= d && gc + 1 < n) {
                const double2 x = *reinterpret_cast<const double2 *>(qrow + gc);
                v[2 * q] = x.x; v[2 * q + 1] = x.y;
            } else {
                v[2 * q] = (rowok && gc >= d && gc < n) ? qrow[gc] : 0.0;
                v[2 * q + 1] = (rowok && gc + 1 >= d && gc + 1 < n) ? qrow[gc + 1] : 0.0;
            }
            if (diag && c0 > r) v[2 * q] = 0.0;
            if (diag && c0 + 1 > r) v[2 * q + 1] = 0.0;
        }
        double racc[D];
#pragma unroll
        for (int a = 0; a < D; a++) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int c0 = 16 * q + 2 * seg;
                acc = fma(v[2 * q], bJ[a][c0], acc);
                acc = fma(v[2 * q + 1], bJ[a][c0 + 1], acc);
            }
            racc[a] = acc;
        }
#pragma unroll
        for (int m = 1; m < 8; m <<= 1)
#pragma unroll
            for (int a = 0; a < D; a++) racc[a] += __shfl_xor(racc[a], m, 64);
        if (seg == 0)
#pragma unroll
            for (int a = 0; a < D; a++) rowres[r][a] = racc[a];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int c0 = 16 * q + 2 * seg;
            slab[rr * 128 + c0] = v[2 * q];
            slab[rr * 128 + c0 + 1] = v[2 * q + 1];
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < 16; k++) {
            const int rl = 16 * h + k, r2 = 32 * s + rl;
            const double x = (diag && cc == r2) ? 0.0 : slab[rl * 128 + cc];
#pragma unroll
            for (int a = 0; a < D; a++) cacc[a] = fma(x, bI[a][r2], cacc[a]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < D; a++) slab[(h * 128 + cc) * D + a] = cacc[a];
    __syncthreads();
    if (tid < 128) {
        const size_t sz = (size_t)128 * D;
#pragma unroll
        for (int a = 0; a < D; a++) {
            const double col = slab[tid * D + a] + slab[(128 + tid) * D + a];
            if (diag) {
                P[((size_t)I * nbk + I) * sz + (size_t)tid * D + a] = rowres[tid][a] + col;
            } else {
                P[((size_t)I * nbk + J) * sz + (size_t)tid * D + a] = rowres[tid][a];
                P[((size_t)J * nbk + I) * sz + (size_t)tid * D + a] = col;
            }
        }
    }
}

// Y[g][a] for the rows g of block row I: 4 groups of 128 threads add every fourth slot each (fixed order), the groups are
// combined in group order.  Rows outside [d, n) are 0.
template <int D>
__global__ __launch_bounds__(512) void datum_y_reduce_kernel(const double *__restrict__ P, int nbk, int n, int d, double *__restrict__ Y) {
    __shared__ double part[4][128][D];
    const int I = blockIdx.x, i = threadIdx.x & 127, grp = threadIdx.x >> 7, g = I * 128 + i;
    const size_t sz = (size_t)128 * D;
    double acc[D];
#pragma unroll
    for (int a = 0; a < D; a++) acc[a] = 0.0;
    for (int s = grp; s < nbk; s += 4) {
        const double *p = P + ((size_t)I * nbk + s) * sz + (size_t)i * D;
#pragma unroll
        for (int a = 0; a < D; a++) acc[a] += p[a];
    }
#pragma unroll
    for (int a = 0; a < D; a++) part[grp][i][a] = acc[a];
    __syncthreads();
    if (grp != 0) return;
    const bool ok = g >= d && g < n;
#pragma unroll
    for (int a = 0; a < D; a++) {
        double y = part[0][i][a];
        for (int q = 1; q < 4; q++) y += part[q][i][a];
        Y[(size_t)g * D + a] = ok ? y : 0.0;
    }
}

// Q'[i][j], j <= i < n: 0 (i < d), Z[i][j] (j < d <= i), Q[i][j] - sum_a (Z[i][a] Y~[j][a] + Y~[i][a] Z[j][a]) otherwise.
// ZY: [row][Z (D) | Y~ (D)].  One workgroup: 256 columns x 32 rows; the column operands stay in registers.
template <int D>
__global__ __launch_bounds__(256) void datum_update_kernel(double *__restrict__ Q, long ld, int n, int d, const double *__restrict__ ZY) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i0 = blockIdx.y * 32;
    if (blockIdx.x * 256 > i0 + 31) return;          // the whole workgroup lies above the diagonal
    double zj[D], yj[D];
#pragma unroll
    for (int a = 0; a < D; a++) {
        zj[a] = j < n ? ZY[(size_t)j * 2 * D + a] : 0.0;
        yj[a] = j < n ? ZY[(size_t)j * 2 * D + D + a] : 0.0;
    }
    for (int r = 0; r < 32; r++) {
        const int i = i0 + r;
        if (i >= n) break;
        if (j > i || j >= n) continue;
        const double *zyi = ZY + (size_t)i * 2 * D;
        double *q = Q + (long)i * ld + j;
        if (i < d) {
            *q = 0.0;
        } else if (j < d) {
            *q = zyi[j];
        } else {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < D; a++) {
                s = fma(zyi[a], yj[a], s);
                s = fma(zyi[D + a], zj[a], s);
            }
            *q = *q - s;
        }
    }
}

template <int D>
static hipError_t launch_y(hipStream_t st, const double *Q, long ld, int n, int d, const double *Bt, int np, int nbk, double *P, double *Y) {
    hipLaunchKernelGGL(datum_y_tile_kernel<D>, dim3(nbk * (nbk + 1) / 2), dim3(256), 0, st, Q, ld, n, d, Bt, np, nbk, P);
    hipLaunchKernelGGL(datum_y_reduce_kernel<D>, dim3(nbk), dim3(512), 0, st, P, nbk, n, d, Y);
    return hipGetLastError();
}

template <int D>
static hipError_t launch_update(hipStream_t st, double *Q, long ld, int n, int d, const double *ZY) {
    hipLaunchKernelGGL(datum_update_kernel<D>, dim3((n + 255) / 256, (n + 31) / 32), dim3(256), 0, st, Q, ld, n, d, ZY);
    return hipGetLastError();
}

static hipError_t launch_y_d(int D, hipStream_t st, const double *Q, long ld, int n, const double *Bt, int np, int nbk, double *P, double *Y) {
    switch (D) {
    case 1: return launch_y<1>(st, Q, ld, n, D, Bt, np, nbk, P, Y);
    case 2: return launch_y<2>(st, Q, ld, n, D, Bt, np, nbk, P, Y);
    case 3: return launch_y<3>(st, Q, ld, n, D, Bt, np, nbk, P, Y);
    case 4: return launch_y<4>(st, Q, ld, n, D, Bt, np, nbk, P, Y);
    case 5: return launch_y<5>(st, Q, ld, n, D, Bt, np, nbk, P, Y);
    case 6: return launch_y<6>(st, Q, ld, n, D, Bt, np, nbk, P, Y);
    default: return launch_y<7>(st, Q, ld, n, D, Bt, np, nbk, P, Y);
    }
}

static hipError_t launch_update_d(int D, hipStream_t st, double *Q, long ld, int n, const double *ZY) {
    switch (D) {
    case 1: return launch_update<1>(st, Q, ld, n, D, ZY);
    case 2: return launch_update<2>(st, Q, ld, n, D, ZY);
    case 3: return launch_update<3>(st, Q, ld, n, D, ZY);
    case 4: return launch_update<4>(st, Q, ld, n, D, ZY);
    case 5: return launch_update<5>(st, Q, ld, n, D, ZY);
    case 6: return launch_update<6>(st, Q, ld, n, D, ZY);
    default: return launch_update<7>(st, Q, ld, n, D, ZY);
    }
}

// inverse of a d x d matrix (d <= 7) by Gauss-Jordan with partial pivoting; false when a pivot falls to 1e-12 of the largest
// entry (the datum rows do not fix the frame: collinear or coincident datum points)
static bool datum_small_inverse(int d, const double *M, double *Minv) {
    double a[7][14], mx = 0.0;
    for (int i = 0; i < d; i++)
        for (int j = 0; j < d; j++) {
            a[i][j] = M[i * d + j];
            a[i][d + j] = i == j ? 1.0 : 0.0;
            mx = std::max(mx, fabs(M[i * d + j]));
        }
    if (!(mx > 0.0) || !std::isfinite(mx)) return false;
    for (int c = 0; c < d; c++) {
        int piv = c;
        for (int r = c + 1; r < d; r++)
            if (fabs(a[r][c]) > fabs(a[piv][c])) piv = r;
        if (!(fabs(a[piv][c]) > 1e-12 * mx)) return false;
        if (piv != c)
            for (int j = 0; j < 2 * d; j++) std::swap(a[c][j], a[piv][j]);
        const double inv = 1.0 / a[c][c];
        for (int j = 0; j < 2 * d; j++) a[c][j] *= inv;
        for (int r = 0; r < d; r++) {
            if (r == c) continue;
            const double f = a[r][c];
            if (f != 0.0)
                for (int j = 0; j < 2 * d; j++) a[r][j] -= f * a[c][j];
        }
    }
    for (int i = 0; i < d; i++)
        for (int j = 0; j < d; j++) Minv[i * d + j] = a[i][d + j];
    return true;
}

}  // namespace jaicov

using namespace jaicov;

extern "C" int jaicov_datum_transform(jaicov_engine *e, const uint8_t *point_datum, int32_t n_points) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    DatumView v;
    engine_datum_view(e, &v);
    if (v.d == 0) FAIL(*v.err, JAICOV_ERR_UNSUPPORTED, "datum transformation: the network has no datum defect (d = 0)");
    if (v.sharded) FAIL(*v.err, JAICOV_ERR_UNSUPPORTED, "datum transformation on a sharded engine");
    if (!v.have_q) FAIL(*v.err, JAICOV_ERR_BAD_STATE, "no cofactor matrix: solve with invert != 0 first");
    if (!point_datum || n_points != v.n_points) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "point_datum must hold one flag per object point");
    const int n = v.order, d = v.d, nbk = (n + 127) / 128, np = nbk * 128;
    std::vector<double> B;
    int rc = engine_datum_rows(e, point_datum, B, np);
    if (rc) return rc;
    HIPE(*v.err, hipSetDevice(v.device));
    // G^: the unknowns x border block (rows d .. n-1, columns 0 .. d-1)
    std::vector<double> G((size_t)n * d, 0.0);
    HIPE(*v.err, hipMemcpy2DAsync(G.data() + (size_t)d * d, d * sizeof(double), v.Q + (long)d * v.ld, v.ld * sizeof(double),
                             d * sizeof(double), n - d, hipMemcpyDeviceToHost, v.stream));
    HIPE(*v.err, hipStreamSynchronize(v.stream));
    // C = (B' G^)^-1, Z = G^ C
    double M[49], Cm[49];
    for (int a = 0; a < d; a++)
        for (int b = 0; b < d; b++) {
            double s = 0.0;
            for (int i = d; i < n; i++) s += B[(size_t)a * np + i] * G[(size_t)i * d + b];
            M[a * d + b] = s;
        }
    if (!datum_small_inverse(d, M, Cm)) FAIL(*v.err, JAICOV_ERR_SINGULAR, "the new datum points do not fix the frame (B' G^ is singular)");
    std::vector<double> Z((size_t)n * d, 0.0);
    for (int i = d; i < n; i++)
        for (int a = 0; a < d; a++) {
            double s = 0.0;
            for (int b = 0; b < d; b++) s += G[(size_t)i * d + b] * Cm[b * d + a];
            Z[(size_t)i * d + a] = s;
        }
    // work buffers, kept with the engine
    if (!*v.state) v.state->reset(new DatumState());
    DatumState *st = v.state->get();
    HIPE(*v.err, st->work.reserve((size_t)d * np * 4 + (size_t)nbk * nbk * 128 * d));
    double *dB = st->work.get(), *dY = dB + (size_t)d * np, *dZY = dY + (size_t)d * np, *dP = dZY + (size_t)2 * d * np;
    HIPE(*v.err, hipMemcpyAsync(dB, B.data(), (size_t)d * np * sizeof(double), hipMemcpyHostToDevice, v.stream));
    HIPE(*v.err, launch_y_d(d, v.stream, v.Q, v.ld, n, dB, np, nbk, dP, dY));
    std::vector<double> Y((size_t)np * d);
    HIPE(*v.err, hipMemcpyAsync(Y.data(), dY, Y.size() * sizeof(double), hipMemcpyDeviceToHost, v.stream));
    HIPE(*v.err, hipStreamSynchronize(v.stream));
    // W = B' Y (symmetric: its two triangles averaged), Y~ = Y - Z W / 2
    double W[49];
    for (int a = 0; a < d; a++)
        for (int b = 0; b < d; b++) {
            double s = 0.0;
            for (int i = d; i < n; i++) s += B[(size_t)a * np + i] * Y[(size_t)i * d + b];
            W[a * d + b] = s;
        }
    for (int a = 0; a < d; a++)
        for (int b = 0; b < a; b++) W[a * d + b] = W[b * d + a] = 0.5 * (W[a * d + b] + W[b * d + a]);
    std::vector<double> ZY((size_t)np * 2 * d, 0.0);
    for (int i = d; i < n; i++)
        for (int a = 0; a < d; a++) {
            double s = 0.0;
            for (int b = 0; b < d; b++) s += Z[(size_t)i * d + b] * W[b * d + a];
            ZY[(size_t)i * 2 * d + a] = Z[(size_t)i * d + a];
            ZY[(size_t)i * 2 * d + d + a] = Y[(size_t)i * d + a] - 0.5 * s;
        }
    HIPE(*v.err, hipMemcpyAsync(dZY, ZY.data(), ZY.size() * sizeof(double), hipMemcpyHostToDevice, v.stream));
    st->valid = false;      // from here on Q changes: the S of an earlier transform no longer applies to it
    HIPE(*v.err, launch_update_d(d, v.stream, v.Q, v.ld, n, dZY));
    HIPE(*v.err, hipStreamSynchronize(v.stream));
    // S = I - Z B' for jaicov_datum_apply
    st->order = n;
    st->d = d;
    st->Z.swap(Z);
    st->B.assign((size_t)d * n, 0.0);
    for (int a = 0; a < d; a++) std::copy(B.begin() + (size_t)a * np, B.begin() + (size_t)a * np + n, st->B.begin() + (size_t)a * n);
    st->valid = true;
    return JAICOV_OK;
}

extern "C" int jaicov_datum_apply(jaicov_engine *e, const double *x, double *out, int32_t n) {
    if (!e || !x || !out) return JAICOV_ERR_BAD_ARGUMENT;
    DatumView v;
    engine_datum_view(e, &v);
    const DatumState *st = v.state->get();
    if (!st || !st->valid) FAIL(*v.err, JAICOV_ERR_BAD_STATE, "no datum transformation since the last inverting solve");
    if (n != st->order) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "n must be the order of the transformed cofactor matrix");
    const int d = st->d;
    double t[7];
    for (int a = 0; a < d; a++) {
        double s = 0.0;
        for (int i = d; i < n; i++) s += st->B[(size_t)a * n + i] * x[i];
        t[a] = s;
    }
    for (int i = 0; i < d; i++) out[i] = 0.0;
    for (int i = d; i < n; i++) {
        double s = 0.0;
        for (int a = 0; a < d; a++) s += st->Z[(size_t)i * d + a] * t[a];
        out[i] = x[i] - s;
    }
    return JAICOV_OK;
}
