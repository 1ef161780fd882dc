// Y = Q_[lo, hi) X over the lower triangle of the cofactor matrix: the product that the datum transformation (datum.hip, D = d <= 7
// columns, bounds [d, n)) and the principal components (precision.hip, D = 8, the bounds of the sub-block) share.
//
// Q: order n, lower part of a row-major square with leading dimension ld.  Entries outside rows / columns [lo, hi) count as zero.
// sym_y_tile_kernel reads every 128 x 128 tile of the lower triangle once; a tile serves its rows and, transposed, its columns.  The
// partial sums go to a [block row][slot] table and sym_y_reduce_kernel adds them in slot order (as the refinement's
// symv_dd_tile_kernel does in refine.hip), so two runs give the same bits.  The bits of jaicov_datum_transform depend on the order
// of operations here: a change of it changes every transformed cofactor matrix.
// LDS of the tile kernel: 32 KB slab + 2 D KB operands + D KB row results (D = 8: 56 KB).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace jaicov {

// One workgroup per lower tile (I, J), J <= I, in four slabs of 32 rows.  Row part: thread (rr, seg) holds row rr of the slab,
// columns 16 q + 2 seg + {0, 1}; the 8 lanes of a row are summed by butterfly.  Column part: thread (h, c) adds rows
// 16 h .. 16 h + 15 of every slab for column c from LDS.  On a diagonal tile the strict upper part is not Q and the diagonal is
// counted once (row part).  A tile without a row or a column in [lo, hi) reads nothing and leaves zeros.
// Xt: [D][np] (column a of X at Xt + a np, zero outside [lo, hi)).
// P[((I nbk + slot) 128 + i) D + a] = contribution of block column `slot` to Y[128 I + i][a].
template <int D>
__global__ __launch_bounds__(256) void sym_y_tile_kernel(const double *__restrict__ Q, long ld, int hi, int lo,
                                                         const double *__restrict__ Xt, int np, int nbk, double *__restrict__ P) {
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
    if (I * 128 >= hi || I * 128 + 128 <= lo || J * 128 >= hi || J * 128 + 128 <= lo) {
        if (tid < 128) {
            const size_t sz = (size_t)128 * D;
#pragma unroll
            for (int a = 0; a < D; a++) {
                P[((size_t)I * nbk + J) * sz + (size_t)tid * D + a] = 0.0;
                if (!diag) P[((size_t)J * nbk + I) * sz + (size_t)tid * D + a] = 0.0;
            }
        }
        return;
    }
    for (int k = tid; k < D * 128; k += 256) {
        const int a = k >> 7, c = k & 127;
        bJ[a][c] = Xt[(long)a * np + J * 128 + c];
        bI[a][c] = Xt[(long)a * np + I * 128 + c];
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
        const bool rowok = gr >= lo && gr < hi;
        const double *qrow = Q + (long)gr * ld;
        double v[16];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int c0 = 16 * q + 2 * seg, gc = J * 128 + c0;
            if (rowok && gc >= lo && gc + 1 < hi) {
                const double2 x = *reinterpret_cast<const double2 *>(qrow + gc);
                v[2 * q] = x.x; v[2 * q + 1] = x.y;
            } else {
                v[2 * q] = (rowok && gc >= lo && gc < hi) ? qrow[gc] : 0.0;
                v[2 * q + 1] = (rowok && gc + 1 >= lo && gc + 1 < hi) ? qrow[gc + 1] : 0.0;
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
// combined in group order.  Rows outside [lo, hi) are 0.
template <int D>
__global__ __launch_bounds__(512) void sym_y_reduce_kernel(const double *__restrict__ P, int nbk, int hi, int lo, double *__restrict__ Y) {
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
    const bool ok = g >= lo && g < hi;
#pragma unroll
    for (int a = 0; a < D; a++) {
        double y = part[0][i][a];
        for (int q = 1; q < 4; q++) y += part[q][i][a];
        Y[(size_t)g * D + a] = ok ? y : 0.0;
    }
}

// Y [np][D] = Q_[lo, hi) X for Xt [D][np]; P: the table [nbk][nbk][128][D], nbk = np / 128 = ceil(n / 128)
template <int D>
inline hipError_t launch_sym_y(hipStream_t st, const double *Q, long ld, int hi, int lo, const double *Xt, int np, int nbk, double *P, double *Y) {
    hipLaunchKernelGGL(sym_y_tile_kernel<D>, dim3(nbk * (nbk + 1) / 2), dim3(256), 0, st, Q, ld, hi, lo, Xt, np, nbk, P);
    hipLaunchKernelGGL(sym_y_reduce_kernel<D>, dim3(nbk), dim3(512), 0, st, P, nbk, hi, lo, Y);
    return hipGetLastError();
}

}  // namespace jaicov
