// Correlations and significance tests of the unknowns, read from the cofactor matrix on the device (include/jaicov_parameters.h).
//
//   par_scale_kernel      s_j = 1 / sqrt(q_jj) and the status of the diagonal; s_j = 0 marks a column that takes no part (border,
//                         padding, q_jj not positive or not finite).
//   par_max_tile_kernel   maxima: one workgroup per 128 x 128 tile of the lower triangle, in the traversal of symtile.h (four slabs of
//                         32 rows, 16-byte loads along the rows).  Scales, classes and items of the tile's 128 rows and 128 columns
//                         are staged once in LDS.  A tile leaves one candidate (largest |rho|, lowest partner) for each of its rows
//                         and, transposed through the LDS slab, for each of its columns, in the table [block row][slot][128].
//   par_max_reduce_kernel reduces the table in ascending slot order with a strict `>`: the lowest partner wins, two runs give the
//                         same bits.
//   par_pairs_kernel      pairs: the same traversal twice -- pass one counts per tile, par_prefix_kernel turns the counts into
//                         offsets in tile order, pass two appends (in any order inside a tile: the host sorts).
//   par_block_kernel      a rectangular block of coefficients, beside engine.hip's gather_sub_kernel.
//   par_tests_kernel      one wave and one workgroup per group: gathers Q_gg into LDS and solves with wave_solve_lds (wavealg.h).
// Nothing here writes to the cofactor matrix or to any other state of the engine but the work buffers of ParamState.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/jaicov_parameters.h"
#include "parameters.h"
#include "qview.h"
#include "status.h"
#include "symtile.h"
#include "wavealg.h"

#pragma clang fp contract(off)

namespace jaicov {

constexpr int PAR_NONE = 0x7fffffff;

__global__ __launch_bounds__(256) void par_scale_kernel(const double *__restrict__ Q, long ld, int lo, int hi, int np, double *__restrict__ s,
                                                        int32_t *__restrict__ st) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= np) return;
    double sj = 0.0;
    int bits = 0;
    if (j >= lo && j < hi) {
        const double q = Q[(long)j * ld + j];
        if (!isfinite(q)) bits = JAICOV_PAR_NOT_FINITE;
        else if (!(q > 0.0)) bits = JAICOV_PAR_NONPOSITIVE;
        else sj = 1.0 / sqrt(q);
    }
    s[j] = sj;
    st[j] = bits;
}

// tile t of the lower triangle in row-major order: (I, J), J <= I
__device__ __forceinline__ void par_tile(int t, int &I, int &J) {
    I = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((long)(I + 1) * (I + 2) / 2 <= t) ++I;
    while ((long)I * (I + 1) / 2 > t) --I;
    J = t - I * (I + 1) / 2;
}

// the 16 entries of thread (rr, seg) in row gr of a slab: columns J 128 + 16 q + 2 seg + {0, 1}; entries outside [lo, hi) are 0
__device__ __forceinline__ void par_load_row(const double *__restrict__ Q, long ld, int gr, int J, int seg, int lo, int hi, double (&v)[16]) {
    const bool rowok = gr >= lo && gr < hi;
    const double *qrow = Q + (long)gr * ld;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int gc = J * 128 + 16 * q + 2 * seg;
        if (rowok && gc >= lo && gc + 1 < hi) {
            const double2 x = *reinterpret_cast<const double2 *>(qrow + gc);
            v[2 * q] = x.x; v[2 * q + 1] = x.y;
        } else {
            v[2 * q] = (rowok && gc >= lo && gc < hi) ? qrow[gc] : 0.0;
            v[2 * q + 1] = (rowok && gc + 1 >= lo && gc + 1 < hi) ? qrow[gc + 1] : 0.0;
        }
    }
}

// the tile's tables: scale, class and item of its rows (I) and columns (J)
struct ParTileTab {
    double sI[128], sJ[128];
    int cI[128], cJ[128], tI[128], tJ[128];
};

__device__ __forceinline__ void par_stage(ParTileTab &T, int I, int J, const double *__restrict__ s, const int32_t *__restrict__ cls,
                                          const int32_t *__restrict__ item) {
    const int tid = threadIdx.x;
    if (tid < 128) {
        T.sI[tid] = s[I * 128 + tid]; T.cI[tid] = cls[I * 128 + tid]; T.tI[tid] = item[I * 128 + tid];
    } else {
        const int c = tid - 128;
        T.sJ[c] = s[J * 128 + c]; T.cJ[c] = cls[J * 128 + c]; T.tJ[c] = item[J * 128 + c];
    }
}

// P[(I nbk + slot) 128 + i]: what block column `slot` offers row 128 I + i
__global__ __launch_bounds__(256) void par_max_tile_kernel(const double *__restrict__ Q, long ld, int hi, int lo, const double *__restrict__ s,
                                                           const int32_t *__restrict__ cls, const int32_t *__restrict__ item, unsigned mask,
                                                           int nbk, ParCand *__restrict__ P) {
    __shared__ double slab[32 * 128];        // rho of one slab; NaN: no pair
    __shared__ ParTileTab T;
    __shared__ double rkey[128], ckey[2][128];
    __shared__ int ridx[128], cidx[2][128], rst[128], cst[128];
    int I, J;
    par_tile(blockIdx.x, I, J);
    const int tid = threadIdx.x;
    const bool diag = I == J;
    if (I * 128 >= hi || I * 128 + 128 <= lo || J * 128 >= hi || J * 128 + 128 <= lo) {
        if (tid < 128) {
            const ParCand none = {-1.0, PAR_NONE, 0};
            P[((size_t)I * nbk + J) * 128 + tid] = none;
            if (!diag) P[((size_t)J * nbk + I) * 128 + tid] = none;
        }
        return;
    }
    par_stage(T, I, J, s, cls, item);
    if (tid < 128) { rst[tid] = 0; cst[tid] = 0; }
    __syncthreads();
    const int rr = tid >> 3, seg = tid & 7;      // row role
    const int cc = tid & 127, h = tid >> 7;      // column role
    double ck = -1.0;
    int ci = PAR_NONE;
#pragma unroll 1
    for (int sl = 0; sl < 4; sl++) {
        const int r = 32 * sl + rr, gr = I * 128 + r;
        const bool rowok = gr >= lo && gr < hi;
        double v[16];
        par_load_row(Q, ld, gr, J, seg, lo, hi, v);
        const double sr = T.sI[r];
        const int clr = T.cI[r], itr = T.tI[r];
        double key = -1.0;
        int idx = PAR_NONE;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int c = 16 * (k >> 1) + 2 * seg + (k & 1), gc = J * 128 + c;
            double rho = NAN;
            if (rowok && gc >= lo && gc < hi && (!diag || c < r)) {
                if (!isfinite(v[k])) {
                    atomicOr(&rst[r], JAICOV_PAR_NOT_FINITE);
                    atomicOr(&cst[c], JAICOV_PAR_NOT_FINITE);
                } else if (sr > 0.0 && T.sJ[c] > 0.0 && itr != T.tJ[c]) {
                    rho = (v[k] * sr) * T.sJ[c];
                }
            }
            slab[rr * 128 + c] = rho;
            if (!isnan(rho) && ((mask >> (4 * clr + T.cJ[c])) & 1u) && fabs(rho) > key) {
                key = fabs(rho);
                idx = 2 * gc + (signbit(rho) ? 1 : 0);
            }
        }
#pragma unroll
        for (int m = 1; m < 8; m <<= 1) wave_argmax_combine(key, idx, m);
        if (seg == 0) { rkey[r] = key; ridx[r] = idx; }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < 16; k++) {
            const int rl = 16 * h + k, r2 = 32 * sl + rl;
            const double rho = slab[rl * 128 + cc];
            if (!isnan(rho) && ((mask >> (4 * T.cJ[cc] + T.cI[r2])) & 1u) && fabs(rho) > ck) {
                ck = fabs(rho);
                ci = 2 * (I * 128 + r2) + (signbit(rho) ? 1 : 0);
            }
        }
        __syncthreads();
    }
    ckey[h][cc] = ck;
    cidx[h][cc] = ci;
    __syncthreads();
    if (tid < 128) {
        ParCand row = {rkey[tid], ridx[tid], rst[tid]};
        ParCand col = {ckey[0][tid], cidx[0][tid], cst[tid]};
        if (ckey[1][tid] > col.key || (ckey[1][tid] == col.key && cidx[1][tid] < col.idx2)) { col.key = ckey[1][tid]; col.idx2 = cidx[1][tid]; }
        if (diag) {                               // the partners of the column part lie behind those of the row part
            if (col.key > row.key) { row.key = col.key; row.idx2 = col.idx2; }
            row.status |= col.status;
            P[((size_t)I * nbk + I) * 128 + tid] = row;
        } else {
            P[((size_t)I * nbk + J) * 128 + tid] = row;
            P[((size_t)J * nbk + I) * 128 + tid] = col;
        }
    }
}

// the candidates of row g = 128 I + i in ascending slot order; st0: the status of the diagonal
__global__ __launch_bounds__(128) void par_max_reduce_kernel(const ParCand *__restrict__ P, int nbk, int hi, int lo, const double *__restrict__ s,
                                                             const int32_t *__restrict__ st0, double *__restrict__ rho,
                                                             int32_t *__restrict__ partner, int32_t *__restrict__ status) {
    const int I = blockIdx.x, i = threadIdx.x, g = I * 128 + i;
    double key = -1.0;
    int idx = PAR_NONE, st = 0;
    for (int sl = 0; sl < nbk; sl++) {
        const ParCand c = P[((size_t)I * nbk + sl) * 128 + i];
        st |= c.status;
        if (c.key > key) { key = c.key; idx = c.idx2; }
    }
    if (g >= hi) return;
    const bool found = s[g] > 0.0 && idx != PAR_NONE;
    rho[g] = found ? ((idx & 1) ? -key : key) : NAN;
    partner[g] = found ? (idx >> 1) : -1;
    status[g] = g >= lo ? (st0[g] | st) : 0;
}

// APPEND == false: cnt[t] = the number of pairs of tile t.  APPEND == true: the pairs of tile t go to cols / rho from off[t] on.
template <bool APPEND>
__global__ __launch_bounds__(256) void par_pairs_kernel(const double *__restrict__ Q, long ld, int hi, int lo, const double *__restrict__ s,
                                                        const int32_t *__restrict__ cls, const int32_t *__restrict__ item, unsigned mask,
                                                        double thr, int64_t *__restrict__ cnt, const int64_t *__restrict__ off, int64_t total,
                                                        int32_t *__restrict__ cols, double *__restrict__ rho_out) {
    __shared__ ParTileTab T;
    __shared__ int n;
    int I, J;
    par_tile(blockIdx.x, I, J);
    const int tid = threadIdx.x;
    const bool diag = I == J;
    if (I * 128 >= hi || I * 128 + 128 <= lo || J * 128 >= hi || J * 128 + 128 <= lo) {
        if (!APPEND && tid == 0) cnt[blockIdx.x] = 0;
        return;
    }
    par_stage(T, I, J, s, cls, item);
    if (tid == 0) n = 0;
    __syncthreads();
    const int rr = tid >> 3, seg = tid & 7;
    const int64_t base = APPEND ? off[blockIdx.x] : 0;
    int mine = 0;
#pragma unroll 1
    for (int sl = 0; sl < 4; sl++) {
        const int r = 32 * sl + rr, gr = I * 128 + r;
        const bool rowok = gr >= lo && gr < hi;
        double v[16];
        par_load_row(Q, ld, gr, J, seg, lo, hi, v);
        const double sr = T.sI[r];
        const int clr = T.cI[r], itr = T.tI[r];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int c = 16 * (k >> 1) + 2 * seg + (k & 1), gc = J * 128 + c;
            if (!(rowok && gc >= lo && gc < hi && (!diag || c < r))) continue;
            if (!isfinite(v[k]) || !(sr > 0.0) || !(T.sJ[c] > 0.0) || itr == T.tJ[c]) continue;
            const int clc = T.cJ[c];
            if (!(((mask >> (4 * clr + clc)) | (mask >> (4 * clc + clr))) & 1u)) continue;
            const double rho = (v[k] * sr) * T.sJ[c];
            if (!(fabs(rho) >= thr)) continue;
            if (APPEND) {
                const int64_t pos = base + atomicAdd(&n, 1);
                if (pos < total) { cols[2 * pos] = gr; cols[2 * pos + 1] = gc; rho_out[pos] = rho; }
            } else {
                ++mine;
            }
        }
    }
    if (!APPEND) {
        if (mine) atomicAdd(&n, mine);
        __syncthreads();
        if (tid == 0) cnt[blockIdx.x] = n;
    }
}

// off[t] = cnt[0] + ... + cnt[t - 1], off[nt] = the total: thread k adds its chunk of tiles, thread 0 the 256 chunk sums in order
__global__ __launch_bounds__(256) void par_prefix_kernel(const int64_t *__restrict__ cnt, int nt, int64_t *__restrict__ off) {
    __shared__ int64_t part[256];
    const int tid = threadIdx.x, chunk = (nt + 255) / 256, b = tid * chunk, e = min(nt, b + chunk);
    int64_t acc = 0;
    for (int t = b; t < e; t++) acc += cnt[t];
    part[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int k = 0; k < 256; k++) { const int64_t x = part[k]; part[k] = run; run += x; }
        off[nt] = run;
    }
    __syncthreads();
    acc = part[tid];
    for (int t = b; t < e; t++) { off[t] = acc; acc += cnt[t]; }
}

// out[a n_c + b] = rho of (rows[a], cols[b])
__global__ __launch_bounds__(256) void par_block_kernel(const double *__restrict__ Q, long ld, const int32_t *__restrict__ rows, int n_r,
                                                        const int32_t *__restrict__ cols, int n_c, double *__restrict__ out) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)n_r * n_c) return;
    const int ca = rows[e / n_c], cb = cols[e % n_c];
    const int i = max(ca, cb), j = min(ca, cb);
    const double qi = Q[(long)i * ld + i], qj = Q[(long)j * ld + j];
    double rho = NAN;
    if (isfinite(qi) && qi > 0.0 && isfinite(qj) && qj > 0.0) rho = i == j ? 1.0 : (Q[(long)i * ld + j] * (1.0 / sqrt(qi))) * (1.0 / sqrt(qj));
    out[e] = rho;
}

// Group g: members gb[g] .. gb[g + 1] of mcol / mslot / mx0 (free members only); gst: the status bits the host found.
// One wave per workgroup: the precondition of wave_solve_lds.
__global__ __launch_bounds__(64) void par_tests_kernel(const double *__restrict__ Q, long ld, const double *__restrict__ vals,
                                                       const int32_t *__restrict__ gb, const int32_t *__restrict__ mcol,
                                                       const int32_t *__restrict__ mslot, const double *__restrict__ mx0,
                                                       const int32_t *__restrict__ gst, double sigma2, double *__restrict__ out,
                                                       int32_t *__restrict__ status) {
    constexpr int K = JAICOV_PAR_MAX_GROUP;
    __shared__ double U[K * (K + 1) / 2], b[K], V[K], W[K], dl[K];
    const int g = blockIdx.x, lane = threadIdx.x;
    const int m0 = wave_uniform(gb[g]), k = wave_uniform(gb[g + 1]) - m0;
    int st = wave_uniform(gst[g]);
    double q = NAN, T = NAN, t = NAN;
    if (k == 0) {
        st |= JAICOV_PAR_EMPTY;
    } else if (k > K) {
        st |= JAICOV_PAR_TOO_LARGE;
    } else {
        auto ix = [k](int i, int j) { return i * k - i * (i - 1) / 2 + (j - i); };
        for (int i = 0; i < k; i++) {                 // row i of the upper triangle: lane j - i holds column j
            const int ci = mcol[m0 + i], j = i + lane;
            if (j < k) {
                const int cj = mcol[m0 + j];
                U[ix(i, j)] = q_sym(Q, ld, ci, cj);
            }
        }
        if (lane < k) b[lane] = dl[lane] = vals[mslot[m0 + lane]] - mx0[m0 + lane];
        __syncthreads();
        const double q00 = U[0];
        // The cofactors of distortion coefficients lie far below the 2^-53 under which wave_solve_lds leaves a row unscaled (and then
        // finds its pivot too small): powers of two bring the diagonal into [1, 4) first, whatever its magnitude, without rounding.
        if (lane < k) {
            const double qd = U[ix(lane, lane)];
            W[lane] = (qd > 0.0 && isfinite(qd)) ? ldexp(1.0, -(ilogb(qd) >> 1)) : 1.0;
        }
        __syncthreads();
        for (int i = 0; i < k; i++) {
            const int j = i + lane;
            if (j < k) U[ix(i, j)] = U[ix(i, j)] * (W[i] * W[j]);
        }
        if (lane < k) b[lane] = W[lane] * b[lane];
        __syncthreads();
        const WaveStatus ws = wave_solve_lds(k, U, b, V);
        if (ws == WAVE_NOT_FINITE) {
            st |= JAICOV_PAR_NOT_FINITE;
        } else if (ws == WAVE_SINGULAR) {
            st |= JAICOV_PAR_SINGULAR;
        } else {
            q = 0.0;
            for (int i = 0; i < k; i++) q += dl[i] * (W[i] * b[i]);
            T = q / ((double)k * sigma2);
            if (k == 1) t = dl[0] / sqrt(sigma2 * q00);
            if (!isfinite(q) || !isfinite(T) || (k == 1 && !isfinite(t))) { st |= JAICOV_PAR_NOT_FINITE; q = T = t = NAN; }
        }
    }
    if (lane == 0) {
        double *o = out + (size_t)JAICOV_PAR_TEST_COLUMNS * g;
        o[0] = q; o[1] = T; o[2] = (double)k; o[3] = t;
        status[g] = st;
    }
}

static const char PAR_SHARDED[] = "parameter correlations and tests on a sharded engine";

static bool par_selection_ok(uint32_t mask, uint32_t flags) {
    return !(mask >> 16) && !(flags & ~(uint32_t)(JAICOV_PAR_SKIP_SAME_POINT | JAICOV_PAR_SKIP_SAME_IMAGE));
}

// class and item of every column from the slot layout [3 P | 3 C | n_dist | 6 I], uploaded with the scales computed behind them.
// Two columns are no pair when their items are equal: the coordinates of a point share the point's number under SKIP_SAME_POINT, the
// elements of an image P + its number under SKIP_SAME_IMAGE; every other column has an item of its own (-1 - column).
static int par_prepare(const QView &v, ParamState *st, uint32_t flags, int np) {
    const DevProblem &p = *v.p;
    std::vector<int32_t> tab((size_t)2 * np);
    for (int c = 0; c < np; c++) { tab[c] = JAICOV_PAR_CLASS_POINT; tab[(size_t)np + c] = -1 - c; }
    const int io0 = 3 * p.n_points, di0 = io0 + 3 * p.n_cameras, eo0 = di0 + p.n_dist, n_slots = (int)v.slot_col->size();
    for (int sl = 0; sl < n_slots; sl++) {
        const int c = (*v.slot_col)[sl];
        if (c < 0 || c >= v.order) continue;
        if (sl < io0) {
            if (flags & JAICOV_PAR_SKIP_SAME_POINT) tab[(size_t)np + c] = sl / 3;
        } else if (sl < di0) {
            tab[c] = JAICOV_PAR_CLASS_INTERIOR;
        } else if (sl < eo0) {
            tab[c] = JAICOV_PAR_CLASS_DISTORTION;
        } else {
            tab[c] = JAICOV_PAR_CLASS_EXTERIOR;
            if (flags & JAICOV_PAR_SKIP_SAME_IMAGE) tab[(size_t)np + c] = p.n_points + (sl - eo0) / 6;
        }
    }
    HIPE(*v.err, st->scale.reserve((size_t)np));
    HIPE(*v.err, st->tab.reserve((size_t)3 * np));
    HIPE(*v.err, hipMemcpyAsync(st->tab.get(), tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(par_scale_kernel, dim3((np + 255) / 256), dim3(256), 0, v.stream, v.Q, v.ld, v.d, v.order, np, st->scale.get(),
                       st->tab.get() + (size_t)2 * np);
    HIPE(*v.err, hipGetLastError());
    HIPE(*v.err, hipStreamSynchronize(v.stream));      // the host table goes out of scope
    return JAICOV_OK;
}

}  // namespace jaicov

using namespace jaicov;

extern "C" int jaicov_par_maxima(jaicov_engine *e, uint32_t pair_mask, uint32_t flags, double *rho, int32_t *partner, int32_t *status, int32_t n) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    TRY(q_guard(v, PAR_SHARDED));
    if (!rho || !partner || !status || n != v.order) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "correlation maxima: NULL output, or n is not the order of the cofactor matrix");
    if (!par_selection_ok(pair_mask, flags)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "correlation maxima: unknown bits in pair_mask or flags");
    if (n == 0) return JAICOV_OK;
    const int nbk = (v.order + 127) / 128, np = nbk * 128;
    HIPE(*v.err, hipSetDevice(v.device));
    ParamState *st = q_state(v.slot->par);
    HIPE(*v.err, st->cand.reserve((size_t)nbk * nbk * 128));
    HIPE(*v.err, st->out_d.reserve((size_t)np));
    HIPE(*v.err, st->out_i.reserve((size_t)2 * np));
    TRY(par_prepare(v, st, flags, np));
    const int32_t *cls = st->tab.get(), *item = cls + np, *st0 = item + np;
    int32_t *d_partner = st->out_i.get(), *d_status = d_partner + np;
    hipLaunchKernelGGL(par_max_tile_kernel, dim3(nbk * (nbk + 1) / 2), dim3(256), 0, v.stream, v.Q, v.ld, v.order, v.d, st->scale.get(), cls, item,
                       pair_mask, nbk, st->cand.get());
    hipLaunchKernelGGL(par_max_reduce_kernel, dim3(nbk), dim3(128), 0, v.stream, st->cand.get(), nbk, v.order, v.d, st->scale.get(), st0,
                       st->out_d.get(), d_partner, d_status);
    HIPE(*v.err, hipGetLastError());
    return q_download(v, {{rho, st->out_d.get(), (size_t)n * sizeof(double)}, {partner, d_partner, (size_t)n * sizeof(int32_t)},
                          {status, d_status, (size_t)n * sizeof(int32_t)}});
}

extern "C" int jaicov_par_pairs(jaicov_engine *e, uint32_t pair_mask, uint32_t flags, double threshold, int64_t capacity, int32_t *cols, double *rho,
                                int64_t *count) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    TRY(q_guard(v, PAR_SHARDED));
    if (!count || capacity < 0 || (capacity > 0 && (!cols || !rho))) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "correlated pairs: NULL output or a negative capacity");
    if (!(threshold > 0.0 && threshold <= 1.0)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "correlated pairs: the threshold must lie in (0, 1]");
    if (!par_selection_ok(pair_mask, flags)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "correlated pairs: unknown bits in pair_mask or flags");
    *count = 0;
    if (v.order == 0) return JAICOV_OK;
    const int nbk = (v.order + 127) / 128, np = nbk * 128, nt = nbk * (nbk + 1) / 2;
    HIPE(*v.err, hipSetDevice(v.device));
    ParamState *st = q_state(v.slot->par);
    HIPE(*v.err, st->count.reserve((size_t)2 * nt + 1));
    TRY(par_prepare(v, st, flags, np));
    const int32_t *cls = st->tab.get(), *item = cls + np;
    int64_t *cnt = st->count.get(), *off = cnt + nt;
    hipLaunchKernelGGL(par_pairs_kernel<false>, dim3(nt), dim3(256), 0, v.stream, v.Q, v.ld, v.order, v.d, st->scale.get(), cls, item, pair_mask,
                       threshold, cnt, (const int64_t *)nullptr, (int64_t)0, (int32_t *)nullptr, (double *)nullptr);
    hipLaunchKernelGGL(par_prefix_kernel, dim3(1), dim3(256), 0, v.stream, cnt, nt, off);
    HIPE(*v.err, hipGetLastError());
    int64_t total = 0;
    TRY(q_download(v, {{&total, off + nt, sizeof(int64_t)}}));
    *count = total;
    if (total == 0 || total > capacity) return JAICOV_OK;
    HIPE(*v.err, st->out_d.reserve((size_t)total));
    HIPE(*v.err, st->out_i.reserve((size_t)2 * total));
    hipLaunchKernelGGL(par_pairs_kernel<true>, dim3(nt), dim3(256), 0, v.stream, v.Q, v.ld, v.order, v.d, st->scale.get(), cls, item, pair_mask,
                       threshold, (int64_t *)nullptr, off, total, st->out_i.get(), st->out_d.get());
    HIPE(*v.err, hipGetLastError());
    std::vector<int32_t> hc((size_t)2 * total);
    std::vector<double> hr((size_t)total);
    TRY(q_download(v, {{hc.data(), st->out_i.get(), hc.size() * sizeof(int32_t)}, {hr.data(), st->out_d.get(), hr.size() * sizeof(double)}}));
    std::vector<int64_t> ord((size_t)total);
    std::iota(ord.begin(), ord.end(), (int64_t)0);
    std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) {
        const double ra = fabs(hr[a]), rb = fabs(hr[b]);
        if (ra != rb) return ra > rb;
        if (hc[2 * a] != hc[2 * b]) return hc[2 * a] < hc[2 * b];
        return hc[2 * a + 1] < hc[2 * b + 1];
    });
    for (int64_t m = 0; m < total; m++) {
        cols[2 * m] = hc[2 * ord[m]];
        cols[2 * m + 1] = hc[2 * ord[m] + 1];
        rho[m] = hr[ord[m]];
    }
    return JAICOV_OK;
}

extern "C" int jaicov_par_block(jaicov_engine *e, const int32_t *row_cols, int32_t n_r, const int32_t *col_cols, int32_t n_c, double *out) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    TRY(q_guard(v, PAR_SHARDED));
    if (!row_cols || !col_cols || !out || n_r < 1 || n_c < 1) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "correlation block: NULL argument or an empty list");
    for (int i = 0; i < n_r + n_c; i++) {
        const int c = i < n_r ? row_cols[i] : col_cols[i - n_r];
        if (c < v.d || c >= v.order) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "correlation block: a column outside [d, order)");
    }
    const size_t cells = (size_t)n_r * n_c;
    HIPE(*v.err, hipSetDevice(v.device));
    ParamState *st = q_state(v.slot->par);
    HIPE(*v.err, st->out_i.reserve((size_t)n_r + n_c));
    HIPE(*v.err, st->out_d.reserve(cells));
    int32_t *d_rows = st->out_i.get(), *d_cols = d_rows + n_r;
    HIPE(*v.err, hipMemcpyAsync(d_rows, row_cols, (size_t)n_r * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    HIPE(*v.err, hipMemcpyAsync(d_cols, col_cols, (size_t)n_c * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(par_block_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, v.stream, v.Q, v.ld, d_rows, n_r, d_cols, n_c,
                       st->out_d.get());
    HIPE(*v.err, hipGetLastError());
    return q_download(v, {{out, st->out_d.get(), cells * sizeof(double)}});
}

extern "C" int jaicov_par_tests(jaicov_engine *e, double sigma2, const int32_t *group_begin, const int32_t *group_slot, const double *x0,
                                int32_t n_groups, double *out, int32_t *status) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    TRY(q_guard(v, PAR_SHARDED));
    if (!group_begin || !out || !status || n_groups < 0) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "parameter tests: NULL argument or a negative count");
    if (!(sigma2 > 0.0)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "parameter tests: sigma2 must be positive");
    if (!ranges_ok(n_groups, group_begin)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "parameter tests: group_begin must ascend from 0");
    const int n_members = group_begin[n_groups], n_slots = (int)v.slot_col->size();
    if (n_members > 0 && !group_slot) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "parameter tests: NULL group_slot");
    for (int m = 0; m < n_members; m++)
        if (group_slot[m] < 0 || group_slot[m] >= n_slots) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "parameter tests: slot out of range");
    // the free members: gb [n + 1] | status bits of the host [n] | column [M] | slot [M]
    const int n = n_groups;
    std::vector<int32_t> tab((size_t)2 * n + 1 + 2 * (size_t)std::max(n_members, 1), 0);
    std::vector<double> hx0((size_t)std::max(n_members, 1), 0.0);
    int M = 0;
    for (int g = 0; g < n; g++) {
        tab[g] = M;
        for (int m = group_begin[g]; m < group_begin[g + 1]; m++) {
            int c;
            TRY(q_column(v, group_slot[m], "parameter tests: a member's column is not in the reduced cofactor matrix", &c));
            if (c < 0) { tab[(size_t)n + 1 + g] |= JAICOV_PAR_PARTIAL; continue; }
            hx0[M] = x0 ? x0[m] : 0.0;
            ++M;
        }
    }
    tab[n] = M;
    if (n == 0) return JAICOV_OK;
    const size_t o_col = (size_t)2 * n + 1, o_slot = o_col + std::max(M, 1);
    M = 0;
    for (int g = 0; g < n; g++)
        for (int m = group_begin[g]; m < group_begin[g + 1]; m++) {
            const int c = (*v.slot_col)[group_slot[m]];
            if (c < 0) continue;
            tab[o_col + M] = c;
            tab[o_slot + M] = group_slot[m];
            ++M;
        }
    const size_t n_tab = o_slot + std::max(M, 1);
    HIPE(*v.err, hipSetDevice(v.device));
    ParamState *st = q_state(v.slot->par);
    HIPE(*v.err, st->out_i.reserve(n_tab + n));
    HIPE(*v.err, st->out_d.reserve((size_t)JAICOV_PAR_TEST_COLUMNS * n + std::max(M, 1)));
    int32_t *d_tab = st->out_i.get(), *d_status = d_tab + n_tab;
    double *d_out = st->out_d.get(), *d_x0 = d_out + (size_t)JAICOV_PAR_TEST_COLUMNS * n;
    HIPE(*v.err, hipMemcpyAsync(d_tab, tab.data(), n_tab * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    HIPE(*v.err, hipMemcpyAsync(d_x0, hx0.data(), (size_t)std::max(M, 1) * sizeof(double), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(par_tests_kernel, dim3(n), dim3(64), 0, v.stream, v.Q, v.ld, v.d_vals, d_tab, d_tab + o_col, d_tab + o_slot, d_x0,
                       d_tab + n + 1, sigma2, d_out, d_status);
    HIPE(*v.err, hipGetLastError());
    return q_download(v, {{out, d_out, (size_t)JAICOV_PAR_TEST_COLUMNS * n * sizeof(double)}, {status, d_status, (size_t)n * sizeof(int32_t)}});
}

// The hook of scripts/param_bench.py: kernel times by events on the engine's stream, `repeats` of each after the tables are ready.
// ms[0 .. 5 repeats): the maxima pass (tile + reduce) | pass one of the pairs (count + prefix) | the yardstick, one product Y = S X of
// symtile.h with D = 8 over [d, order) (tile + reduce) | par_max_tile_kernel alone | sym_y_tile_kernel<8> alone.
extern "C" int jaicov_debug_par_kernel_ms(jaicov_engine *e, uint32_t pair_mask, double threshold, int32_t repeats, double *ms) {
    if (!e || !ms || repeats < 1) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    TRY(q_guard(v, PAR_SHARDED));
    if (v.order == 0 || !par_selection_ok(pair_mask, 0)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "parameter bench: no columns or a bad mask");
    const int nbk = (v.order + 127) / 128, np = nbk * 128, nt = nbk * (nbk + 1) / 2;
    HIPE(*v.err, hipSetDevice(v.device));
    ParamState *st = q_state(v.slot->par);
    HIPE(*v.err, st->cand.reserve((size_t)nbk * nbk * 128));
    HIPE(*v.err, st->count.reserve((size_t)2 * nt + 1));
    HIPE(*v.err, st->out_d.reserve((size_t)np));
    HIPE(*v.err, st->out_i.reserve((size_t)2 * np));
    TRY(par_prepare(v, st, 0, np));
    DevBuf<double> Xt, Pt, Y;
    HIPE(*v.err, Xt.reserve((size_t)8 * np));
    HIPE(*v.err, Pt.reserve((size_t)nbk * nbk * 128 * 8));
    HIPE(*v.err, Y.reserve((size_t)8 * np));
    HIPE(*v.err, hipMemsetAsync(Xt.get(), 0, (size_t)8 * np * sizeof(double), v.stream));
    DevEvent a, b;
    HIPE(*v.err, a.create());
    HIPE(*v.err, b.create());
    const int32_t *cls = st->tab.get(), *item = cls + np, *st0 = item + np;
    int32_t *d_partner = st->out_i.get(), *d_status = d_partner + np;
    int64_t *cnt = st->count.get(), *off = cnt + nt;
    hipStream_t s = v.stream;
    auto max_tile = [&] {
        hipLaunchKernelGGL(par_max_tile_kernel, dim3(nt), dim3(256), 0, s, v.Q, v.ld, v.order, v.d, st->scale.get(), cls, item, pair_mask, nbk,
                           st->cand.get());
    };
    auto max_reduce = [&] {
        hipLaunchKernelGGL(par_max_reduce_kernel, dim3(nbk), dim3(128), 0, s, st->cand.get(), nbk, v.order, v.d, st->scale.get(), st0,
                           st->out_d.get(), d_partner, d_status);
    };
    auto pairs_count = [&] {
        hipLaunchKernelGGL(par_pairs_kernel<false>, dim3(nt), dim3(256), 0, s, v.Q, v.ld, v.order, v.d, st->scale.get(), cls, item, pair_mask,
                           threshold, cnt, (const int64_t *)nullptr, (int64_t)0, (int32_t *)nullptr, (double *)nullptr);
        hipLaunchKernelGGL(par_prefix_kernel, dim3(1), dim3(256), 0, s, cnt, nt, off);
    };
    auto sym_tile = [&] {
        hipLaunchKernelGGL(sym_y_tile_kernel<8>, dim3(nt), dim3(256), 0, s, v.Q, v.ld, v.order, v.d, Xt.get(), np, nbk, Pt.get());
    };
    auto sym_reduce = [&] { hipLaunchKernelGGL(sym_y_reduce_kernel<8>, dim3(nbk), dim3(512), 0, s, Pt.get(), nbk, v.order, v.d, Y.get()); };
    for (int r = 0; r < repeats; r++) {
        for (int what = 0; what < 5; what++) {
            HIPE(*v.err, hipEventRecord(a.get(), s));
            if (what == 0) { max_tile(); max_reduce(); }
            else if (what == 1) pairs_count();
            else if (what == 2) { sym_tile(); sym_reduce(); }
            else if (what == 3) max_tile();
            else sym_tile();
            HIPE(*v.err, hipGetLastError());
            HIPE(*v.err, hipEventRecord(b.get(), s));
            HIPE(*v.err, hipEventSynchronize(b.get()));
            float t = 0.f;
            HIPE(*v.err, hipEventElapsedTime(&t, a.get(), b.get()));
            ms[(size_t)what * repeats + r] = t;
        }
    }
    return JAICOV_OK;
}
