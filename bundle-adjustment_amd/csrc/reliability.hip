// Redundancy numbers and outlier test values of every observation (include/jaicov_reliability.h), formed next to the cofactor
// matrix.  gfx950 only.
//
//   rel_v_kernel        v = A dx - w of every image coordinate (engine order)
//   rel_points_kernel   image points with 2 x 2 weights: one workgroup per chunk of <= 64 points of one image, Q[shared, shared] in LDS,
//                       the 2 x 2 H = A_p Q A_p' of each point in registers, then r, P Q_vv P, q_vv and t
//   rel_prep_kernel     dense image blocks, per row: y = Q[S, P(row)] a_p and u = y + Q[S, S] a_s (S = the image's shared columns)
//   rel_pp_kernel       dense image blocks: the point x point part of H = A Q A', one workgroup per pair of 16-point chunks
//   (gemm_f64)          H += [Y | A_s] [A_s | U]' (the shared-column part of A Q A'), then G = H P on the fp64 matrix cores
//   rel_pad_kernel      P = sigma0^2 inv(D) of a block, zero-padded to the GEMM's size
//   rel_block_kernel    dense image blocks: r = 1 - G_ii, (P Q_vv P)_ii = P_ii - sum_j P_ji G_ji, q_vv, (P v)_i, t
//   rel_scalebar_kernel, rel_direct_kernel   the other observation groups
//   rel_summary_kernel  sum r, max |t| and its row, NaN count, min r in one workgroup
//
// Leave-one-out table of every image point (include/jaicov_reliability_points.h), launched by jaicov_rel_run_points only, after
// the kernels above, which it runs unchanged:
//   rel_points_loo_kernel     image points with 2 x 2 weights: H from the same rl_point, then M = P - P H P, nabla^ = -inv(M) g
//                             and the shift -Q[P(q), cols(q)] A_q' P nabla^ over the point's own 3 + kc columns, all per lane
//   rel_block_points_kernel   dense blocks, one thread per image point, after G = H P: g, M = P_S - (P G)_SS (sums over
//                             j = 0 .. m-1 in order), the closed-form columns; nabla^ goes to a work buffer
//   rel_shift_pp_kernel       dense blocks: sum_j Q[P(q), P(j)] a_p(j) c_q[j], c_q = P[:, S_q] nabla^_q, one workgroup per pair of
//                             16-point chunks (the same rl_stage_pair as rel_pp_kernel), one partial sum per (point, chunk)
//   rel_shift_kernel          dense blocks, one thread per image point: A_s' c_q (kc sums over j in order), Q[P(q), S] of it, the
//                             partial sums added in chunk order; the sum order does not depend on the images per batch
//
// Shared parts.  Layout, 2 x 2 weight, scale-bar and directly observed row: obsmodel.h.  Here: rl_stage_shared (scol and Q[S, S] of an
// image), rl_point (a_s and H of an image point), rl_stage_pair (chunk pair, a_p and Q[cols(a), cols(b)]).  Host: rel_run_impl hands one
// RelRun to rel_run_points2x2, rel_run_dense and rel_run_rest; which blocks are dense is q_image_blocks (qview.h), as for vce.hip.
//
// H of a dense block.  A row of image point q has its 3 point columns P(q) and the kc <= 29 shared columns S of the image (IO,
// distortion, EO).  With a_p, a_s the two parts of a row:
//   H_rs = a_p(r)' Q[P(r), P(s)] a_p(s) + y(r)' a_s(s) + a_s(r)' u(s),   y(r) = Q[S, P(r)] a_p(r),  u(s) = y(s) + Q[S, S] a_s(s).
// The first term reads the 3 x 3 point blocks of Q once per pair of chunks (rel_pp_kernel); the rest is a GEMM of inner dimension 2 kc.
// Every output is one fixed-order sum: two runs give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/jaicov_reliability.h"
#include "../../include/jaicov_reliability_points.h"
#include "gemm_f64.h"
#include "obsmodel.h"
#include "qview.h"
#include "reliability.h"
#include "status.h"

namespace jaicov {

constexpr int RL_PTS = 64;                // points per workgroup of rel_points_kernel, rows per workgroup of rel_prep_kernel
constexpr int RL_TP = 16;                 // points per chunk of rel_pp_kernel
constexpr int RL_PC = 3 * RL_TP;          // point columns of a chunk (48)
constexpr int RL_RC = 2 * RL_TP;          // rows of a chunk (32)
constexpr int RL_K = 64;                  // inner dimension of the shared-column GEMM: [Y | A_s], 2 KC_MAX = 58 padded to 16
constexpr double RL_UNCONTROLLED = 1e-10; // (P Q_vv P)_ii <= this * P_ii: the observation is not controlled, t = NaN
static_assert(2 * KC_MAX <= RL_K && RL_K % GEMM_BK == 0, "[Y | A_s] must fit the inner dimension of the shared-column GEMM");

__device__ __forceinline__ long rl_row(const int32_t *__restrict__ new2old, int ip, int c) {
    return 2 * (long)(new2old ? new2old[ip] : ip) + c;
}
__device__ __forceinline__ double rl_t(double pv, double ppp, double pii, double s2t) {
    return ppp > RL_UNCONTROLLED * pii ? pv / sqrt(s2t * ppp) : (double)NAN;
}
__device__ __forceinline__ void rl_store(double *__restrict__ out, long n_rows, long row, double v, double qvv, double r, double t) {
    out[row] = v;
    out[n_rows + row] = qvv;
    out[2 * n_rows + row] = r;
    out[3 * n_rows + row] = t;
}

// v = A dx - w of every image coordinate, engine order: v[2 ip + c]
__global__ __launch_bounds__(256) void rel_v_kernel(DevProblem p, const double *__restrict__ rowsA, const double *__restrict__ rowsW,
                                                    const double *__restrict__ dx, double *__restrict__ v) {
    const int ip = blockIdx.x * 256 + threadIdx.x;
    if (ip >= p.n_ip) return;
    const long S = p.n_ip;
    const int img = p.ip_image[ip], cam = p.image_camera[img], pt = p.ip_point[ip];
    const int jb = p.cam_dist_begin[cam], nd = p.cam_dist_begin[cam + 1] - jb;
    double v0 = -rowsW[ip], v1 = -rowsW[S + ip];
    for (int l = 0; l < 12 + nd; l++) {
        const int col = obs_row_col(p, pt, img, cam, jb, l);
        if (col < 0) continue;
        const double d = dx[col];
        v0 = fma(rowsA[(long)(2 * l) * S + ip], d, v0);
        v1 = fma(rowsA[(long)(2 * l + 1) * S + ip], d, v1);
    }
    v[2 * (long)ip] = v0;
    v[2 * (long)ip + 1] = v1;
}

// A workgroup of RL_PTS threads stages what it needs of the shared columns S of image img: scol[c] = the global column of shared local
// column c, sQ = Q[S, S] (row length KC_MAX, zero in the fixed columns).  Returns kc; the last barrier is behind it.
__device__ __forceinline__ int rl_stage_shared(const DevProblem &p, int img, const double *Q, long ld, int *scol, double *sQ) {
    const int tid = threadIdx.x;
    const int cam = p.image_camera[img], jb = p.cam_dist_begin[cam], kc = obs_kc(p, cam);
    if (tid < kc) scol[tid] = obs_shared_col(p, img, cam, jb, tid);
    __syncthreads();
    for (int i = tid; i < kc * kc; i += RL_PTS) {
        const int a = i / kc, b = i - a * kc;
        const int qa = scol[a], qb = scol[b];
        sQ[a * KC_MAX + b] = (qa < 0 || qb < 0) ? 0.0 : q_sym(Q, ld, qa, qb);
    }
    __syncthreads();
    return kc;
}

// An image point with 2 x 2 weights: its point columns pc, their coefficients ap (zero where fixed) and the 2 x 2 H = A Q A' of its rows
struct RelPoint {
    int pc[3];
    double ap[2][3];
    double h00, h01, h11;
};

// Fills o for engine image point ip and leaves the shared part a_s of its two rows in LDS: column c of row 0 / 1 at my0 / my1[c * RL_PTS]
// (zero where fixed).  scol, sQ: rl_stage_shared's.  No barrier: a lane reads its own a_s only.
__device__ __forceinline__ void rl_point(const DevProblem &p, int ip, int kc, const int *scol, const double *sQ, double *my0, double *my1,
                                         const double *Q, long ld, const double *rowsA, RelPoint &o) {
    const long S = p.n_ip;
    const int pt = p.ip_point[ip];
    for (int c = 0; c < kc; c++) {
        const bool f = scol[c] >= 0;
        my0[c * RL_PTS] = f ? rowsA[(long)(2 * obs_shared_row(c)) * S + ip] : 0.0;
        my1[c * RL_PTS] = f ? rowsA[(long)(2 * obs_shared_row(c) + 1) * S + ip] : 0.0;
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        o.pc[a] = p.point_col[3 * pt + a];
        o.ap[0][a] = o.pc[a] >= 0 ? rowsA[(long)(2 * a) * S + ip] : 0.0;
        o.ap[1][a] = o.pc[a] >= 0 ? rowsA[(long)(2 * a + 1) * S + ip] : 0.0;
    }
    double h00 = 0.0, h01 = 0.0, h11 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            if (o.pc[a] < 0 || o.pc[b] < 0) continue;
            const double q = q_sym(Q, ld, o.pc[a], o.pc[b]);
            h00 = fma(o.ap[0][a], q * o.ap[0][b], h00);
            h01 = fma(o.ap[0][a], q * o.ap[1][b], h01);
            h11 = fma(o.ap[1][a], q * o.ap[1][b], h11);
        }
    for (int c = 0; c < kc; c++) {
        const int qc = scol[c];
        if (qc < 0) continue;
        double y0 = 0.0, y1 = 0.0, z0 = 0.0, z1 = 0.0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (o.pc[a] < 0) continue;
            const double q = q_sym(Q, ld, qc, o.pc[a]);
            y0 = fma(q, o.ap[0][a], y0);
            y1 = fma(q, o.ap[1][a], y1);
        }
        for (int b = 0; b < kc; b++) {
            const double q = sQ[c * KC_MAX + b];
            z0 = fma(q, my0[b * RL_PTS], z0);
            z1 = fma(q, my1[b * RL_PTS], z1);
        }
        const double a0 = my0[c * RL_PTS], a1 = my1[c * RL_PTS];
        h00 += a0 * (2.0 * y0 + z0);
        h11 += a1 * (2.0 * y1 + z1);
        h01 += y0 * a1 + a0 * (y1 + z1);
    }
    o.h00 = h00; o.h01 = h01; o.h11 = h11;
}

// chunks[i] = (first engine image point, count <= RL_PTS), all of one image, all with 2 x 2 weights
__global__ __launch_bounds__(RL_PTS) void rel_points_kernel(DevProblem p, const int2 *__restrict__ chunks, const double *__restrict__ Q, long ld,
                                                            const double *__restrict__ rowsA, const double *__restrict__ v,
                                                            const double *__restrict__ lld, const int32_t *__restrict__ new2old, double s0,
                                                            double s2t, long n_rows, double *__restrict__ out) {
    __shared__ double sQ[KC_MAX * KC_MAX];
    __shared__ double sA[2 * KC_MAX * RL_PTS];   // the shared part a_s of both rows of every point: [row][column][lane]
    __shared__ int scol[KC_MAX];
    const int tid = threadIdx.x;
    const int2 ch = chunks[blockIdx.x];
    const int kc = rl_stage_shared(p, p.ip_image[ch.x], Q, ld, scol, sQ);
    if (tid >= ch.y) return;
    const int ip = ch.x + tid;
    RelPoint k;
    rl_point(p, ip, kc, scol, sQ, sA + tid, sA + KC_MAX * RL_PTS + tid, Q, ld, rowsA, k);
    double p00, p01, p11;
    obs_weight(p, ip, s0, p00, p01, p11);
    // g01 as an fma: which of its two products is fused must not hang on the order in which obs_weight defines its results
    const double g00 = k.h00 * p00 + k.h01 * p01, g01 = fma(k.h00, p01, k.h01 * p11);
    const double g10 = k.h01 * p00 + k.h11 * p01, g11 = k.h01 * p01 + k.h11 * p11;
    const double ppp0 = p00 - (p00 * g00 + p01 * g10), ppp1 = p11 - (p01 * g01 + p11 * g11);
    const double v0 = v[2 * (long)ip], v1 = v[2 * (long)ip + 1];
    const double pv0 = p00 * v0 + p01 * v1, pv1 = p01 * v0 + p11 * v1;
    rl_store(out, n_rows, rl_row(new2old, ip, 0), v0, lld[2 * (long)ip] / s0 - k.h00, 1.0 - g00, rl_t(pv0, ppp0, p00, s2t));
    rl_store(out, n_rows, rl_row(new2old, ip, 1), v1, lld[2 * (long)ip + 1] / s0 - k.h11, 1.0 - g11, rl_t(pv1, ppp1, p11, s2t));
}

// Dense blocks, per row i < m of block bl[blockIdx.y]: L[i] = [y(i) | a_s(i)], R[i] = [a_s(i) | u(i)] (KC_MAX each, zero beyond kc and
// in the padding rows up to mpad).  L, R: [batch][mpad][RL_K].
__global__ __launch_bounds__(RL_PTS) void rel_prep_kernel(DevProblem p, const int32_t *__restrict__ bl, int mpad, const double *__restrict__ Q, long ld,
                                                          const double *__restrict__ rowsA, double *__restrict__ L, double *__restrict__ R) {
    __shared__ double sQ[KC_MAX * KC_MAX];
    __shared__ double sA[KC_MAX * RL_PTS];       // a_s of every row of the workgroup: [column][lane]
    __shared__ int scol[KC_MAX];
    const int tid = threadIdx.x;
    const int g = bl[blockIdx.y];
    const int ipb = p.blk_ip_begin[g], m = 2 * (p.blk_ip_begin[g + 1] - ipb);
    const int kc = rl_stage_shared(p, p.ip_image[ipb], Q, ld, scol, sQ);
    const long S = p.n_ip;
    const int i = blockIdx.x * RL_PTS + tid;
    if (i >= mpad) return;
    double *Lr = L + ((long)blockIdx.y * mpad + i) * RL_K, *Rr = R + ((long)blockIdx.y * mpad + i) * RL_K;
    if (i >= m) {
        for (int k = 0; k < RL_K; k++) { Lr[k] = 0.0; Rr[k] = 0.0; }
        return;
    }
    const int ip = ipb + (i >> 1), r = i & 1, pt = p.ip_point[ip];
    double *my = sA + tid;
    for (int c = 0; c < kc; c++) my[c * RL_PTS] = scol[c] >= 0 ? rowsA[(long)(2 * obs_shared_row(c) + r) * S + ip] : 0.0;
    int pc[3];
    double ap[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        pc[a] = p.point_col[3 * pt + a];
        ap[a] = pc[a] >= 0 ? rowsA[(long)(2 * a + r) * S + ip] : 0.0;
    }
    for (int c = 0; c < KC_MAX; c++) {
        double y = 0.0, u = 0.0, as = 0.0;
        if (c < kc && scol[c] >= 0) {
#pragma unroll
            for (int a = 0; a < 3; a++)
                if (pc[a] >= 0) y = fma(q_sym(Q, ld, scol[c], pc[a]), ap[a], y);
            double z = 0.0;
            for (int b = 0; b < kc; b++) z = fma(sQ[c * KC_MAX + b], my[b * RL_PTS], z);
            u = y + z;
            as = my[c * RL_PTS];
        }
        Lr[c] = y; Lr[KC_MAX + c] = as;
        Rr[c] = as; Rr[KC_MAX + c] = u;
    }
    for (int k = 2 * KC_MAX; k < RL_K; k++) { Lr[k] = 0.0; Rr[k] = 0.0; }
}

// The chunk pair b <= a of workgroup blockIdx.x of block bl[blockIdx.y]: false where the block has fewer pairs (the whole workgroup
// leaves).  Otherwise colA / colB = the point columns of the chunks' points (-1: none), sAa / sAb = a_p of their 32 rows each,
// sQ = Q[cols(a), cols(b)] (row length RL_PC + 1, zero where a column is none); the last barrier is behind it.
struct RelPair {
    long a, b;                 // chunks
    int pa0, pb0, na, nb;      // first point and points of either chunk
};
__device__ __forceinline__ bool rl_stage_pair(const DevProblem &p, const int32_t *bl, const double *Q, long ld,
                                              const double *rowsA, double *sQ, double *sAa, double *sAb, int *colA, int *colB,
                                              RelPair &o) {
    const int tid = threadIdx.x;
    const int g = bl[blockIdx.y];
    const int ipb = p.blk_ip_begin[g], mp = p.blk_ip_begin[g + 1] - ipb;
    const long nch = (mp + RL_TP - 1) / RL_TP, tiles = nch * (nch + 1) / 2, t = blockIdx.x;
    if (t >= tiles) return false;
    long a = (long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (a * (a + 1) / 2 > t) a--;
    while ((a + 1) * (a + 2) / 2 <= t) a++;
    const long b = t - a * (a + 1) / 2;
    const int pa0 = (int)a * RL_TP, pb0 = (int)b * RL_TP;
    const int na = min(RL_TP, mp - pa0), nb = min(RL_TP, mp - pb0);
    const long S = p.n_ip;
    if (tid < RL_PC) {
        const int k = tid / 3, c = tid - 3 * k;
        colA[tid] = k < na ? p.point_col[3 * p.ip_point[ipb + pa0 + k] + c] : -1;
        colB[tid] = k < nb ? p.point_col[3 * p.ip_point[ipb + pb0 + k] + c] : -1;
    }
    __syncthreads();
    if (tid < 2 * RL_RC) {   // a_p of the 32 rows of chunk a (threads 0-31) and of chunk b (32-63)
        const int side = tid / RL_RC, k = tid - side * RL_RC, q = k >> 1, r = k & 1;
        const int n = side ? nb : na, p0 = side ? pb0 : pa0;
        const int *cl = side ? colB : colA;
        double *dst = (side ? sAb : sAa) + 3 * k;
        for (int c = 0; c < 3; c++) dst[c] = (q < n && cl[3 * q + c] >= 0) ? rowsA[(long)(2 * c + r) * S + ipb + p0 + q] : 0.0;
    }
    // stage Q[cols(a), cols(b)]: lower entries along the column index, mirrored ones along the row index
    for (int i = tid; i < RL_PC * RL_PC; i += 256) {
        const int r = i / RL_PC, c = i - r * RL_PC;
        const int qr = colA[r], qc = colB[c];
        if (qr < 0 || qc < 0) sQ[r * (RL_PC + 1) + c] = 0.0;
        else if (qr >= qc) sQ[r * (RL_PC + 1) + c] = Q[(long)qr * ld + qc];
    }
    for (int i = tid; i < RL_PC * RL_PC; i += 256) {
        const int c = i / RL_PC, r = i - c * RL_PC;
        const int qr = colA[r], qc = colB[c];
        if (qr >= 0 && qc >= 0 && qr < qc) sQ[r * (RL_PC + 1) + c] = Q[(long)qc * ld + qr];
    }
    __syncthreads();
    o.a = a; o.b = b; o.pa0 = pa0; o.pb0 = pb0; o.na = na; o.nb = nb;
    return true;
}

// Dense blocks: H[bi][rows of chunk a][rows of chunk b] = a_p Q[P, P] a_p' (and its mirror), one workgroup per chunk pair b <= a.
// grid (most chunk pairs of a block of the batch, blocks of the batch)
__global__ __launch_bounds__(256) void rel_pp_kernel(DevProblem p, const int32_t *__restrict__ bl, int mpad, const double *__restrict__ Q, long ld,
                                                     const double *__restrict__ rowsA, double *__restrict__ H) {
    __shared__ double sQ[RL_PC * (RL_PC + 1)];
    __shared__ double sAa[RL_RC * 3], sAb[RL_RC * 3];
    __shared__ int colA[RL_PC], colB[RL_PC];
    const int tid = threadIdx.x;
    RelPair t;
    if (!rl_stage_pair(p, bl, Q, ld, rowsA, sQ, sAa, sAb, colA, colB, t)) return;
    const long a = t.a, b = t.b;
    const int pa0 = t.pa0, pb0 = t.pb0, na = t.na, nb = t.nb;
    double *Hb = H + (long)blockIdx.y * mpad * mpad;
    const int ra = 2 * pa0, rb = 2 * pb0;
    for (int i = tid; i < RL_RC * RL_RC; i += 256) {
        const int x = i / RL_RC, y = i - x * RL_RC;
        if (x >= 2 * na || y >= 2 * nb) continue;
        const double *qa = sQ + 3 * (x >> 1) * (RL_PC + 1) + 3 * (y >> 1);
        const double *ua = sAa + 3 * x, *ub = sAb + 3 * y;
        double h = 0.0;
#pragma unroll
        for (int u = 0; u < 3; u++) {
            const double z = fma(qa[u * (RL_PC + 1)], ub[0], fma(qa[u * (RL_PC + 1) + 1], ub[1], qa[u * (RL_PC + 1) + 2] * ub[2]));
            h = fma(ua[u], z, h);
        }
        Hb[(long)(ra + x) * mpad + rb + y] = h;
        if (a != b) Hb[(long)(rb + y) * mpad + ra + x] = h;
    }
}

// P = sigma0^2 inv(D) of block bl[blockIdx.z], zero-padded to mpad x mpad; grid (ceil(mpad / 256), mpad, batch)
__global__ __launch_bounds__(256) void rel_pad_kernel(DevProblem p, const int32_t *__restrict__ bl, int mpad, double s0, double *__restrict__ P) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= mpad) return;
    const int g = bl[blockIdx.z];
    const int m = 2 * (p.blk_ip_begin[g + 1] - p.blk_ip_begin[g]);
    const double *W = p.blk_w + p.blk_w_offset[g];
    P[((long)blockIdx.z * mpad + i) * mpad + j] = (i < m && j < m) ? s0 * W[(long)i * m + j] : 0.0;
}

// grid (ceil(mpad / 256), batch): row i of block bl[blockIdx.y]
__global__ __launch_bounds__(256) void rel_block_kernel(DevProblem p, const int32_t *__restrict__ bl, int mpad, const double *__restrict__ H,
                                                        const double *__restrict__ P, const double *__restrict__ G, const double *__restrict__ v,
                                                        const double *__restrict__ lld, const int32_t *__restrict__ new2old, double s0, double s2t,
                                                        long n_rows, double *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int g = bl[blockIdx.y];
    const int ipb = p.blk_ip_begin[g], m = 2 * (p.blk_ip_begin[g + 1] - ipb);
    if (i >= m) return;
    const long off = (long)blockIdx.y * mpad * mpad;
    const double *Pb = P + off, *Gb = G + off, *vb = v + 2 * (long)ipb;
    double php = 0.0, pv = 0.0;
    for (int j = 0; j < m; j++) {
        const double pji = Pb[(long)j * mpad + i];
        php = fma(pji, Gb[(long)j * mpad + i], php);
        pv = fma(pji, vb[j], pv);
    }
    const double pii = Pb[(long)i * mpad + i];
    const double h = H[off + (long)i * mpad + i], gii = Gb[(long)i * mpad + i];
    rl_store(out, n_rows, rl_row(new2old, ipb + (i >> 1), i & 1), vb[i], lld[2 * (long)ipb + i] / s0 - h, 1.0 - gii, rl_t(pv, pii - php, pii, s2t));
}

// ---- leave-one-out table of every image point (include/jaicov_reliability_points.h) ----------------------------------------------
struct RelPointArgs {
    double lambda0, omega;
    int dof;
};

// Columns 0-10 of image point o (the caller's index) of the table pt[JAICOV_REL_POINT_COLUMNS][n] from g = (P v)_S, P_S and
// N = (P A Qxx A' P)_SS; M = P_S - N.  Returns nabla^ = -inv(M) g, NaN where the point is not controlled.  The eigenvalues of M and
// of inv(M) N (= those of inv(M) P_S less 1) are the closed forms of a 2 x 2 matrix.
__device__ __forceinline__ double2 rl_point_columns(double g0, double g1, double pxx, double pxy, double pyy, double nxx, double nxy,
                                                    double nyy, double s2t, RelPointArgs pa, long n, long o, double *__restrict__ pt) {
    const double mxx = pxx - nxx, mxy = pxy - nxy, myy = pyy - nyy;
    const double half = 0.5 * (mxx + myy), dev = hypot(0.5 * (mxx - myy), mxy);
    const double mu_max = half + dev;
    const double det = fma(mxx, myy, -(mxy * mxy));
    const double mu_min = mu_max > 0.0 ? det / mu_max : half - dev;
    pt[5 * n + o] = mxx;
    pt[6 * n + o] = mxy;
    pt[7 * n + o] = myy;
    const double nan = (double)NAN;
    if (!(mu_min > RL_UNCONTROLLED * fmax(pxx, pyy))) {
        for (int c = 0; c < 5; c++) pt[c * n + o] = nan;
        for (int c = 8; c < 11; c++) pt[c * n + o] = nan;
        return make_double2(nan, nan);
    }
    const double nx = -(myy * g0 - mxy * g1) / det, ny = -(mxx * g1 - mxy * g0) / det;
    const double q = -(g0 * nx + g1 * ny);
    pt[o] = q;
    pt[n + o] = q / (2.0 * s2t);
    const double rest = pa.omega - q;
    pt[2 * n + o] = (pa.dof > 2 && pa.omega > 0.0 && rest > 0.0) ? (0.5 * q) / (rest / (double)(pa.dof - 2)) : nan;
    pt[3 * n + o] = nx;
    pt[4 * n + o] = ny;
    pt[8 * n + o] = sqrt(pa.lambda0 * s2t / mu_min);
    pt[9 * n + o] = sqrt(pa.lambda0 * s2t / mu_max);
    // lambda_max(inv(M) N): the larger root of det(M) l^2 - (mxx nyy + myy nxx - 2 mxy nxy) l + det(N) = 0
    const double tr = mxx * nyy + myy * nxx - 2.0 * mxy * nxy, detn = fma(nxx, nyy, -(nxy * nxy));
    const double lmax = (tr + sqrt(fmax(tr * tr - 4.0 * det * detn, 0.0))) / (2.0 * det);
    pt[10 * n + o] = sqrt(pa.lambda0 * fmax(lmax, 0.0));
    return make_double2(nx, ny);
}

// The image points of rel_points_kernel's chunks once more: the same rl_point, then the point's columns and its shift.
__global__ __launch_bounds__(RL_PTS) void rel_points_loo_kernel(DevProblem p, const int2 *__restrict__ chunks, const double *__restrict__ Q, long ld,
                                                                const double *__restrict__ rowsA, const double *__restrict__ v,
                                                                const int32_t *__restrict__ new2old, double s0, double s2t, RelPointArgs pa,
                                                                double *__restrict__ pt) {
    __shared__ double sQ[KC_MAX * KC_MAX];
    __shared__ double sA[2 * KC_MAX * RL_PTS];   // the shared part a_s of both rows of every point: [row][column][lane]
    __shared__ int scol[KC_MAX];
    const int tid = threadIdx.x;
    const int2 ch = chunks[blockIdx.x];
    const int kc = rl_stage_shared(p, p.ip_image[ch.x], Q, ld, scol, sQ);
    if (tid >= ch.y) return;
    const int ip = ch.x + tid;
    double *my0 = sA + tid, *my1 = sA + KC_MAX * RL_PTS + tid;
    RelPoint k;
    rl_point(p, ip, kc, scol, sQ, my0, my1, Q, ld, rowsA, k);
    // P written out, not obs_weight: rl_point_columns fuses the products of q and tr by the rank of P's entries, and the table's bits
    // are those of this order of definition (the dense blocks' kernel, which loads P, has its own)
    double p00, p01, p11;
    {
        const double vx = p.ip_var_x[ip], vy = p.ip_var_y[ip], rho = p.ip_rho[ip];
        if (rho == 0) {
            p00 = s0 / vx; p11 = s0 / vy; p01 = 0.0;
        } else {
            const double invDet = s0 / ((1.0 - rho * rho) * vx * vy);
            p00 = invDet * vy; p11 = invDet * vx; p01 = -invDet * rho * sqrt(vx * vy);
        }
    }
    // N = P H P (H has no entries outside the point's own two rows: P is 2 x 2)
    const double g00 = k.h00 * p00 + k.h01 * p01, g01 = k.h00 * p01 + k.h01 * p11;
    const double g10 = k.h01 * p00 + k.h11 * p01, g11 = k.h01 * p01 + k.h11 * p11;
    const double nxx = p00 * g00 + p01 * g10, nxy = p00 * g01 + p01 * g11, nyy = p01 * g01 + p11 * g11;
    const double v0 = v[2 * (long)ip], v1 = v[2 * (long)ip + 1];
    const long n = p.n_ip, o = new2old ? new2old[ip] : ip;
    const double2 nab = rl_point_columns(p00 * v0 + p01 * v1, p01 * v0 + p11 * v1, p00, p01, p11, nxx, nxy, nyy, s2t, pa, n, o, pt);
    // shift = -Q[P(q), cols(q)] b,  b = A_q' c over the point's 3 + kc columns,  c = P nabla^
    const double c0 = p00 * nab.x + p01 * nab.y, c1 = p01 * nab.x + p11 * nab.y;
    double sh[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int b = 0; b < 3; b++) {
        if (k.pc[b] < 0) continue;
        const double bp = k.ap[0][b] * c0 + k.ap[1][b] * c1;
#pragma unroll
        for (int a = 0; a < 3; a++)
            if (k.pc[a] >= 0) sh[a] = fma(q_sym(Q, ld, k.pc[a], k.pc[b]), bp, sh[a]);
    }
    for (int c = 0; c < kc; c++) {
        const int qc = scol[c];
        if (qc < 0) continue;
        const double bs = my0[c * RL_PTS] * c0 + my1[c * RL_PTS] * c1;
#pragma unroll
        for (int a = 0; a < 3; a++)
            if (k.pc[a] >= 0) sh[a] = fma(q_sym(Q, ld, k.pc[a], qc), bs, sh[a]);
    }
    const bool ok = !isnan(nab.x);
#pragma unroll
    for (int a = 0; a < 3; a++) pt[(11 + a) * n + o] = ok ? (k.pc[a] >= 0 ? -sh[a] : 0.0) : (double)NAN;
}

// Dense blocks, image point q of block bl[blockIdx.y]: grid (ceil(mpad / 2 / 256), batch).  nab: [batch][mpad / 2][2]
__global__ __launch_bounds__(256) void rel_block_points_kernel(DevProblem p, const int32_t *__restrict__ bl, int mpad, const double *__restrict__ P,
                                                               const double *__restrict__ G, const double *__restrict__ v,
                                                               const int32_t *__restrict__ new2old, double s2t, RelPointArgs pa,
                                                               double *__restrict__ nab, double *__restrict__ pt) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int g = bl[blockIdx.y];
    const int ipb = p.blk_ip_begin[g], mp = p.blk_ip_begin[g + 1] - ipb, m = 2 * mp;
    if (q >= mp) return;
    const long off = (long)blockIdx.y * mpad * mpad;
    const double *Pb = P + off + 2 * q, *Gb = G + off + 2 * q, *vb = v + 2 * (long)ipb;
    double gx = 0.0, gy = 0.0, nxx = 0.0, nxy = 0.0, nyy = 0.0;
    for (int j = 0; j < m; j++) {
        const double pjx = Pb[(long)j * mpad], pjy = Pb[(long)j * mpad + 1];
        const double gjx = Gb[(long)j * mpad], gjy = Gb[(long)j * mpad + 1];
        nxx = fma(pjx, gjx, nxx);
        nxy = fma(pjx, gjy, nxy);
        nyy = fma(pjy, gjy, nyy);
        gx = fma(pjx, vb[j], gx);
        gy = fma(pjy, vb[j], gy);
    }
    const double pxx = Pb[(long)(2 * q) * mpad], pxy = Pb[(long)(2 * q) * mpad + 1], pyy = Pb[(long)(2 * q + 1) * mpad + 1];
    const long o = new2old ? new2old[ipb + q] : ipb + q;
    const double2 nb = rl_point_columns(gx, gy, pxx, pxy, pyy, nxx, nxy, nyy, s2t, pa, p.n_ip, o, pt);
    double *dst = nab + (long)blockIdx.y * mpad + 2 * q;
    dst[0] = nb.x;
    dst[1] = nb.y;
}

// Dense blocks: part[bi][q][chunk][3] = sum over the points k of the chunk of Q[P(q), P(k)] (a_p(2k) c_q[2k] + a_p(2k+1) c_q[2k+1]),
// c_q = P[:, S_q] nabla^_q.  One workgroup per chunk pair b <= a (rel_pp_kernel's grid and staging): thread (qi, ki) forms the term of
// point qi of chunk a and point ki of chunk b and, where a != b, of point qi of chunk b and point ki of chunk a; the 16 terms of a
// point are then added in the order of ki.  Every (point, chunk) of a block is written exactly once.  part: [batch][mpad / 2][mpad / 32][3]
__global__ __launch_bounds__(256) void rel_shift_pp_kernel(DevProblem p, const int32_t *__restrict__ bl, int mpad, const double *__restrict__ Q, long ld,
                                                           const double *__restrict__ rowsA, const double *__restrict__ P,
                                                           const double *__restrict__ nab, double *__restrict__ part) {
    __shared__ double sQ[RL_PC * (RL_PC + 1)];
    __shared__ double sAa[RL_RC * 3], sAb[RL_RC * 3];
    __shared__ double sT[2][RL_TP * RL_TP * 3];
    __shared__ int colA[RL_PC], colB[RL_PC];
    const int tid = threadIdx.x;
    RelPair t;
    if (!rl_stage_pair(p, bl, Q, ld, rowsA, sQ, sAa, sAb, colA, colB, t)) return;
    const long a = t.a, b = t.b;
    const int pa0 = t.pa0, pb0 = t.pb0, na = t.na, nb = t.nb;
    const double *Pb = P + (long)blockIdx.y * mpad * mpad, *nb_ = nab + (long)blockIdx.y * mpad;
    const int qi = tid / RL_TP, ki = tid - qi * RL_TP;
    const int dirs = a != b ? 2 : 1;
    for (int d = 0; d < dirs; d++) {
        const int nq = d ? nb : na, nk = d ? na : nb, q0 = d ? pb0 : pa0, k0 = d ? pa0 : pb0;
        double o[3] = {0.0, 0.0, 0.0};
        if (qi < nq && ki < nk) {
            const int cq = 2 * (q0 + qi), rk = 2 * (k0 + ki);
            const double nx = nb_[cq], ny = nb_[cq + 1];
            const double c0 = fma(Pb[(long)rk * mpad + cq], nx, Pb[(long)rk * mpad + cq + 1] * ny);
            const double c1 = fma(Pb[(long)(rk + 1) * mpad + cq], nx, Pb[(long)(rk + 1) * mpad + cq + 1] * ny);
            const double *ak = (d ? sAa : sAb) + 6 * ki;
            double w[3];
#pragma unroll
            for (int x = 0; x < 3; x++) w[x] = fma(ak[x], c0, ak[3 + x] * c1);
#pragma unroll
            for (int u = 0; u < 3; u++) {
                const double *qr = d ? sQ + (3 * ki) * (RL_PC + 1) + 3 * qi + u : sQ + (3 * qi + u) * (RL_PC + 1) + 3 * ki;
                const int st = d ? RL_PC + 1 : 1;
                o[u] = fma(qr[0], w[0], fma(qr[st], w[1], qr[2 * st] * w[2]));
            }
        }
#pragma unroll
        for (int u = 0; u < 3; u++) sT[d][(qi * RL_TP + ki) * 3 + u] = o[u];
    }
    __syncthreads();
    if (tid < dirs * RL_PC) {
        const int d = tid / RL_PC, x = tid - d * RL_PC, q = x / 3, u = x - 3 * q;
        const int nq = d ? nb : na, q0 = d ? pb0 : pa0;
        if (q < nq) {
            double s = 0.0;
            for (int k = 0; k < RL_TP; k++) s += sT[d][(q * RL_TP + k) * 3 + u];
            const long chunk = d ? a : b;
            part[(((long)blockIdx.y * (mpad / 2) + q0 + q) * (mpad / RL_RC) + chunk) * 3 + u] = s;
        }
    }
}

// Dense blocks, image point q of block bl[blockIdx.y]: grid (ceil(mpad / 2 / RL_PTS), batch).  R: rel_prep_kernel's [a_s | u] rows (a_s is
// zero in its fixed columns and beyond kc).  shift = -(sum of the chunk partials in chunk order + Q[P(q), S] (A_s' c_q)).
__global__ __launch_bounds__(RL_PTS) void rel_shift_kernel(DevProblem p, const int32_t *__restrict__ bl, int mpad, const double *__restrict__ Q, long ld,
                                                           const double *__restrict__ P, const double *__restrict__ R,
                                                           const double *__restrict__ nab, const double *__restrict__ part,
                                                           const int32_t *__restrict__ new2old, double *__restrict__ pt) {
    const int q = blockIdx.x * RL_PTS + threadIdx.x;
    const int g = bl[blockIdx.y];
    const int ipb = p.blk_ip_begin[g], mp = p.blk_ip_begin[g + 1] - ipb, m = 2 * mp;
    if (q >= mp) return;
    const int img = p.ip_image[ipb], cam = p.image_camera[img], jb = p.cam_dist_begin[cam], kc = obs_kc(p, cam);
    const double *Pb = P + (long)blockIdx.y * mpad * mpad + 2 * q, *Rb = R + (long)blockIdx.y * mpad * RL_K;
    const double nx = nab[(long)blockIdx.y * mpad + 2 * q], ny = nab[(long)blockIdx.y * mpad + 2 * q + 1];
    double acc[KC_MAX];
#pragma unroll
    for (int c = 0; c < KC_MAX; c++) acc[c] = 0.0;
    for (int j = 0; j < m; j++) {
        const double cj = fma(Pb[(long)j * mpad], nx, Pb[(long)j * mpad + 1] * ny);
        const double *as = Rb + (long)j * RL_K;
#pragma unroll
        for (int c = 0; c < KC_MAX; c++) acc[c] = fma(as[c], cj, acc[c]);
    }
    const int pnt = p.ip_point[ipb + q];
    int pc[3];
    double sh[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 3; a++) pc[a] = p.point_col[3 * pnt + a];
    const long nch = (mp + RL_TP - 1) / RL_TP;
    const double *pq = part + ((long)blockIdx.y * (mpad / 2) + q) * (mpad / RL_RC) * 3;
    for (long c = 0; c < nch; c++)
#pragma unroll
        for (int a = 0; a < 3; a++) sh[a] += pq[3 * c + a];
#pragma unroll
    for (int c = 0; c < KC_MAX; c++) {
        const int qc = c < kc ? obs_shared_col(p, img, cam, jb, c) : -1;
        if (qc < 0) continue;
#pragma unroll
        for (int a = 0; a < 3; a++)
            if (pc[a] >= 0) sh[a] = fma(q_sym(Q, ld, pc[a], qc), acc[c], sh[a]);
    }
    const long n = p.n_ip, o = new2old ? new2old[ipb + q] : ipb + q;
    const bool ok = !isnan(nx);
#pragma unroll
    for (int a = 0; a < 3; a++) pt[(11 + a) * n + o] = ok ? (pc[a] >= 0 ? -sh[a] : 0.0) : (double)NAN;
}

// scale bars (PDF:210-283): one thread each; row = row0 + s
__global__ __launch_bounds__(64) void rel_scalebar_kernel(DevProblem p, const double *__restrict__ vals, const double *__restrict__ Q, long ld,
                                                          const double *__restrict__ dx, double s0, double s2t, long row0, long n_rows,
                                                          double *__restrict__ out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= p.n_sb) return;
    int col[6];
    double ev[6], len;
    obs_scalebar_row(p, vals, s, col, ev, len);
    double v = len - p.sb_len[s], h = 0.0;     // v = A dx - w, w = observed - computed
    for (int k = 0; k < 6; k++) {
        if (col[k] < 0) continue;
        v = fma(ev[k], dx[col[k]], v);
        double z = 0.0;
        for (int l = 0; l < 6; l++)
            if (col[l] >= 0) z = fma(q_sym(Q, ld, col[k], col[l]), ev[l], z);
        h = fma(ev[k], z, h);
    }
    const double P = s0 / p.sb_var[s];
    const double r = 1.0 - h * P;
    rl_store(out, n_rows, row0 + s, v, p.sb_var[s] / s0 - h, r, rl_t(P * v, P - P * h * P, P, s2t));
}

// directly observed parameter groups (PDF:447-473): A is a selection matrix, H = Q[cols, cols]; one workgroup per group, a thread per row.
// lld[r]: diag(D) of direct row r (the dispersion's diagonal for a dense group, dg_var otherwise)
__global__ __launch_bounds__(256) void rel_direct_kernel(DevProblem p, const double *__restrict__ vals, const double *__restrict__ Q, long ld,
                                                         const double *__restrict__ dx, const double *__restrict__ lld, double s0, double s2t,
                                                         long row0, long n_rows, double *__restrict__ out) {
    const int g = blockIdx.x;
    const int b = p.dg_row_begin[g], m = p.dg_row_begin[g + 1] - b;
    const long woff = p.dg_w_offset[g];
    const double *W = woff >= 0 ? p.dg_w + woff : nullptr;
    auto col_of = [&](int k) { return obs_direct_col(p, b + k); };
    // v = A dx - w = 0 - (w - A dx): the exact negative, and 0 - x leaves a zero its positive sign as (value - observed) + dx does
    auto v_of = [&](int k) { return 0.0 - obs_direct_w(p, vals, dx, b + k, col_of(k)); };
    auto h_of = [&](int k, int l) {
        const int ck = col_of(k), cl = col_of(l);
        return (ck < 0 || cl < 0) ? 0.0 : q_sym(Q, ld, ck, cl);
    };
    for (int i = threadIdx.x; i < m; i += 256) {
        const double hii = h_of(i, i), vi = v_of(i);
        double pii, gii, php, pv;
        if (W) {
            // G = H P: G_ii = sum_j H_ij P_ji;  (P H P)_ii = sum_j P_ij G_ji
            pii = s0 * W[(long)i * m + i];
            gii = 0.0; php = 0.0; pv = 0.0;
            for (int j = 0; j < m; j++) {
                const double pij = s0 * W[(long)i * m + j];
                double gji = 0.0;
                for (int k = 0; k < m; k++) gji = fma(h_of(j, k), s0 * W[(long)k * m + i], gji);
                gii = fma(h_of(i, j), s0 * W[(long)j * m + i], gii);
                php = fma(pij, gji, php);
                pv = fma(pij, v_of(j), pv);
            }
        } else {
            pii = s0 / p.dg_var[b + i];
            gii = hii * pii;
            php = pii * gii;
            pv = pii * vi;
        }
        rl_store(out, n_rows, row0 + b + i, vi, lld[b + i] / s0 - hii, 1.0 - gii, rl_t(pv, pii - php, pii, s2t));
    }
}

// [0] sum r  [1] max |t|  [2] its row (first of equals)  [3] rows with NaN t  [4] min r; one workgroup, fixed order
__global__ __launch_bounds__(256) void rel_summary_kernel(const double *__restrict__ out, long n_rows, double *__restrict__ sum) {
    __shared__ double s_r[256], s_t[256], s_min[256], s_nan[256];
    __shared__ long s_row[256];
    const int tid = threadIdx.x;
    const double *r = out + 2 * n_rows, *t = out + 3 * n_rows;
    double sr = 0.0, mt = -1.0, mr = INFINITY, nn = 0.0;
    long row = -1;
    for (long i = tid; i < n_rows; i += 256) {
        sr += r[i];
        mr = fmin(mr, r[i]);
        const double at = fabs(t[i]);
        if (isnan(at)) nn += 1.0;
        else if (at > mt) { mt = at; row = i; }
    }
    s_r[tid] = sr; s_t[tid] = mt; s_min[tid] = mr; s_nan[tid] = nn; s_row[tid] = row;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            s_r[tid] += s_r[tid + h];
            s_min[tid] = fmin(s_min[tid], s_min[tid + h]);
            s_nan[tid] += s_nan[tid + h];
            const double o = s_t[tid + h];
            const long orow = s_row[tid + h];
            if (o > s_t[tid] || (o == s_t[tid] && orow >= 0 && (s_row[tid] < 0 || orow < s_row[tid]))) { s_t[tid] = o; s_row[tid] = orow; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        sum[0] = s_r[0];
        sum[1] = s_row[0] >= 0 ? s_t[0] : (double)NAN;
        sum[2] = (double)s_row[0];
        sum[3] = s_nan[0];
        sum[4] = n_rows > 0 ? s_min[0] : (double)NAN;
    }
}

}  // namespace jaicov

using namespace jaicov;

namespace {
constexpr size_t RL_BATCH_BYTES = (size_t)1 << 30;   // work buffers of the dense blocks per batch
}  // namespace

// What the three parts of a run share (w frees the run's device buffers on every exit).  pa != nullptr: the table of the image points
// as well (jaicov_rel_run_points); everything it adds is launched after the plain run's kernels of the same group
struct RelRun {
    const QView &v;
    DevBag &w;
    double s2t;
    const RelPointArgs *pa;
    long n_rows;
    double *d_res, *d_pt, *d_dx, *d_v;   // the result [4][n_rows], the table of the image points, the step, the residuals
    int32_t *d_new2old;
};

// the image points with 2 x 2 weights, in chunks of one image
static int rel_run_points2x2(const RelRun &r, const QImageBlocks &ib) {
    const QView &v = r.v;
    const DevProblem &p = *v.p;
    const long n_ip = p.n_ip;
    const hipStream_t st = v.stream;
    std::vector<int32_t> ip_image(n_ip);
    HIPE(*v.err, hipMemcpyAsync(ip_image.data(), p.ip_image, (size_t)n_ip * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPE(*v.err, hipStreamSynchronize(st));
    std::vector<int2> chunks;
    for (long q = 0; q < n_ip;) {
        if (ib.dense[q]) { q++; continue; }
        long en = q;
        while (en < n_ip && !ib.dense[en] && ip_image[en] == ip_image[q] && en - q < RL_PTS) en++;
        chunks.push_back(make_int2((int)q, (int)(en - q)));
        q = en;
    }
    if (chunks.empty()) return JAICOV_OK;
    int2 *d_chunks = nullptr;
    HIPE(*v.err, r.w.alloc(&d_chunks, chunks.size()));
    HIPE(*v.err, hipMemcpyAsync(d_chunks, chunks.data(), chunks.size() * sizeof(int2), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(rel_points_kernel, dim3((unsigned)chunks.size()), dim3(RL_PTS), 0, st, p, d_chunks, v.Q, v.ld, v.rowsA, r.d_v,
                       v.ll_diag, r.d_new2old, v.sigma2, r.s2t, r.n_rows, r.d_res);
    HIPE(*v.err, hipGetLastError());
    if (r.pa) {
        hipLaunchKernelGGL(rel_points_loo_kernel, dim3((unsigned)chunks.size()), dim3(RL_PTS), 0, st, p, d_chunks, v.Q, v.ld, v.rowsA,
                           r.d_v, r.d_new2old, v.sigma2, r.s2t, *r.pa, r.d_pt);
        HIPE(*v.err, hipGetLastError());
    }
    return JAICOV_OK;
}

// the dense image blocks, as many at a time as the work buffers hold
static int rel_run_dense(const RelRun &r, const QImageBlocks &ib) {
    if (ib.blocks.empty()) return JAICOV_OK;
    const QView &v = r.v;
    const DevProblem &p = *v.p;
    const RelPointArgs *pa = r.pa;
    const double s0 = v.sigma2;
    const hipStream_t st = v.stream;
    DevBag &w = r.w;
    const std::vector<int32_t> &bb = *v.blk_ip_begin;
    const int nd = (int)ib.blocks.size();
    const int mpad = (ib.max_m + 127) / 128 * 128;
    const size_t sq = (size_t)mpad * mpad;
    const size_t n_nab = (size_t)mpad, n_part = (size_t)(mpad / 2) * (mpad / RL_RC) * 3;   // per block, table run only
    const size_t per = (3 * sq + 2 * (size_t)mpad * RL_K + (pa ? n_nab + n_part : 0)) * sizeof(double);
    size_t cap = RL_BATCH_BYTES / per;
    if (const char *hook = getenv("JAICOV_REL_BATCH")) cap = std::min<size_t>(cap, (size_t)std::max(1, atoi(hook)));   // test hook
    const int nb = (int)std::max<size_t>(1, std::min<size_t>((size_t)nd, cap));
    int32_t *d_bl = nullptr;
    double *d_H = nullptr, *d_P = nullptr, *d_G = nullptr, *d_L = nullptr, *d_R = nullptr;
    HIPE(*v.err, w.alloc(&d_bl, (size_t)nd));
    HIPE(*v.err, w.alloc(&d_H, nb * sq));
    HIPE(*v.err, w.alloc(&d_P, nb * sq));
    HIPE(*v.err, w.alloc(&d_G, nb * sq));
    HIPE(*v.err, w.alloc(&d_L, (size_t)nb * mpad * RL_K));
    HIPE(*v.err, w.alloc(&d_R, (size_t)nb * mpad * RL_K));
    double *d_nab = nullptr, *d_part = nullptr;
    if (pa) {
        HIPE(*v.err, w.alloc(&d_nab, nb * n_nab));
        HIPE(*v.err, w.alloc(&d_part, nb * n_part));
    }
    HIPE(*v.err, hipMemcpyAsync(d_bl, ib.blocks.data(), (size_t)nd * sizeof(int32_t), hipMemcpyHostToDevice, st));
    for (int b0 = 0; b0 < nd; b0 += nb) {
        const int n = std::min(nb, nd - b0);
        const int32_t *bl = d_bl + b0;
        long tmax = 0;
        for (int k = b0; k < b0 + n; k++) {
            const long mp = bb[ib.blocks[k] + 1] - bb[ib.blocks[k]], nch = (mp + RL_TP - 1) / RL_TP;
            tmax = std::max(tmax, nch * (nch + 1) / 2);
        }
        HIPE(*v.err, hipMemsetAsync(d_H, 0, n * sq * sizeof(double), st));
        hipLaunchKernelGGL(rel_prep_kernel, dim3(mpad / RL_PTS, n), dim3(RL_PTS), 0, st, p, bl, mpad, v.Q, v.ld, v.rowsA, d_L, d_R);
        hipLaunchKernelGGL(rel_pp_kernel, dim3((unsigned)tmax, n), dim3(256), 0, st, p, bl, mpad, v.Q, v.ld, v.rowsA, d_H);
        hipLaunchKernelGGL(rel_pad_kernel, dim3(mpad / 256 + (mpad % 256 ? 1 : 0), mpad, n), dim3(256), 0, st, p, bl, mpad, s0, d_P);
        HIPE(*v.err, hipGetLastError());
        GemmArgs g1{};   // H += [Y | A_s] [A_s | U]'
        g1.A = d_L; g1.lda = RL_K; g1.B = d_R; g1.ldb = RL_K; g1.C = d_H; g1.ldc = mpad;
        g1.M = mpad; g1.N = mpad; g1.K = RL_K; g1.alpha = 1.0; g1.beta = 1.0; g1.kmode = KMODE_FULL;
        g1.strideA = (long)mpad * RL_K; g1.strideB = (long)mpad * RL_K; g1.strideC = (long)sq;
        HIPE(*v.err, gemm_f64(st, LAY_KC, LAY_KC, g1, n));
        GemmArgs g2{};   // G = H P  (P symmetric: P(k, j) = P[j][k])
        g2.A = d_H; g2.lda = mpad; g2.B = d_P; g2.ldb = mpad; g2.C = d_G; g2.ldc = mpad;
        g2.M = mpad; g2.N = mpad; g2.K = mpad; g2.alpha = 1.0; g2.beta = 0.0; g2.kmode = KMODE_FULL;
        g2.strideA = (long)sq; g2.strideB = (long)sq; g2.strideC = (long)sq;
        HIPE(*v.err, gemm_f64(st, LAY_KC, LAY_KC, g2, n));
        hipLaunchKernelGGL(rel_block_kernel, dim3(mpad / 256 + (mpad % 256 ? 1 : 0), n), dim3(256), 0, st, p, bl, mpad, d_H, d_P, d_G,
                           r.d_v, v.ll_diag, r.d_new2old, s0, r.s2t, r.n_rows, r.d_res);
        HIPE(*v.err, hipGetLastError());
        if (pa) {
            const int mp_pad = mpad / 2;
            hipLaunchKernelGGL(rel_block_points_kernel, dim3((mp_pad + 255) / 256, n), dim3(256), 0, st, p, bl, mpad, d_P, d_G, r.d_v,
                               r.d_new2old, r.s2t, *pa, d_nab, r.d_pt);
            hipLaunchKernelGGL(rel_shift_pp_kernel, dim3((unsigned)tmax, n), dim3(256), 0, st, p, bl, mpad, v.Q, v.ld, v.rowsA, d_P,
                               d_nab, d_part);
            hipLaunchKernelGGL(rel_shift_kernel, dim3((mp_pad + RL_PTS - 1) / RL_PTS, n), dim3(RL_PTS), 0, st, p, bl, mpad, v.Q, v.ld,
                               d_P, d_R, d_nab, d_part, r.d_new2old, r.d_pt);
            HIPE(*v.err, hipGetLastError());
        }
    }
    return JAICOV_OK;
}

// scale bars and directly observed groups, then the summary over all rows
static int rel_run_rest(const RelRun &r, RelState *s) {
    const QView &v = r.v;
    const DevProblem &p = *v.p;
    const double s0 = v.sigma2;
    const long n_ip = p.n_ip;
    const hipStream_t st = v.stream;
    double *d_sum = nullptr;
    HIPE(*v.err, r.w.alloc(&d_sum, 5));
    if (p.n_sb > 0) {
        hipLaunchKernelGGL(rel_scalebar_kernel, dim3((p.n_sb + 63) / 64), dim3(64), 0, st, p, v.d_vals, v.Q, v.ld, r.d_dx, s0, r.s2t, 2 * n_ip,
                           r.n_rows, r.d_res);
        HIPE(*v.err, hipGetLastError());
    }
    if (p.n_dg > 0) {
        hipLaunchKernelGGL(rel_direct_kernel, dim3(p.n_dg), dim3(256), 0, st, p, v.d_vals, v.Q, v.ld, r.d_dx, v.ll_diag + 2 * n_ip, s0, r.s2t,
                           2 * n_ip + p.n_sb, r.n_rows, r.d_res);
        HIPE(*v.err, hipGetLastError());
    }
    hipLaunchKernelGGL(rel_summary_kernel, dim3(1), dim3(256), 0, st, r.d_res, r.n_rows, d_sum);
    HIPE(*v.err, hipGetLastError());
    HIPE(*v.err, hipMemcpyAsync(s->summary, d_sum, 5 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPE(*v.err, hipStreamSynchronize(st));
    return JAICOV_OK;
}

static int rel_run_impl(const QView &v, RelState *s, double s2t, const double *dx, const RelPointArgs *pa) {
    const long n_ip = v.p->n_ip, n_rows = s->n_rows;
    const hipStream_t st = v.stream;
    DevBag w;
    s->summary[5] = v.lambda;
    HIPE(*v.err, s->out.reserve(std::max<size_t>(4 * (size_t)n_rows, 1)));   // the result belongs to the state
    if (pa) {
        HIPE(*v.err, s->points.reserve(std::max<size_t>(JAICOV_REL_POINT_COLUMNS * (size_t)n_ip, 1)));
        s->n_points = n_ip;
    }
    if (n_rows == 0) return JAICOV_OK;
    RelRun r{v, w, s2t, pa, n_rows, s->out.get(), s->points.get(), nullptr, nullptr, nullptr};
    HIPE(*v.err, w.alloc(&r.d_dx, (size_t)v.U));
    HIPE(*v.err, w.alloc(&r.d_v, 2 * (size_t)n_ip));
    if (dx) HIPE(*v.err, hipMemcpyAsync(r.d_dx, dx, (size_t)v.U * sizeof(double), hipMemcpyHostToDevice, st));
    else HIPE(*v.err, hipMemsetAsync(r.d_dx, 0, (size_t)v.U * sizeof(double), st));
    if (n_ip > 0) {
        const QImageBlocks ib = q_image_blocks(v);
        if (!ib.new2old.empty()) {
            HIPE(*v.err, w.alloc(&r.d_new2old, (size_t)n_ip));
            HIPE(*v.err, hipMemcpyAsync(r.d_new2old, ib.new2old.data(), (size_t)n_ip * sizeof(int32_t), hipMemcpyHostToDevice, st));
            HIPE(*v.err, hipStreamSynchronize(st));        // ib is a host temporary
        }
        hipLaunchKernelGGL(rel_v_kernel, dim3((unsigned)((n_ip + 255) / 256)), dim3(256), 0, st, *v.p, v.rowsA, v.rowsW, r.d_dx, r.d_v);
        HIPE(*v.err, hipGetLastError());
        TRY(rel_run_points2x2(r, ib));
        TRY(rel_run_dense(r, ib));
    }
    return rel_run_rest(r, s);
}

// The run once state and arguments are accepted: from here on the previous result goes.
static int rel_run_accepted(jaicov_engine *e, const QView &v, double sigma2_test, const double *dx, const RelPointArgs *pa, long rows) {
    HIPE(*v.err, hipSetDevice(v.device));
    int rc = engine_ensure_rows(e);    // the compact rows of the current parameter values
    if (rc != JAICOV_OK) return rc;
    v.slot->rel.reset();
    std::unique_ptr<RelState> s(new RelState());
    s->n_rows = rows;
    rc = rel_run_impl(v, s.get(), sigma2_test, dx, pa);
    if (rc != JAICOV_OK) {
        hipStreamSynchronize(v.stream);
        return rc;
    }
    v.slot->rel = std::move(s);
    return JAICOV_OK;
}

int jaicov::rel_run_plain(jaicov_engine *e, const QView &v, double sigma2_test, const double *dx, long rows) {
    return rel_run_accepted(e, v, sigma2_test, dx, nullptr, rows);
}

// jaicov_rel_run (pa == nullptr) and jaicov_rel_run_points
static int rel_run_checked(jaicov_engine *e, double sigma2_test, const double *dx, const RelPointArgs *pa, int32_t *n_rows,
                           int32_t *n_image_points) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    if (v.sharded) FAIL(*v.err, JAICOV_ERR_UNSUPPORTED, "reliability needs an engine that holds every observation (not a shard)");
    if (!(sigma2_test > 0) || !std::isfinite(sigma2_test)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "sigma2_test must be positive and finite");
    if (pa && (!(pa->lambda0 > 0) || !std::isfinite(pa->lambda0))) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "lambda0 must be positive and finite");
    if (!v.full_q)
        FAIL(*v.err, JAICOV_ERR_BAD_STATE, "no full cofactor matrix: solve with JAICOV_INVERT_FULL or JAICOV_INVERT_FULL_EXPANDED first");
    const DevProblem &p0 = *v.p;
    const long rows = 2 * (long)p0.n_ip + p0.n_sb + p0.n_dg_rows;
    if (rows > INT32_MAX) FAIL(*v.err, JAICOV_ERR_UNSUPPORTED, "more than 2^31 - 1 observation rows");
    TRY(rel_run_accepted(e, v, sigma2_test, dx, pa, rows));
    if (n_rows) *n_rows = (int32_t)rows;
    if (n_image_points) *n_image_points = (int32_t)p0.n_ip;
    return JAICOV_OK;
}

extern "C" int jaicov_rel_run(jaicov_engine *e, double sigma2_test, const double *dx, int32_t *n_rows) {
    return rel_run_checked(e, sigma2_test, dx, nullptr, n_rows, nullptr);
}

extern "C" int jaicov_rel_run_points(jaicov_engine *e, double sigma2_test, const double *dx, double lambda0, double omega, int32_t dof,
                                     int32_t *n_rows, int32_t *n_image_points) {
    const RelPointArgs pa{lambda0, omega, (int)dof};
    return rel_run_checked(e, sigma2_test, dx, &pa, n_rows, n_image_points);
}

static const char RL_NONE[] = "no reliability result: call jaicov_rel_run first";

extern "C" int jaicov_rel_get(jaicov_engine *e, double *vres, double *qvv, double *r, double *t, int32_t n) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    RelState *s = q_result(v, v.slot->rel, RL_NONE);
    if (!s) return JAICOV_ERR_BAD_STATE;
    if (n != s->n_rows) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "n must equal the number of observation rows of the last run");
    if (n == 0) return JAICOV_OK;
    const double *src = s->out.get();
    const size_t col = (size_t)n, bytes = col * sizeof(double);
    return q_download(v, {{vres, src, bytes}, {qvv, src + col, bytes}, {r, src + 2 * col, bytes}, {t, src + 3 * col, bytes}});
}

extern "C" int jaicov_rel_get_points(jaicov_engine *e, double *out, int32_t n) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    RelState *s = q_result(v, v.slot->rel, RL_NONE);
    if (!s) return JAICOV_ERR_BAD_STATE;
    if (s->n_points < 0) FAIL(*v.err, JAICOV_ERR_BAD_STATE, "no table of the image points: the last run was a plain jaicov_rel_run");
    if (n != s->n_points || (n > 0 && !out))
        FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "n must equal the number of image points of the last run, and out must not be NULL");
    if (n == 0) return JAICOV_OK;
    return q_download(v, {{out, s->points.get(), JAICOV_REL_POINT_COLUMNS * (size_t)n * sizeof(double)}});
}

extern "C" int jaicov_rel_summary(jaicov_engine *e, double *out, int32_t n) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    RelState *s = q_result(v, v.slot->rel, RL_NONE);
    if (!s) return JAICOV_ERR_BAD_STATE;
    if ((n != 5 && n != 6) || !out) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "the summary has 5 entries (6 with the damping value)");
    memcpy(out, s->summary, (size_t)n * sizeof(double));
    return JAICOV_OK;
}

extern "C" int jaicov_rel_release(jaicov_engine *e) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    q_release(v, v.slot->rel);
    return JAICOV_OK;
}
