// The object-space reader of the cofactor matrix on the device (include/jaicov_newpoints.h): object points that were not part of the
// adjustment, intersected from measurements in the adjusted images with the adjustment's own rows, their cofactors with the share
// of the cameras and stations gathered from Qxx, and lengths between them with the correlations this sharing causes.
//
//   rows               J and w of every ray come from the adjustment's own rows (pairrows.h) on a problem whose image points are the
//                      call's rays and whose object points are the new points; it reads a private slot vector
//                      [X, Y, Z of the new points | the engine's slots behind its object points], so slot_io, slot_dist and slot_eo
//                      hold as they are.  The formulas are written once.
//   newpt_step_kernel  one Gauss-Newton step, one wave per point, lane k owns ray k: the nine sums of N and n meet in an xor butterfly
//                      (fixed order, the same bits in every lane), every lane solves the 3 x 3 system (wave_solve of wavealg.h), lane 0
//                      moves the point in the private slot vector.  A converged or failed point leaves at once.  The host enqueues
//                      rows and step alternately without a synchronisation; after every fourth step it reads one counter of the
//                      points that still move and stops when there is none.
//   newpt_gain_kernel  at the final X, one wave per point: Q_meas, G_k = Q_meas A_k' P_k per lane into LDS, then F (3 x M, M <= 448, in
//                      LDS) ray by ray in ascending k, lane b taking local column b of the ray: a fixed order without atomics.  Q_sys
//                      reads only the lower part of Q: row a of the point's sorted columns after row a - 1, the lanes over the entries
//                      b <= a of the row (an image's six and a camera's columns are contiguous, so a row is read in short runs).
//   newpt_pair_kernel  one wave per pair: both members' columns and F in LDS, the M_A x M_B gather dealt to the lanes entry by entry,
//                      nine sums through the butterfly, then the 6 x 6 figures of jaicov_prec_lengths.
// Nothing here writes to the cofactor matrix or to any other state of the engine but the buffers of NewPointState.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/jaicov_newpoints.h"
#include "ba_kernels.h"
#include "newpoints.h"
#include "pairrows.h"
#include "qview.h"
#include "status.h"
#include "wavealg.h"

namespace jaicov {

constexpr int NP_S = KC_MAX;                                 // shared local columns of one ray: io (3), eo (6), dist (<= 20)
constexpr int NP_C = JAICOV_NEWPT_MAX_COLS;
constexpr int NP_MOVING = 0, NP_CONVERGED = -1;              // state of a point between the steps; > 0: the status bits of a failure
constexpr int NP_CHECK_EVERY = 4;                            // steps between two reads of the counter of moving points
static_assert(JAICOV_NEWPT_MAX_RAYS == 64, "one lane per ray");
static_assert(NP_S <= 64, "one lane per shared local column of a ray");
static_assert(NP_C >= 64 * 6 + 2 * (3 + MAXD), "64 distinct images and two cameras of the largest size");

// Ray k of the sorted call: A (2 x 3), w, the weights, and its terms of N (6), n (3) and Omega.  n: rays of the call.
struct NpRay {
    double a[2][3], w[2], p11, p12, p22;
};
__device__ __forceinline__ void np_ray(const double *__restrict__ rowsA, const double *__restrict__ rowsW, const double *__restrict__ disp,
                                       long n, long k, double s0, NpRay &r, double *t) {
#pragma unroll
    for (int c = 0; c < 3; c++) { r.a[0][c] = rowsA[(long)(2 * c) * n + k]; r.a[1][c] = rowsA[(long)(2 * c + 1) * n + k]; }
    r.w[0] = rowsW[k]; r.w[1] = rowsW[n + k];
    obs_weight(disp[3 * k], disp[3 * k + 1], disp[3 * k + 2], s0, r.p11, r.p12, r.p22);
    double pa0[3], pa1[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { pa0[c] = r.p11 * r.a[0][c] + r.p12 * r.a[1][c]; pa1[c] = r.p12 * r.a[0][c] + r.p22 * r.a[1][c]; }
    const double pw0 = r.p11 * r.w[0] + r.p12 * r.w[1], pw1 = r.p12 * r.w[0] + r.p22 * r.w[1];
    t[0] = r.a[0][0] * pa0[0] + r.a[1][0] * pa1[0]; t[1] = r.a[0][0] * pa0[1] + r.a[1][0] * pa1[1]; t[2] = r.a[0][0] * pa0[2] + r.a[1][0] * pa1[2];
    t[3] = r.a[0][1] * pa0[1] + r.a[1][1] * pa1[1]; t[4] = r.a[0][1] * pa0[2] + r.a[1][1] * pa1[2]; t[5] = r.a[0][2] * pa0[2] + r.a[1][2] * pa1[2];
    t[6] = r.a[0][0] * pw0 + r.a[1][0] * pw1; t[7] = r.a[0][1] * pw0 + r.a[1][1] * pw1; t[8] = r.a[0][2] * pw0 + r.a[1][2] * pw1;
    t[9] = r.w[0] * pw0 + r.w[1] * pw1;
}

// One Gauss-Newton step of every point that still moves.  q: the problem of the rays (its object points are the new points), vals: the
// private slot vector.  moving (may be null): counts the points that move on after this step.
__global__ __launch_bounds__(64) void newpt_step_kernel(DevProblem q, double *__restrict__ vals, const int32_t *__restrict__ ray_begin,
                                                        const double *__restrict__ rowsA, const double *__restrict__ rowsW,
                                                        const double *__restrict__ disp, double s0, int32_t *__restrict__ state,
                                                        int32_t *__restrict__ iters, int32_t *__restrict__ moving) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (wave_uniform(state[i]) != NP_MOVING) return;
    const int k0 = wave_uniform(ray_begin[i]), m = wave_uniform(ray_begin[i + 1]) - k0;      // 2 <= m <= 64: the host set the state otherwise
    double t[10];
#pragma unroll
    for (int a = 0; a < 10; a++) t[a] = 0.0;
    if (lane < m) {
        NpRay r;
        np_ray(rowsA, rowsW, disp, q.n_ip, k0 + lane, s0, r, t);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int a = 0; a < 9; a++) t[a] += __shfl_xor(t[a], off);
    double dx[3];
    const WaveStatus ws = wave_solve<3>(t, t + 6, dx, nullptr);
    const double SQRT_EPS = sqrt(ldexp(1.0, -53));
    int st = NP_MOVING;
    double X[3];
#pragma unroll
    for (int a = 0; a < 3; a++) X[a] = vals[3 * (long)i + a];
    if (ws == WAVE_SINGULAR) st = JAICOV_NEWPT_SINGULAR;
    else if (ws == WAVE_NOT_FINITE || !(isfinite(dx[0]) && isfinite(dx[1]) && isfinite(dx[2]))) st = JAICOV_NEWPT_NOT_FINITE;
    else {
        const double *X0 = vals + slot_eo(q, q.ip_image[k0]);
        double step = 0.0, size = 0.0;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            X[a] += dx[a];
            step = fmax(step, fabs(dx[a]));
            size = fmax(size, fabs(X[a] - X0[a]));
        }
        if (step <= SQRT_EPS * fmax(1.0, size)) st = NP_CONVERGED;
    }
    if (lane == 0) {
        if (st <= 0)
#pragma unroll
            for (int a = 0; a < 3; a++) vals[3 * (long)i + a] = X[a];
        state[i] = st;
        iters[i] += 1;
        if (st == NP_MOVING && moving) atomicAdd(moving, 1);
    }
}

// The figures of every point at its final X.  flag: what the host knows (PARTIAL, TOO_FEW_RAYS, TOO_MANY); cols [col_begin[i] ..): the
// point's sorted columns; rpos [NP_S] per ray: position of the ray's shared local column in them, -1 without one.  F: [3][M] per point
// from 3 col_begin[i] on.
__global__ __launch_bounds__(64) void newpt_gain_kernel(const double *__restrict__ Q, long ld, DevProblem q, const double *__restrict__ vals,
                                                        const int32_t *__restrict__ ray_begin, const int32_t *__restrict__ col_begin,
                                                        const int32_t *__restrict__ flag, const int32_t *__restrict__ cols,
                                                        const int32_t *__restrict__ rpos, const double *__restrict__ rowsA,
                                                        const double *__restrict__ rowsW, const double *__restrict__ disp, double s0,
                                                        double sigma2, const int32_t *__restrict__ state, double *__restrict__ out,
                                                        double *__restrict__ F, double *__restrict__ ray_w, int32_t *__restrict__ status) {
    __shared__ double Fs[3][NP_C];
    __shared__ double Gs[JAICOV_NEWPT_MAX_RAYS][6];
    __shared__ int cs[NP_C];
    const int i = blockIdx.x, lane = threadIdx.x;
    const long n = q.n_ip;
    const int k0 = wave_uniform(ray_begin[i]), m = wave_uniform(ray_begin[i + 1]) - k0;
    const int c0 = wave_uniform(col_begin[i]), M = wave_uniform(col_begin[i + 1]) - c0;       // <= NP_C: the host stores no columns otherwise
    const int st0 = wave_uniform(state[i]), fl = wave_uniform(flag[i]);
    double *o = out + (size_t)JAICOV_NEWPT_COLUMNS * i;
    auto give_up = [&](int bits) {
        if (lane < JAICOV_NEWPT_COLUMNS) o[lane] = NAN;
        for (int t = lane; t < 2 * m; t += 64) ray_w[2 * (long)k0 + t] = NAN;
        if (lane == 0) status[i] = fl | bits;
    };
    if (st0 > 0) { give_up(st0); return; }
    double t[10];
#pragma unroll
    for (int a = 0; a < 10; a++) t[a] = 0.0;
    NpRay r = {};
    if (lane < m) np_ray(rowsA, rowsW, disp, n, k0 + lane, s0, r, t);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int a = 0; a < 10; a++) t[a] += __shfl_xor(t[a], off);
    double Qm[6];
    const double omega = t[9];
    const WaveStatus ws = wave_solve<3>(t, t + 6, nullptr, Qm);
    if (ws != WAVE_OK) { give_up(ws == WAVE_SINGULAR ? JAICOV_NEWPT_SINGULAR : JAICOV_NEWPT_NOT_FINITE); return; }
    // G_k = Q_meas A_k' P_k (3 x 2) of the lane's ray; the point's columns; F = 0
    if (lane < m) {
        double pa0[3], pa1[3];
#pragma unroll
        for (int c = 0; c < 3; c++) { pa0[c] = r.p11 * r.a[0][c] + r.p12 * r.a[1][c]; pa1[c] = r.p12 * r.a[0][c] + r.p22 * r.a[1][c]; }
        const double q3[3][3] = {{Qm[0], Qm[1], Qm[2]}, {Qm[1], Qm[3], Qm[4]}, {Qm[2], Qm[4], Qm[5]}};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            Gs[lane][2 * a] = (q3[a][0] * pa0[0] + q3[a][1] * pa0[1]) + q3[a][2] * pa0[2];
            Gs[lane][2 * a + 1] = (q3[a][0] * pa1[0] + q3[a][1] * pa1[1]) + q3[a][2] * pa1[2];
        }
    }
    for (int b = lane; b < M; b += 64) {
        cs[b] = cols[c0 + b];
        Fs[0][b] = 0.0; Fs[1][b] = 0.0; Fs[2][b] = 0.0;
    }
    __syncthreads();
    // F[:, pos] += H_k[:, b] = -G_k B_k[:, b], ray after ray; within a ray the positions of the lanes are distinct
    for (int k = 0; k < m; k++) {
        const int pos = lane < NP_S ? rpos[(size_t)NP_S * (k0 + k) + lane] : -1;
        if (pos >= 0) {
            const double bx = rowsA[(long)(2 * (lane + 3)) * n + k0 + k], by = rowsA[(long)(2 * (lane + 3) + 1) * n + k0 + k];
#pragma unroll
            for (int a = 0; a < 3; a++) Fs[a][pos] += -(Gs[k][2 * a] * bx + Gs[k][2 * a + 1] * by);
        }
        __syncthreads();
    }
    // Q_sys over the lower part: s = xx xy xz yy yz zz
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int a = 0; a < M; a++) {
        const double *qrow = Q + (long)cs[a] * ld;
        const double fa0 = Fs[0][a], fa1 = Fs[1][a], fa2 = Fs[2][a];
        for (int b = lane; b <= a; b += 64) {
            const double qv = qrow[cs[b]];
            const double fb0 = Fs[0][b], fb1 = Fs[1][b], fb2 = Fs[2][b];
            if (b == a) {
                s[0] += qv * (fa0 * fa0); s[1] += qv * (fa0 * fa1); s[2] += qv * (fa0 * fa2);
                s[3] += qv * (fa1 * fa1); s[4] += qv * (fa1 * fa2); s[5] += qv * (fa2 * fa2);
            } else {
                s[0] += qv * (2.0 * (fa0 * fb0)); s[1] += qv * (fa0 * fb1 + fb0 * fa1); s[2] += qv * (fa0 * fb2 + fb0 * fa2);
                s[3] += qv * (2.0 * (fa1 * fb1)); s[4] += qv * (fa1 * fb2 + fb1 * fa2); s[5] += qv * (2.0 * (fa2 * fb2));
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int a = 0; a < 6; a++) s[a] += __shfl_xor(s[a], off);
    double X[3], fin = (omega + sigma2) * 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) { X[a] = vals[3 * (long)i + a]; fin += X[a] * 0.0; }
#pragma unroll
    for (int a = 0; a < 6; a++) fin += (Qm[a] + s[a]) * 0.0;
    if (wave_uniform(!(fin == 0.0))) { give_up(JAICOV_NEWPT_NOT_FINITE); return; }
    for (int b = lane; b < M; b += 64) {
        double *f = F + 3 * (size_t)c0;
        f[b] = Fs[0][b]; f[(size_t)M + b] = Fs[1][b]; f[2 * (size_t)M + b] = Fs[2][b];
    }
    if (lane < m) { ray_w[2 * (long)(k0 + lane)] = r.w[0]; ray_w[2 * (long)(k0 + lane) + 1] = r.w[1]; }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) o[a] = X[a];
#pragma unroll
        for (int a = 0; a < 6; a++) { o[3 + a] = Qm[a]; o[9 + a] = Qm[a] + s[a]; }
        o[15] = omega;
        o[16] = (double)(2 * m - 3);
        o[17] = sqrt(sigma2 * fmax(Qm[0] + s[0], 0.0));
        o[18] = sqrt(sigma2 * fmax(Qm[3] + s[3], 0.0));
        o[19] = sqrt(sigma2 * fmax(Qm[5] + s[5], 0.0));
        status[i] = fl | (st0 == NP_MOVING ? JAICOV_NEWPT_NOT_CONVERGED : 0);
    }
}

// Pair j: members pairs[2j], pairs[2j + 1]; >= 0 a new point of the call (out, F, cols, pt_status as newpt_gain_kernel left them),
// -1 - P object point P of the problem p (evals: the engine's slot vector).
__global__ __launch_bounds__(64) void newpt_pair_kernel(const double *__restrict__ Q, long ld, DevProblem p, const double *__restrict__ evals,
                                                        const int32_t *__restrict__ pairs, const int32_t *__restrict__ col_begin,
                                                        const int32_t *__restrict__ cols, const double *__restrict__ out,
                                                        const double *__restrict__ F, const int32_t *__restrict__ pt_status, double sigma2,
                                                        double *__restrict__ pout, int32_t *__restrict__ pstatus) {
    __shared__ double Fm[2][3][NP_C];
    __shared__ int cm[2][NP_C];
    const int j = blockIdx.x, lane = threadIdx.x;
    double X[2][3], QX[2][6];
    int Mm[2], st = 0;
    bool failed = false;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int mem = wave_uniform(pairs[2 * (size_t)j + h]);
        if (mem >= 0) {
            const int ps = wave_uniform(pt_status[mem]);
            if (ps & JAICOV_NEWPT_PARTIAL) st |= JAICOV_NEWPT_PAIR_PARTIAL;
            failed = failed || (ps & JAICOV_NEWPT_FAILED) != 0;
            const int c0 = wave_uniform(col_begin[mem]), M = (ps & JAICOV_NEWPT_FAILED) ? 0 : wave_uniform(col_begin[mem + 1]) - c0;
            Mm[h] = M;
            for (int b = lane; b < M; b += 64) {
                cm[h][b] = cols[c0 + b];
#pragma unroll
                for (int a = 0; a < 3; a++) Fm[h][a][b] = F[3 * (size_t)c0 + (size_t)a * M + b];
            }
            const double *o = out + (size_t)JAICOV_NEWPT_COLUMNS * mem;
#pragma unroll
            for (int a = 0; a < 3; a++) X[h][a] = o[a];
#pragma unroll
            for (int a = 0; a < 6; a++) QX[h][a] = o[9 + a];
        } else {
            const int P = -1 - mem;
            int pc[3];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                pc[a] = p.point_col[3 * (size_t)P + a];
                if (pc[a] < 0) st |= JAICOV_NEWPT_PAIR_PARTIAL;
                X[h][a] = evals[3 * (size_t)P + a];
            }
            Mm[h] = 3;
            if (lane < 3) {
                cm[h][lane] = p.point_col[3 * (size_t)P + lane];
#pragma unroll
                for (int a = 0; a < 3; a++) Fm[h][a][lane] = a == lane ? 1.0 : 0.0;
            }
            QX[h][0] = q_at(Q, ld, pc[0], pc[0]); QX[h][1] = q_at(Q, ld, pc[0], pc[1]); QX[h][2] = q_at(Q, ld, pc[0], pc[2]);
            QX[h][3] = q_at(Q, ld, pc[1], pc[1]); QX[h][4] = q_at(Q, ld, pc[1], pc[2]); QX[h][5] = q_at(Q, ld, pc[2], pc[2]);
        }
    }
    __syncthreads();
    double *o = pout + (size_t)JAICOV_NEWPT_PAIR_COLUMNS * j;
    auto give_up = [&]() {
        if (lane < JAICOV_NEWPT_PAIR_COLUMNS) o[lane] = NAN;
        if (lane == 0) pstatus[j] = st | JAICOV_NEWPT_PAIR_NOT_FINITE;
    };
    if (wave_uniform(failed)) { give_up(); return; }
    // the cross block C = F_A Q[cols_A, cols_B] F_B': entry e = a M_B + b by lane e mod 64
    double c[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    const int MB = Mm[1], cnt = Mm[0] * MB;
    for (int e = lane; e < cnt; e += 64) {
        const int a = e / MB, b = e - a * MB;
        const double qv = q_at(Q, ld, cm[0][a], cm[1][b]);
#pragma unroll
        for (int s = 0; s < 3; s++) {
            const double qf = qv * Fm[1][s][b];
#pragma unroll
            for (int r = 0; r < 3; r++) c[r][s] += Fm[0][r][a] * qf;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int s = 0; s < 3; s++) c[r][s] += __shfl_xor(c[r][s], off);
    // Q6 of (A, B), with and without the cross block; g = [-u, u] (jaicov_prec_lengths)
    double q6[6][6];
    const int tri[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int s = 0; s < 3; s++) {
            q6[r][s] = QX[0][tri[r][s]]; q6[3 + r][3 + s] = QX[1][tri[r][s]];
            q6[r][3 + s] = c[r][s]; q6[3 + s][r] = c[r][s];
        }
    double D[3], g[6];
#pragma unroll
    for (int k = 0; k < 3; k++) D[k] = X[1][k] - X[0][k];
    const double L = sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) { g[3 + k] = D[k] / L; g[k] = -g[3 + k]; }
    double var = 0.0, var0 = 0.0, chk = sigma2 + L;
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double sr = 0.0, s0 = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) {
            chk += q6[r][k];
            sr += q6[r][k] * g[k];
            if ((r < 3) == (k < 3)) s0 += q6[r][k] * g[k];
        }
        var += g[r] * sr;
        var0 += g[r] * s0;
    }
    if (wave_uniform(!isfinite(chk))) { give_up(); return; }
    double sd[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double dv = (q6[k][k] + q6[3 + k][3 + k]) - 2.0 * q6[3 + k][k];
        if (dv < 0.0) st |= JAICOV_NEWPT_PAIR_NEGATIVE;
        sd[k] = sqrt(sigma2 * fmax(dv, 0.0));
    }
    if (lane == 0) {
        o[0] = L;
        if (L == 0.0) {
            st |= JAICOV_NEWPT_PAIR_DEGENERATE;
            o[1] = NAN; o[5] = NAN; o[6] = NAN;
        } else {
            if (var < 0.0) st |= JAICOV_NEWPT_PAIR_NEGATIVE;
            o[1] = sqrt(sigma2 * fmax(var, 0.0)); o[5] = var; o[6] = var0;
        }
        o[2] = sd[0]; o[3] = sd[1]; o[4] = sd[2];
        pstatus[j] = st;
    }
}

// the two tables of the problem the host needs for the column lists, read from the device once per engine
static int newpt_tables(const QView &v, NewPointState *st) {
    if (st->have_tables) return JAICOV_OK;
    st->image_camera.resize((size_t)v.p->n_images);
    st->cam_dist_begin.resize((size_t)v.p->n_cameras + 1);
    TRY(q_download(v, {{st->image_camera.data(), v.p->image_camera, st->image_camera.size() * sizeof(int32_t)},
                       {st->cam_dist_begin.data(), v.p->cam_dist_begin, st->cam_dist_begin.size() * sizeof(int32_t)}}));
    st->have_tables = true;
    return JAICOV_OK;
}

}  // namespace jaicov

using namespace jaicov;

extern "C" int jaicov_newpt_intersect(jaicov_engine *e, double sigma2, int32_t n_points, const int32_t *ray_begin, const int32_t *ray_image,
                                      const double *xy, const double *disp, const double *start, int32_t max_iterations, const int32_t *pairs,
                                      int32_t n_pairs, double *out, int32_t *status, int32_t *iterations, double *ray_w, double *pout,
                                      int32_t *pstatus) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    TRY(q_guard(v, "new points on a sharded engine", "new points need all of Qxx on the device: solve with invert FULL or FULL_EXPANDED first"));
    const DevProblem &p = *v.p;
    const char *what = "new points: NULL argument, a negative count, sigma2 negative or max_iterations < 1";
    if (n_points < 0 || n_pairs < 0 || !(sigma2 >= 0.0) || max_iterations < 1) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, what);
    if (n_points > 0 && (!ray_begin || !start || !out || !status)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, what);
    if (n_pairs > 0 && (!pairs || !pout || !pstatus)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, what);
    long n_rays = 0;
    if (n_points > 0) {
        if (!ranges_ok(n_points, ray_begin)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "new points: ray_begin must ascend from 0");
        n_rays = ray_begin[n_points];
    }
    if (n_rays > 0 && (!ray_image || !xy || !disp)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, what);
    for (long k = 0; k < n_rays; k++)
        if (ray_image[k] < 0 || ray_image[k] >= p.n_images) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "new points: image index out of range");
    if (!dispersions_ok(disp, n_rays)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "new points: var must be positive and |rho| below 1");
    for (int j = 0; j < n_pairs; j++) {
        const long a = pairs[2 * (size_t)j], b = pairs[2 * (size_t)j + 1];
        if (a >= n_points || b >= n_points || -1 - a >= p.n_points || -1 - b >= p.n_points)
            FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "new points: a member of a pair is out of range");
        if (a == b || (a < 0 && b < 0))
            FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "new points: a pair names one member twice, or two points of the block (jaicov_prec_lengths)");
    }
    if (n_points == 0) return JAICOV_OK;
    HIPE(*v.err, hipSetDevice(v.device));
    NewPointState *st = q_state(v.slot->newpt);
    TRY(newpt_tables(v, st));

    // the host's part: every point's sorted columns, every ray's map into them, and what is known before the first step
    const size_t N = (size_t)n_points, R = (size_t)n_rays, G = (size_t)n_pairs;
    const std::vector<int32_t> &sc = *v.slot_col;
    const size_t s_io = 3 * (size_t)p.n_points, s_dist = s_io + 3 * (size_t)p.n_cameras, s_eo = s_dist + (size_t)p.n_dist;
    std::vector<int32_t> col_begin(N + 1, 0), flag(N, 0), cols, rpos(NP_S * R, -1), loc(NP_S), uni, seen_img, seen_cam;
    for (size_t i = 0; i < N; i++) {
        const long k0 = ray_begin[i], m = ray_begin[i + 1] - k0;
        if (m < 2) flag[i] |= JAICOV_NEWPT_TOO_FEW_RAYS;
        if (m > JAICOV_NEWPT_MAX_RAYS) flag[i] |= JAICOV_NEWPT_TOO_MANY;
        uni.clear();
        auto local = [&](long k) {       // the ray's shared local columns: io, eo, the camera's coefficients
            const int image = ray_image[k], cam = st->image_camera[image];
            const int jb = st->cam_dist_begin[cam], ns = 9 + (st->cam_dist_begin[cam + 1] - jb);
            for (int b = 0; b < ns; b++)
                loc[b] = b < 3 ? sc[s_io + 3 * (size_t)cam + b] : b < 9 ? sc[s_eo + 6 * (size_t)image + b - 3] : sc[s_dist + jb + b - 9];
            return ns;
        };
        if (!(flag[i] & JAICOV_NEWPT_FAILED)) {
            // an image's six and a camera's columns go into the list once, however many rays name them: the sort stays short
            seen_img.clear(); seen_cam.clear();
            for (long k = k0; k < k0 + m; k++) {
                const int image = ray_image[k], cam = st->image_camera[image];
                const bool new_img = std::find(seen_img.begin(), seen_img.end(), image) == seen_img.end();
                const bool new_cam = std::find(seen_cam.begin(), seen_cam.end(), cam) == seen_cam.end();
                if (!new_img) continue;
                seen_img.push_back(image);
                if (new_cam) seen_cam.push_back(cam);
                const int ns = local(k);
                for (int b = 0; b < ns; b++) {
                    if (b >= 3 && b < 9 ? false : !new_cam) continue;
                    if (loc[b] < 0) flag[i] |= JAICOV_NEWPT_PARTIAL;
                    else uni.push_back(loc[b]);
                }
            }
            std::sort(uni.begin(), uni.end());
            uni.erase(std::unique(uni.begin(), uni.end()), uni.end());
            if (uni.size() > (size_t)JAICOV_NEWPT_MAX_COLS) {
                flag[i] |= JAICOV_NEWPT_TOO_MANY;
                uni.clear();
            } else {
                for (long k = k0; k < k0 + m; k++) {
                    const int ns = local(k);
                    for (int b = 0; b < ns; b++)
                        if (loc[b] >= 0) rpos[NP_S * (size_t)k + b] = (int32_t)(std::lower_bound(uni.begin(), uni.end(), loc[b]) - uni.begin());
                }
            }
        }
        cols.insert(cols.end(), uni.begin(), uni.end());
        col_begin[i + 1] = (int32_t)cols.size();
    }
    const size_t Cn = cols.size();
    const size_t o_pt = R, o_rb = 2 * R, o_cb = o_rb + N + 1, o_flag = o_cb + N + 1, o_cols = o_flag + N, o_pos = o_cols + Cn,
                 o_pairs = o_pos + NP_S * R, o_state = o_pairs + 2 * G, n_up = o_state + N, o_iter = n_up, o_status = o_iter + N,
                 o_pstatus = o_status + N, o_moving = o_pstatus + G, n_tab = o_moving + 1;
    std::vector<int32_t> tab(n_up, 0);
    for (size_t i = 0; i < N; i++)
        for (long k = ray_begin[i]; k < ray_begin[i + 1]; k++) { tab[k] = ray_image[k]; tab[o_pt + k] = (int32_t)i; }
    std::copy(ray_begin, ray_begin + N + 1, tab.begin() + o_rb);
    std::copy(col_begin.begin(), col_begin.end(), tab.begin() + o_cb);
    std::copy(flag.begin(), flag.end(), tab.begin() + o_flag);
    std::copy(cols.begin(), cols.end(), tab.begin() + o_cols);
    std::copy(rpos.begin(), rpos.end(), tab.begin() + o_pos);
    if (G) std::copy(pairs, pairs + 2 * G, tab.begin() + o_pairs);
    for (size_t i = 0; i < N; i++) tab[o_state + i] = flag[i] & JAICOV_NEWPT_FAILED;         // NP_MOVING without a failure
    // out: out | F | pout | ray_w
    PairRows pr(R);
    const size_t o_F = JAICOV_NEWPT_COLUMNS * N, o_pout = o_F + 3 * Cn, o_rw = o_pout + JAICOV_NEWPT_PAIR_COLUMNS * G, n_out = o_rw + 2 * R;
    const size_t n_shared = (size_t)p.n_slots - s_io, n_vals = 3 * N + n_shared;
    HIPE(*v.err, st->tab.reserve(n_tab));
    HIPE(*v.err, st->rows.reserve(std::max<size_t>(pr.size, 1)));
    HIPE(*v.err, st->vals.reserve(n_vals));
    HIPE(*v.err, st->out.reserve(n_out));
    int32_t *d_tab = st->tab.get();
    double *d_vals = st->vals.get(), *d_out = st->out.get();
    pr.bind(st->rows.get());
    HIPE(*v.err, hipMemcpyAsync(d_tab, tab.data(), n_up * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    HIPE(*v.err, hipMemsetAsync(d_tab + o_iter, 0, N * sizeof(int32_t), v.stream));
    HIPE(*v.err, pr.stage(v.stream, xy, disp, nullptr));
    HIPE(*v.err, hipMemcpyAsync(d_vals, start, 3 * N * sizeof(double), hipMemcpyHostToDevice, v.stream));
    if (n_shared > 0)
        HIPE(*v.err, hipMemcpyAsync(d_vals + 3 * N, v.d_vals + s_io, n_shared * sizeof(double), hipMemcpyDeviceToDevice, v.stream));
    DevProblem q = pr.problem(p, d_tab, d_tab + o_pt);
    q.n_points = n_points; q.n_slots = (int)n_vals;
    QTimer<4> timer(v.stream);
    HIPE(*v.err, timer.arm(st->timing));
    const double s0 = v.sigma2;
    HIPE(*v.err, timer.mark(0));
    st->steps = 0;
    for (int it = 0; it < max_iterations; it++) {
        const bool look = it % NP_CHECK_EVERY == NP_CHECK_EVERY - 1 && it + 1 < max_iterations;
        HIPE(*v.err, pr.rows(v.stream, q, d_vals));
        if (look) HIPE(*v.err, hipMemsetAsync(d_tab + o_moving, 0, sizeof(int32_t), v.stream));
        hipLaunchKernelGGL(newpt_step_kernel, dim3((unsigned)N), dim3(64), 0, v.stream, q, d_vals, d_tab + o_rb, pr.J, pr.w,
                           pr.disp, s0, d_tab + o_state, d_tab + o_iter, look ? d_tab + o_moving : nullptr);
        HIPE(*v.err, hipGetLastError());
        st->steps++;
        if (look) {
            int32_t moving = 0;
            TRY(q_download(v, {{&moving, d_tab + o_moving, sizeof(int32_t)}}));
            if (moving == 0) break;
        }
    }
    HIPE(*v.err, pr.rows(v.stream, q, d_vals));
    HIPE(*v.err, timer.mark(1));
    hipLaunchKernelGGL(newpt_gain_kernel, dim3((unsigned)N), dim3(64), 0, v.stream, v.Q, v.ld, q, d_vals, d_tab + o_rb, d_tab + o_cb, d_tab + o_flag,
                       d_tab + o_cols, d_tab + o_pos, pr.J, pr.w, pr.disp, s0, sigma2, d_tab + o_state, d_out, d_out + o_F,
                       d_out + o_rw, d_tab + o_status);
    HIPE(*v.err, hipGetLastError());
    HIPE(*v.err, timer.mark(2));
    if (G > 0) {
        hipLaunchKernelGGL(newpt_pair_kernel, dim3((unsigned)G), dim3(64), 0, v.stream, v.Q, v.ld, p, v.d_vals, d_tab + o_pairs, d_tab + o_cb,
                           d_tab + o_cols, d_out, d_out + o_F, d_tab + o_status, sigma2, d_out + o_pout, d_tab + o_pstatus);
        HIPE(*v.err, hipGetLastError());
    }
    HIPE(*v.err, timer.mark(3));
    TRY(q_download(v, {{out, d_out, JAICOV_NEWPT_COLUMNS * N * sizeof(double)},
                       {status, d_tab + o_status, N * sizeof(int32_t)},
                       {iterations, d_tab + o_iter, N * sizeof(int32_t)},
                       {ray_w, d_out + o_rw, 2 * R * sizeof(double)},
                       {pout, d_out + o_pout, JAICOV_NEWPT_PAIR_COLUMNS * G * sizeof(double)},
                       {pstatus, d_tab + o_pstatus, G * sizeof(int32_t)}}));
    HIPE(*v.err, timer.read(st->ms));
    return JAICOV_OK;
}

// The hook of scripts/newpoint_bench.py: on != 0 makes the following calls time their kernels by events on the engine's stream;
// ms[0 .. 2]: what the Gauss-Newton loop (rows and steps, the reads of the counter included), newpt_gain_kernel and
// newpt_pair_kernel of the last call took; steps (may be NULL): the steps that call enqueued.
extern "C" int jaicov_debug_newpt_timing(jaicov_engine *e, int on, float *ms, int32_t *steps) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    NewPointState *st = on ? q_state(v.slot->newpt) : v.slot->newpt.get();       // asking an engine that never ran the call allocates nothing
    if (st) st->timing = on != 0;
    if (ms)
        for (int k = 0; k < 3; k++) ms[k] = st ? st->ms[k] : 0.f;
    if (steps) *steps = st ? st->steps : 0;
    return JAICOV_OK;
}
