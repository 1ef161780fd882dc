// simil.hip -- absolute orientation of many models in one launch (include/jaicov_simil.h): the spatial similarity transformation
// between two sets of the same points, and the call that carries a model's points and orientations into the target frame.  The calls
// have no counterpart in the reference; the rotation is that of derivation/PartialDerivativeFactory.java (PDF), the preconditioning
// that of NormalEquationSystem.java (NES).
//
// One wave (one workgroup of 64 lanes) works one model; the means, the closed start, every Gauss-Newton step, the evaluation and the
// rejection rounds all run inside it, with no host round trip.  The layout is that of relorient.hip:
//   Sums.  Lane l takes points l, l + 64, ... and keeps the partial sums of the pass; the lanes are combined by an xor butterfly,
//   whose order is fixed and which leaves the same bits in every lane.  What follows is therefore wave-uniform: the sums and the
//   model's state (T_c, m, angles, R, sbar, dbar) lie in LDS, where every lane stores the same words; every lane runs the small
//   algebra on them (Jacobi of order 3 and Cholesky of order 7 in registers), and every branch on its outcome is taken by the whole
//   wave.  Points are staged SIMIL_CHUNK at a time in LDS with their cofactors; a model with at most SIMIL_CHUNK keeps them resident.
//   One pass routine serves every kind of sum (means, closed start, step, evaluation), so that it is compiled once.
// Floating-point contraction is off in this file: every product and sum is rounded on its own, as tests/similarity_reference.py rounds it.
#include <hip/hip_runtime.h>

#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jaicov_simil.h"
#include "batchcall.h"
#include "simil.h"
#include "wavealg.h"

#pragma clang fp contract(off)

namespace jaicov {
namespace {

enum { SM_MEAN = 0, SM_START, SM_STEP, SM_FINAL };

// the solves' statuses (wavealg.h) go out as the call's own
static_assert(JAICOV_SIMIL_OK == WAVE_OK && JAICOV_SIMIL_SINGULAR == WAVE_SINGULAR && JAICOV_SIMIL_NOT_FINITE == WAVE_NOT_FINITE,
              "wavealg.h returns the public status values");

// where the state of a model lies in LDS (doubles): every lane stores the same words there and reads them back
enum { SM_TC = 0, SM_M = 3, SM_ANG = 4, SM_R = 7, SM_SO = 16, SM_CO = 17, SM_SB = 18, SM_DB = 21, SM_NSTATE = 24 };

// the three columns of d(m R x)/d(omega, phi, kappa) at r = R x (PDF:125-135 is Rx(omega) Ry(phi) Rz(kappa))
__device__ inline void sm_angle_columns(const double *R, double so, double co, double m, double x0, double x1, const double *r,
                                        double *ao, double *ap, double *ak) {
    ao[0] = 0.0; ao[1] = -(m * r[2]); ao[2] = m * r[1];
    ap[0] = m * (co * r[2] - so * r[1]); ap[1] = m * (so * r[0]); ap[2] = -(m * (co * r[0]));
#pragma unroll
    for (int i = 0; i < 3; i++) ak[i] = m * (R[3 * i + 1] * x0 - R[3 * i] * x1);
}

__global__ __launch_bounds__(SIMIL_LANES) void simil_models_kernel(const int32_t *__restrict__ pt_begin, const double *__restrict__ src,
                                                         const double *__restrict__ dst, const double *__restrict__ cof_src,
                                                         const double *__restrict__ cof_dst, const double *__restrict__ start,
                                                         int max_iter, double thr2, int min_points, double *__restrict__ out,
                                                         int32_t *__restrict__ outcome, uint8_t *used, double *__restrict__ pt_q) {
    __shared__ double ss[3][SIMIL_CHUNK], sd[3][SIMIL_CHUNK], sqs[6][SIMIL_CHUNK], sqd[6][SIMIL_CHUNK];
    __shared__ uint8_t sused[SIMIL_CHUNK];
    // The sums of the last pass, the same in every lane after the butterfly (sA), and the model's state (sP).  The workgroup is one
    // wave, and all of this rests on it: every lane stores the same value to the same word and reads it back, and no barrier stands
    // between such a store and the reads that follow, because the LDS operations of one wave complete in order.
    static_assert(SIMIL_LANES == 64, "one wave per model: the uniform state in LDS relies on it");
    __shared__ double sA[SIMIL_NACC], sP[SM_NSTATE];
    // the model's whole-number state, the same in every lane: in LDS like the rest of the uniform state (relorient.hip)
    __shared__ int sI[8];
    const int g = blockIdx.x, lane = threadIdx.x;
    const long k0 = pt_begin[g];
    const int m = pt_begin[g + 1] - pt_begin[g];
    double *og = out + (long)JAICOV_SIMIL_OUT_PER_MODEL * g;
    int &iters = sI[0], &nused = sI[1], &kind = sI[2], &cst = sI[3], &it = sI[4], &new_state = sI[5], &centre = sI[6], &failed = sI[7];
    iters = 0; nused = m; kind = JAICOV_SIMIL_START_GIVEN; cst = JAICOV_SIMIL_NOT_CONVERGED; it = 0; new_state = 0; centre = 0;
    bool given = start != nullptr;
#pragma unroll
    for (int k = 0; k < 7; k++) given = given && isfinite(start[7L * g + k]);
    given = wave_uniform(given);
    const bool resident = m <= SIMIL_CHUNK;
    const bool has_qs = cof_src != nullptr;
    // points c0 .. c0 + nc - 1 into LDS with their cofactors (cof_src == NULL: 0, cof_dst == NULL: I)
    auto stage = [&](int c0, int nc) {
        __syncthreads();
        for (int t = lane; t < nc; t += 64) {
            const long k = k0 + c0 + t;
#pragma unroll
            for (int i = 0; i < 3; i++) { ss[i][t] = src[3 * k + i]; sd[i][t] = dst[3 * k + i]; }
#pragma unroll
            for (int i = 0; i < 6; i++) {
                sqs[i][t] = cof_src ? cof_src[6 * k + i] : 0.0;
                sqd[i][t] = cof_dst ? cof_dst[6 * k + i] : (i == 0 || i == 3 || i == 5 ? 1.0 : 0.0);
            }
            sused[t] = used[k];
        }
        __syncthreads();
    };

    // one pass over the model's points: the sums of the used ones, combined over the lanes, into sA; SM_FINAL also writes q of every
    // point and finds the used one with the largest q (the lowest index among equal values).  bad: a used point whose C is not positive.
    auto pass = [&](int mode, double &qmax, int &qidx, int &bad) {
        double acc[SIMIL_NACC];
#pragma unroll
        for (int a = 0; a < SIMIL_NACC; a++) acc[a] = 0.0;
        qmax = -1.0; qidx = INT_MAX; bad = 0;
        const bool want_q = mode == SM_FINAL && pt_q;
        for (int c0 = 0; c0 < m; c0 += SIMIL_CHUNK) {
            const int nc = min(SIMIL_CHUNK, m - c0);
            if (!resident) stage(c0, nc);
            for (int t = lane; t < nc; t += 64) {
                const bool in = sused[t] != 0;
                if (!in && !want_q) continue;
                if (mode == SM_MEAN) {
#pragma unroll
                    for (int i = 0; i < 3; i++) { acc[i] += ss[i][t]; acc[3 + i] += sd[i][t]; }
                    continue;
                }
                const double *sb = sP + SM_SB;
                const double x0 = ss[0][t] - sb[0], x1 = ss[1][t] - sb[1], x2 = ss[2][t] - sb[2];
                if (mode == SM_START) {
                    const double *db = sP + SM_DB;
                    const double y[3] = {sd[0][t] - db[0], sd[1][t] - db[1], sd[2][t] - db[2]};
#pragma unroll
                    for (int i = 0; i < 3; i++) { acc[3 * i] += y[i] * x0; acc[3 * i + 1] += y[i] * x1; acc[3 * i + 2] += y[i] * x2; }
                    acc[9] += x0 * x0 + x1 * x1 + x2 * x2;
                    continue;
                }
                // the condition at the unknowns
                const double *R = sP + SM_R, *tc = sP + SM_TC;
                const double sc = sP[SM_M], so = sP[SM_SO], co = sP[SM_CO];
                double r[3], e[3], c[6];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    r[i] = R[3 * i] * x0 + R[3 * i + 1] * x1 + R[3 * i + 2] * x2;
                    e[i] = (sd[i][t] - tc[i]) - sc * r[i];
                }
#pragma unroll
                for (int i = 0; i < 6; i++) c[i] = sqd[i][t];
                if (has_qs) {                             // C = Q_d + m^2 (R Q_s) R'
                    const double m2 = sc * sc;
                    const double Q[9] = {sqs[0][t], sqs[1][t], sqs[2][t], sqs[1][t], sqs[3][t], sqs[4][t], sqs[2][t], sqs[4][t], sqs[5][t]};
                    double B[9];
#pragma unroll
                    for (int i = 0; i < 3; i++)
#pragma unroll
                        for (int j = 0; j < 3; j++) B[3 * i + j] = R[3 * i] * Q[j] + R[3 * i + 1] * Q[3 + j] + R[3 * i + 2] * Q[6 + j];
#pragma unroll
                    for (int i = 0; i < 3; i++)
#pragma unroll
                        for (int j = i; j < 3; j++)
                            c[tri_ix<3>(i, j)] += m2 * (B[3 * i] * R[3 * j] + B[3 * i + 1] * R[3 * j + 1] + B[3 * i + 2] * R[3 * j + 2]);
                }
                // P = adj(C) / det(C)
                double p[6];
                p[0] = c[3] * c[5] - c[4] * c[4]; p[1] = c[2] * c[4] - c[1] * c[5]; p[2] = c[1] * c[4] - c[2] * c[3];
                p[3] = c[0] * c[5] - c[2] * c[2]; p[4] = c[1] * c[2] - c[0] * c[4]; p[5] = c[0] * c[3] - c[1] * c[1];
                const double det = c[0] * p[0] + c[1] * p[1] + c[2] * p[2];
                const bool positive = c[0] > 0.0 && p[5] > 0.0 && det > 0.0;
                const double idet = 1.0 / det;
#pragma unroll
                for (int i = 0; i < 6; i++) p[i] = p[i] * idet;
                const double pe[3] = {p[0] * e[0] + p[1] * e[1] + p[2] * e[2], p[1] * e[0] + p[3] * e[1] + p[4] * e[2],
                                      p[2] * e[0] + p[4] * e[1] + p[5] * e[2]};
                const double q = e[0] * pe[0] + e[1] * pe[1] + e[2] * pe[2];
                if (want_q) pt_q[k0 + c0 + t] = q;
                if (!in) continue;
                if (!positive) bad = 1;
                double a[4][3], pa[4][3];                 // the columns of A after the unit matrix, and P times them
#pragma unroll
                for (int i = 0; i < 3; i++) a[0][i] = r[i];
                sm_angle_columns(R, so, co, sc, x0, x1, r, a[1], a[2], a[3]);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    pa[k][0] = p[0] * a[k][0] + p[1] * a[k][1] + p[2] * a[k][2];
                    pa[k][1] = p[1] * a[k][0] + p[3] * a[k][1] + p[4] * a[k][2];
                    pa[k][2] = p[2] * a[k][0] + p[4] * a[k][1] + p[5] * a[k][2];
                }
#pragma unroll
                for (int i = 0; i < 3; i++) {
#pragma unroll
                    for (int j = i; j < 3; j++) acc[tri_ix<7>(i, j)] += p[tri_ix<3>(i, j)];
#pragma unroll
                    for (int k = 0; k < 4; k++) acc[tri_ix<7>(i, 3 + k)] += pa[k][i];
                    acc[28 + i] += pe[i];
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
#pragma unroll
                    for (int l = k; l < 4; l++) acc[tri_ix<7>(3 + k, 3 + l)] += a[k][0] * pa[l][0] + a[k][1] * pa[l][1] + a[k][2] * pa[l][2];
                    acc[31 + k] += a[k][0] * pe[0] + a[k][1] * pe[1] + a[k][2] * pe[2];
                }
                acc[35] += q;
                if (mode == SM_FINAL && q > qmax) { qmax = q; qidx = c0 + t; }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int a = 0; a < SIMIL_NACC_START; a++) acc[a] += __shfl_xor(acc[a], off);
            if (mode == SM_STEP || mode == SM_FINAL) {
#pragma unroll
                for (int a = SIMIL_NACC_START; a < SIMIL_NACC; a++) acc[a] += __shfl_xor(acc[a], off);
            }
            wave_argmax_combine(qmax, qidx, off);
            bad |= __shfl_xor(bad, off);
        }
        __syncthreads();                                  // the last reads of the state and of the sums before
#pragma unroll
        for (int a = 0; a < SIMIL_NACC; a++) sA[a] = acc[a];
        __syncthreads();
    };

    const double SQRT_EPS = sqrt(ldexp(1.0, -53));
    double qmax = -1.0;
    int qidx = INT_MAX, bad = 0;
    failed = m < 3 ? JAICOV_SIMIL_TOO_FEW_POINTS : -1;
    if (wave_uniform(resident && failed < 0)) stage(0, m);
    // one loop over the passes of all rounds, so that the pass and the rotation are compiled once:
    // MEAN (-> START) -> STEP ... STEP -> FINAL (-> MEAN of the next round)
    int mode = SM_MEAN;
    while (wave_uniform(failed < 0)) {
        mode = wave_uniform(mode);
        if (wave_uniform(new_state != 0)) {
            double so, co, sp, cp, sk, ck;
            wave_sincos3(lane, sP[SM_ANG], sP[SM_ANG + 1], sP[SM_ANG + 2], so, co, sp, cp, sk, ck);
            double *R = sP + SM_R;
            rotation_opk(so, co, sk, ck, sp, cp, R);
            sP[SM_SO] = so; sP[SM_CO] = co;
            if (wave_uniform(centre != 0)) {              // given start values: T_c = T + m R sbar
                const double *sb = sP + SM_SB;
                const double sc = sP[SM_M];
#pragma unroll
                for (int i = 0; i < 3; i++) sP[SM_TC + i] = sP[SM_TC + i] + sc * (R[3 * i] * sb[0] + R[3 * i + 1] * sb[1] + R[3 * i + 2] * sb[2]);
                centre = 0;
            }
            new_state = 0;
        }
        pass(mode, qmax, qidx, bad);
        if (mode == SM_MEAN) {
            if (wave_uniform(nused < 3)) {
                failed = JAICOV_SIMIL_TOO_FEW_POINTS;
            } else {
                const double n = (double)nused;
                double z = 0.0;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const double sb = sA[i] / n, db = sA[3 + i] / n;
                    sP[SM_SB + i] = sb; sP[SM_DB + i] = db;
                    z += sb * 0.0; z += db * 0.0;
                }
                if (wave_uniform(z != 0.0)) {
                    failed = JAICOV_SIMIL_NOT_FINITE;
                } else if (given) {
                    const double *s = start + 7L * g;
#pragma unroll
                    for (int k = 0; k < 7; k++) sP[SM_TC + k] = s[k];
                    if (wave_uniform(!(s[3] > 0.0))) failed = JAICOV_SIMIL_SINGULAR;
                    kind = JAICOV_SIMIL_START_GIVEN;
                    new_state = 1; centre = 1; cst = JAICOV_SIMIL_NOT_CONVERGED; it = 0;
                    mode = SM_STEP;
                } else {
                    mode = SM_START;
                }
            }
        } else if (mode == SM_START) {
            double M[9], S[6], lam[3], V[9];
            double z = 0.0;
#pragma unroll
            for (int k = 0; k < 9; k++) { M[k] = sA[k]; z += M[k] * 0.0; }
            const double s2 = sA[9];
            z += s2 * 0.0;
            if (wave_uniform(z != 0.0)) {
                failed = JAICOV_SIMIL_NOT_FINITE;
            } else {
                S[0] = M[0] * M[0] + M[3] * M[3] + M[6] * M[6]; S[1] = M[0] * M[1] + M[3] * M[4] + M[6] * M[7];
                S[2] = M[0] * M[2] + M[3] * M[5] + M[6] * M[8]; S[3] = M[1] * M[1] + M[4] * M[4] + M[7] * M[7];
                S[4] = M[1] * M[2] + M[4] * M[5] + M[7] * M[8]; S[5] = M[2] * M[2] + M[5] * M[5] + M[8] * M[8];
                wave_eigen3<SIMIL_SWEEPS3>(S, lam, V);
                if (wave_uniform(!(lam[1] > SQRT_EPS * lam[0]))) {
                    failed = JAICOV_SIMIL_SINGULAR;
                } else {
                    const double *v1 = V, *v2 = V + 3, *v3 = V + 6;
                    double u1[3], u2[3], u3[3], w[3], R[9];
#pragma unroll
                    for (int i = 0; i < 3; i++) {
                        u1[i] = M[3 * i] * v1[0] + M[3 * i + 1] * v1[1] + M[3 * i + 2] * v1[2];
                        w[i] = M[3 * i] * v2[0] + M[3 * i + 1] * v2[1] + M[3 * i + 2] * v2[2];
                    }
                    const double l1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
#pragma unroll
                    for (int i = 0; i < 3; i++) u1[i] = u1[i] / l1;
                    const double h = u1[0] * w[0] + u1[1] * w[1] + u1[2] * w[2];
#pragma unroll
                    for (int i = 0; i < 3; i++) u2[i] = w[i] - h * u1[i];
                    const double l2 = sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]);
#pragma unroll
                    for (int i = 0; i < 3; i++) u2[i] = u2[i] / l2;
                    u3[0] = u1[1] * u2[2] - u1[2] * u2[1]; u3[1] = u1[2] * u2[0] - u1[0] * u2[2]; u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
#pragma unroll
                    for (int i = 0; i < 3; i++)
#pragma unroll
                        for (int j = 0; j < 3; j++) R[3 * i + j] = u1[i] * v1[j] + u2[i] * v2[j] + u3[i] * v3[j];
                    double tr = 0.0;
#pragma unroll
                    for (int k = 0; k < 9; k++) tr += R[k] * M[k];
                    const double sc = tr / s2;
                    wave_angles(lane, R[5], R[8], R[1], R[0], R[2], sP + SM_ANG);
                    sP[SM_M] = sc;
#pragma unroll
                    for (int i = 0; i < 3; i++) sP[SM_TC + i] = sP[SM_DB + i];
                    if (wave_uniform(!(sc > 0.0))) failed = JAICOV_SIMIL_SINGULAR;
                    kind = JAICOV_SIMIL_START_CLOSED;
                    new_state = 1; centre = 0; cst = JAICOV_SIMIL_NOT_CONVERGED; it = 0;
                    mode = SM_STEP;
                }
            }
        } else if (mode == SM_STEP) {
            if (wave_uniform(bad != 0)) {
                failed = JAICOV_SIMIL_SINGULAR;
            } else {
                double A[28], b[7], dx[7];
#pragma unroll
                for (int k = 0; k < 28; k++) A[k] = sA[k];
#pragma unroll
                for (int k = 0; k < 7; k++) b[k] = sA[28 + k];
                int st = wave_solve<7>(A, b, dx, nullptr);
                iters++;
                if (st == JAICOV_SIMIL_OK) {
                    double z = 0.0;                       // NaN unless every value is finite
#pragma unroll
                    for (int k = 0; k < 7; k++) z += dx[k] * 0.0;
                    if (wave_uniform(z != 0.0)) st = JAICOV_SIMIL_NOT_FINITE;
                }
                if (st != JAICOV_SIMIL_OK) {
                    failed = st;
                } else {
                    double step = 0.0;
#pragma unroll
                    for (int k = 0; k < 7; k++) { sP[SM_TC + k] = sP[SM_TC + k] + dx[k]; step = fmax(step, fabs(dx[k])); }
                    new_state = 1;
                    if (wave_uniform(!(sP[SM_M] > 0.0))) failed = JAICOV_SIMIL_SINGULAR;
                    else if (wave_uniform(step <= SQRT_EPS)) { cst = JAICOV_SIMIL_OK; mode = SM_FINAL; }
                    else if (wave_uniform(++it >= max_iter)) mode = SM_FINAL;
                }
            }
        } else {                                          // SM_FINAL: Q is taken from these sums after the loop
            if (wave_uniform(bad != 0)) {
                failed = JAICOV_SIMIL_SINGULAR;
            } else if (wave_uniform(thr2 > 0.0 && nused > min_points && qmax > thr2 && qidx < m)) {
                if (lane == 0) { used[k0 + qidx] = 0; if (resident) sused[qidx] = 0; }
                __syncthreads();                          // the withdrawal is visible to every lane before the next pass reads it
                nused--;
                mode = SM_MEAN;
            } else {
                break;
            }
        }
    }
    double o[JAICOV_SIMIL_OUT_PER_MODEL];
    if (wave_uniform(failed < 0)) {
        double A[28], b[7], Q[28];
#pragma unroll
        for (int k = 0; k < 28; k++) A[k] = sA[k];
#pragma unroll
        for (int k = 0; k < 7; k++) b[k] = sA[28 + k];
        const int se = wave_solve<7>(A, b, nullptr, Q);
        if (se != JAICOV_SIMIL_OK) failed = se;
        // T = T_c - m R sbar, and J = I except dT/dm = -R sbar, dT/dangle = -m dR/dangle sbar: G holds these four columns
        const double *R = sP + SM_R, *sb = sP + SM_SB;
        const double sc = sP[SM_M];
        double rb[3], col[4][3], G[3][4], H[3][4];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            rb[i] = R[3 * i] * sb[0] + R[3 * i + 1] * sb[1] + R[3 * i + 2] * sb[2];
            o[i] = sP[SM_TC + i] - sc * rb[i];
            col[0][i] = rb[i];
        }
        sm_angle_columns(R, sP[SM_SO], sP[SM_CO], sc, sb[0], sb[1], rb, col[1], col[2], col[3]);
#pragma unroll
        for (int k = 3; k < 7; k++) o[k] = sP[SM_TC + k];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 4; k++) G[i][k] = -col[k][i];
#pragma unroll
        for (int i = 0; i < 3; i++)                       // H = Q_tp + G Q_pp
#pragma unroll
            for (int k = 0; k < 4; k++) {
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < 4; l++) s += G[i][l] * Q[l <= k ? tri_ix<7>(3 + l, 3 + k) : tri_ix<7>(3 + k, 3 + l)];
                H[i][k] = Q[tri_ix<7>(i, 3 + k)] + s;
            }
#pragma unroll
        for (int i = 0; i < 7; i++)
#pragma unroll
            for (int j = i; j < 7; j++) {
                double v;
                if (j < 3) {                              // Q_tt + G Q_pt + H G'
                    double s = 0.0, t = 0.0;
#pragma unroll
                    for (int l = 0; l < 4; l++) s += G[i][l] * Q[tri_ix<7>(j, 3 + l)];
#pragma unroll
                    for (int l = 0; l < 4; l++) t += H[i][l] * G[j][l];
                    v = (Q[tri_ix<7>(i, j)] + s) + t;
                } else if (i < 3) {
                    v = H[i][j - 3];
                } else {
                    v = Q[tri_ix<7>(i, j)];
                }
                o[7 + tri_ix<7>(i, j)] = v;
            }
        o[35] = sA[35];
        double z = 0.0;
#pragma unroll
        for (int k = 0; k < JAICOV_SIMIL_OUT_PER_MODEL; k++) z += o[k] * 0.0;
        if (wave_uniform(failed < 0 && z != 0.0)) failed = JAICOV_SIMIL_NOT_FINITE;
    }
    if (wave_uniform(failed >= 0)) {                      // start kind 0
        wave_fail_item<3>(lane, og, JAICOV_SIMIL_OUT_PER_MODEL, outcome, g, wave_uniform(failed), iters, k0, m, used, pt_q);
        return;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < JAICOV_SIMIL_OUT_PER_MODEL; k++) og[k] = o[k];
        outcome[3L * g] = cst;
        outcome[3L * g + 1] = iters;
        outcome[3L * g + 2] = kind;
    }
}

// one thread per item: the points of all models first, then their orientations.  item_model: the model of every item.
constexpr int SIMIL_APPLY_THREADS = 256;
__global__ __launch_bounds__(SIMIL_APPLY_THREADS) void simil_apply_kernel(long n_pts, long n_img, const double *__restrict__ par,
                                                                          const int32_t *__restrict__ pt_model,
                                                                          const int32_t *__restrict__ img_model, const double *xyz,
                                                                          const double *cof, const double *eo, double *xyz_out,
                                                                          double *cof_out, double *eo_out) {
    const long n = n_pts + n_img, stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const bool point = i < n_pts;
        const long k = point ? i : i - n_pts;
        const double *p = par + 7L * (point ? pt_model[k] : img_model[k]);
        double z = 0.0;
#pragma unroll
        for (int j = 0; j < 7; j++) z += p[j] * 0.0;
        const bool finite = z == 0.0;
        double so, co, sp, cp, sk, ck, R[9];
        sincos(p[4], &so, &co); sincos(p[5], &sp, &cp); sincos(p[6], &sk, &ck);
        rotation_opk(so, co, sk, ck, sp, cp, R);
        const double sc = p[3];
        const double *x = point ? xyz + 3 * k : eo + 6 * k;
        double *y = point ? xyz_out + 3 * k : eo_out + 6 * k;
        const double x0 = x[0], x1 = x[1], x2 = x[2];
#pragma unroll
        for (int j = 0; j < 3; j++) y[j] = finite ? p[j] + sc * (R[3 * j] * x0 + R[3 * j + 1] * x1 + R[3 * j + 2] * x2) : NAN;
        if (point) {
            if (cof_out) {
                const double *q = cof + 6 * k;
                const double Q[9] = {q[0], q[1], q[2], q[1], q[3], q[4], q[2], q[4], q[5]};
                const double m2 = sc * sc;
                double B[9];
#pragma unroll
                for (int a = 0; a < 3; a++)
#pragma unroll
                    for (int b = 0; b < 3; b++) B[3 * a + b] = R[3 * a] * Q[b] + R[3 * a + 1] * Q[3 + b] + R[3 * a + 2] * Q[6 + b];
#pragma unroll
                for (int a = 0; a < 3; a++)
#pragma unroll
                    for (int b = a; b < 3; b++)
                        cof_out[6 * k + tri_ix<3>(a, b)] =
                            finite ? m2 * (B[3 * a] * R[3 * b] + B[3 * a + 1] * R[3 * b + 1] + B[3 * a + 2] * R[3 * b + 2]) : NAN;
            }
        } else {
            double sk2, ck2, Ri[9], Rn[9];
            const double a0 = x[3], a1 = x[4], a2 = x[5];
            sincos(a0, &so, &co); sincos(a1, &sp, &cp); sincos(a2, &sk2, &ck2);
            rotation_opk(so, co, sk2, ck2, sp, cp, Ri);
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) Rn[3 * a + b] = R[3 * a] * Ri[b] + R[3 * a + 1] * Ri[3 + b] + R[3 * a + 2] * Ri[6 + b];
            y[3] = finite ? atan2(-Rn[5], Rn[8]) : NAN;
            y[4] = finite ? asin(fmin(1.0, fmax(-1.0, Rn[2]))) : NAN;
            y[5] = finite ? atan2(-Rn[1], Rn[0]) : NAN;
        }
    }
}

// cof (may be NULL) holds n 3 x 3 cofactor matrices (qXX qXY qXZ qYY qYZ qZZ): every diagonal entry is >= 0, or > 0 where strict
inline bool cofactors_ok(const double *cof, long n, bool strict) {
    if (!cof) return true;
    for (long k = 0; k < n; k++)
        for (int d : {0, 3, 5}) {
            const double v = cof[6 * k + d];
            if (strict ? !(v > 0.0) : !(v >= 0.0)) return false;
        }
    return true;
}

// the model of every item of n ranges
inline std::vector<int32_t> models_of(int32_t n, const int32_t *begin) {
    std::vector<int32_t> model(begin ? (size_t)begin[n] : 0);
    for (int32_t g = 0; begin && g < n; g++)
        for (int32_t k = begin[g]; k < begin[g + 1]; k++) model[k] = g;
    return model;
}

}  // namespace
}  // namespace jaicov

using namespace jaicov;

extern "C" int jaicov_simil_models(int32_t n_models, const int32_t *pt_begin, const double *src, const double *dst, const double *cof_src,
                                   const double *cof_dst, const double *start, int32_t max_iterations, double reject_threshold,
                                   int32_t min_points, double *out, int32_t *status, int32_t *iterations, int32_t *start_kind,
                                   uint8_t *pt_used, double *pt_q, double *ms_out) {
    // argument checks, host only
    if (n_models < 0 || !pt_begin) return JAICOV_ERR_BAD_ARGUMENT;
    if (max_iterations < 1 || min_points < 3 || !(reject_threshold >= 0.0) || !isfinite(reject_threshold)) return JAICOV_ERR_BAD_ARGUMENT;
    if (n_models > 0 && (!out || !status)) return JAICOV_ERR_BAD_ARGUMENT;
    if (!ranges_ok(n_models, pt_begin)) return JAICOV_ERR_BAD_ARGUMENT;
    const long n_pts = pt_begin[n_models];
    if (n_pts > 0 && (!src || !dst)) return JAICOV_ERR_BAD_ARGUMENT;
    if (!cofactors_ok(cof_src, n_pts, false) || !cofactors_ok(cof_dst, n_pts, true)) return JAICOV_ERR_BAD_ARGUMENT;

    if (!device_is_gfx950()) return JAICOV_ERR_NO_DEVICE;
    if (ms_out) *ms_out = 0.0;
    if (n_models == 0) return JAICOV_OK;

    BatchCall call;
    const size_t nm = (size_t)n_models, np = (size_t)n_pts;
    const int32_t *d_begin = call.in(pt_begin, nm + 1);
    const double *d_src = call.in(src, 3 * np), *d_dst = call.in(dst, 3 * np), *d_qs = call.in(cof_src, 6 * np), *d_qd = call.in(cof_dst, 6 * np),
                 *d_start = call.in(start, 7 * nm);
    double *d_out = call.alloc<double>(JAICOV_SIMIL_OUT_PER_MODEL * nm), *d_q = pt_q ? call.alloc<double>(np) : nullptr;
    int32_t *d_outcome = call.alloc<int32_t>(3 * nm);
    uint8_t *d_used = call.filled<uint8_t>(np, 1);                     // every point starts as used
    call.run([&](hipStream_t s) {
        hipLaunchKernelGGL(simil_models_kernel, dim3(n_models), dim3(SIMIL_LANES), 0, s, d_begin, d_src, d_dst, d_qs, d_qd, d_start,
                           (int)max_iterations, reject_threshold * reject_threshold, (int)min_points, d_out, d_outcome, d_used, d_q);
    });
    call.out(out, d_out, JAICOV_SIMIL_OUT_PER_MODEL * nm);
    call.outcomes(d_outcome, nm, 3, status, iterations, start_kind);
    call.out(pt_used, d_used, np);
    call.out(pt_q, d_q, np);
    return call.finish(ms_out);
}

extern "C" int jaicov_simil_apply(int32_t n_models, const double *par, const int32_t *pt_begin, const double *xyz, const double *cof,
                                  const int32_t *img_begin, const double *eo, double *xyz_out, double *cof_out, double *eo_out) {
    // argument checks, host only
    if (n_models < 0 || (n_models > 0 && !par)) return JAICOV_ERR_BAD_ARGUMENT;
    if ((pt_begin && !ranges_ok(n_models, pt_begin)) || (img_begin && !ranges_ok(n_models, img_begin))) return JAICOV_ERR_BAD_ARGUMENT;
    const long n_pts = pt_begin ? pt_begin[n_models] : 0, n_img = img_begin ? img_begin[n_models] : 0;
    if (n_pts > 0 && (!xyz || !xyz_out)) return JAICOV_ERR_BAD_ARGUMENT;
    if ((cof == nullptr) != (cof_out == nullptr)) return JAICOV_ERR_BAD_ARGUMENT;
    if (n_img > 0 && (!eo || !eo_out)) return JAICOV_ERR_BAD_ARGUMENT;

    if (!device_is_gfx950()) return JAICOV_ERR_NO_DEVICE;
    if (n_pts + n_img == 0) return JAICOV_OK;

    BatchCall call(false);             // this call reports no device time
    const size_t np = (size_t)n_pts, ni = (size_t)n_img;
    const std::vector<int32_t> h_pm = models_of(n_models, pt_begin), h_im = models_of(n_models, img_begin);   // alive until finish()
    const double *d_par = call.in(par, 7 * (size_t)n_models);
    const int32_t *d_pm = call.in(h_pm);
    double *d_xyz = call.in(xyz, 3 * np), *d_cof = call.in(cof, 6 * np);
    const int32_t *d_im = call.in(h_im);
    double *d_eo = call.in(eo, 6 * ni);
    // every item is read and written by its own thread, in place
    const long n = n_pts + n_img;
    const int threads = SIMIL_APPLY_THREADS, blocks = (int)((n + threads - 1) / threads < 65536 ? (n + threads - 1) / threads : 65536);
    call.run([&](hipStream_t s) {
        hipLaunchKernelGGL(simil_apply_kernel, dim3(blocks), dim3(threads), 0, s, n_pts, n_img, d_par, d_pm, d_im, d_xyz, np ? d_cof : nullptr,
                           d_eo, d_xyz, np ? d_cof : nullptr, d_eo);
    });
    call.out(xyz_out, d_xyz, 3 * np);
    call.out(cof_out, d_cof, 6 * np);
    call.out(eo_out, d_eo, 6 * ni);
    return call.finish();
}
