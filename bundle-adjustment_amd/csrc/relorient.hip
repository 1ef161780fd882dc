// relorient.hip -- relative orientation of many image pairs in one launch (include/jaicov_relorient.h): start values of the first two
// exterior orientations of a block without control points, from the image points two images share.  The call has no counterpart in
// the reference; its rotation is that of derivation/PartialDerivativeFactory.java (PDF), its dispersions PDF:308-319 inverted, its
// preconditioning that of NormalEquationSystem.java (NES).
//
// One wave (one workgroup of 64 lanes) works one pair; the two linear starts, the cheirality count, every Gauss-Newton run, the
// choice and the rejection rounds all run inside it, with no host round trip.  The layout is that of resect.hip:
//   Sums.  Lane l takes observations l, l + 64, ... and keeps the partial sums of the pass; the lanes are combined by an xor butterfly,
//   whose order is fixed and which leaves the same bits in every lane.  What follows is therefore wave-uniform: the sums, the
//   candidate slots, the starts and the pair's state (b, angles, R, the tangent basis) lie in LDS, where every lane stores the same
//   words; every lane runs the small algebra on them (Jacobi sweeps of order 9 and Cholesky of order 8 in place in LDS, Jacobi of
//   order 3 and Cholesky of order 5 in registers), and every branch on its outcome is taken by the whole wave.  Observations are
//   staged RELOR_CHUNK at a time in LDS as rays and ray cofactors; a pair with at most RELOR_CHUNK keeps them resident.
//   One pass routine serves every kind of sum (space start, plane start, cheirality, step, evaluation), so that it is compiled once;
//   its RELOR_NACC accumulators are the large per-lane state, and every index into them is a compile-time constant.
// Floating-point contraction is off in this file: every product and sum is rounded on its own, as tests/relorient_reference.py rounds it.
#include <hip/hip_runtime.h>

#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jaicov_relorient.h"
#include "batchcall.h"
#include "relorient.h"
#include "wavealg.h"

#pragma clang fp contract(off)

namespace jaicov {
namespace {

enum { RO_BEGIN = 0, RO_SPACE, RO_PLANE, RO_CHEIR, RO_STEP, RO_EVAL, RO_FINAL };

// the solves' statuses (wavealg.h) go out as the call's own
static_assert(JAICOV_RELOR_OK == WAVE_OK && JAICOV_RELOR_SINGULAR == WAVE_SINGULAR && JAICOV_RELOR_NOT_FINITE == WAVE_NOT_FINITE,
              "wavealg.h returns the public status values");

// RELOR_SWEEPS9 sweeps of cyclic Jacobi over the symmetric 9 x 9 matrix A (full, in LDS); W (in LDS, the unit matrix on entry): its rows
// become the eigenvectors.  Every lane runs it on the same words; the loops stay rolled.
__device__ inline void ro_jacobi9(double *A, double *W) {
    for (int sweep = 0; sweep < RELOR_SWEEPS9; sweep++)
        for (int p = 0; p < 8; p++)
            for (int q = p + 1; q < 9; q++) {
                const double apq = A[9 * p + q];
                if (wave_uniform(apq == 0.0)) continue;
                double t, c, s;
                jacobi_angle(A[9 * p + p], A[9 * q + q], apq, t, c, s);
                for (int k = 0; k < 9; k++) {
                    if (k == p || k == q) continue;
                    const double akp = A[9 * k + p], akq = A[9 * k + q];
                    const double kp = c * akp - s * akq, kq = s * akp + c * akq;
                    A[9 * k + p] = kp; A[9 * p + k] = kp;
                    A[9 * k + q] = kq; A[9 * q + k] = kq;
                }
                A[9 * p + p] = A[9 * p + p] - t * apq;
                A[9 * q + q] = A[9 * q + q] + t * apq;
                A[9 * p + q] = 0.0; A[9 * q + p] = 0.0;
                for (int k = 0; k < 9; k++) {
                    const double wp = W[9 * p + k], wq = W[9 * q + k];
                    W[9 * p + k] = c * wp - s * wq;
                    W[9 * q + k] = s * wp + c * wq;
                }
            }
}

__device__ inline void ro_cross(const double *a, const double *b, double *c) {
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// a candidate slot: M, b and M b
__device__ inline void ro_slot(double *slot, const double *M, const double *b, double sign) {
    const double bs[3] = {sign * b[0], sign * b[1], sign * b[2]};
#pragma unroll
    for (int k = 0; k < 9; k++) slot[k] = M[k];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        slot[9 + k] = bs[k];
        slot[12 + k] = M[3 * k] * bs[0] + M[3 * k + 1] * bs[1] + M[3 * k + 2] * bs[2];
    }
}

// where the state of a pair lies in LDS (doubles): every lane stores the same words there and reads them back
enum { RO_PAR = 0, RO_R = 6, RO_SO = 15, RO_CO = 16, RO_E1 = 17, RO_E2 = 20, RO_NSTATE = 23 };

__global__ __launch_bounds__(RELOR_LANES) void relorient_pairs_kernel(const int32_t *__restrict__ obs_begin, const double *__restrict__ xy_a,
                                                            const double *__restrict__ xy_b, const double *__restrict__ var_a,
                                                            const double *__restrict__ var_b, const double *__restrict__ pair_io,
                                                            const double *__restrict__ start, double s0, int max_iter, double thr2,
                                                            int min_points, double *__restrict__ out, int32_t *__restrict__ outcome,
                                                            uint8_t *used, double *__restrict__ obs_q) {
    __shared__ double sua[RELOR_CHUNK], sva[RELOR_CHUNK], sub[RELOR_CHUNK], svb[RELOR_CHUNK];
    __shared__ double sqa[3][RELOR_CHUNK], sqb[3][RELOR_CHUNK];
    __shared__ uint8_t sused[RELOR_CHUNK];
    __shared__ int scount[RELOR_SLOTS * RELOR_LANES];     // points in front, per slot and lane
    // The sums of the last pass, the same in every lane after the butterfly (sA: the 9 x 9 matrix and its eigenvectors, or the
    // homography's system, or a step's), the candidate slots (sC), the starts and the best run so far (sS, sB: b, angles, Omega) and
    // the pair's state (sP).  The workgroup is one wave, and all of this rests on it: every lane stores the same value to the same word
    // and reads it back, and no barrier stands between such a store and the reads that follow, because the LDS operations of one wave
    // complete in order.
    static_assert(RELOR_LANES == 64, "one wave per pair: the uniform state in LDS relies on it");
    __shared__ double sA[81 + 81], sV[8], sC[RELOR_SLOTS * RELOR_SLOT_LEN], sS[RELOR_STARTS * 6], sB[7], sP[RO_NSTATE];
    const int g = blockIdx.x, lane = threadIdx.x;
    const long k0 = obs_begin[g];
    const int m = obs_begin[g + 1] - obs_begin[g];
    double *og = out + (long)JAICOV_RELOR_OUT_PER_PAIR * g;
    // the pair's whole-number state (counters, masks, statuses), the same in every lane.  It lies in LDS like the rest of the uniform
    // state: held in scalar registers across the passes it cost 22 more spilled SGPRs.
    __shared__ int sI[14];
    int &iters = sI[0];
    iters = 0;
    const double *io = pair_io + 6L * g;                   // x0, y0, c of a, then of b: read where they are used, not held
    bool given = start != nullptr;
#pragma unroll
    for (int k = 0; k < 6; k++) given = given && isfinite(start[6L * g + k]);
    const int few = given ? 5 : 6;
    const bool resident = m <= RELOR_CHUNK;
    // observations c0 .. c0 + nc - 1 into LDS as rays, with the cofactors of the rays (PDF:308-319 inverted, over sigma2 and c^2)
    auto stage = [&](int c0, int nc) {
        __syncthreads();
        const double xa0 = io[0], ya0 = io[1], ca = io[2], xb0 = io[3], yb0 = io[4], cb = io[5];
        const double ca2 = ca * ca, cb2 = cb * cb;
        for (int t = lane; t < nc; t += 64) {
            const long k = k0 + c0 + t;
            sua[t] = -(xy_a[2 * k] - xa0) / ca; sva[t] = -(xy_a[2 * k + 1] - ya0) / ca;
            sub[t] = -(xy_b[2 * k] - xb0) / cb; svb[t] = -(xy_b[2 * k + 1] - yb0) / cb;
            double q11 = 1.0 / ca2, q12 = 0.0, q22 = 1.0 / ca2;
            if (var_a) {
                const double vx = var_a[3 * k], vy = var_a[3 * k + 1], rho = var_a[3 * k + 2];
                q11 = vx / s0 / ca2; q22 = vy / s0 / ca2;
                q12 = rho == 0.0 ? 0.0 : rho * sqrt(vx * vy) / s0 / ca2;
            }
            sqa[0][t] = q11; sqa[1][t] = q12; sqa[2][t] = q22;
            q11 = 1.0 / cb2; q12 = 0.0; q22 = 1.0 / cb2;
            if (var_b) {
                const double vx = var_b[3 * k], vy = var_b[3 * k + 1], rho = var_b[3 * k + 2];
                q11 = vx / s0 / cb2; q22 = vy / s0 / cb2;
                q12 = rho == 0.0 ? 0.0 : rho * sqrt(vx * vy) / s0 / cb2;
            }
            sqb[0][t] = q11; sqb[1][t] = q12; sqb[2][t] = q22;
            sused[t] = used[k];
        }
        __syncthreads();
    };

    int &mask = sI[1];                                    // the candidate slots that exist
    mask = 0;
    // one pass over the pair's observations: the sums of the used ones, combined over the lanes, into sA; RO_FINAL also writes q of
    // every observation and finds the used one with the largest q (the lowest index among equal values)
    auto pass = [&](int mode, double &qmax, int &qidx) {
        double acc[RELOR_NACC];
#pragma unroll
        for (int a = 0; a < RELOR_NACC; a++) acc[a] = 0.0;
        qmax = -1.0; qidx = INT_MAX;
        const bool want_q = mode == RO_FINAL && obs_q;
        if (mode == RO_CHEIR) {
#pragma unroll 1
            for (int s = 0; s < RELOR_SLOTS; s++) scount[64 * s + lane] = 0;
        }
        for (int c0 = 0; c0 < m; c0 += RELOR_CHUNK) {
            const int nc = min(RELOR_CHUNK, m - c0);
            if (!resident) stage(c0, nc);
            for (int t = lane; t < nc; t += 64) {
                const bool in = sused[t] != 0;
                if (!in && !want_q) continue;
                const double ua = sua[t], va = sva[t], ub = sub[t], vb = svb[t];
                if (mode == RO_SPACE) {
                    const double k[9] = {ub * ua, ub * va, ub, vb * ua, vb * va, vb, ua, va, 1.0};
#pragma unroll
                    for (int i = 0; i < 9; i++)
#pragma unroll
                        for (int j = i; j < 9; j++) acc[tri_ix<9>(i, j)] += k[i] * k[j];
                } else if (mode == RO_PLANE) {
                    const double a[8] = {ua, va, 1.0, 0.0, 0.0, 0.0, -(ub * ua), -(ub * va)};
                    const double b[8] = {0.0, 0.0, 0.0, ua, va, 1.0, -(vb * ua), -(vb * va)};
#pragma unroll
                    for (int i = 0; i < 8; i++) {
#pragma unroll
                        for (int j = i; j < 8; j++) acc[tri_ix<8>(i, j)] += a[i] * a[j] + b[i] * b[j];
                        acc[36 + i] += a[i] * ub + b[i] * vb;
                    }
                } else if (mode == RO_CHEIR) {
                    // the slots' counts are kept per lane in LDS, not among the sums: the loop over the slots stays rolled, and a slot's
                    // M is read where it is used instead of being held for all twelve across the loop over the observations
                    const double bb = ub * ub + vb * vb + 1.0, ca = io[2], cb = io[5];
#pragma unroll 1
                    for (int s = 0; s < RELOR_SLOTS; s++) {
                        if (!wave_uniform((mask >> s) & 1)) continue;
                        const double *M = sC + RELOR_SLOT_LEN * s, *mb = M + 12;
                        const double a0 = M[0] * ua + M[1] * va + M[2], a1 = M[3] * ua + M[4] * va + M[5], a2 = M[6] * ua + M[7] * va + M[8];
                        const double aa = a0 * a0 + a1 * a1 + a2 * a2;
                        const double ab = a0 * ub + a1 * vb + a2;
                        const double ra = a0 * mb[0] + a1 * mb[1] + a2 * mb[2];
                        const double rb = ub * mb[0] + vb * mb[1] + mb[2];
                        const double det = aa * bb - ab * ab, na = ra * bb - ab * rb, nb = ab * ra - aa * rb;
                        if (det > 0.0 && ca * na < 0.0 && cb * nb < 0.0) scount[64 * s + lane] += 1;
                    }
                } else {                                  // the coplanarity condition at the unknowns
                    const double *b = sP + RO_PAR, *R = sP + RO_R, *e1 = sP + RO_E1, *e2 = sP + RO_E2;
                    const double so = sP[RO_SO], co = sP[RO_CO];
                    const double p0 = b[1] - b[2] * va, p1 = b[2] * ua - b[0], p2 = b[0] * va - b[1] * ua;
                    const double r0 = R[0] * ub + R[1] * vb + R[2], r1 = R[3] * ub + R[4] * vb + R[5], r2 = R[6] * ub + R[7] * vb + R[8];
                    const double gk = r0 * p0 + r1 * p1 + r2 * p2;
                    const double t0 = R[0] * p0 + R[3] * p1 + R[6] * p2, t1 = R[1] * p0 + R[4] * p1 + R[7] * p2;
                    const double g0 = r1 * b[2] - r2 * b[1], g1 = r2 * b[0] - r0 * b[2];
                    const double qa11 = sqa[0][t], qa12 = sqa[1][t], qa22 = sqa[2][t], qb11 = sqb[0][t], qb12 = sqb[1][t], qb22 = sqb[2][t];
                    const double cof = (g0 * (qa11 * g0 + qa12 * g1) + g1 * (qa12 * g0 + qa22 * g1)) +
                                       (t0 * (qb11 * t0 + qb12 * t1) + t1 * (qb12 * t0 + qb22 * t1));
                    const double pw = 1.0 / cof, pg = pw * gk, q = pg * gk;
                    if (want_q) obs_q[k0 + c0 + t] = q;
                    if (!in) continue;
                    double a[5];
                    {
                        const double f0 = e1[1] - e1[2] * va, f1 = e1[2] * ua - e1[0], f2 = e1[0] * va - e1[1] * ua;
                        a[0] = r0 * f0 + r1 * f1 + r2 * f2;
                    }
                    {
                        const double f0 = e2[1] - e2[2] * va, f1 = e2[2] * ua - e2[0], f2 = e2[0] * va - e2[1] * ua;
                        a[1] = r0 * f0 + r1 * f1 + r2 * f2;
                    }
                    a[2] = p2 * r1 - p1 * r2;
                    a[3] = p0 * (co * r2 - so * r1) + p1 * (so * r0) - p2 * (co * r0);
                    a[4] = ub * t1 - vb * t0;
#pragma unroll
                    for (int i = 0; i < 5; i++) {
#pragma unroll
                        for (int j = i; j < 5; j++) acc[tri_ix<5>(i, j)] += a[i] * (pw * a[j]);
                        acc[15 + i] += -(a[i] * pg);
                    }
                    acc[20] += q;
                    if (mode == RO_FINAL && q > qmax) { qmax = q; qidx = c0 + t; }
                }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int a = 0; a < RELOR_NACC_STEP; a++) acc[a] += __shfl_xor(acc[a], off);
            if (mode == RO_SPACE || mode == RO_PLANE) {
#pragma unroll
                for (int a = RELOR_NACC_STEP; a < RELOR_NACC; a++) acc[a] += __shfl_xor(acc[a], off);
            }
            wave_argmax_combine(qmax, qidx, off);
        }
        __syncthreads();                                  // the last reads of the state and of the sums before
        if (mode == RO_CHEIR) {                           // whole numbers: their sum does not depend on its order
#pragma unroll 1
            for (int s = 0; s < RELOR_SLOTS; s++) {
                int n = scount[64 * s + lane];
                for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
                sA[s] = (double)n;
            }
        } else if (mode == RO_SPACE) {
#pragma unroll
            for (int i = 0; i < 9; i++)
#pragma unroll
                for (int j = 0; j < 9; j++) {
                    sA[9 * i + j] = acc[i <= j ? tri_ix<9>(i, j) : tri_ix<9>(j, i)];
                    sA[81 + 9 * i + j] = i == j ? 1.0 : 0.0;
                }
        } else {
#pragma unroll
            for (int a = 0; a < RELOR_NACC_PLANE; a++) sA[a] = acc[a];
        }
        __syncthreads();
    };

    const double SQRT_EPS = sqrt(ldexp(1.0, -53));
    int &nused = sI[2], &kind = sI[3];
    nused = m; kind = JAICOV_RELOR_START_GIVEN;
    double qmax = -1.0;
    int qidx = INT_MAX;
    // the starts of the round (sS) with their kinds (2 bits each), the one that runs (cur) and its status, the best run so far (sB)
    int &nstarts = sI[4], &kinds = sI[5], &cur = sI[6], &cst = sI[7], &it = sI[8], &bst = sI[9], &bkind = sI[10];
    nstarts = 0; kinds = 0; cur = 0; cst = JAICOV_RELOR_NOT_CONVERGED; it = 0; bst = -1; bkind = 0;
    int &not_finite = sI[11], &new_state = sI[12], &failed = sI[13];
    not_finite = 0; new_state = 0;
    failed = m < few ? JAICOV_RELOR_TOO_FEW_POINTS : -1;
    if (wave_uniform(resident && failed < 0)) stage(0, m);
    // one loop over the passes of all rounds, so that the pass, the rotation and the angles of a start are compiled once:
    // BEGIN (-> SPACE) -> PLANE -> CHEIR -> [STEP ... STEP -> EVAL] per start -> FINAL (-> BEGIN of the next round)
    int mode = RO_BEGIN;
    while (wave_uniform(failed < 0)) {
        mode = wave_uniform(mode);
        if (wave_uniform(new_state != 0)) {
            double so, co, sp, cp, sk, ck;
            wave_sincos3(lane, sP[RO_PAR + 3], sP[RO_PAR + 4], sP[RO_PAR + 5], so, co, sp, cp, sk, ck);
            rotation_opk(so, co, sk, ck, sp, cp, sP + RO_R);
            sP[RO_SO] = so; sP[RO_CO] = co;
            // the tangent basis at b
            const double b[3] = {sP[RO_PAR], sP[RO_PAR + 1], sP[RO_PAR + 2]};
            int ax = 0;
            if (fabs(b[1]) < fabs(b[0])) ax = 1;
            if (fabs(b[2]) < fabs(ax == 0 ? b[0] : b[1])) ax = 2;
            ax = wave_uniform(ax);
            const double e[3] = {ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0};
            double f[3], e1[3], e2[3];
            ro_cross(b, e, f);
            const double ln = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
#pragma unroll
            for (int k = 0; k < 3; k++) e1[k] = f[k] / ln;
            ro_cross(b, e1, e2);
#pragma unroll
            for (int k = 0; k < 3; k++) { sP[RO_E1 + k] = e1[k]; sP[RO_E2 + k] = e2[k]; }
            new_state = 0;
        }
        if (mode != RO_BEGIN) pass(mode, qmax, qidx);
        bool advance = false;                             // the running start is done: the next one, or the choice
        if (mode == RO_BEGIN) {
            nstarts = 0; kinds = 0; cur = 0; bst = -1; not_finite = 0; mask = 0;
            if (wave_uniform(nused < few)) {
                failed = JAICOV_RELOR_TOO_FEW_POINTS;
            } else if (given) {
                const double *s = start + 6L * g;
                const double ln = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
#pragma unroll
                for (int k = 0; k < 3; k++) { sP[RO_PAR + k] = s[k] / ln; sP[RO_PAR + 3 + k] = s[3 + k]; }
                nstarts = 1; kinds = JAICOV_RELOR_START_GIVEN;
                new_state = 1; cst = JAICOV_RELOR_NOT_CONVERGED; it = 0;
                mode = RO_STEP;
            } else {
                mode = wave_uniform(nused >= 8) ? RO_SPACE : RO_PLANE;
            }
        } else if (mode == RO_SPACE) {
            mode = RO_PLANE;
            bool finite = true;
            for (int k = 0; k < 81; k++) finite = finite && isfinite(sA[k]);
            if (wave_uniform(!finite)) {
                not_finite = 1;
            } else {
                ro_jacobi9(sA, sA + 81);
                int i0 = 0;
                for (int i = 1; i < 9; i++)
                    if (sA[10 * i] < sA[10 * i0]) i0 = i;
                i0 = wave_uniform(i0);
                double l1 = INFINITY, lmax = sA[10 * i0];
                for (int i = 0; i < 9; i++) {
                    const double l = sA[10 * i];
                    if (i != i0 && l < l1) l1 = l;
                    if (l > lmax) lmax = l;
                }
                if (wave_uniform(l1 > SQRT_EPS * lmax)) {
                    const double r2 = sqrt(2.0);
                    double E[9], S[6], lam[3], V[9], C[9], D[9], Mp[9], Mm[9];
#pragma unroll
                    for (int k = 0; k < 9; k++) E[k] = sA[81 + 9 * i0 + k] * r2;
                    S[0] = E[0] * E[0] + E[3] * E[3] + E[6] * E[6]; S[1] = E[0] * E[1] + E[3] * E[4] + E[6] * E[7];
                    S[2] = E[0] * E[2] + E[3] * E[5] + E[6] * E[8]; S[3] = E[1] * E[1] + E[4] * E[4] + E[7] * E[7];
                    S[4] = E[1] * E[2] + E[4] * E[5] + E[7] * E[8]; S[5] = E[2] * E[2] + E[5] * E[5] + E[8] * E[8];
                    wave_eigen3<RELOR_SWEEPS3>(S, lam, V);
                    const double *n = V + 6;
                    ro_cross(E + 3, E + 6, C); ro_cross(E + 6, E, C + 3); ro_cross(E, E + 3, C + 6);
                    ro_cross(E, n, D); ro_cross(E + 3, n, D + 3); ro_cross(E + 6, n, D + 6);
#pragma unroll
                    for (int k = 0; k < 9; k++) { Mp[k] = C[k] - D[k]; Mm[k] = C[k] + D[k]; }
                    ro_slot(sC, Mp, n, 1.0); ro_slot(sC + RELOR_SLOT_LEN, Mp, n, -1.0);
                    ro_slot(sC + 2 * RELOR_SLOT_LEN, Mm, n, 1.0); ro_slot(sC + 3 * RELOR_SLOT_LEN, Mm, n, -1.0);
                    mask |= 0xF;
                }
            }
        } else if (mode == RO_PLANE) {
            const int ps = wave_solve_lds(8, sA, sA + 36, sV);
            if (ps == JAICOV_RELOR_NOT_FINITE) not_finite = 1;
            if (ps == JAICOV_RELOR_OK) {
                const double *h = sA + 36;
                double H[9] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], 1.0}, S[6], lam[3], V[9];
                S[0] = H[0] * H[0] + H[3] * H[3] + H[6] * H[6]; S[1] = H[0] * H[1] + H[3] * H[4] + H[6] * H[7];
                S[2] = H[0] * H[2] + H[3] * H[5] + H[6] * H[8]; S[3] = H[1] * H[1] + H[4] * H[4] + H[7] * H[7];
                S[4] = H[1] * H[2] + H[4] * H[5] + H[7] * H[8]; S[5] = H[2] * H[2] + H[5] * H[5] + H[8] * H[8];
                wave_eigen3<RELOR_SWEEPS3>(S, lam, V);
                const double l1 = lam[0] / lam[1], l3 = lam[2] / lam[1];
                if (wave_uniform(lam[1] > 0.0 && l1 - l3 > SQRT_EPS)) {
                    const double f = sqrt(lam[1]);
#pragma unroll
                    for (int k = 0; k < 9; k++) H[k] = H[k] / f;
                    const double wa = sqrt(fmax(1.0 - l3, 0.0)), wc = sqrt(fmax(l1 - 1.0, 0.0)), den = sqrt(l1 - l3);
                    const double *v1 = V, *v2 = V + 3, *v3 = V + 6;
#pragma unroll 1
                    for (int is = 0; is < 2; is++) {
                        const double s = is == 0 ? 1.0 : -1.0;
                        double u[3], nr[3], h2[3], hu[3], hn[3];
#pragma unroll
                        for (int k = 0; k < 3; k++) u[k] = (wa * v1[k] + s * (wc * v3[k])) / den;
                        ro_cross(v2, u, nr);
#pragma unroll
                        for (int i = 0; i < 3; i++) {
                            h2[i] = H[3 * i] * v2[0] + H[3 * i + 1] * v2[1] + H[3 * i + 2] * v2[2];
                            hu[i] = H[3 * i] * u[0] + H[3 * i + 1] * u[1] + H[3 * i + 2] * u[2];
                            hn[i] = H[3 * i] * nr[0] + H[3 * i + 1] * nr[1] + H[3 * i + 2] * nr[2];
                        }
#pragma unroll 1
                        for (int ig = 0; ig < 2; ig++) {
                            const double sg = ig == 0 ? 1.0 : -1.0;
                            const double w1[3] = {sg * h2[0], sg * h2[1], sg * h2[2]}, w2[3] = {sg * hu[0], sg * hu[1], sg * hu[2]};
                            double w3[3], M[9], t[3], bd[3];
                            ro_cross(w1, w2, w3);
#pragma unroll
                            for (int i = 0; i < 3; i++) {
#pragma unroll
                                for (int j = 0; j < 3; j++) M[3 * i + j] = w1[i] * v2[j] + w2[i] * u[j] + w3[i] * nr[j];
                                t[i] = sg * hn[i] - w3[i];
                            }
#pragma unroll
                            for (int k = 0; k < 3; k++) bd[k] = -(M[k] * t[0] + M[3 + k] * t[1] + M[6 + k] * t[2]);
                            const double ln = sqrt(bd[0] * bd[0] + bd[1] * bd[1] + bd[2] * bd[2]);
                            if (wave_uniform(!(ln > 0.0))) continue;
#pragma unroll
                            for (int k = 0; k < 3; k++) bd[k] = bd[k] / ln;
                            const int slot = 4 + 4 * is + 2 * ig;
                            ro_slot(sC + RELOR_SLOT_LEN * slot, M, bd, 1.0);
                            ro_slot(sC + RELOR_SLOT_LEN * (slot + 1), M, bd, -1.0);
                            mask |= 3 << slot;
                        }
                    }
                }
            }
            if (wave_uniform(mask == 0)) failed = wave_uniform(not_finite != 0) ? JAICOV_RELOR_NOT_FINITE : JAICOV_RELOR_SINGULAR;
            else mode = RO_CHEIR;
        } else if (mode == RO_CHEIR) {
            // the slots that go on, 4 bits each: the best of the space start, the (at most two) best of the plane start
            int picks = 0, space = -1, plane = -1;
            for (int s = 0; s < 4; s++)
                if (((mask >> s) & 1) && (space < 0 || sA[s] > sA[space])) space = s;
            for (int s = 4; s < RELOR_SLOTS; s++)
                if (((mask >> s) & 1) && (plane < 0 || sA[s] > sA[plane])) plane = s;
            space = wave_uniform(space); plane = wave_uniform(plane);
            if (space >= 0) { picks |= space << (4 * nstarts); kinds |= JAICOV_RELOR_START_SPACE << (2 * nstarts); nstarts++; }
            if (plane >= 0) {
                int taken = 0;
                for (int s = plane; s < RELOR_SLOTS && taken < 2; s++)
                    if (wave_uniform(((mask >> s) & 1) && sA[s] == sA[plane])) {
                        picks |= s << (4 * nstarts); kinds |= JAICOV_RELOR_START_PLANE << (2 * nstarts); nstarts++; taken++;
                    }
            }
            nstarts = wave_uniform(nstarts); picks = wave_uniform(picks); kinds = wave_uniform(kinds);
#pragma unroll 1
            for (int j = 0; j < wave_uniform(nstarts); j++) {
                // b and the angles of R = M': r23 = M[2][1], r33 = M[2][2], r12 = M[1][0], r11 = M[0][0], r13 = M[2][0]
                const double *M = sC + RELOR_SLOT_LEN * ((picks >> (4 * j)) & 15);
                double *par = sS + 6 * j;
                par[0] = M[9]; par[1] = M[10]; par[2] = M[11];
                wave_angles(lane, M[7], M[8], M[3], M[0], M[6], par + 3);
            }
#pragma unroll
            for (int k = 0; k < 6; k++) sP[RO_PAR + k] = sS[k];
            new_state = 1; cst = JAICOV_RELOR_NOT_CONVERGED; it = 0; cur = 0;
            mode = RO_STEP;
        } else if (mode == RO_STEP) {
            double A[15], b[5], dx[5];
#pragma unroll
            for (int k = 0; k < 15; k++) A[k] = sA[k];
#pragma unroll
            for (int k = 0; k < 5; k++) b[k] = sA[15 + k];
            int ss = wave_solve<5>(A, b, dx, nullptr);
            iters++;
            if (ss == JAICOV_RELOR_OK) {
                double z = 0.0;                           // NaN unless every value is finite
#pragma unroll
                for (int k = 0; k < 5; k++) z += dx[k] * 0.0;
                if (wave_uniform(z != 0.0)) ss = JAICOV_RELOR_NOT_FINITE;
            }
            if (ss != JAICOV_RELOR_OK) {
                if (ss == JAICOV_RELOR_NOT_FINITE) not_finite = 1;
                advance = true;
            } else {
                double bn[3], step = 0.0;
#pragma unroll
                for (int k = 0; k < 3; k++) bn[k] = sP[RO_PAR + k] + (dx[0] * sP[RO_E1 + k] + dx[1] * sP[RO_E2 + k]);
                const double ln = sqrt(bn[0] * bn[0] + bn[1] * bn[1] + bn[2] * bn[2]);
#pragma unroll
                for (int k = 0; k < 3; k++) { sP[RO_PAR + k] = bn[k] / ln; sP[RO_PAR + 3 + k] = sP[RO_PAR + 3 + k] + dx[2 + k]; }
#pragma unroll
                for (int k = 0; k < 5; k++) step = fmax(step, fabs(dx[k]));
                new_state = 1;
                if (wave_uniform(step <= SQRT_EPS)) { cst = JAICOV_RELOR_OK; mode = RO_EVAL; }
                else if (wave_uniform(++it >= max_iter)) mode = RO_EVAL;
            }
        } else if (mode == RO_EVAL) {
            const double omega = sA[20];
            if (wave_uniform(!isfinite(omega))) {
                not_finite = 1;
            } else if (wave_uniform(bst < 0 || cst < bst || (cst == bst && omega < sB[6] - SQRT_EPS * sB[6]))) {
#pragma unroll
                for (int k = 0; k < 6; k++) sB[k] = sP[RO_PAR + k];
                sB[6] = omega;
                bst = cst; bkind = (kinds >> (2 * cur)) & 3;
            }
            advance = true;
        } else {                                          // RO_FINAL: Q is taken from these sums after the loop
            if (wave_uniform(thr2 > 0.0 && nused > min_points && qmax > thr2 && qidx < m)) {
                if (lane == 0) { used[k0 + qidx] = 0; if (resident) sused[qidx] = 0; }
                __syncthreads();                          // the withdrawal is visible to every lane before the next pass reads it
                nused--;
                mode = RO_BEGIN;
            } else {
                break;
            }
        }
        if (advance) {
            cur++;
            if (wave_uniform(cur < nstarts)) {
#pragma unroll
                for (int k = 0; k < 6; k++) sP[RO_PAR + k] = sS[6 * cur + k];
                new_state = 1; cst = JAICOV_RELOR_NOT_CONVERGED; it = 0;
                mode = RO_STEP;
            } else if (wave_uniform(bst < 0)) {
                failed = wave_uniform(not_finite != 0) ? JAICOV_RELOR_NOT_FINITE : JAICOV_RELOR_SINGULAR;
            } else {
#pragma unroll
                for (int k = 0; k < 6; k++) sP[RO_PAR + k] = sB[k];
                new_state = 1; kind = bkind;
                mode = RO_FINAL;
            }
        }
    }
    double o[JAICOV_RELOR_OUT_PER_PAIR];
    if (wave_uniform(failed < 0)) {
        double A[15], b[5], Q[15];
#pragma unroll
        for (int k = 0; k < 15; k++) A[k] = sA[k];
#pragma unroll
        for (int k = 0; k < 5; k++) b[k] = sA[15 + k];
        const int se = wave_solve<5>(A, b, nullptr, Q);
        if (se != JAICOV_RELOR_OK) failed = se;
        const double *e1 = sP + RO_E1, *e2 = sP + RO_E2;
#pragma unroll
        for (int k = 0; k < 6; k++) o[k] = sP[RO_PAR + k];
#pragma unroll
        for (int i = 0; i < 6; i++)                       // J Q5 J', J = [e1 e2 0; 0 0 I3]
#pragma unroll
            for (int j = i; j < 6; j++) {
                double v;
                if (i < 3 && j < 3) {
                    const double t0 = e1[i] * Q[tri_ix<5>(0, 0)] + e2[i] * Q[tri_ix<5>(0, 1)];
                    const double t1 = e1[i] * Q[tri_ix<5>(0, 1)] + e2[i] * Q[tri_ix<5>(1, 1)];
                    v = t0 * e1[j] + t1 * e2[j];
                } else if (i < 3) {
                    v = e1[i] * Q[tri_ix<5>(0, j - 1)] + e2[i] * Q[tri_ix<5>(1, j - 1)];
                } else {
                    v = Q[tri_ix<5>(i - 1, j - 1)];
                }
                o[6 + tri_ix<6>(i, j)] = v;
            }
        o[27] = sA[20];
        double z = 0.0;
#pragma unroll
        for (int k = 0; k < JAICOV_RELOR_OUT_PER_PAIR; k++) z += o[k] * 0.0;
        if (wave_uniform(failed < 0 && z != 0.0)) failed = JAICOV_RELOR_NOT_FINITE;
    }
    if (wave_uniform(failed >= 0)) {                      // start kind 0
        wave_fail_item<3>(lane, og, JAICOV_RELOR_OUT_PER_PAIR, outcome, g, wave_uniform(failed), iters, k0, m, used, obs_q);
        return;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < JAICOV_RELOR_OUT_PER_PAIR; k++) og[k] = o[k];
        outcome[3L * g] = bst;
        outcome[3L * g + 1] = iters;
        outcome[3L * g + 2] = kind;
    }
}

}  // namespace
}  // namespace jaicov

using namespace jaicov;

extern "C" int jaicov_relorient_pairs(int32_t n_pairs, const int32_t *obs_begin, const double *xy_a, const double *xy_b, const double *var_a,
                                      const double *var_b, const double *pair_io, const double *start, double sigma2apriori,
                                      int32_t max_iterations, double reject_threshold, int32_t min_points, double *out, int32_t *status,
                                      int32_t *iterations, int32_t *start_kind, uint8_t *obs_used, double *obs_q, double *ms_out) {
    // argument checks, host only
    if (n_pairs < 0 || !obs_begin) return JAICOV_ERR_BAD_ARGUMENT;
    if (!(sigma2apriori > 0.0) || max_iterations < 1 || min_points < 5 || !(reject_threshold >= 0.0)) return JAICOV_ERR_BAD_ARGUMENT;
    if (n_pairs > 0 && (!out || !status || !pair_io)) return JAICOV_ERR_BAD_ARGUMENT;
    if (!ranges_ok(n_pairs, obs_begin)) return JAICOV_ERR_BAD_ARGUMENT;
    const long n_obs = obs_begin[n_pairs];
    if (n_obs > 0 && (!xy_a || !xy_b)) return JAICOV_ERR_BAD_ARGUMENT;
    if (!dispersions_ok(var_a, n_obs) || !dispersions_ok(var_b, n_obs)) return JAICOV_ERR_BAD_ARGUMENT;

    if (!device_is_gfx950()) return JAICOV_ERR_NO_DEVICE;
    if (ms_out) *ms_out = 0.0;
    if (n_pairs == 0) return JAICOV_OK;

    BatchCall call;
    const size_t np = (size_t)n_pairs, no = (size_t)n_obs;
    const int32_t *d_begin = call.in(obs_begin, np + 1);
    const double *d_xa = call.in(xy_a, 2 * no), *d_xb = call.in(xy_b, 2 * no), *d_va = call.in(var_a, 3 * no), *d_vb = call.in(var_b, 3 * no),
                 *d_io = call.in(pair_io, 6 * np), *d_start = call.in(start, 6 * np);
    double *d_out = call.alloc<double>(JAICOV_RELOR_OUT_PER_PAIR * np), *d_q = obs_q ? call.alloc<double>(no) : nullptr;
    int32_t *d_outcome = call.alloc<int32_t>(3 * np);
    uint8_t *d_used = call.filled<uint8_t>(no, 1);                     // every observation starts as used
    call.run([&](hipStream_t s) {
        hipLaunchKernelGGL(relorient_pairs_kernel, dim3(n_pairs), dim3(RELOR_LANES), 0, s, d_begin, d_xa, d_xb, d_va, d_vb, d_io, d_start,
                           sigma2apriori, (int)max_iterations, reject_threshold * reject_threshold, (int)min_points, d_out, d_outcome, d_used,
                           d_q);
    });
    call.out(out, d_out, JAICOV_RELOR_OUT_PER_PAIR * np);
    call.outcomes(d_outcome, np, 3, status, iterations, start_kind);
    call.out(obs_used, d_used, no);
    call.out(obs_q, d_q, no);
    return call.finish(ms_out);
}
