// resect.hip -- spatial resection of many images in one launch (include/jaicov_resect.h): start values of the exterior orientation
// from known object points and a known interior orientation.  The call has no counterpart in the reference; its collinearity
// equations, derivatives and weights are those of derivation/PartialDerivativeFactory.java (PDF), its preconditioning that of
// NormalEquationSystem.java (NES).
//
// One wave (one workgroup of 64 lanes) works one image; the reduction, the two linear starts, the Gauss-Newton loop, the evaluation
// pass and the rejection rounds all run inside it, with no host round trip.  As for the DLT and the intersection
// the work per image is a chain of small dependent steps: latency bounds it, and many resident single-wave workgroups hide it.
//   Sums.  Lane l takes observations l, l + 64, ... and keeps the partial sums of the pass; the lanes are combined by an xor butterfly,
//   whose order is fixed and which leaves the same bits in every lane.  What follows is therefore wave-uniform: the sums and the
//   image's state (reduction, unknowns, rotation, the plane's axes) lie in LDS, where every lane stores the same words; every lane
//   runs the small algebra on them (Cholesky of order 11 and 8 in place in LDS, of order 6 in registers, the polar factor, the Jacobi
//   sweeps), and every branch on its outcome is taken by the whole wave.  Observations are staged RESECT_CHUNK at a time in LDS; an
//   image with at most RESECT_CHUNK keeps them resident.
//   One pass routine serves every kind of sum (centroid, scatter, space start, plane start, step, evaluation), so that it is compiled
//   once; its RESECT_NACC accumulators are the large per-lane state, and every index into them is a compile-time constant.
// Floating-point contraction is off in this file: every product and sum is rounded on its own, as tests/resection_reference.py rounds it.
#include <hip/hip_runtime.h>

#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jaicov_resect.h"
#include "batchcall.h"
#include "resect.h"
#include "wavealg.h"

#pragma clang fp contract(off)

namespace jaicov {
namespace {

enum { RS_CENTROID = 0, RS_SCATTER, RS_SPACE, RS_EVAL_SPACE, RS_PLANE, RS_EVAL_PLANE, RS_STEP, RS_EVAL };

// the solves' statuses (wavealg.h) go out as the call's own
static_assert(JAICOV_RESECT_OK == WAVE_OK && JAICOV_RESECT_SINGULAR == WAVE_SINGULAR && JAICOV_RESECT_NOT_FINITE == WAVE_NOT_FINITE,
              "wavealg.h returns the public status values");

// the orthogonal polar factor of X (3 x 3, row-major), in place: Newton's iteration from X / sqrt(|X|_F^2 / 3)
__device__ inline void rs_polar(double *X) {
    double f = 0.0;
#pragma unroll
    for (int k = 0; k < 9; k++) f += X[k] * X[k];
    f = sqrt(f / 3.0);
#pragma unroll
    for (int k = 0; k < 9; k++) X[k] = X[k] / f;
    for (int step = 0; step < RESECT_POLAR_STEPS; step++) {
        double C[9];                                      // cofactors: row i of C = row i+1 x row i+2
        C[0] = X[4] * X[8] - X[5] * X[7]; C[1] = X[5] * X[6] - X[3] * X[8]; C[2] = X[3] * X[7] - X[4] * X[6];
        C[3] = X[7] * X[2] - X[8] * X[1]; C[4] = X[8] * X[0] - X[6] * X[2]; C[5] = X[6] * X[1] - X[7] * X[0];
        C[6] = X[1] * X[5] - X[2] * X[4]; C[7] = X[2] * X[3] - X[0] * X[5]; C[8] = X[0] * X[4] - X[1] * X[3];
        const double det = X[0] * C[0] + X[1] * C[1] + X[2] * C[2];
#pragma unroll
        for (int k = 0; k < 9; k++) X[k] = 0.5 * (X[k] + C[k] / det);
    }
}

// eigenvectors of the scatter matrix S (00 01 02 11 12 22) as the rows of E: e1, e2 (falling eigenvalue), n with det = +1
__device__ inline void rs_eigen(const double *S, double *E) {
    double lam[3];
    wave_eigen3<RESECT_JACOBI_SWEEPS>(S, lam, E);
}

// R(omega, phi, kappa) of the unknowns par, with the sine and cosine of kappa.  Lanes 0, 1, 2 take the sine and cosine of one angle
// each and hand them to the wave, as wave_sincos3 does; this kernel keeps the lines themselves, in which a lane loads only the angle
// it works, because its scalar registers grow when all three angles are loaded and passed ("One shell").
__device__ inline void rs_rotation(int lane, const double *par, double *R, double &sk, double &ck) {
    const double angle = lane == 0 ? par[3] : lane == 1 ? par[4] : par[5];
    double sn, cs;
    sincos(angle, &sn, &cs);
    const double so = __shfl(sn, 0), co = __shfl(cs, 0), sp = __shfl(sn, 1), cp = __shfl(cs, 1);
    sk = __shfl(sn, 2); ck = __shfl(cs, 2);
    rotation_opk(so, co, sk, ck, sp, cp, R);
}

// the six reduced unknowns of the pose p = M P + t (M row-major): X0 = -R t with R = M', and the angles of R
__device__ inline void rs_pose(int lane, const double *M, const double *t, double *par) {
#pragma unroll
    for (int k = 0; k < 3; k++) par[k] = -(M[k] * t[0] + M[3 + k] * t[1] + M[6 + k] * t[2]);
    wave_angles(lane, M[7], M[8], M[3], M[0], M[6], par + 3);     // r23 = M[2][1], r33 = M[2][2], r12 = M[1][0], r11 = M[0][0], r13 = M[2][0]
}

// where the state of an image lies in LDS (doubles): every lane stores the same words there and reads them back
enum { RS_XC = 0, RS_S = 3, RS_PAR = 4, RS_R = 10, RS_SK = 19, RS_CK = 20, RS_E = 21, RS_CAND = 30, RS_NSTATE = 37 };

__global__ __launch_bounds__(RESECT_LANES) void resect_images_kernel(const int32_t *__restrict__ obs_begin, const double *__restrict__ xy,
                                                           const double *__restrict__ xyz, const double *__restrict__ var,
                                                           const double *__restrict__ image_io, const double *__restrict__ eo_start,
                                                           double s0, int max_iter, double thr2, int min_points,
                                                           double *__restrict__ out, int32_t *__restrict__ outcome, uint8_t *used,
                                                           double *__restrict__ obs_q) {
    __shared__ double sx[RESECT_CHUNK], sy[RESECT_CHUNK], sp11[RESECT_CHUNK], sp12[RESECT_CHUNK], sp22[RESECT_CHUNK];
    __shared__ double sX[RESECT_CHUNK], sY[RESECT_CHUNK], sZ[RESECT_CHUNK];
    __shared__ uint8_t sused[RESECT_CHUNK];
    // The sums of the last pass, the same in every lane after the butterfly, and the image's state: Xc, s, the six unknowns, R with
    // sin and cos of kappa, the plane's axes e1 e2 n, the space candidate's unknowns and Omega.  They live in LDS, not in registers:
    // between two passes the registers hold the small algebra, during a pass the lane's partial sums, never both.
    // The workgroup is one wave (RESECT_LANES == 64, the launch and the launch bound use the same constant), and all of this rests on
    // it: every lane stores the same value to the same word and reads it back, wave_solve_lds reads and rewrites sA in place, and no
    // barrier stands between such a store and the reads that follow, because the LDS operations of one wave complete in order.
    // With more than one wave per workgroup none of it would hold.
    static_assert(RESECT_LANES == 64, "one wave per image: the uniform state in LDS relies on it");
    __shared__ double sA[66 + 11 + 1], sV[11], sP[RS_NSTATE];
    const int g = blockIdx.x, lane = threadIdx.x;
    const long k0 = obs_begin[g];
    const int m = obs_begin[g + 1] - obs_begin[g];
    double *og = out + (long)JAICOV_RESECT_OUT_PER_IMAGE * g;
    int iters = 0;
    const double x0 = image_io[3L * g], y0 = image_io[3L * g + 1], c = image_io[3L * g + 2];
    bool given = eo_start != nullptr;
#pragma unroll
    for (int k = 0; k < 6; k++) given = given && isfinite(eo_start[6L * g + k]);
    const bool too_few = m < (given ? 3 : 4);
    const bool resident = m <= RESECT_CHUNK;
    // observations c0 .. c0 + nc - 1 into LDS, with their weights (PDF:308-319)
    auto stage = [&](int c0, int nc) {
        __syncthreads();
        for (int t = lane; t < nc; t += 64) {
            const long k = k0 + c0 + t;
            sx[t] = xy[2 * k]; sy[t] = xy[2 * k + 1];
            sX[t] = xyz[3 * k]; sY[t] = xyz[3 * k + 1]; sZ[t] = xyz[3 * k + 2];
            double p11 = 1.0, p12 = 0.0, p22 = 1.0;
            if (var) obs_weight(var[3 * k], var[3 * k + 1], var[3 * k + 2], s0, p11, p12, p22);
            sp11[t] = p11; sp12[t] = p12; sp22[t] = p22;
            sused[t] = used[k];
        }
        __syncthreads();
    };

    // one pass over the image's observations: the sums of the used ones, combined over the lanes, into sA; RS_EVAL also writes q of
    // every observation and finds the used one with the largest q (the lowest index among equal values)
    auto pass = [&](int mode, double &qmax, int &qidx) {
        double acc[RESECT_NACC];
#pragma unroll
        for (int a = 0; a < RESECT_NACC; a++) acc[a] = 0.0;
        qmax = -1.0; qidx = INT_MAX;
        const bool want_q = mode == RS_EVAL && obs_q;
        for (int c0 = 0; c0 < m; c0 += RESECT_CHUNK) {
            const int nc = min(RESECT_CHUNK, m - c0);
            if (!resident) stage(c0, nc);
            for (int t = lane; t < nc; t += 64) {
                const bool in = sused[t] != 0;
                if (!in && !want_q) continue;
                if (mode == RS_CENTROID) {
                    acc[0] += sX[t]; acc[1] += sY[t]; acc[2] += sZ[t];
                    continue;
                }
                const double d0 = sX[t] - sP[RS_XC], d1 = sY[t] - sP[RS_XC + 1], d2 = sZ[t] - sP[RS_XC + 2];
                if (mode == RS_SCATTER) {
                    acc[0] += d0 * d0; acc[1] += d0 * d1; acc[2] += d0 * d2; acc[3] += d1 * d1; acc[4] += d1 * d2; acc[5] += d2 * d2;
                    continue;
                }
                const double s = sP[RS_S];
                const double P0 = d0 / s, P1 = d1 / s, P2 = d2 / s;
                if (mode == RS_SPACE) {
                    const double u = -(sx[t] - x0) / c, v = -(sy[t] - y0) / c;
                    // Of the 66 + 11 sums of the two rows a = (P 1 | 0 | -u P), b = (0 | P 1 | -v P) only 51 differ: the blocks of
                    // m1 and of m2 are the same sums, the block between them is zero, and a term a_i a_j + b_i b_j with one
                    // product zero is the other product to the bit.  They are dealt out to the 11 x 11 system after the butterfly.
                    const double G[4] = {P0, P1, P2, 1.0};
                    const double au[3] = {-(u * P0), -(u * P1), -(u * P2)}, bv[3] = {-(v * P0), -(v * P1), -(v * P2)};
#pragma unroll
                    for (int i = 0; i < 4; i++) {
#pragma unroll
                        for (int j = i; j < 4; j++) acc[tri_ix<4>(i, j)] += G[i] * G[j];
#pragma unroll
                        for (int j = 0; j < 3; j++) { acc[10 + 3 * i + j] += G[i] * au[j]; acc[22 + 3 * i + j] += G[i] * bv[j]; }
                        acc[40 + i] += G[i] * u;
                        acc[44 + i] += G[i] * v;
                    }
#pragma unroll
                    for (int i = 0; i < 3; i++) {
#pragma unroll
                        for (int j = i; j < 3; j++) acc[34 + tri_ix<3>(i, j)] += au[i] * au[j] + bv[i] * bv[j];
                        acc[48 + i] += au[i] * u + bv[i] * v;
                    }
                } else if (mode == RS_PLANE) {
                    const double u = -(sx[t] - x0) / c, v = -(sy[t] - y0) / c;
                    const double pa = sP[RS_E] * P0 + sP[RS_E + 1] * P1 + sP[RS_E + 2] * P2;
                    const double pb = sP[RS_E + 3] * P0 + sP[RS_E + 4] * P1 + sP[RS_E + 5] * P2;
                    const double a[8] = {pa, pb, 1.0, 0.0, 0.0, 0.0, -(u * pa), -(u * pb)};
                    const double b[8] = {0.0, 0.0, 0.0, pa, pb, 1.0, -(v * pa), -(v * pb)};
#pragma unroll
                    for (int i = 0; i < 8; i++) {
#pragma unroll
                        for (int j = i; j < 8; j++) acc[tri_ix<8>(i, j)] += a[i] * a[j] + b[i] * b[j];
                        acc[36 + i] += a[i] * u + b[i] * v;
                    }
                } else {                                  // the collinearity equations at the unknowns, in the reduced coordinates
                    const double *R = sP + RS_R;
                    const double sk = sP[RS_SK], ck = sP[RS_CK];
                    const double dX = P0 - sP[RS_PAR], dY = P1 - sP[RS_PAR + 1], dZ = P2 - sP[RS_PAR + 2];
                    const double kx = R[0] * dX + R[3] * dY + R[6] * dZ;                   // PDF:141-143
                    const double ky = R[1] * dX + R[4] * dY + R[7] * dZ;
                    const double N = R[2] * dX + R[5] * dY + R[8] * dZ;
                    const double xs = -c * (kx / N), ys = -c * (ky / N);                  // PDF:145-149
                    const double go = R[8] * dY - R[5] * dZ, gp = ky * sk - kx * ck;
                    const double ax[6] = {(R[2] * xs + c * R[0]) / N, (R[5] * xs + c * R[3]) / N, (R[8] * xs + c * R[6]) / N,   // PDF:165-167
                                          (xs * go + c * (R[6] * dY - R[3] * dZ)) / N, (xs * gp + c * N * ck) / N, ys};        // PDF:169-171
                    const double ay[6] = {(R[2] * ys + c * R[1]) / N, (R[5] * ys + c * R[4]) / N, (R[8] * ys + c * R[7]) / N,   // PDF:183-185
                                          (ys * go + c * (R[7] * dY - R[4] * dZ)) / N, (ys * gp - c * N * sk) / N, -xs};       // PDF:187-189
                    const double w0 = sx[t] - (x0 + xs), w1 = sy[t] - (y0 + ys);
                    const double p11 = sp11[t], p12 = sp12[t], p22 = sp22[t];
                    const double pw0 = p11 * w0 + p12 * w1, pw1 = p12 * w0 + p22 * w1;
                    const double q = w0 * pw0 + w1 * pw1;
                    if (want_q) obs_q[k0 + c0 + t] = q;
                    if (!in) continue;
                    double px[6], py[6];
#pragma unroll
                    for (int i = 0; i < 6; i++) { px[i] = p11 * ax[i] + p12 * ay[i]; py[i] = p12 * ax[i] + p22 * ay[i]; }
#pragma unroll
                    for (int i = 0; i < 6; i++) {
#pragma unroll
                        for (int j = i; j < 6; j++) acc[tri_ix<6>(i, j)] += ax[i] * px[j] + ay[i] * py[j];
                        acc[21 + i] += ax[i] * pw0 + ay[i] * pw1;
                    }
                    acc[27] += q;
                    if (q > qmax) { qmax = q; qidx = c0 + t; }
                }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int a = 0; a < RESECT_NACC_STEP; a++) acc[a] += __shfl_xor(acc[a], off);
            if (mode == RS_SPACE || mode == RS_PLANE) {
#pragma unroll
                for (int a = RESECT_NACC_STEP; a < RESECT_NACC; a++) acc[a] += __shfl_xor(acc[a], off);
            }
            wave_argmax_combine(qmax, qidx, off);
        }
        __syncthreads();                                  // the last reads of the state and of the sums before
        if (mode == RS_SPACE) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
#pragma unroll
                for (int j = i; j < 4; j++) sA[tri_ix<11>(i, j)] = sA[tri_ix<11>(4 + i, 4 + j)] = acc[tri_ix<4>(i, j)];
#pragma unroll
                for (int j = 0; j < 4; j++) sA[tri_ix<11>(i, 4 + j)] = 0.0;
#pragma unroll
                for (int j = 0; j < 3; j++) { sA[tri_ix<11>(i, 8 + j)] = acc[10 + 3 * i + j]; sA[tri_ix<11>(4 + i, 8 + j)] = acc[22 + 3 * i + j]; }
                sA[66 + i] = acc[40 + i];
                sA[70 + i] = acc[44 + i];
            }
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int j = i; j < 3; j++) sA[tri_ix<11>(8 + i, 8 + j)] = acc[34 + tri_ix<3>(i, j)];
                sA[74 + i] = acc[48 + i];
            }
        } else {
#pragma unroll
            for (int a = 0; a < RESECT_NACC_PLANE; a++) sA[a] = acc[a];
        }
        __syncthreads();
    };

    if (resident && !too_few) stage(0, m);
    const double SQRT_EPS = sqrt(ldexp(1.0, -53));
    int nused = m, st = JAICOV_RESECT_OK, kind = JAICOV_RESECT_START_GIVEN;
    double qmax = -1.0;
    int qidx = INT_MAX, cand_st = JAICOV_RESECT_SINGULAR; // the space candidate (sP[RS_CAND ...]) exists, or why it does not
    bool have_cand = false, new_angles = false;
    int failed = too_few ? JAICOV_RESECT_TOO_FEW_POINTS : -1;
    // one loop over the passes of all rounds, so that the pass, the rotation and the pose are compiled once:
    // CENTROID -> SCATTER (-> SPACE -> EVAL_SPACE) -> PLANE -> EVAL_PLANE -> STEP ... STEP -> EVAL (-> CENTROID of the next round)
    int mode = RS_CENTROID, it = 0;
    while (failed < 0) {
        mode = wave_uniform(mode);
        if (new_angles) { rs_rotation(lane, sP + RS_PAR, sP + RS_R, sP[RS_SK], sP[RS_CK]); new_angles = false; }
        pass(mode, qmax, qidx);
        double M[9], t[3];                                // a linear start's pose p = M P + t, when it has one
        bool new_pose = false, choose = false;
        int plane_st = JAICOV_RESECT_OK;
        if (mode == RS_CENTROID) {
#pragma unroll
            for (int k = 0; k < 3; k++) sP[RS_XC + k] = sA[k] / (double)nused;
            mode = RS_SCATTER;
        } else if (mode == RS_SCATTER) {
            const double s2 = ((sA[0] + sA[3]) + sA[5]) / (double)nused, s = sqrt(s2);
            sP[RS_S] = s;
            st = JAICOV_RESECT_NOT_CONVERGED; it = 0;
            if (wave_uniform(!isfinite(s2))) {
                failed = JAICOV_RESECT_NOT_FINITE;
            } else if (wave_uniform(!(s > 0.0))) {
                failed = JAICOV_RESECT_SINGULAR;
            } else if (given) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    sP[RS_PAR + k] = (eo_start[6L * g + k] - sP[RS_XC + k]) / s;
                    sP[RS_PAR + 3 + k] = eo_start[6L * g + 3 + k];
                }
                new_angles = true;
                kind = JAICOV_RESECT_START_GIVEN;
                mode = RS_STEP;
            } else if (nused < 4) {
                failed = JAICOV_RESECT_TOO_FEW_POINTS;
            } else {
                double S[6], E[9];
#pragma unroll
                for (int k = 0; k < 6; k++) S[k] = sA[k];
                rs_eigen(S, E);
#pragma unroll
                for (int k = 0; k < 9; k++) sP[RS_E + k] = E[k];
                have_cand = false; cand_st = JAICOV_RESECT_SINGULAR;
                mode = nused >= 6 ? RS_SPACE : RS_PLANE;
            }
        } else if (mode == RS_SPACE) {
            cand_st = wave_solve_lds(11, sA, sA + 66, sV);
            mode = RS_PLANE;
            if (cand_st == JAICOV_RESECT_OK) {
                const double *h = sA + 66;
                double Mt[9] = {h[0], h[1], h[2], h[4], h[5], h[6], h[8], h[9], h[10]};
                t[0] = h[3]; t[1] = h[7]; t[2] = 1.0;
                const double det = Mt[0] * (Mt[4] * Mt[8] - Mt[5] * Mt[7]) + Mt[1] * (Mt[5] * Mt[6] - Mt[3] * Mt[8]) +
                                   Mt[2] * (Mt[3] * Mt[7] - Mt[4] * Mt[6]);
                const double sg = det < 0.0 ? -1.0 : 1.0;
#pragma unroll
                for (int k = 0; k < 9; k++) { Mt[k] = sg * Mt[k]; M[k] = Mt[k]; }
#pragma unroll
                for (int k = 0; k < 3; k++) t[k] = sg * t[k];
                rs_polar(M);
                double mu = 0.0;
#pragma unroll
                for (int k = 0; k < 9; k++) mu += M[k] * Mt[k];
                mu = mu / 3.0;
#pragma unroll
                for (int k = 0; k < 3; k++) t[k] = t[k] / mu;
                new_pose = true;
                mode = RS_EVAL_SPACE;
            }
        } else if (mode == RS_EVAL_SPACE) {
            have_cand = wave_uniform(isfinite(sA[27]));
            if (!have_cand) cand_st = JAICOV_RESECT_NOT_FINITE;
            sP[RS_CAND + 6] = sA[27];
#pragma unroll
            for (int k = 0; k < 6; k++) sP[RS_CAND + k] = sP[RS_PAR + k];
            mode = RS_PLANE;
        } else if (mode == RS_PLANE) {
            plane_st = wave_solve_lds(8, sA, sA + 36, sV);
            choose = plane_st != JAICOV_RESECT_OK;
            if (plane_st == JAICOV_RESECT_OK) {
                const double *h = sA + 36, *E = sP + RS_E;
                const double l1 = sqrt(h[0] * h[0] + h[3] * h[3] + h[6] * h[6]), l2 = sqrt(h[1] * h[1] + h[4] * h[4] + h[7] * h[7]);
                const double lam = (l1 + l2) / 2.0, sg = c > 0.0 ? -1.0 : 1.0;                    // c t3 < 0, t3 = sg / lam
                const double r1[3] = {sg * (h[0] / lam), sg * (h[3] / lam), sg * (h[6] / lam)};
                const double r2[3] = {sg * (h[1] / lam), sg * (h[4] / lam), sg * (h[7] / lam)};
                t[0] = sg * (h[2] / lam); t[1] = sg * (h[5] / lam); t[2] = sg * (1.0 / lam);
                const double r3[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
                double B[9] = {r1[0], r2[0], r3[0], r1[1], r2[1], r3[1], r1[2], r2[2], r3[2]};           // columns r1 r2 r3
                rs_polar(B);
#pragma unroll
                for (int i = 0; i < 3; i++)                                                           // B [e1 e2 n]': the rows of E
#pragma unroll
                    for (int j = 0; j < 3; j++) M[3 * i + j] = B[3 * i] * E[j] + B[3 * i + 1] * E[3 + j] + B[3 * i + 2] * E[6 + j];
                new_pose = true;
                mode = RS_EVAL_PLANE;
            }
        } else if (mode == RS_EVAL_PLANE) {
            plane_st = wave_uniform(isfinite(sA[27])) ? JAICOV_RESECT_OK : JAICOV_RESECT_NOT_FINITE;
            choose = true;
        } else if (mode == RS_STEP) {
            double A[21], b[6], dx[6];
#pragma unroll
            for (int k = 0; k < 21; k++) A[k] = sA[k];
#pragma unroll
            for (int k = 0; k < 6; k++) b[k] = sA[21 + k];
            int ss = wave_solve<6>(A, b, dx, nullptr);
            iters++;
            if (ss == JAICOV_RESECT_OK) {
                double z = 0.0;                           // NaN unless every value is finite
#pragma unroll
                for (int k = 0; k < 6; k++) z += dx[k] * 0.0;
                if (wave_uniform(z != 0.0)) ss = JAICOV_RESECT_NOT_FINITE;
            }
            if (ss != JAICOV_RESECT_OK) {
                failed = ss;
            } else {
                double step = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) { sP[RS_PAR + k] = sP[RS_PAR + k] + dx[k]; step = fmax(step, fabs(dx[k])); }
                new_angles = true;
                if (wave_uniform(step <= SQRT_EPS)) { st = JAICOV_RESECT_OK; mode = RS_EVAL; }
                else if (++it >= max_iter) mode = RS_EVAL;
            }
        } else {                                          // RS_EVAL: Q is taken from these sums after the loop
            if (wave_uniform(thr2 > 0.0 && nused > min_points && qmax > thr2 && qidx < m)) {
                if (lane == 0) { used[k0 + qidx] = 0; if (resident) sused[qidx] = 0; }
                __syncthreads();                          // the withdrawal is visible to every lane before the next pass reads it
                nused--;
                mode = RS_CENTROID;
            } else {
                break;
            }
        }
        if (choose) {                  // the choice: the smaller Omega at the start values, on a tie the plane start
            const bool have_plane = plane_st == JAICOV_RESECT_OK;
            if (!have_plane && !have_cand) {
                failed = plane_st == JAICOV_RESECT_NOT_FINITE || cand_st == JAICOV_RESECT_NOT_FINITE ? JAICOV_RESECT_NOT_FINITE
                                                                                                     : JAICOV_RESECT_SINGULAR;
            } else if (wave_uniform(have_cand && (!have_plane || sP[RS_CAND + 6] < sA[27]))) {
#pragma unroll
                for (int k = 0; k < 6; k++) sP[RS_PAR + k] = sP[RS_CAND + k];
                new_angles = true;
                kind = JAICOV_RESECT_START_SPACE;
            } else {
                kind = JAICOV_RESECT_START_PLANE;
            }
            mode = RS_STEP;
        }
        if (new_pose) { rs_pose(lane, M, t, sP + RS_PAR); new_angles = true; }
    }
    double o[JAICOV_RESECT_OUT_PER_IMAGE];
    if (failed < 0) {
        double A[21], b[6], Q[21];
#pragma unroll
        for (int k = 0; k < 21; k++) A[k] = sA[k];
#pragma unroll
        for (int k = 0; k < 6; k++) b[k] = sA[21 + k];
        const int se = wave_solve<6>(A, b, nullptr, Q);
        if (se != JAICOV_RESECT_OK) failed = se;
        const double s = sP[RS_S];
#pragma unroll
        for (int k = 0; k < 3; k++) { o[k] = sP[RS_XC + k] + s * sP[RS_PAR + k]; o[3 + k] = sP[RS_PAR + 3 + k]; }
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = i; j < 6; j++) {
                const double f = (i < 3 ? s : 1.0) * (j < 3 ? s : 1.0);     // X0 = Xc + s X0r
                o[6 + tri_ix<6>(i, j)] = Q[tri_ix<6>(i, j)] * f;
            }
        o[27] = sA[27];
        double z = 0.0;
#pragma unroll
        for (int k = 0; k < JAICOV_RESECT_OUT_PER_IMAGE; k++) z += o[k] * 0.0;
        if (failed < 0 && wave_uniform(z != 0.0)) failed = JAICOV_RESECT_NOT_FINITE;
    }
    if (failed >= 0) {                                    // start kind 0
        wave_fail_item<3>(lane, og, JAICOV_RESECT_OUT_PER_IMAGE, outcome, g, failed, iters, k0, m, used, obs_q);
        return;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < JAICOV_RESECT_OUT_PER_IMAGE; k++) og[k] = o[k];
        outcome[3L * g] = st;
        outcome[3L * g + 1] = iters;
        outcome[3L * g + 2] = kind;
    }
}

}  // namespace
}  // namespace jaicov

using namespace jaicov;

extern "C" int jaicov_resect_images(int32_t n_images, const int32_t *obs_begin, const double *xy, const double *xyz, const double *var,
                                    const double *image_io, const double *eo_start, double sigma2apriori, int32_t max_iterations,
                                    double reject_threshold, int32_t min_points, double *out, int32_t *status, int32_t *iterations,
                                    int32_t *start_kind, uint8_t *obs_used, double *obs_q, double *ms_out) {
    // argument checks, host only
    if (n_images < 0 || !obs_begin) return JAICOV_ERR_BAD_ARGUMENT;
    if (!(sigma2apriori > 0.0) || max_iterations < 1 || min_points < 3 || !(reject_threshold >= 0.0)) return JAICOV_ERR_BAD_ARGUMENT;
    if (n_images > 0 && (!out || !status || !image_io)) return JAICOV_ERR_BAD_ARGUMENT;
    if (!ranges_ok(n_images, obs_begin)) return JAICOV_ERR_BAD_ARGUMENT;
    const long n_obs = obs_begin[n_images];
    if (n_obs > 0 && (!xy || !xyz)) return JAICOV_ERR_BAD_ARGUMENT;
    if (!dispersions_ok(var, n_obs)) return JAICOV_ERR_BAD_ARGUMENT;

    if (!device_is_gfx950()) return JAICOV_ERR_NO_DEVICE;
    if (ms_out) *ms_out = 0.0;
    if (n_images == 0) return JAICOV_OK;

    BatchCall call;
    const size_t ni = (size_t)n_images, no = (size_t)n_obs;
    const int32_t *d_begin = call.in(obs_begin, ni + 1);
    const double *d_xy = call.in(xy, 2 * no), *d_xyz = call.in(xyz, 3 * no), *d_var = call.in(var, 3 * no), *d_io = call.in(image_io, 3 * ni),
                 *d_eo = call.in(eo_start, 6 * ni);
    double *d_out = call.alloc<double>(JAICOV_RESECT_OUT_PER_IMAGE * ni), *d_q = obs_q ? call.alloc<double>(no) : nullptr;
    int32_t *d_outcome = call.alloc<int32_t>(3 * ni);
    uint8_t *d_used = call.filled<uint8_t>(no, 1);                     // every observation starts as used
    call.run([&](hipStream_t s) {
        hipLaunchKernelGGL(resect_images_kernel, dim3(n_images), dim3(RESECT_LANES), 0, s, d_begin, d_xy, d_xyz, d_var, d_io, d_eo, sigma2apriori,
                           (int)max_iterations, reject_threshold * reject_threshold, (int)min_points, d_out, d_outcome, d_used, d_q);
    });
    call.out(out, d_out, JAICOV_RESECT_OUT_PER_IMAGE * ni);
    call.outcomes(d_outcome, ni, 3, status, iterations, start_kind);
    call.out(obs_used, d_used, no);
    call.out(obs_q, d_q, no);
    return call.finish(ms_out);
}
