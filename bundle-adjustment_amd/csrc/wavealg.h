// wavealg.h -- the small algebra that the single-wave start-value kernels (intersect.hip, resect.hip, relorient.hip, simil.hip) run on
// wave-uniform values.  What the kernels rely on:
//   Every lane runs these routines on the same words.  Their inputs come out of an xor butterfly, whose order is fixed and which
//   leaves the same bits in every lane, so every lane computes the same results and every branch is taken by the whole wave.  The
//   compiler cannot know that: wave_uniform says so, or it would mask every such branch lane by lane and keep both sides' values
//   alive across it.
//   The LDS variants (wave_solve_lds) read and rewrite their system in place.  Every lane stores what every other lane stores, and no
//   barrier stands between such a store and the reads that follow: the workgroup is one wave, and the LDS operations of one wave
//   complete in order.  With more than one wave per workgroup none of it would hold.
// Floating-point contraction is off in this header: every product and sum is rounded on its own, in the order written here, which is
// the order of the restatements in tests/resection_reference.py (solve, rotate, eigen).
// The intersection's isect_solve3 is not here: it is a hand-unrolled solve of order 3 with another summation order and a restatement
// of its own (tests/intersect_reference.py: solve3).
// Also here, once for all four kernels: R(omega, phi, kappa) (rotation.h), the lane idioms around it (wave_sincos3, wave_angles) and
// what a failed item leaves behind (wave_fail_item).
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#ifdef JAICOV_OBSMODEL_H
#error "wavealg.h after obsmodel.h: obs_weight would keep the engine's contraction in the start-value algebra"
#endif
#define JAICOV_WAVEALG_H
#pragma clang fp contract(off)

#include "obsweight.h"     // below the pragma: obs_weight and
#include "rotation.h"      // R(omega, phi, kappa) with every product and sum rounded on its own

namespace jaicov {

// what a solve returns; the public JAICOV_*_OK, _SINGULAR and _NOT_FINITE of the calls that use it have these values
enum WaveStatus { WAVE_OK = 0, WAVE_SINGULAR = 3, WAVE_NOT_FINITE = 4 };

// a value that is the same in every lane, said so to the compiler
__device__ inline int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline bool wave_uniform(bool v) { return __builtin_amdgcn_readfirstlane((int)v) != 0; }

// index of (i, j >= i) in an upper triangle of order N packed row by row
template <int N>
__device__ constexpr int tri_ix(int i, int j) { return i * N - i * (i - 1) / 2 + (j - i); }

// A (packed upper, order N) x = b by Jacobi preconditioning (NES:82-91) and Cholesky; Q (may be NULL, packed upper): the inverse of A.
// A is overwritten by the factor, so that no second triangle is live beside the caller's sums.  Everything is unrolled into registers.
template <int N>
__device__ inline WaveStatus wave_solve(double *U, const double *b, double *x, double *Q) {
    const double EPS = ldexp(1.0, -53), SQRT_EPS = sqrt(EPS);
    constexpr int LEN = N * (N + 1) / 2;
    double z = 0.0;                       // NaN unless every value is finite
#pragma unroll
    for (int k = 0; k < LEN; k++) z += U[k] * 0.0;
#pragma unroll
    for (int k = 0; k < N; k++) z += b[k] * 0.0;
    if (wave_uniform(z != 0.0)) return WAVE_NOT_FINITE;
    double V[N];                          // U'U = V A V, U upper
#pragma unroll
    for (int i = 0; i < N; i++) V[i] = U[tri_ix<N>(i, i)] > EPS ? 1.0 / sqrt(U[tri_ix<N>(i, i)]) : 1.0;
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = i; j < N; j++) U[tri_ix<N>(i, j)] = U[tri_ix<N>(i, j)] * (V[i] * V[j]);
    bool singular = false;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < j; k++) s += U[tri_ix<N>(k, j)] * U[tri_ix<N>(k, j)];
        const double p = U[tri_ix<N>(j, j)] - s;
        singular = singular || !(p > SQRT_EPS);
        const double d = sqrt(p);
        U[tri_ix<N>(j, j)] = d;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double r = 0.0;
#pragma unroll
            for (int k = 0; k < j; k++) r += U[tri_ix<N>(k, i)] * U[tri_ix<N>(k, j)];
            U[tri_ix<N>(j, i)] = (U[tri_ix<N>(j, i)] - r) / d;
        }
    }
    if (wave_uniform(singular)) return WAVE_SINGULAR;             // every pivot after the first bad one is garbage and is not used
    if (x) {
        double y[N];
#pragma unroll
        for (int i = 0; i < N; i++) {
            double r = 0.0;
#pragma unroll
            for (int k = 0; k < i; k++) r += U[tri_ix<N>(k, i)] * y[k];
            y[i] = (V[i] * b[i] - r) / U[tri_ix<N>(i, i)];
        }
#pragma unroll
        for (int i = N - 1; i >= 0; i--) {
            double r = 0.0;
#pragma unroll
            for (int k = i + 1; k < N; k++) r += U[tri_ix<N>(i, k)] * y[k];
            y[i] = (y[i] - r) / U[tri_ix<N>(i, i)];
        }
#pragma unroll
        for (int i = 0; i < N; i++) x[i] = V[i] * y[i];
    }
    if (Q) {
        double W[LEN];                    // W = inverse of U, upper: W[i][j], j >= i
#pragma unroll
        for (int j = 0; j < N; j++) {
            W[tri_ix<N>(j, j)] = 1.0 / U[tri_ix<N>(j, j)];
#pragma unroll
            for (int i = j - 1; i >= 0; i--) {
                double r = 0.0;
#pragma unroll
                for (int k = i + 1; k <= j; k++) r += U[tri_ix<N>(i, k)] * W[tri_ix<N>(k, j)];
                W[tri_ix<N>(i, j)] = -r / U[tri_ix<N>(i, i)];
            }
        }
#pragma unroll
        for (int i = 0; i < N; i++)
#pragma unroll
            for (int j = i; j < N; j++) {                 // inverse of V A V = W W'
                double r = 0.0;
#pragma unroll
                for (int k = j; k < N; k++) r += W[tri_ix<N>(i, k)] * W[tri_ix<N>(j, k)];
                Q[tri_ix<N>(i, j)] = r * (V[i] * V[j]);
            }
    }
    return WAVE_OK;
}

// The same solve on a system of order n held in LDS: U (packed upper, overwritten by the factor), b (overwritten by x), V (n words).
// Its loops stay rolled: a triangle of order 11 unrolled into registers beside a pass's sums does not fit the register file.
__device__ inline WaveStatus wave_solve_lds(int n, double *U, double *b, double *V) {
    const double EPS = ldexp(1.0, -53), SQRT_EPS = sqrt(EPS);
    auto ix = [n](int i, int j) { return i * n - i * (i - 1) / 2 + (j - i); };
    bool finite = true;
    for (int k = 0; k < n * (n + 1) / 2; k++) finite = finite && isfinite(U[k]);
    for (int k = 0; k < n; k++) finite = finite && isfinite(b[k]);
    if (wave_uniform(!finite)) return WAVE_NOT_FINITE;
    for (int i = 0; i < n; i++) V[i] = U[ix(i, i)] > EPS ? 1.0 / sqrt(U[ix(i, i)]) : 1.0;
    for (int i = 0; i < n; i++)
        for (int j = i; j < n; j++) U[ix(i, j)] = U[ix(i, j)] * (V[i] * V[j]);
    for (int j = 0; j < n; j++) {
        double s = 0.0;
        for (int k = 0; k < j; k++) s += U[ix(k, j)] * U[ix(k, j)];
        const double p = U[ix(j, j)] - s;
        if (wave_uniform(!(p > SQRT_EPS))) return WAVE_SINGULAR;
        const double d = sqrt(p);
        U[ix(j, j)] = d;
        for (int i = j + 1; i < n; i++) {
            double r = 0.0;
            for (int k = 0; k < j; k++) r += U[ix(k, i)] * U[ix(k, j)];
            U[ix(j, i)] = (U[ix(j, i)] - r) / d;
        }
    }
    for (int i = 0; i < n; i++) {
        double r = 0.0;
        for (int k = 0; k < i; k++) r += U[ix(k, i)] * b[k];
        b[i] = (V[i] * b[i] - r) / U[ix(i, i)];
    }
    for (int i = n - 1; i >= 0; i--) {
        double r = 0.0;
        for (int k = i + 1; k < n; k++) r += U[ix(i, k)] * b[k];
        b[i] = (b[i] - r) / U[ix(i, i)];
    }
    for (int i = 0; i < n; i++) b[i] = V[i] * b[i];
    return WAVE_OK;
}

// ---- Lane-parallel routines on a packed upper triangle of order n <= 64 in LDS, for one wave per workgroup (forms.hip).  Where
// wave_solve_lds has every lane repeat the whole serial solve, these give lane i the entries of index i; the sum of every entry
// still runs over r in one fixed order, so the bits do not depend on which lane forms it.  A barrier stands between the stores of
// one column and the loads of the next: with one wave it costs nothing and tells the compiler what the hardware does anyway.

// index of (i, j >= i) in an upper triangle of order n packed row by row
__device__ inline int tri_ix_n(int n, int i, int j) { return i * n - i * (i - 1) / 2 + (j - i); }

// The scaling in front of wave_chol_lds, A (packed upper) in place: powers of two bring the diagonal into [1, 4) without rounding,
// whatever its magnitude (Sc), then the Jacobi scaling to a unit diagonal (Sv); row i of the system takes Sc[i] Sv[i].  z, to which
// the caller has added 0 x its own values, comes back NaN in some lane unless every entry of A is finite too.
__device__ inline void wave_equilibrate_lds(int n, double *U, double *Sc, double *Sv, double &z, int lane) {
    const double EPS = ldexp(1.0, -53);
    if (lane < n) {
        const double qd = U[tri_ix_n(n, lane, lane)];
        Sc[lane] = (qd > 0.0 && isfinite(qd)) ? ldexp(1.0, -(ilogb(qd) >> 1)) : 1.0;
    }
    __syncthreads();
    for (int i = 0; i < n; i++) {
        const int j = i + lane;
        if (j < n) {
            const double a = U[tri_ix_n(n, i, j)];
            z += a * 0.0;
            U[tri_ix_n(n, i, j)] = a * (Sc[i] * Sc[j]);
        }
    }
    __syncthreads();
    if (lane < n) {
        const double a = U[tri_ix_n(n, lane, lane)];
        Sv[lane] = a > EPS ? 1.0 / sqrt(a) : 1.0;
    }
    __syncthreads();
    for (int i = 0; i < n; i++) {
        const int j = i + lane;
        if (j < n) U[tri_ix_n(n, i, j)] = U[tri_ix_n(n, i, j)] * (Sv[i] * Sv[j]);
    }
    __syncthreads();
}

// U'U = A in place (A packed upper, already scaled to a unit diagonal).  At column j every lane forms the pivot, lane i > j the
// entry U_ji: p = U_jj - sum_{r<j} U_rj U_rj; U_ji = (U_ji - sum_{r<j} U_ri U_rj) / sqrt(p), r ascending.
__device__ inline WaveStatus wave_chol_lds(int n, double *U, int lane) {
    const double SQRT_EPS = sqrt(ldexp(1.0, -53));
    for (int j = 0; j < n; j++) {
        const bool mine = lane > j && lane < n;
        const int li = mine ? lane : j;                // a lane without an entry follows the pivot's loads
        double sp = 0.0, si = 0.0;
        for (int r = 0; r < j; r++) {
            const double a = U[tri_ix_n(n, r, j)];
            sp += a * a;
            si += U[tri_ix_n(n, r, li)] * a;
        }
        const double p = U[tri_ix_n(n, j, j)] - sp;
        if (wave_uniform(!(p > SQRT_EPS))) return WAVE_SINGULAR;
        const double d = sqrt(p);
        const double uji = U[tri_ix_n(n, j, li)];
        __syncthreads();
        if (mine) U[tri_ix_n(n, j, lane)] = (uji - si) / d;
        if (lane == j) U[tri_ix_n(n, j, j)] = d;
        __syncthreads();
    }
    return WAVE_OK;
}

// U' Z = B for NR right-hand sides at once, reusing the factor: lane i holds row i of B in z and leaves row i of Z there.
// z_i = (b_i - sum_{r<i} U_ri z_r) / U_ii, r ascending.  Lanes >= n keep what they had.
template <int NR>
__device__ inline void wave_forward_lds(int n, const double *U, double (&z)[NR], int lane) {
    double acc[NR];
#pragma unroll
    for (int c = 0; c < NR; c++) acc[c] = 0.0;
    for (int r = 0; r < n; r++) {
        const double urr = U[tri_ix_n(n, r, r)];
        const double uri = (lane > r && lane < n) ? U[tri_ix_n(n, r, lane)] : 0.0;
#pragma unroll
        for (int c = 0; c < NR; c++) {
            if (lane == r) z[c] = (z[c] - acc[c]) / urr;
            const double zr = __shfl(z[c], r);
            acc[c] += uri * zr;
        }
    }
}

// U z = y for one right-hand side: lane i holds y_i and leaves z_i.  z_i = (y_i - sum_{r>i} U_ir z_r) / U_ii, r descending.
__device__ inline void wave_backward_lds(int n, const double *U, double &y, int lane) {
    double acc = 0.0;
    for (int r = n - 1; r >= 0; r--) {
        const double urr = U[tri_ix_n(n, r, r)];
        const double uir = lane < r ? U[tri_ix_n(n, lane, r)] : 0.0;
        if (lane == r) y = (y - acc) / urr;
        const double yr = __shfl(y, r);
        acc += uir * yr;
    }
}

// Z = the inverse of the factor U (both packed upper, Z apart from U): lane j solves U z = e_j for column j,
// Z_jj = 1 / U_jj, Z_ij = -(sum_{k=i+1..j} U_ik Z_kj) / U_ii for i = j-1 .. 0, k ascending.  A lane reads no column but its own.
__device__ inline void wave_trinv_lds(int n, const double *U, double *Z, int lane) {
    if (lane < n) {
        const int j = lane;
        Z[tri_ix_n(n, j, j)] = 1.0 / U[tri_ix_n(n, j, j)];
        for (int i = j - 1; i >= 0; i--) {
            double r = 0.0;
            for (int k = i + 1; k <= j; k++) r += U[tri_ix_n(n, i, k)] * Z[tri_ix_n(n, k, j)];
            Z[tri_ix_n(n, i, j)] = -r / U[tri_ix_n(n, i, i)];
        }
    }
    __syncthreads();
}

// the Jacobi rotation that annuls a_pq: t = tan, c = cos, s = sin of its angle
__device__ inline void jacobi_angle(double app, double aqq, double apq, double &t, double &c, double &s) {
    const double theta = (aqq - app) / (2.0 * apq);
    t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    c = 1.0 / sqrt(t * t + 1.0);
    s = t * c;
}

// one Jacobi rotation in the plane (p, q) of a symmetric 3 x 3 matrix; r is the third index; wp, wq: the eigenvector rows p and q
__device__ inline void jacobi_rotate3(double &app, double &aqq, double &apq, double &arp, double &arq, double *wp, double *wq) {
    if (wave_uniform(apq == 0.0)) return;
    double t, c, s;
    jacobi_angle(app, aqq, apq, t, c, s);
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    app = app - t * apq; aqq = aqq + t * apq; apq = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double vp = c * wp[k] - s * wq[k], vq = s * wp[k] + c * wq[k];
        wp[k] = vp; wq[k] = vq;
    }
}

// eigenvalues (falling) and eigenvectors (rows of E, det = +1) of the symmetric matrix S (00 01 02 11 12 22), by SWEEPS cyclic sweeps
template <int SWEEPS>
__device__ inline void wave_eigen3(const double *S, double *lam, double *E) {
    double a00 = S[0], a01 = S[1], a02 = S[2], a11 = S[3], a12 = S[4], a22 = S[5];
    double W[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < SWEEPS; sweep++) {
        jacobi_rotate3(a00, a11, a01, a02, a12, W, W + 3);
        jacobi_rotate3(a00, a22, a02, a01, a12, W, W + 6);
        jacobi_rotate3(a11, a22, a12, a01, a02, W + 3, W + 6);
    }
    auto order = [&](double &la, double &lb, double *wa, double *wb) {      // the larger eigenvalue first; equal ones keep their order
        if (wave_uniform(!(la < lb))) return;
        const double l = la; la = lb; lb = l;
#pragma unroll
        for (int k = 0; k < 3; k++) { const double w = wa[k]; wa[k] = wb[k]; wb[k] = w; }
    };
    order(a00, a11, W, W + 3);
    order(a11, a22, W + 3, W + 6);
    order(a00, a11, W, W + 3);
    const double n0 = W[1] * W[5] - W[2] * W[4], n1 = W[2] * W[3] - W[0] * W[5], n2 = W[0] * W[4] - W[1] * W[3];   // e1 x e2
    if (n0 * W[6] + n1 * W[7] + n2 * W[8] < 0.0) { W[6] = -W[6]; W[7] = -W[7]; W[8] = -W[8]; }
    lam[0] = a00; lam[1] = a11; lam[2] = a22;
#pragma unroll
    for (int k = 0; k < 9; k++) E[k] = W[k];
}

// one step of the xor butterfly over (largest q, lowest index among equal values)
__device__ inline void wave_argmax_combine(double &qmax, int &qidx, int off) {
    const double oq = __shfl_xor(qmax, off);
    const int oi = __shfl_xor(qidx, off);
    if (oq > qmax || (oq == qmax && oi < qidx)) { qmax = oq; qidx = oi; }
}

// sines and cosines of three wave-uniform angles: lanes 0, 1, 2 take one angle each and hand its pair to the wave, so that a kernel
// holds one copy of sincos and of its constants, not three.  (resect.hip keeps lines of its own for this: see rs_rotation there.)
__device__ inline void wave_sincos3(int lane, double a0, double a1, double a2, double &s0, double &c0, double &s1, double &c1, double &s2,
                                    double &c2) {
    const double angle = lane == 0 ? a0 : lane == 1 ? a1 : a2;
    double sn, cs;
    sincos(angle, &sn, &cs);
    s0 = __shfl(sn, 0); c0 = __shfl(cs, 0); s1 = __shfl(sn, 1); c1 = __shfl(cs, 1); s2 = __shfl(sn, 2); c2 = __shfl(cs, 2);
}

// omega, phi, kappa of R(omega, phi, kappa) from its entries r23, r33, r12, r11, r13 (rotation.h) into ang[0 .. 2]: omega by lane 0,
// kappa by lane 1 (one copy of atan2), phi with r13 held to [-1, 1]
__device__ inline void wave_angles(int lane, double r23, double r33, double r12, double r11, double r13, double *ang) {
    const double a = atan2(lane == 0 ? -r23 : -r12, lane == 0 ? r33 : r11);
    ang[0] = __shfl(a, 0);
    ang[1] = asin(fmin(1.0, fmax(-1.0, r13)));
    ang[2] = __shfl(a, 1);
}

// Item g has failed, taken by the whole wave: NaN in its n_values values and in q (may be NULL) of its m observations from k0 on,
// none of them used; its record among the outcome records of WIDTH words gets the status, the solves so far and, where WIDTH is
// 3, start kind 0.  It takes the records and g, not the item's record, the width at compile time, and g and the solve count (which
// two kernels keep in LDS) by reference: the index is formed and the count is read inside the lane-0 branch, not before the call.
// What must hold after a change here: the four kernels' entries of kernel_resources.json are what they were before it.
template <int WIDTH>
__device__ inline void wave_fail_item(int lane, double *values, int n_values, int32_t *outcome, const int &g, int st, const int &iters,
                                      long k0, int m, uint8_t *used, double *q) {
    static_assert(WIDTH == 2 || WIDTH == 3, "status and solves, or these and the start kind");
    if (lane < n_values) values[lane] = NAN;
    if (lane == 0) {
        outcome[(long)WIDTH * g] = st; outcome[(long)WIDTH * g + 1] = iters;
        if (WIDTH == 3) outcome[(long)WIDTH * g + 2] = 0;
    }
    for (int t = lane; t < m; t += 64) {
        used[k0 + t] = 0;
        if (q) q[k0 + t] = NAN;
    }
}

}  // namespace jaicov
