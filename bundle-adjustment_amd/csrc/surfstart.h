// Start values of cylinders and cones by a search over candidate axes (include/jaicov_surfaces.h: the header is the specification).
//
//   surf_start_kernel   one wave and one workgroup per form.  Lane l takes the candidates l, l + 64, ...: each lane runs its own
//                       linear least squares (a Jacobi-scaled Cholesky of order 5 in registers, fully unrolled) and its own cost
//                       over the members, which all lanes read from LDS at the same address.  The wave then agrees on the smallest
//                       cost by an xor butterfly and the winner's lane hands out its parameters.
// It writes row g of `start` and nothing else; a row that the caller gave, a form of another type and a form that the fit kernel
// refuses for its size are left alone.  A form without a candidate keeps its NaN, which the fit kernel reports as DEGENERATE.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/jaicov_surfaces.h"
#include "wavealg.h"

#pragma clang fp contract(off)

namespace jaicov {

constexpr int SURF_REACH = 5;                                                                        // max(|i|, |j|, |l|) of a candidate
constexpr int SURF_CANDIDATES = ((2 * SURF_REACH + 1) * (2 * SURF_REACH + 1) * (2 * SURF_REACH + 1) -
                                 (2 * SURF_REACH - 1) * (2 * SURF_REACH - 1) * (2 * SURF_REACH - 1)) / 2;
static_assert(SURF_CANDIDATES == 301, "the header counts them");

struct SurfCandidates { signed char v[SURF_CANDIDATES][3]; };
constexpr SurfCandidates surf_candidates() {
    SurfCandidates c{};
    int n = 0;
    for (int i = -SURF_REACH; i <= SURF_REACH; i++)
        for (int j = -SURF_REACH; j <= SURF_REACH; j++)
            for (int l = -SURF_REACH; l <= SURF_REACH; l++) {
                const int ai = i < 0 ? -i : i, aj = j < 0 ? -j : j, al = l < 0 ? -l : l;
                const int big = ai > aj ? (ai > al ? ai : al) : (aj > al ? aj : al);
                const int first = i != 0 ? i : j != 0 ? j : l;
                if (big != SURF_REACH || first <= 0) continue;
                c.v[n][0] = (signed char)i; c.v[n][1] = (signed char)j; c.v[n][2] = (signed char)l;
                ++n;
            }
    return c;
}
__constant__ const SurfCandidates SURF_CAND = surf_candidates();

// the tangent basis of forms.hip (form_basis), declared there
__device__ inline void form_basis(double n0, double n1, double n2, double *e1, double *e2);

// N (packed upper, order 5) x = b in one lane: V_a = 1 / sqrt(N_aa), U'U = V N V, a pivot <= 2^-40 or a non-finite value: false
__device__ inline bool surf_solve5(double *U, const double *b, double *x) {
    constexpr int N = 5;
    const double PIVOT = ldexp(1.0, -40);
    double V[N];
#pragma unroll
    for (int i = 0; i < N; i++) V[i] = U[tri_ix<N>(i, i)] > 0.0 ? 1.0 / sqrt(U[tri_ix<N>(i, i)]) : 1.0;
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = i; j < N; j++) U[tri_ix<N>(i, j)] = U[tri_ix<N>(i, j)] * (V[i] * V[j]);
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < j; k++) s += U[tri_ix<N>(k, j)] * U[tri_ix<N>(k, j)];
        const double p = U[tri_ix<N>(j, j)] - s;
        ok = ok && p > PIVOT;
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
    return ok;
}

// Form g of type ftype[g] with the members fbegin[g] .. fbegin[g + 1] of fpoint; start [n][7], row g is written if its first entry is NaN
__global__ __launch_bounds__(64) void surf_start_kernel(const double *__restrict__ vals, const int32_t *__restrict__ ftype,
                                                        const int32_t *__restrict__ fbegin, const int32_t *__restrict__ fpoint,
                                                        double *__restrict__ start) {
    __shared__ double X[3][JAICOV_FORM_MAX_ROWS];
    const int g = blockIdx.x, lane = threadIdx.x;
    const int type = wave_uniform(ftype[g]);
    if (type != JAICOV_SURF_CYLINDER && type != JAICOV_SURF_CONE) return;
    const bool cone = type == JAICOV_SURF_CONE;
    const int m0 = wave_uniform(fbegin[g]), k = wave_uniform(fbegin[g + 1]) - m0;
    if (k < (cone ? 6 : 5) || k > JAICOV_FORM_MAX_ROWS) return;
    double *row = start + (size_t)JAICOV_FORM_MAX_PARAMS * g;
    const double first = row[0];
    if (wave_uniform(first == first)) return;

    // ---- the members, their centroid in member order, y = x / extent
    if (lane < k) {
        const int p = fpoint[m0 + lane];
#pragma unroll
        for (int a = 0; a < 3; a++) X[a][lane] = vals[3 * (size_t)p + a];
    }
    __syncthreads();
    double G[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < k; i++) { G[0] += X[0][i]; G[1] += X[1][i]; G[2] += X[2][i]; }
    G[0] = G[0] / (double)k; G[1] = G[1] / (double)k; G[2] = G[2] / (double)k;
    __syncthreads();
    if (lane < k) { X[0][lane] = X[0][lane] - G[0]; X[1][lane] = X[1][lane] - G[1]; X[2][lane] = X[2][lane] - G[2]; }
    __syncthreads();
    double ext = 0.0;
    for (int i = 0; i < k; i++) {
        const double x = X[0][i], y = X[1][i], z = X[2][i];
        ext = fmax(ext, sqrt(x * x + y * y + z * z));
    }
    __syncthreads();
    if (lane < k) { X[0][lane] = X[0][lane] / ext; X[1][lane] = X[1][lane] / ext; X[2][lane] = X[2][lane] / ext; }
    __syncthreads();

    // ---- the lane's candidates: the best of them stays in (cost, best, th, sig)
    double cost = INFINITY, th[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, sig = 1.0;
    int best = SURF_CANDIDATES;
    for (int ci = lane; ci < SURF_CANDIDATES; ci += 64) {
        const double i0 = (double)SURF_CAND.v[ci][0], i1 = (double)SURF_CAND.v[ci][1], i2 = (double)SURF_CAND.v[ci][2];
        const double len = sqrt((i0 * i0 + i1 * i1) + i2 * i2);
        const double d0 = i0 / len, d1 = i1 / len, d2 = i2 / len;
        double e1[3], e2[3];
        form_basis(d0, d1, d2, e1, e2);
        double Nn[15], bn[5], x[5];
#pragma unroll
        for (int a = 0; a < 15; a++) Nn[a] = 0.0;
#pragma unroll
        for (int a = 0; a < 5; a++) bn[a] = 0.0;
        for (int i = 0; i < k; i++) {
            const double px = X[0][i], py = X[1][i], pz = X[2][i];
            const double q0 = (e1[0] * px + e1[1] * py) + e1[2] * pz, q1 = (e2[0] * px + e2[1] * py) + e2[2] * pz;
            const double s = (d0 * px + d1 * py) + d2 * pz;
            const double a[5] = {2.0 * q0, 2.0 * q1, 1.0, cone ? s * s : 0.0, cone ? 2.0 * s : 0.0};
            const double rhs = q0 * q0 + q1 * q1;
#pragma unroll
            for (int r = 0; r < 5; r++) {
#pragma unroll
                for (int c = r; c < 5; c++) Nn[tri_ix<5>(r, c)] += a[r] * a[c];
                bn[r] += a[r] * rhs;
            }
        }
        // the cylinder has three unknowns: the two others get N_aa = 1 and stay 0, the leading factor is that of order 3
        if (!cone) { Nn[tri_ix<5>(3, 3)] = 1.0; Nn[tri_ix<5>(4, 4)] = 1.0; }
        bool ok = surf_solve5(Nn, bn, x);
        double c = 0.0, sg = 1.0;
        if (!cone) {
            const double r2 = x[2] + (x[0] * x[0] + x[1] * x[1]);
            ok = ok && r2 > 0.0;
            const double r = sqrt(r2);
            for (int i = 0; i < k; i++) {
                const double px = X[0][i], py = X[1][i], pz = X[2][i];
                const double q0 = ((e1[0] * px + e1[1] * py) + e1[2] * pz) - x[0], q1 = ((e2[0] * px + e2[1] * py) + e2[2] * pz) - x[1];
                const double f = sqrt(q0 * q0 + q1 * q1) - r;
                c += f * f;
            }
            x[3] = r;
        } else {
            ok = ok && x[3] > 0.0;
            const double kappa = sqrt(x[3]), r0 = x[4] / kappa, sa = -(r0 / kappa);
            double sw = 0.0;
            for (int i = 0; i < k; i++) sw += ((d0 * X[0][i] + d1 * X[1][i]) + d2 * X[2][i]) - sa;
            if (sw < 0.0) sg = -1.0;
            for (int i = 0; i < k; i++) {
                const double px = X[0][i], py = X[1][i], pz = X[2][i];
                const double q0 = ((e1[0] * px + e1[1] * py) + e1[2] * pz) - x[0], q1 = ((e2[0] * px + e2[1] * py) + e2[2] * pz) - x[1];
                const double s = (d0 * px + d1 * py) + d2 * pz;
                const double f = sqrt(q0 * q0 + q1 * q1) - (sg * kappa) * (s - sa);
                c += f * f;
            }
            c = c / (1.0 + x[3]);
            x[3] = kappa; x[4] = sa;
        }
        if (ok && c < cost) {                                   // NaN and +inf never win; the lane's candidates ascend
            cost = c; best = ci; sig = sg;
#pragma unroll
            for (int a = 0; a < 5; a++) th[a] = x[a];
        }
    }
    // ---- the wave's winner: the smallest cost, the lowest index among equals
    double wc = cost;
    int wi = best;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double oc = __shfl_xor(wc, off);
        const int oi = __shfl_xor(wi, off);
        if (oc < wc || (oc == wc && oi < wi)) { wc = oc; wi = oi; }
    }
    wi = wave_uniform(wi);
    if (wi >= SURF_CANDIDATES) return;
    const int src = wi & 63;
    const double c1 = __shfl(th[0], src), c2 = __shfl(th[1], src), t3 = __shfl(th[3], src), t4 = __shfl(th[4], src), sgw = __shfl(sig, src);
    if (lane == 0) {
        const double i0 = (double)SURF_CAND.v[wi][0], i1 = (double)SURF_CAND.v[wi][1], i2 = (double)SURF_CAND.v[wi][2];
        const double len = sqrt((i0 * i0 + i1 * i1) + i2 * i2);
        const double d[3] = {i0 / len, i1 / len, i2 / len};
        double e1[3], e2[3];
        form_basis(d[0], d[1], d[2], e1, e2);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double foot = c1 * e1[a] + c2 * e2[a];
            row[a] = ext * (cone ? foot + t4 * d[a] : foot) + G[a];
            row[3 + a] = sgw * d[a];
        }
        row[6] = cone ? atan(t3) : ext * t3;
    }
}

}  // namespace jaicov
