// Planes, spheres, lines and circles through adjusted object points, fitted on the device as a Gauss-Helmert model with the members'
// whole block of the cofactor matrix (include/jaicov_forms.h: the header is the specification, every formula is written out there).
//
//   form_fit_kernel   one wave and one workgroup per form.  The m x m matrix M = B Q_ll B' lives packed in LDS; B, A, w and lambda
//                     are held per row by the lanes.  M is formed from 3 x 3 blocks of Q read through the view (a lane takes the
//                     member pairs (i, i + lane)); Q_ll itself is never staged, and v = Q_ll B' lambda reads the blocks once more at
//                     the end of a step.  The factorisation and the substitutions are the lane-parallel routines of wavealg.h
//                     (wave_chol_lds, wave_forward_lds, wave_backward_lds, wave_trinv_lds); the system of the u <= 6 free
//                     parameters is solved by every lane with wave_solve<6>.
// Cylinders, cones and start values from the caller (include/jaicov_surfaces.h) are a second entry to the same kernel and the same host
// shell: form_fit_kernel<.., SURF>, with the start search of the two surfaces in surfstart.h (surf_start_kernel) in front of it.
// Nothing here writes to the cofactor matrix or to any other state of the engine but the work buffers of FormState.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/jaicov_forms.h"
#include "../../include/jaicov_surfaces.h"
#include "forms.h"
#include "qview.h"
#include "status.h"
#include "surfstart.h"
#include "wavealg.h"

#pragma clang fp contract(off)

namespace jaicov {

constexpr int FORM_R = JAICOV_FORM_MAX_ROWS;
constexpr int FORM_TRI = FORM_R * (FORM_R + 1) / 2;
constexpr int FORM_SWEEPS = 10;
static_assert(FORM_R == 64, "one row per lane of one wave");

// e1 = (e_k x n) / |e_k x n| with k the index of the smallest |n_k| (the first among equals), e2 = n x e1
__device__ inline void form_basis(double n0, double n1, double n2, double *e1, double *e2) {
    int k = 0;
    double am = fabs(n0);
    if (fabs(n1) < am) { k = 1; am = fabs(n1); }
    if (fabs(n2) < am) k = 2;
    double c0, c1, c2;
    if (k == 0) { c0 = 0.0; c1 = -n2; c2 = n1; }
    else if (k == 1) { c0 = n2; c1 = 0.0; c2 = -n0; }
    else { c0 = -n1; c1 = n0; c2 = 0.0; }
    const double l = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    e1[0] = c0 / l; e1[1] = c1 / l; e1[2] = c2 / l;
    e2[0] = n1 * e1[2] - n2 * e1[1];
    e2[1] = n2 * e1[0] - n0 * e1[2];
    e2[2] = n0 * e1[1] - n1 * e1[0];
}

// h' Ni g for two vectors of 6 and the symmetric Ni (packed upper, order 6): sum_a h_a (sum_b Ni_ab g_b), a and b ascending
__device__ inline double form_quad6(const double *h, const double *Ni, const double *g) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 6; a++) {
        double t = 0.0;
#pragma unroll
        for (int b = 0; b < 6; b++) t += Ni[a <= b ? tri_ix<6>(a, b) : tri_ix<6>(b, a)] * g[b];
        s += h[a] * t;
    }
    return s;
}

// (a, b >= a) of index e in an upper triangle of order n packed row by row
__device__ inline void form_untri(int n, int e, int &a, int &b) {
    a = 0;
    while (e >= n - a) { e -= n - a; ++a; }
    b = a + e;
}

// Form g: type ftype[g], members fbegin[g] .. fbegin[g + 1] of fpoint / fcols (3 columns per member, -1: fixed); fhost: the status
// bits the host found.  One wave per workgroup: the precondition of the LDS routines of wavealg.h.
// SERIAL (the hook of scripts/forms_bench.py): M is factorised by wave_solve_lds, where every lane repeats the whole serial solve, in
// the place of wave_chol_lds; everything else is the same.
// SURF (jaicov_surf_fit, include/jaicov_surfaces.h): the cylinder and the cone beside the four forms, and start [n][7], whose row g
// holds the start values of form g in the reported order and the engine's frame unless its first entry is NaN.  Without SURF none
// of that is compiled in and start is not read.
template <bool SERIAL, bool SURF>
__global__ __launch_bounds__(64) void form_fit_kernel(const double *__restrict__ Q, long ld, const double *__restrict__ vals,
                                                      const int32_t *__restrict__ ftype, const int32_t *__restrict__ fbegin,
                                                      const int32_t *__restrict__ fhost, const int32_t *__restrict__ fpoint,
                                                      const int32_t *__restrict__ fcols, const double *__restrict__ start, double sigma2,
                                                      int max_it, double tol, double *__restrict__ out, double *__restrict__ qpp,
                                                      double *__restrict__ mem_out, int32_t *__restrict__ status,
                                                      int32_t *__restrict__ mem_status) {
    __shared__ double U[FORM_TRI], Z[FORM_TRI];
    __shared__ double X[3][FORM_R], Vv[3][FORM_R], Bt[3][FORM_R], Bl[3][FORM_R], At[7][FORM_R], Sc[FORM_R], Sv[FORM_R], Lm[FORM_R];
    __shared__ double Nl[28], Jm[7][6];
    __shared__ int col[3][FORM_R];
    const int g = blockIdx.x, lane = threadIdx.x;
    const int type = wave_uniform(ftype[g]);
    const int m0 = wave_uniform(fbegin[g]), k = wave_uniform(fbegin[g + 1]) - m0;
    int st = wave_uniform(fhost[g]);
    const bool cyl = SURF && type == JAICOV_SURF_CYLINDER, cone = SURF && type == JAICOV_SURF_CONE, surf = cyl || cone;
    const int c = surf ? 1 : type >= JAICOV_FORM_LINE ? 2 : 1;
    const int u = cyl ? 5 : cone ? 6 : type == JAICOV_FORM_PLANE ? 3 : type == JAICOV_FORM_CIRCLE ? 6 : 4;
    const int npar = surf ? 7 : type == JAICOV_FORM_LINE ? 6 : type == JAICOV_FORM_CIRCLE ? 7 : 4;
    const int least = surf ? u : type == JAICOV_FORM_PLANE ? 3 : type == JAICOV_FORM_SPHERE ? 4 : type == JAICOV_FORM_LINE ? 2 : 3;
    const int m = c * k;
    int iters = 0;
    auto ix = [m](int i, int j) { return tri_ix_n(m, i, j); };
    // the form has failed, taken by the whole wave: NaN in its figures and in its members', the steps begun excepted
    auto fail = [&](int bit) {
        if (lane < JAICOV_FORM_COLUMNS) out[(size_t)JAICOV_FORM_COLUMNS * g + lane] = lane == 19 ? (double)iters : NAN;
        if (lane < JAICOV_FORM_QPP_COLUMNS) qpp[(size_t)JAICOV_FORM_QPP_COLUMNS * g + lane] = NAN;
        for (int t = lane; t < JAICOV_FORM_MEMBER_COLUMNS * k; t += 64) mem_out[(size_t)JAICOV_FORM_MEMBER_COLUMNS * m0 + t] = NAN;
        for (int t = lane; t < k; t += 64) mem_status[m0 + t] = 0;
        if (lane == 0) status[g] = st | bit;
    };
    if (k < least) { fail(JAICOV_FORM_TOO_SMALL); return; }
    if (m > FORM_R) { fail(JAICOV_FORM_TOO_LARGE); return; }

    // ---- the members, their centroid in member order, the centred coordinates
    if (lane < k) {
        const int p = fpoint[m0 + lane];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            col[a][lane] = fcols[3 * (size_t)(m0 + lane) + a];
            X[a][lane] = vals[3 * (size_t)p + a];
            Vv[a][lane] = 0.0;
        }
    }
    __syncthreads();
    double G[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < k; i++) { G[0] += X[0][i]; G[1] += X[1][i]; G[2] += X[2][i]; }
    G[0] = G[0] / (double)k; G[1] = G[1] / (double)k; G[2] = G[2] / (double)k;
    __syncthreads();
    if (lane < k) { X[0][lane] = X[0][lane] - G[0]; X[1][lane] = X[1][lane] - G[1]; X[2][lane] = X[2][lane] - G[2]; }
    __syncthreads();
    double ext = 0.0, fin = 0.0, S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < k; i++) {
        const double x = X[0][i], y = X[1][i], z = X[2][i];
        ext = fmax(ext, sqrt(x * x + y * y + z * z));
        fin += ((x + y) + z) * 0.0;
        S[0] += x * x; S[1] += x * y; S[2] += x * z; S[3] += y * y; S[4] += y * z; S[5] += z * z;
    }
    if (wave_uniform(!(fin == 0.0))) { fail(JAICOV_FORM_NOT_FINITE); return; }

    // ---- start values
    double n[3] = {0.0, 0.0, 0.0}, pc[3] = {0.0, 0.0, 0.0}, pr = 0.0;       // n or t | c or x0 | r or d_c
    double e1[3] = {0.0, 0.0, 0.0}, e2[3] = {0.0, 0.0, 0.0};
    bool given = false;
    if (SURF) {
        // a start row (the caller's, or the search's for a cylinder or a cone) is brought into working form
        double sv[JAICOV_FORM_MAX_PARAMS];
#pragma unroll
        for (int a = 0; a < JAICOV_FORM_MAX_PARAMS; a++) sv[a] = start[(size_t)JAICOV_FORM_MAX_PARAMS * g + a];
        given = wave_uniform(sv[0] == sv[0]);
        if (!given && surf) { fail(JAICOV_FORM_DEGENERATE); return; }          // the search was left without a candidate
        if (given) {
            bool bad = false;
            if (type == JAICOV_FORM_PLANE) {
                n[0] = sv[0]; n[1] = sv[1]; n[2] = sv[2]; pr = sv[3];
            } else {
                pc[0] = sv[0] - G[0]; pc[1] = sv[1] - G[1]; pc[2] = sv[2] - G[2];
                if (type == JAICOV_FORM_SPHERE) pr = sv[3];
                else { n[0] = sv[3]; n[1] = sv[4]; n[2] = sv[5]; }
                if (type == JAICOV_FORM_CIRCLE || surf) pr = sv[6];
            }
            if (type != JAICOV_FORM_SPHERE) {
                const double l = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
                bad = !(l > 0.0);
                n[0] = n[0] / l; n[1] = n[1] / l; n[2] = n[2] / l;
            }
            if (type == JAICOV_FORM_PLANE) pr = pr - ((n[0] * G[0] + n[1] * G[1]) + n[2] * G[2]);
            if (type == JAICOV_FORM_LINE || cyl) {
                const double s = (n[0] * pc[0] + n[1] * pc[1]) + n[2] * pc[2];
                pc[0] = pc[0] - s * n[0]; pc[1] = pc[1] - s * n[1]; pc[2] = pc[2] - s * n[2];
            }
            if (type == JAICOV_FORM_SPHERE || type == JAICOV_FORM_CIRCLE || cyl) bad = bad || !(pr > 0.0);
            if (cone) bad = bad || !(pr > 0.0 && pr < M_PI);
            if (wave_uniform(bad)) { fail(JAICOV_FORM_DEGENERATE); return; }
        }
    }
    if (!given) {
        double lam[3], E[9];
        wave_eigen3<FORM_SWEEPS>(S, lam, E);
        if (type == JAICOV_FORM_PLANE || type == JAICOV_FORM_CIRCLE) {
            if (wave_uniform(lam[1] <= 1e-12 * lam[0])) { fail(JAICOV_FORM_DEGENERATE); return; }
            n[0] = E[6]; n[1] = E[7]; n[2] = E[8];
        } else if (type == JAICOV_FORM_LINE) {
            if (wave_uniform(!(lam[0] > 0.0))) { fail(JAICOV_FORM_DEGENERATE); return; }
            n[0] = E[0]; n[1] = E[1]; n[2] = E[2];
        }
    }
    if (!given && (type == JAICOV_FORM_SPHERE || type == JAICOV_FORM_CIRCLE)) {
        // |q|^2 - 2 c.q + t = 0 in (c, t): rows [-2 q, 1], right-hand side -|q|^2; the circle has q = (e1.x, e2.x, 0) and N_22 = 1
        const bool circle = type == JAICOV_FORM_CIRCLE;
        if (circle) form_basis(n[0], n[1], n[2], e1, e2);
        double Nn[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, bn[4] = {0.0, 0.0, 0.0, 0.0}, th[4];
        for (int i = 0; i < k; i++) {
            const double x = X[0][i], y = X[1][i], z = X[2][i];
            const double q0 = circle ? (e1[0] * x + e1[1] * y) + e1[2] * z : x;
            const double q1 = circle ? (e2[0] * x + e2[1] * y) + e2[2] * z : y;
            const double q2 = circle ? 0.0 : z;
            const double a0 = -2.0 * q0, a1 = -2.0 * q1, a2 = -2.0 * q2, b = -((q0 * q0 + q1 * q1) + q2 * q2);
            Nn[0] += a0 * a0; Nn[1] += a0 * a1; Nn[2] += a0 * a2; Nn[3] += a0;
            Nn[4] += a1 * a1; Nn[5] += a1 * a2; Nn[6] += a1;
            Nn[7] += a2 * a2; Nn[8] += a2;
            Nn[9] += 1.0;
            bn[0] += a0 * b; bn[1] += a1 * b; bn[2] += a2 * b; bn[3] += b;
        }
        if (circle) Nn[7] = 1.0;
        const WaveStatus ws = wave_solve<4>(Nn, bn, th, nullptr);
        if (wave_uniform(ws != WAVE_OK)) { fail(ws == WAVE_NOT_FINITE ? JAICOV_FORM_NOT_FINITE : JAICOV_FORM_DEGENERATE); return; }
        const double r2 = ((th[0] * th[0] + th[1] * th[1]) + th[2] * th[2]) - th[3];
        if (wave_uniform(!(r2 > 0.0))) { fail(JAICOV_FORM_DEGENERATE); return; }
        pr = sqrt(r2);
        if (circle) {
#pragma unroll
            for (int a = 0; a < 3; a++) pc[a] = th[0] * e1[a] + th[1] * e2[a];
        } else {
            pc[0] = th[0]; pc[1] = th[1]; pc[2] = th[2];
        }
    }

    // ---- the steps
    const int mi = c == 2 ? lane >> 1 : lane;            // the member of row `lane`
    const int cq = c == 2 ? (lane & 1) : 0;              // and which of its conditions
    if (tol == 0.0) tol = 1e-12;
    double Qn[21], x0l[3] = {0.0, 0.0, 0.0};
    double omega = 0.0, lam_r = 0.0, srow = 0.0;
    bool conv = false;
    for (;;) {
        ++iters;
        if (type != JAICOV_FORM_SPHERE) form_basis(n[0], n[1], n[2], e1, e2);
        x0l[0] = pc[0]; x0l[1] = pc[1]; x0l[2] = pc[2];
        double Br[3] = {0.0, 0.0, 0.0}, Ar[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w = 0.0;
        double ca = 0.0, sa = 0.0;                           // of the cone's alpha, held in pr
        if (cone) { ca = cos(pr); sa = sin(pr); }
        if (lane < m) {
            const double v0 = Vv[0][mi], v1 = Vv[1][mi], v2 = Vv[2][mi];
            const double xh0 = X[0][mi] + v0, xh1 = X[1][mi] + v1, xh2 = X[2][mi] + v2;
            const double d0 = xh0 - pc[0], d1 = xh1 - pc[1], d2 = xh2 - pc[2];
            double f = 0.0;
            if (type == JAICOV_FORM_PLANE) {
                Br[0] = n[0]; Br[1] = n[1]; Br[2] = n[2];
                Ar[0] = (e1[0] * xh0 + e1[1] * xh1) + e1[2] * xh2;
                Ar[1] = (e2[0] * xh0 + e2[1] * xh1) + e2[2] * xh2;
                Ar[2] = -1.0;
                f = ((n[0] * xh0 + n[1] * xh1) + n[2] * xh2) - pr;
            } else if (type == JAICOV_FORM_SPHERE) {
                const double rho = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
                Br[0] = d0 / rho; Br[1] = d1 / rho; Br[2] = d2 / rho;
                Ar[0] = -Br[0]; Ar[1] = -Br[1]; Ar[2] = -Br[2]; Ar[3] = -1.0;
                f = rho - pr;
            } else if (type == JAICOV_FORM_LINE) {
                const double s = (n[0] * d0 + n[1] * d1) + n[2] * d2;
                if (cq == 0) {
                    Br[0] = e1[0]; Br[1] = e1[1]; Br[2] = e1[2];
                    Ar[0] = -1.0; Ar[2] = -s;
                } else {
                    Br[0] = e2[0]; Br[1] = e2[1]; Br[2] = e2[2];
                    Ar[1] = -1.0; Ar[3] = -s;
                }
                f = (Br[0] * d0 + Br[1] * d1) + Br[2] * d2;
            } else if (surf) {
                const double s = (n[0] * d0 + n[1] * d1) + n[2] * d2;
                const double p0 = d0 - s * n[0], p1 = d1 - s * n[1], p2 = d2 - s * n[2];
                const double rho = sqrt((p0 * p0 + p1 * p1) + p2 * p2);
                const double g0 = p0 / rho, g1 = p1 / rho, g2 = p2 / rho;
                const double ge1 = (g0 * e1[0] + g1 * e1[1]) + g2 * e1[2], ge2 = (g0 * e2[0] + g1 * e2[1]) + g2 * e2[2];
                if (cyl) {
                    Br[0] = g0; Br[1] = g1; Br[2] = g2;
                    Ar[0] = -ge1; Ar[1] = -ge2; Ar[2] = -(s * ge1); Ar[3] = -(s * ge2); Ar[4] = -1.0;
                    f = rho - pr;
                } else {
                    const double q = s * ca + rho * sa;
                    Br[0] = g0 * ca - n[0] * sa; Br[1] = g1 * ca - n[1] * sa; Br[2] = g2 * ca - n[2] * sa;
                    Ar[0] = -Br[0]; Ar[1] = -Br[1]; Ar[2] = -Br[2]; Ar[3] = -(q * ge1); Ar[4] = -(q * ge2); Ar[5] = -q;
                    f = rho * ca - s * sa;
                }
            } else {
                if (cq == 0) {
                    Br[0] = n[0]; Br[1] = n[1]; Br[2] = n[2];
                    Ar[0] = -n[0]; Ar[1] = -n[1]; Ar[2] = -n[2];
                    Ar[3] = (e1[0] * d0 + e1[1] * d1) + e1[2] * d2;
                    Ar[4] = (e2[0] * d0 + e2[1] * d1) + e2[2] * d2;
                    f = (n[0] * d0 + n[1] * d1) + n[2] * d2;
                } else {
                    const double rho = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
                    Br[0] = d0 / rho; Br[1] = d1 / rho; Br[2] = d2 / rho;
                    Ar[0] = -Br[0]; Ar[1] = -Br[1]; Ar[2] = -Br[2]; Ar[5] = -1.0;
                    f = rho - pr;
                }
            }
            w = f - ((Br[0] * v0 + Br[1] * v1) + Br[2] * v2);
            Bt[0][lane] = Br[0]; Bt[1][lane] = Br[1]; Bt[2][lane] = Br[2];
        }
        __syncthreads();
        // M = B Q_ll B': the lane takes the member pair (i, i + lane)
        for (int i = 0; i < k; i++) {
            const int j = i + lane;
            if (j < k) {
                double q[3][3];
#pragma unroll
                for (int a = 0; a < 3; a++)
#pragma unroll
                    for (int b = 0; b < 3; b++) q[a][b] = q_at(Q, ld, col[a][i], col[b][j]);
                for (int qa = 0; qa < c; qa++)
                    for (int qb = 0; qb < c; qb++) {
                        const int r = c * i + qa, s = c * j + qb;
                        if (s < r) continue;
                        const double b0 = Bt[0][s], b1 = Bt[1][s], b2 = Bt[2][s];
                        const double t0 = (q[0][0] * b0 + q[0][1] * b1) + q[0][2] * b2;
                        const double t1 = (q[1][0] * b0 + q[1][1] * b1) + q[1][2] * b2;
                        const double t2 = (q[2][0] * b0 + q[2][1] * b1) + q[2][2] * b2;
                        U[ix(r, s)] = (Bt[0][r] * t0 + Bt[1][r] * t1) + Bt[2][r] * t2;
                    }
            }
        }
        __syncthreads();
        // NaN in z unless every value is finite
        double z = w * 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) z += Ar[a] * 0.0;
        wave_equilibrate_lds(m, U, Sc, Sv, z, lane);
        if (wave_uniform(__any(!(z == 0.0)) != 0)) { fail(JAICOV_FORM_NOT_FINITE); return; }
        if (SERIAL) {
            if (lane < m) { Bl[0][lane] = 0.0; Bl[1][lane] = 0.0; }
            __syncthreads();
            if (wave_solve_lds(m, U, Bl[0], Bl[1]) != WAVE_OK) { fail(JAICOV_FORM_SINGULAR); return; }
            __syncthreads();
        } else if (wave_chol_lds(m, U, lane) != WAVE_OK) {
            fail(JAICOV_FORM_SINGULAR);
            return;
        }
        // At = U^-T (S A), wt = U^-T (S w)
        srow = lane < m ? Sc[lane] * Sv[lane] : 0.0;
        double zz[7];
#pragma unroll
        for (int a = 0; a < 6; a++) zz[a] = srow * Ar[a];
        zz[6] = srow * w;
        wave_forward_lds<7>(m, U, zz, lane);
        if (lane < m) {
#pragma unroll
            for (int a = 0; a < 7; a++) At[a][lane] = zz[a];
        }
        __syncthreads();
        // N = At' At (21 entries) and g = At' wt (6): lane e forms entry e over the rows ascending
        if (lane < 27) {
            int a, b;
            if (lane < 21) form_untri(6, lane, a, b);
            else { a = lane - 21; b = 6; }
            double s = 0.0;
            for (int r = 0; r < m; r++) s += At[a][r] * At[b][r];
            if (lane < 21 && a == b && a >= u) s = 1.0;
            Nl[lane] = s;
        }
        __syncthreads();
        double Un[21], gn[6], dx[6];
#pragma unroll
        for (int e = 0; e < 21; e++) Un[e] = Nl[e];
#pragma unroll
        for (int a = 0; a < 6; a++) gn[a] = Nl[21 + a];
        const WaveStatus ws = wave_solve<6>(Un, gn, dx, Qn);
        if (wave_uniform(ws != WAVE_OK)) { fail(ws == WAVE_NOT_FINITE ? JAICOV_FORM_NOT_FINITE : JAICOV_FORM_SINGULAR); return; }
#pragma unroll
        for (int a = 0; a < 6; a++) dx[a] = -dx[a];
        double y = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) y += zz[a] * dx[a];
        y = lane < m ? y + zz[6] : 0.0;
        if (lane < m) Lm[lane] = y;
        __syncthreads();
        omega = 0.0;
        for (int r = 0; r < m; r++) omega += Lm[r] * Lm[r];
        __syncthreads();
        wave_backward_lds(m, U, y, lane);
        lam_r = -(srow * y);
        if (lane < m) Lm[lane] = lam_r;
        __syncthreads();
        if (lane < k) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                double s = 0.0;
                for (int qa = 0; qa < c; qa++) s += Bt[a][c * lane + qa] * Lm[c * lane + qa];
                Bl[a][lane] = s;
            }
        }
        __syncthreads();
        // v = Q_ll B' lambda: the lane takes member `lane` and reads its block row
        if (lane < k) {
            double v0 = 0.0, v1 = 0.0, v2 = 0.0;
            const int ca = col[0][lane], cb = col[1][lane], cc = col[2][lane];
            for (int j = 0; j < k; j++) {
                const int j0 = col[0][j], j1 = col[1][j], j2 = col[2][j];
                const double b0 = Bl[0][j], b1 = Bl[1][j], b2 = Bl[2][j];
                v0 += (q_at(Q, ld, ca, j0) * b0 + q_at(Q, ld, ca, j1) * b1) + q_at(Q, ld, ca, j2) * b2;
                v1 += (q_at(Q, ld, cb, j0) * b0 + q_at(Q, ld, cb, j1) * b1) + q_at(Q, ld, cb, j2) * b2;
                v2 += (q_at(Q, ld, cc, j0) * b0 + q_at(Q, ld, cc, j1) * b1) + q_at(Q, ld, cc, j2) * b2;
            }
            Vv[0][lane] = v0; Vv[1][lane] = v1; Vv[2][lane] = v2;
        }
        __syncthreads();
        // the parameters take Delta
        double big;
        if (type == JAICOV_FORM_PLANE) {
#pragma unroll
            for (int a = 0; a < 3; a++) n[a] = (n[a] + dx[0] * e1[a]) + dx[1] * e2[a];
            pr = pr + dx[2];
            big = fmax(fmax(fabs(dx[0]), fabs(dx[1])), fabs(dx[2]) / ext);
        } else if (type == JAICOV_FORM_SPHERE) {
            pc[0] = pc[0] + dx[0]; pc[1] = pc[1] + dx[1]; pc[2] = pc[2] + dx[2];
            pr = pr + dx[3];
            big = fmax(fmax(fabs(dx[0]), fabs(dx[1])), fmax(fabs(dx[2]), fabs(dx[3]))) / ext;
        } else if (type == JAICOV_FORM_LINE) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                pc[a] = (pc[a] + dx[0] * e1[a]) + dx[1] * e2[a];
                n[a] = (n[a] + dx[2] * e1[a]) + dx[3] * e2[a];
            }
            big = fmax(fmax(fabs(dx[0]) / ext, fabs(dx[1]) / ext), fmax(fabs(dx[2]), fabs(dx[3])));
        } else if (cyl) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                pc[a] = (pc[a] + dx[0] * e1[a]) + dx[1] * e2[a];
                n[a] = (n[a] + dx[2] * e1[a]) + dx[3] * e2[a];
            }
            pr = pr + dx[4];
            big = fmax(fmax(fmax(fabs(dx[0]), fabs(dx[1])), fabs(dx[4])) / ext, fmax(fabs(dx[2]), fabs(dx[3])));
        } else if (cone) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                pc[a] = pc[a] + dx[a];
                n[a] = (n[a] + dx[3] * e1[a]) + dx[4] * e2[a];
            }
            pr = pr + dx[5];
            big = fmax(fmax(fmax(fabs(dx[0]), fabs(dx[1])), fabs(dx[2])) / ext, fmax(fmax(fabs(dx[3]), fabs(dx[4])), fabs(dx[5])));
        } else {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                pc[a] = pc[a] + dx[a];
                n[a] = (n[a] + dx[3] * e1[a]) + dx[4] * e2[a];
            }
            pr = pr + dx[5];
            big = fmax(fmax(fmax(fabs(dx[0]), fabs(dx[1])), fmax(fabs(dx[2]), fabs(dx[5]))) / ext, fmax(fabs(dx[3]), fabs(dx[4])));
        }
        if (type != JAICOV_FORM_SPHERE) {
            const double l = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            n[0] = n[0] / l; n[1] = n[1] / l; n[2] = n[2] / l;
        }
        if (type == JAICOV_FORM_LINE || cyl) {
            const double s = (n[0] * pc[0] + n[1] * pc[1]) + n[2] * pc[2];
            pc[0] = pc[0] - s * n[0]; pc[1] = pc[1] - s * n[1]; pc[2] = pc[2] - s * n[2];
        }
        const double chk = ((((big + omega) + pr) + ((n[0] + n[1]) + n[2])) + ((pc[0] + pc[1]) + pc[2])) * 0.0;
        if (wave_uniform(!(chk == 0.0))) { fail(JAICOV_FORM_NOT_FINITE); return; }
        if (surf && wave_uniform(cyl ? !(pr > 0.0) : !(pr > 0.0 && pr < M_PI))) { fail(JAICOV_FORM_DEGENERATE); return; }
        if (wave_uniform(big <= tol)) { conv = true; break; }
        if (iters >= max_it) break;
    }
    if (!conv) st |= JAICOV_FORM_NOT_CONVERGED;

    // ---- the sign rule, Q_pp = J N^-1 J' and the form's figures
    double sg = 1.0;
    if (cone && pr > 0.5 * M_PI) sg = -1.0;                  // the cone's t turns with alpha, not by its largest component
    if (type != JAICOV_FORM_SPHERE && !cone) {
        double bigc = n[0];
        if (fabs(n[1]) > fabs(bigc)) bigc = n[1];
        if (fabs(n[2]) > fabs(bigc)) bigc = n[2];
        if (bigc < 0.0) sg = -1.0;
    }
    if (lane < 42) Jm[lane / 6][lane % 6] = 0.0;
    __syncthreads();
    if (lane == 0) {
        if (type == JAICOV_FORM_PLANE) {
            for (int a = 0; a < 3; a++) { Jm[a][0] = sg * e1[a]; Jm[a][1] = sg * e2[a]; }
            Jm[3][0] = sg * ((e1[0] * G[0] + e1[1] * G[1]) + e1[2] * G[2]);
            Jm[3][1] = sg * ((e2[0] * G[0] + e2[1] * G[1]) + e2[2] * G[2]);
            Jm[3][2] = sg;
        } else if (type == JAICOV_FORM_SPHERE) {
            for (int a = 0; a < 4; a++) Jm[a][a] = 1.0;
        } else if (type == JAICOV_FORM_LINE || cyl) {
            const double s1 = (e1[0] * x0l[0] + e1[1] * x0l[1]) + e1[2] * x0l[2], s2 = (e2[0] * x0l[0] + e2[1] * x0l[1]) + e2[2] * x0l[2];
            for (int a = 0; a < 3; a++) {
                Jm[a][0] = e1[a]; Jm[a][1] = e2[a]; Jm[a][2] = -s1 * n[a]; Jm[a][3] = -s2 * n[a];
                Jm[3 + a][2] = sg * e1[a]; Jm[3 + a][3] = sg * e2[a];
            }
            if (cyl) Jm[6][4] = 1.0;
        } else {
            for (int a = 0; a < 3; a++) { Jm[a][a] = 1.0; Jm[3 + a][3] = sg * e1[a]; Jm[3 + a][4] = sg * e2[a]; }
            Jm[6][5] = cone ? sg : 1.0;
        }
    }
    __syncthreads();
    n[0] = sg * n[0]; n[1] = sg * n[1]; n[2] = sg * n[2];
    if (type == JAICOV_FORM_PLANE) pr = sg * pr;
    if (cone && sg < 0.0) pr = M_PI - pr;
    double *o = out + (size_t)JAICOV_FORM_COLUMNS * g;
    if (lane < JAICOV_FORM_QPP_COLUMNS) {
        int i, j;
        form_untri(JAICOV_FORM_MAX_PARAMS, lane, i, j);
        double val = 0.0;
        if (j < npar) {
            double hi[6], hj[6];
#pragma unroll
            for (int a = 0; a < 6; a++) { hi[a] = Jm[i][a]; hj[a] = Jm[j][a]; }
            val = form_quad6(hi, Qn, hj);
        }
        qpp[(size_t)JAICOV_FORM_QPP_COLUMNS * g + lane] = val;
        if (i == j) o[7 + i] = i < npar ? sqrt(sigma2 * fmax(val, 0.0)) : NAN;
    }
    // the distances of the uncorrected members
    double dist = 0.0;
    if (lane < k) {
        const double x = X[0][lane], y = X[1][lane], zc = X[2][lane];
        if (type == JAICOV_FORM_PLANE) {
            dist = ((n[0] * x + n[1] * y) + n[2] * zc) - pr;
        } else {
            const double d0 = x - pc[0], d1 = y - pc[1], d2 = zc - pc[2];
            if (type == JAICOV_FORM_SPHERE) {
                dist = sqrt((d0 * d0 + d1 * d1) + d2 * d2) - pr;
            } else {
                const double s = (n[0] * d0 + n[1] * d1) + n[2] * d2;
                const double p0 = d0 - s * n[0], p1 = d1 - s * n[1], p2 = d2 - s * n[2];
                const double perp = sqrt((p0 * p0 + p1 * p1) + p2 * p2);
                if (cyl) dist = perp - pr;
                else if (cone) dist = perp * cos(pr) - s * sin(pr);
                else dist = type == JAICOV_FORM_LINE ? perp : sqrt(s * s + (perp - pr) * (perp - pr));
            }
        }
        Bl[0][lane] = dist;
    }
    __syncthreads();
    const int fdof = m - u;
    if (lane == 0) {
        double dmax = 0.0, d2 = 0.0;
        for (int i = 0; i < k; i++) { dmax = fmax(dmax, fabs(Bl[0][i])); d2 += Bl[0][i] * Bl[0][i]; }
        for (int a = 0; a < 7; a++) o[a] = NAN;
        if (type == JAICOV_FORM_PLANE) {
            o[0] = n[0]; o[1] = n[1]; o[2] = n[2];
            o[3] = pr + ((n[0] * G[0] + n[1] * G[1]) + n[2] * G[2]);
        } else {
            o[0] = pc[0] + G[0]; o[1] = pc[1] + G[1]; o[2] = pc[2] + G[2];
            if (type == JAICOV_FORM_SPHERE) {
                o[3] = pr;
            } else {
                o[3] = n[0]; o[4] = n[1]; o[5] = n[2];
                if (type == JAICOV_FORM_CIRCLE || surf) o[6] = pr;
            }
        }
        o[14] = omega;
        o[15] = (double)fdof;
        o[16] = fdof > 0 ? omega / ((double)fdof * sigma2) : NAN;
        o[17] = dmax;
        o[18] = sqrt(d2 / (double)k);
        o[19] = (double)iters;
        status[g] = st;
    }

    // ---- the members: Q_kk,ii from Z = U^-1, the last At and N^-1
    wave_trinv_lds(m, U, Z, lane);
    double dd = 0.0, xc = 0.0, h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int partner = c == 2 ? (lane ^ 1) : lane, hi_row = lane | (c - 1);
    for (int kk = 0; kk < m; kk++) {
        if (lane < m && kk >= lane) {
            const double zr = Z[ix(lane, kk)];
            dd += zr * zr;
#pragma unroll
            for (int a = 0; a < 6; a++) h[a] += zr * At[a][kk];
            if (c == 2 && kk >= hi_row) xc += zr * Z[ix(partner, kk)];
        }
    }
    const double mrr = (srow * srow) * dd;
    const double qrr = (srow * srow) * (dd - form_quad6(h, Qn, h));
    double hp[6];
#pragma unroll
    for (int a = 0; a < 6; a++) hp[a] = __shfl_xor(h[a], 1);
    const double sp = __shfl_xor(srow, 1);
    const double q12 = (srow * sp) * (xc - form_quad6(h, Qn, hp));
    const double q22 = __shfl_xor(qrr, 1), m22 = __shfl_xor(mrr, 1), l2 = __shfl_xor(lam_r, 1);
    double nab0 = NAN, nab1 = NAN, Ti = NAN;
    bool ok = fdof > 0;
    if (c == 1) {
        ok = ok && qrr > 1e-12 * mrr;
        if (ok) {
            const double a = lam_r / qrr;
            nab0 = -a;
            Ti = (lam_r * a) / sigma2;
        }
    } else {
        ok = ok && qrr > 1e-12 * mrr;
        const double p2 = ok ? q22 - q12 * q12 / qrr : -1.0;
        ok = ok && p2 > 1e-12 * m22;
        if (ok) {
            const double b = (l2 - q12 * lam_r / qrr) / p2;
            const double a = (lam_r - q12 * b) / qrr;
            nab0 = -a; nab1 = -b;
            Ti = (lam_r * a + l2 * b) / (2.0 * sigma2);
        }
    }
    if (type != JAICOV_FORM_SPHERE && !cyl) nab0 = sg * nab0;
    if (lane < m && cq == 0) {
        double *mo = mem_out + (size_t)JAICOV_FORM_MEMBER_COLUMNS * (m0 + mi);
        mo[0] = Vv[0][mi]; mo[1] = Vv[1][mi]; mo[2] = Vv[2][mi];
        mo[3] = Bl[0][mi];
        mo[4] = nab0; mo[5] = nab1; mo[6] = Ti;
        mem_status[m0 + mi] = ok ? 0 : JAICOV_FORM_MEMBER_UNTESTED;
    }
}

}  // namespace jaicov

using namespace jaicov;

// the three entries to the fit: jaicov_form_fit, its serial variant for the benchmark, and jaicov_surf_fit with `start` (may be NULL)
enum FormEntry { FORM_ENTRY_FIT, FORM_ENTRY_SERIAL, FORM_ENTRY_SURF };

static int form_run(jaicov_engine *e, FormEntry entry, double sigma2, int32_t n_forms, const int32_t *form_type, const int32_t *form_begin,
                    const int32_t *form_point, const double *start, int32_t max_iterations, double tol, double *out, double *qpp,
                    double *member_out, int32_t *status, int32_t *member_status, float *ms_out) {
    const bool surf = entry == FORM_ENTRY_SURF;
    const int last_type = surf ? JAICOV_SURF_CONE : JAICOV_FORM_CIRCLE;
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    TRY(q_guard(v, "forms on a sharded engine"));
    if (!form_type || !form_begin || !out || !status || n_forms < 0) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "forms: NULL argument or a negative count");
    for (int g = 0; g < n_forms; g++)
        if (form_type[g] < JAICOV_FORM_PLANE || form_type[g] > last_type) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "forms: unknown form type");
    if (!ranges_ok(n_forms, form_begin)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "forms: form_begin must ascend from 0");
    const int n = n_forms, M = form_begin[n_forms];
    if (M > 0 && !form_point) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "forms: NULL form_point");
    for (int i = 0; i < M; i++)
        if (form_point[i] < 0 || form_point[i] >= v.n_points) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "forms: point index out of range");
    std::vector<int32_t> sorted;
    for (int g = 0; g < n; g++) {
        sorted.assign(form_point + form_begin[g], form_point + form_begin[g + 1]);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "forms: a form names the same point twice");
    }
    if (!(sigma2 > 0.0)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "forms: sigma2 must be positive");
    if (!(tol >= 0.0)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "forms: tol must not be negative");
    if (max_iterations < 1) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "forms: max_iterations must be at least 1");
    // the start rows as the kernels read them: NaN in front where the form finds its own; does any cylinder or cone have to search?
    static const int reported[] = {4, 4, 6, 7, 7, 7};
    std::vector<double> rows;
    bool search = false;
    if (surf) {
        rows.assign((size_t)JAICOV_FORM_MAX_PARAMS * std::max(n, 1), NAN);
        for (int g = 0; g < n; g++) {
            const double *row = start ? start + (size_t)JAICOV_FORM_MAX_PARAMS * g : nullptr;
            if (!row || std::isnan(row[0])) {
                search = search || form_type[g] >= JAICOV_SURF_CYLINDER;
                continue;
            }
            for (int a = 0; a < reported[form_type[g]]; a++) {
                if (!std::isfinite(row[a])) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "surfaces: a start row holds a non-finite value behind its first entry");
                rows[(size_t)JAICOV_FORM_MAX_PARAMS * g + a] = row[a];
            }
        }
    }
    // type [n] | begin [n + 1] | status bits of the host [n] | point [M] | columns [3 M]
    const size_t Mx = (size_t)std::max(M, 1), o_begin = (size_t)n, o_host = o_begin + n + 1, o_point = o_host + n, o_cols = o_point + Mx,
                 n_tab = o_cols + 3 * Mx;
    std::vector<int32_t> tab(n_tab, 0);
    for (int g = 0; g < n; g++) {
        tab[g] = form_type[g];
        tab[o_begin + g] = form_begin[g];
        for (int i = form_begin[g]; i < form_begin[g + 1]; i++) {
            tab[o_point + i] = form_point[i];
            for (int a = 0; a < 3; a++) {
                int c;
                TRY(q_column(v, 3 * (size_t)form_point[i] + a, "forms: a member's columns are not in the reduced cofactor matrix", &c));
                if (c < 0) tab[o_host + g] |= JAICOV_FORM_PARTIAL;
                tab[o_cols + 3 * (size_t)i + a] = c;
            }
        }
    }
    tab[o_begin + n] = M;
    if (ms_out) *ms_out = 0.f;
    if (n == 0) return JAICOV_OK;
    HIPE(*v.err, hipSetDevice(v.device));
    FormState *st = q_state(v.slot->form);
    HIPE(*v.err, st->tab.reserve(n_tab + n + Mx));
    HIPE(*v.err, st->out.reserve((size_t)(JAICOV_FORM_COLUMNS + JAICOV_FORM_QPP_COLUMNS + JAICOV_FORM_MAX_PARAMS) * n + JAICOV_FORM_MEMBER_COLUMNS * Mx));
    int32_t *d_tab = st->tab.get(), *d_status = d_tab + n_tab, *d_mstatus = d_status + n;
    double *d_out = st->out.get(), *d_qpp = d_out + (size_t)JAICOV_FORM_COLUMNS * n, *d_mem = d_qpp + (size_t)JAICOV_FORM_QPP_COLUMNS * n,
           *d_start = d_mem + JAICOV_FORM_MEMBER_COLUMNS * Mx;
    QTimer<2> timer(v.stream);
    HIPE(*v.err, timer.arm(ms_out != nullptr));
    HIPE(*v.err, hipMemcpyAsync(d_tab, tab.data(), n_tab * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    if (surf) HIPE(*v.err, hipMemcpyAsync(d_start, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, v.stream));
    HIPE(*v.err, timer.mark(0));
    if (surf) {
        if (search) hipLaunchKernelGGL(surf_start_kernel, dim3(n), dim3(64), 0, v.stream, v.d_vals, d_tab, d_tab + o_begin, d_tab + o_point, d_start);
        hipLaunchKernelGGL((form_fit_kernel<false, true>), dim3(n), dim3(64), 0, v.stream, v.Q, v.ld, v.d_vals, d_tab, d_tab + o_begin, d_tab + o_host,
                           d_tab + o_point, d_tab + o_cols, d_start, sigma2, max_iterations, tol, d_out, d_qpp, d_mem, d_status, d_mstatus);
    } else if (entry == FORM_ENTRY_SERIAL)
        hipLaunchKernelGGL((form_fit_kernel<true, false>), dim3(n), dim3(64), 0, v.stream, v.Q, v.ld, v.d_vals, d_tab, d_tab + o_begin, d_tab + o_host,
                           d_tab + o_point, d_tab + o_cols, (const double *)nullptr, sigma2, max_iterations, tol, d_out, d_qpp, d_mem, d_status, d_mstatus);
    else
        hipLaunchKernelGGL((form_fit_kernel<false, false>), dim3(n), dim3(64), 0, v.stream, v.Q, v.ld, v.d_vals, d_tab, d_tab + o_begin, d_tab + o_host,
                           d_tab + o_point, d_tab + o_cols, (const double *)nullptr, sigma2, max_iterations, tol, d_out, d_qpp, d_mem, d_status, d_mstatus);
    HIPE(*v.err, hipGetLastError());
    HIPE(*v.err, timer.mark(1));
    TRY(q_download(v, {{out, d_out, (size_t)JAICOV_FORM_COLUMNS * n * sizeof(double)},
                       {qpp, d_qpp, (size_t)JAICOV_FORM_QPP_COLUMNS * n * sizeof(double)},
                       {member_out, d_mem, (size_t)JAICOV_FORM_MEMBER_COLUMNS * M * sizeof(double)},
                       {status, d_status, (size_t)n * sizeof(int32_t)},
                       {member_status, d_mstatus, (size_t)M * sizeof(int32_t)}}));
    HIPE(*v.err, timer.read(ms_out));
    return JAICOV_OK;
}

extern "C" int jaicov_form_fit(jaicov_engine *e, double sigma2, int32_t n_forms, const int32_t *form_type, const int32_t *form_begin,
                               const int32_t *form_point, int32_t max_iterations, double tol, double *out, double *qpp, double *member_out,
                               int32_t *status, int32_t *member_status, float *ms_out) {
    return form_run(e, FORM_ENTRY_FIT, sigma2, n_forms, form_type, form_begin, form_point, nullptr, max_iterations, tol, out, qpp, member_out, status,
                    member_status, ms_out);
}

extern "C" int jaicov_surf_fit(jaicov_engine *e, double sigma2, int32_t n_forms, const int32_t *form_type, const int32_t *form_begin,
                               const int32_t *form_point, const double *start, int32_t max_iterations, double tol, double *out, double *qpp,
                               double *member_out, int32_t *status, int32_t *member_status, float *ms_out) {
    return form_run(e, FORM_ENTRY_SURF, sigma2, n_forms, form_type, form_begin, form_point, start, max_iterations, tol, out, qpp, member_out, status,
                    member_status, ms_out);
}

// The hook of scripts/forms_bench.py: the same call with M factorised by wave_solve_lds in the place of wave_chol_lds.
extern "C" int jaicov_debug_form_fit_serial(jaicov_engine *e, double sigma2, int32_t n_forms, const int32_t *form_type, const int32_t *form_begin,
                                            const int32_t *form_point, int32_t max_iterations, double tol, double *out, int32_t *status, float *ms_out) {
    return form_run(e, FORM_ENTRY_SERIAL, sigma2, n_forms, form_type, form_begin, form_point, nullptr, max_iterations, tol, out, nullptr, nullptr, status,
                    nullptr, ms_out);
}
