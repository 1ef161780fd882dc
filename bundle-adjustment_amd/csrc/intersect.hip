// intersect.hip -- spatial forward intersection of many object points in one launch (include/jaicov_intersect.h): start values of the
// object points from oriented images.  The call has no counterpart in the reference; its collinearity equations, derivatives and
// weights are those of derivation/PartialDerivativeFactory.java (PDF), its preconditioning that of NormalEquationSystem.java (NES).
//
// A prologue kernel writes one record per image (R, X0, x0, y0, c), so that the sines and cosines are taken once per image.  Then one
// wave (one workgroup of 64 lanes) works one point; the linear start, the Gauss-Newton loop, the evaluation pass and the rejection
// rounds all run inside it, with no host round trip.  As for the DLT (dlt.hip) the work per point is a chain of small
// dependent steps: latency bounds it, and many resident single-wave workgroups per SIMD hide that latency.
//   Sums.  Lane l takes rays l, l + 64, ... and keeps the partial sums of N (6), n (3) and Omega; the lanes are combined by an xor
//   butterfly, whose order is fixed and which leaves the same bits in every lane.  The 3 x 3 algebra that follows is therefore
//   wave-uniform: every lane computes it, no lane waits for another, and every branch on its outcome is taken by the whole wave.
//   Rays are staged ISECT_CHUNK at a time in LDS; a point with at most ISECT_CHUNK rays keeps them resident over all iterations and rounds.
//   The angle loop deals the pairs (i, j > i) of used rays to the lanes by j.
// Floating-point contraction is off in this file: every product and sum is rounded on its own, as tests/intersect_reference.py rounds it.
#include <hip/hip_runtime.h>

#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/jaicov_intersect.h"
#include "batchcall.h"
#include "intersect.h"
#include "wavealg.h"

#pragma clang fp contract(off)

namespace jaicov {
namespace {

// one set of status values in all the start-value kernels (wavealg.h)
static_assert(JAICOV_ISECT_OK == WAVE_OK && JAICOV_ISECT_SINGULAR == WAVE_SINGULAR && JAICOV_ISECT_NOT_FINITE == WAVE_NOT_FINITE,
              "wavealg.h returns the public status values");

enum { ISECT_START = 0, ISECT_STEP = 1, ISECT_EVAL = 2 };
constexpr int ISECT_NACC = 10;        // N00 N01 N02 N11 N12 N22, n0 n1 n2, Omega

__global__ void isect_image_kernel(int n_images, const double *__restrict__ io, const double *__restrict__ eo, IsectImage *__restrict__ rec) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_images) return;
    const double omega = eo[6L * i + 3], phi = eo[6L * i + 4], kappa = eo[6L * i + 5];
    const double co = cos(omega), so = sin(omega), cp = cos(phi), sp = sin(phi), ck = cos(kappa), sk = sin(kappa);
    IsectImage m;
    rotation_opk(so, co, sk, ck, sp, cp, m.r);
    for (int k = 0; k < 3; k++) m.X0[k] = eo[6L * i + k];
    m.x0 = io[3L * i]; m.y0 = io[3L * i + 1]; m.c = io[3L * i + 2];
    rec[i] = m;
}

// One ray's terms of the sums.  START: the two linear rows, unit weights.  STEP / EVAL: A'PA, A'Pw and q = w'Pw at the reduced point Xr.
__device__ inline void isect_ray(int mode, const IsectImage &im, double x, double y, double p11, double p12, double p22, const double *Xc,
                                 const double *Xr, double *t, double &q) {
    const double *r = im.r;
    const double T0 = im.X0[0] - Xc[0], T1 = im.X0[1] - Xc[1], T2 = im.X0[2] - Xc[2];
    const double c = im.c;
    if (mode == ISECT_START) {
        const double u = x - im.x0, v = y - im.y0;
        const double b00 = u * r[2] + c * r[0], b01 = u * r[5] + c * r[3], b02 = u * r[8] + c * r[6];
        const double b10 = v * r[2] + c * r[1], b11 = v * r[5] + c * r[4], b12 = v * r[8] + c * r[7];
        const double g0 = b00 * T0 + b01 * T1 + b02 * T2, g1 = b10 * T0 + b11 * T1 + b12 * T2;
        t[0] = b00 * b00 + b10 * b10; t[1] = b00 * b01 + b10 * b11; t[2] = b00 * b02 + b10 * b12;
        t[3] = b01 * b01 + b11 * b11; t[4] = b01 * b02 + b11 * b12; t[5] = b02 * b02 + b12 * b12;
        t[6] = b00 * g0 + b10 * g1; t[7] = b01 * g0 + b11 * g1; t[8] = b02 * g0 + b12 * g1;
        q = 0.0;
        return;
    }
    const double d0 = Xr[0] - T0, d1 = Xr[1] - T1, d2 = Xr[2] - T2;
    const double kx = r[0] * d0 + r[3] * d1 + r[6] * d2;                   // PDF:141-143
    const double ky = r[1] * d0 + r[4] * d1 + r[7] * d2;
    const double N = r[2] * d0 + r[5] * d1 + r[8] * d2;
    const double xs = -c * (kx / N), ys = -c * (ky / N);                  // PDF:145-149
    const double a00 = -(r[2] * xs + c * r[0]) / N, a01 = -(r[5] * xs + c * r[3]) / N, a02 = -(r[8] * xs + c * r[6]) / N;   // PDF:157-159
    const double a10 = -(r[2] * ys + c * r[1]) / N, a11 = -(r[5] * ys + c * r[4]) / N, a12 = -(r[8] * ys + c * r[7]) / N;   // PDF:175-177
    const double w0 = x - (im.x0 + xs), w1 = y - (im.y0 + ys);
    const double pa00 = p11 * a00 + p12 * a10, pa01 = p11 * a01 + p12 * a11, pa02 = p11 * a02 + p12 * a12;
    const double pa10 = p12 * a00 + p22 * a10, pa11 = p12 * a01 + p22 * a11, pa12 = p12 * a02 + p22 * a12;
    const double pw0 = p11 * w0 + p12 * w1, pw1 = p12 * w0 + p22 * w1;
    t[0] = a00 * pa00 + a10 * pa10; t[1] = a00 * pa01 + a10 * pa11; t[2] = a00 * pa02 + a10 * pa12;
    t[3] = a01 * pa01 + a11 * pa11; t[4] = a01 * pa02 + a11 * pa12; t[5] = a02 * pa02 + a12 * pa12;
    t[6] = a00 * pw0 + a10 * pw1; t[7] = a01 * pw0 + a11 * pw1; t[8] = a02 * pw0 + a12 * pw1;
    q = w0 * pw0 + w1 * pw1;
}

// N (packed upper: 00 01 02 11 12 22) x = n by Jacobi preconditioning (NES:82-91) and Cholesky; Q (may be NULL): the inverse of N.
__device__ int isect_solve3(const double *N, const double *n, double *x, double *Q) {
    const double EPS = ldexp(1.0, -53), SQRT_EPS = sqrt(EPS);
    for (int k = 0; k < 6; k++)
        if (!isfinite(N[k])) return JAICOV_ISECT_NOT_FINITE;
    for (int k = 0; k < 3; k++)
        if (!isfinite(n[k])) return JAICOV_ISECT_NOT_FINITE;
    const double V0 = N[0] > EPS ? 1.0 / sqrt(N[0]) : 1.0, V1 = N[3] > EPS ? 1.0 / sqrt(N[3]) : 1.0, V2 = N[5] > EPS ? 1.0 / sqrt(N[5]) : 1.0;
    const double M00 = N[0] * (V0 * V0), M01 = N[1] * (V0 * V1), M02 = N[2] * (V0 * V2);
    const double M11 = N[3] * (V1 * V1), M12 = N[4] * (V1 * V2), M22 = N[5] * (V2 * V2);
    if (!(M00 > SQRT_EPS)) return JAICOV_ISECT_SINGULAR;
    const double l00 = sqrt(M00), l10 = M01 / l00, l20 = M02 / l00;
    const double p1 = M11 - l10 * l10;
    if (!(p1 > SQRT_EPS)) return JAICOV_ISECT_SINGULAR;
    const double l11 = sqrt(p1), l21 = (M12 - l20 * l10) / l11;
    const double p2 = M22 - (l20 * l20 + l21 * l21);
    if (!(p2 > SQRT_EPS)) return JAICOV_ISECT_SINGULAR;
    const double l22 = sqrt(p2);
    if (x) {
        const double y0 = V0 * n[0] / l00, y1 = (V1 * n[1] - l10 * y0) / l11, y2 = (V2 * n[2] - l20 * y0 - l21 * y1) / l22;
        const double z2 = y2 / l22, z1 = (y1 - l21 * z2) / l11, z0 = (y0 - l10 * z1 - l20 * z2) / l00;
        x[0] = V0 * z0; x[1] = V1 * z1; x[2] = V2 * z2;
    }
    if (Q) {
        const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;             // inverse of L, then inv(M) = inv(L)' inv(L)
        const double i10 = -l10 * i00 * i11, i21 = -l21 * i11 * i22, i20 = -(l20 * i00 + l21 * i10) * i22;
        Q[0] = (i00 * i00 + i10 * i10 + i20 * i20) * (V0 * V0);
        Q[1] = (i10 * i11 + i20 * i21) * (V0 * V1);
        Q[2] = (i20 * i22) * (V0 * V2);
        Q[3] = (i11 * i11 + i21 * i21) * (V1 * V1);
        Q[4] = (i21 * i22) * (V1 * V2);
        Q[5] = (i22 * i22) * (V2 * V2);
    }
    return JAICOV_ISECT_OK;
}

__global__ __launch_bounds__(64) void isect_points_kernel(const int32_t *__restrict__ ray_begin, const int32_t *__restrict__ ray_image,
                                                          const double *__restrict__ xy, const double *__restrict__ var,
                                                          const IsectImage *__restrict__ images, double s0, int max_iter, double thr2,
                                                          int min_rays, double *__restrict__ out, int32_t *__restrict__ outcome,
                                                          uint8_t *used, double *__restrict__ ray_q) {
    __shared__ double sx[ISECT_CHUNK], sy[ISECT_CHUNK], sp11[ISECT_CHUNK], sp12[ISECT_CHUNK], sp22[ISECT_CHUNK];
    __shared__ double sd0[ISECT_CHUNK], sd1[ISECT_CHUNK], sd2[ISECT_CHUNK];
    __shared__ int simg[ISECT_CHUNK];
    __shared__ uint8_t sused[ISECT_CHUNK];
    const int p = blockIdx.x, lane = threadIdx.x;
    const long k0 = ray_begin[p];
    const int m = ray_begin[p + 1] - ray_begin[p];
    double *op = out + (long)JAICOV_ISECT_OUT_PER_POINT * p;
    int iters = 0;
    // this point has failed (Q3): wave_fail_item with the point's own arguments, for the four places that give up
    auto give_up = [&](int st) { wave_fail_item<2>(lane, op, JAICOV_ISECT_OUT_PER_POINT, outcome, p, st, iters, k0, m, used, ray_q); };
    if (m < 2) { give_up(JAICOV_ISECT_TOO_FEW_RAYS); return; }
    const bool resident = m <= ISECT_CHUNK;
    // rays c0 .. c0 + nc - 1 into LDS, with their weights (PDF:308-319)
    auto stage = [&](int c0, int nc) {
        __syncthreads();
        for (int t = lane; t < nc; t += 64) {
            const long k = k0 + c0 + t;
            simg[t] = ray_image[k];
            sx[t] = xy[2 * k]; sy[t] = xy[2 * k + 1];
            double p11 = 1.0, p12 = 0.0, p22 = 1.0;
            if (var) obs_weight(var[3 * k], var[3 * k + 1], var[3 * k + 2], s0, p11, p12, p22);
            sp11[t] = p11; sp12[t] = p12; sp22[t] = p22;
            sused[t] = used[k];
        }
        __syncthreads();
    };
    // one pass over the point's rays: the sums of the used rays, combined over the lanes; EVAL also writes q of every ray and finds
    // the used ray with the largest q (the lowest index among equal values)
    auto pass = [&](int mode, const double *Xc, const double *Xr, double *acc, double &qmax, int &qidx) {
        for (int a = 0; a < ISECT_NACC; a++) acc[a] = 0.0;
        qmax = -1.0; qidx = INT_MAX;
        for (int c0 = 0; c0 < m; c0 += ISECT_CHUNK) {
            const int nc = min(ISECT_CHUNK, m - c0);
            if (!resident) stage(c0, nc);
            for (int t = lane; t < nc; t += 64) {
                if (!sused[t] && !(mode == ISECT_EVAL && ray_q)) continue;
                double term[9], q;
                isect_ray(mode, images[simg[t]], sx[t], sy[t], sp11[t], sp12[t], sp22[t], Xc, Xr, term, q);
                if (mode == ISECT_EVAL && ray_q) ray_q[k0 + c0 + t] = q;
                if (!sused[t]) continue;
                for (int a = 0; a < 9; a++) acc[a] += term[a];
                acc[9] += q;
                if (q > qmax) { qmax = q; qidx = c0 + t; }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            for (int a = 0; a < ISECT_NACC; a++) acc[a] += __shfl_xor(acc[a], off);
            wave_argmax_combine(qmax, qidx, off);
        }
    };

    if (resident) stage(0, m);
    const double SQRT_EPS = sqrt(ldexp(1.0, -53));
    int nused = m, st = JAICOV_ISECT_OK;
    double Xc[3], Xr[3], Q[6], acc[ISECT_NACC], qmax;
    int qidx;
    // one loop over the passes of all rounds, so that the pass is compiled once: START -> STEP ... STEP -> EVAL (-> START of the next round)
    int mode = ISECT_START, it = 0;
    for (;;) {
        if (mode == ISECT_START) {                               // a round begins: Xc = projection centre of the first used ray
            __syncthreads();                                     // a withdrawal is visible to every lane
            int first = m - 1;                                   // in bounds whatever `used` holds; at least min_rays rays stay used
            for (int t = lane; t < m; t += 64)
                if (used[k0 + t]) { first = t; break; }
            for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off));
            const IsectImage &ic = images[ray_image[k0 + first]];
            for (int k = 0; k < 3; k++) { Xc[k] = ic.X0[k]; Xr[k] = 0.0; }
        }
        pass(mode, Xc, Xr, acc, qmax, qidx);
        if (mode != ISECT_EVAL) {
            double dx[3];
            int ss = isect_solve3(acc, acc + 6, dx, nullptr);
            if (ss == JAICOV_ISECT_OK && !(isfinite(dx[0]) && isfinite(dx[1]) && isfinite(dx[2]))) ss = JAICOV_ISECT_NOT_FINITE;
            if (ss != JAICOV_ISECT_OK) { if (mode == ISECT_STEP) iters++; give_up(ss); return; }
            for (int k = 0; k < 3; k++) Xr[k] += dx[k];          // START: Xr was 0
            if (mode == ISECT_START) { mode = ISECT_STEP; it = 0; st = JAICOV_ISECT_NOT_CONVERGED; continue; }
            iters++;
            const double step = fmax(fabs(dx[0]), fmax(fabs(dx[1]), fabs(dx[2])));
            const double size = fmax(fabs(Xr[0]), fmax(fabs(Xr[1]), fabs(Xr[2])));
            if (step <= SQRT_EPS * fmax(1.0, size)) { st = JAICOV_ISECT_OK; mode = ISECT_EVAL; }
            else if (++it >= max_iter) mode = ISECT_EVAL;
            continue;
        }
        int se = isect_solve3(acc, acc + 6, nullptr, Q);
        if (se == JAICOV_ISECT_OK) {
            bool finite = isfinite(acc[9]);
            for (int k = 0; k < 6; k++) finite = finite && isfinite(Q[k]);
            if (!finite) se = JAICOV_ISECT_NOT_FINITE;
        }
        if (se != JAICOV_ISECT_OK) { give_up(se); return; }
        if (!(thr2 > 0.0 && nused > min_rays && qmax > thr2 && qidx < m)) break;
        if (lane == 0) { used[k0 + qidx] = 0; if (resident) sused[qidx] = 0; }
        nused--;
        mode = ISECT_START;
    }
    // the largest angle between two used rays, d = X - X0
    if (resident) {
        __syncthreads();
        for (int t = lane; t < m; t += 64) {
            const IsectImage &im = images[simg[t]];
            sd0[t] = Xr[0] - (im.X0[0] - Xc[0]); sd1[t] = Xr[1] - (im.X0[1] - Xc[1]); sd2[t] = Xr[2] - (im.X0[2] - Xc[2]);
        }
        __syncthreads();
    }
    auto direction = [&](int t, double *d) {
        if (resident) { d[0] = sd0[t]; d[1] = sd1[t]; d[2] = sd2[t]; return; }
        const IsectImage &im = images[ray_image[k0 + t]];
        for (int k = 0; k < 3; k++) d[k] = Xr[k] - (im.X0[k] - Xc[k]);
    };
    auto is_used = [&](int t) { return resident ? sused[t] != 0 : used[k0 + t] != 0; };
    double angle = 0.0;
    for (int i = 0; i + 1 < m; i++) {
        if (!is_used(i)) continue;
        double di[3];
        direction(i, di);
        for (int j = i + 1 + lane; j < m; j += 64) {
            if (!is_used(j)) continue;
            double dj[3];
            direction(j, dj);
            const double c0 = di[1] * dj[2] - di[2] * dj[1], c1 = di[2] * dj[0] - di[0] * dj[2], c2 = di[0] * dj[1] - di[1] * dj[0];
            angle = fmax(angle, atan2(sqrt(c0 * c0 + c1 * c1 + c2 * c2), di[0] * dj[0] + di[1] * dj[1] + di[2] * dj[2]));
        }
    }
    for (int off = 32; off > 0; off >>= 1) angle = fmax(angle, __shfl_xor(angle, off));
    double o[JAICOV_ISECT_OUT_PER_POINT];
    for (int k = 0; k < 3; k++) o[k] = Xr[k] + Xc[k];
    for (int k = 0; k < 6; k++) o[3 + k] = Q[k];
    o[9] = acc[9];
    o[10] = angle;
    bool finite = true;
    for (int k = 0; k < JAICOV_ISECT_OUT_PER_POINT; k++) finite = finite && isfinite(o[k]);
    if (!finite) { give_up(JAICOV_ISECT_NOT_FINITE); return; }
    if (lane == 0) {
        for (int k = 0; k < JAICOV_ISECT_OUT_PER_POINT; k++) op[k] = o[k];
        outcome[2L * p] = st;
        outcome[2L * p + 1] = iters;
    }
}

}  // namespace
}  // namespace jaicov

using namespace jaicov;

extern "C" int jaicov_isect_points(int32_t n_points, const int32_t *ray_begin, const int32_t *ray_image, const double *xy, const double *var,
                                   int32_t n_images, const double *image_io, const double *image_eo, double sigma2apriori,
                                   int32_t max_iterations, double reject_threshold, int32_t min_rays, double *out, int32_t *status,
                                   int32_t *iterations, uint8_t *ray_used, double *ray_q, double *ms_out) {
    // argument checks, host only
    if (n_points < 0 || n_images < 0 || !ray_begin) return JAICOV_ERR_BAD_ARGUMENT;
    if (!(sigma2apriori > 0.0) || max_iterations < 1 || min_rays < 2 || !(reject_threshold >= 0.0)) return JAICOV_ERR_BAD_ARGUMENT;
    if (n_points > 0 && (!out || !status)) return JAICOV_ERR_BAD_ARGUMENT;
    if (n_images > 0 && (!image_io || !image_eo)) return JAICOV_ERR_BAD_ARGUMENT;
    if (!ranges_ok(n_points, ray_begin)) return JAICOV_ERR_BAD_ARGUMENT;
    const long n_rays = ray_begin[n_points];
    if (n_rays > 0 && (!ray_image || !xy)) return JAICOV_ERR_BAD_ARGUMENT;
    for (long k = 0; k < n_rays; k++)
        if (ray_image[k] < 0 || ray_image[k] >= n_images) return JAICOV_ERR_BAD_ARGUMENT;
    if (!dispersions_ok(var, n_rays)) return JAICOV_ERR_BAD_ARGUMENT;

    if (!device_is_gfx950()) return JAICOV_ERR_NO_DEVICE;
    if (ms_out) *ms_out = 0.0;
    if (n_points == 0) return JAICOV_OK;

    BatchCall call;
    const size_t np = (size_t)n_points, nr = (size_t)n_rays, ni = (size_t)n_images;
    const int32_t *d_begin = call.in(ray_begin, np + 1), *d_image = call.in(ray_image, nr);
    const double *d_xy = call.in(xy, 2 * nr), *d_var = call.in(var, 3 * nr), *d_io = call.in(image_io, 3 * ni), *d_eo = call.in(image_eo, 6 * ni);
    IsectImage *d_rec = call.alloc<IsectImage>(ni);
    double *d_out = call.alloc<double>(JAICOV_ISECT_OUT_PER_POINT * np), *d_q = ray_q ? call.alloc<double>(nr) : nullptr;
    int32_t *d_outcome = call.alloc<int32_t>(2 * np);
    uint8_t *d_used = call.filled<uint8_t>(nr, 1);                     // every ray starts as used
    call.run([&](hipStream_t s) {
        if (n_images > 0)
            hipLaunchKernelGGL(isect_image_kernel, dim3((n_images + 255) / 256), dim3(256), 0, s, (int)n_images, d_io, d_eo, d_rec);
        hipLaunchKernelGGL(isect_points_kernel, dim3(n_points), dim3(64), 0, s, d_begin, d_image, d_xy, d_var, d_rec, sigma2apriori,
                           (int)max_iterations, reject_threshold * reject_threshold, (int)min_rays, d_out, d_outcome, d_used, d_q);
    });
    call.out(out, d_out, JAICOV_ISECT_OUT_PER_POINT * np);
    call.outcomes(d_outcome, np, 2, status, iterations, nullptr);
    call.out(ray_used, d_used, nr);
    call.out(ray_q, d_q, nr);
    return call.finish(ms_out);
}
