// lens.hip -- lens-distortion correction of many image points in one launch (include/jaicov_lens.h): the measured coordinates are
// reduced to those of the distortion-free camera by a Newton iteration per point, with their 2 x 2 dispersion, and the inverse
// applies the model.  The model is the reference's, in the order and form of rows.hip (ASF:37-81, TDF:39-134, RSF:39-90, RDF:39-161,
// ZDF:41-227 via DMF:33-101); rows.hip is the adjustment's own evaluation and is not shared with this file
// (tests/test_gpu_lens.py holds the two together through jaicov_neq_get_rows).
//
// One lane works one point.  The coefficients of a point's camera are read through tables that the host builds per call: what
// depends on the coefficient alone (r0^2e, the Zernike n, m and the products of normalisation, sign and binomials of every term) is
// computed there once.  A wave whose points share a camera -- the normal case, callers pass points image by image -- reads the tables
// with an index that is the same in every lane, i.e. by scalar loads, and its coefficient loops are taken by the whole wave; a wave
// with several cameras works them one after the other (the loop over the waiting lanes below), each with uniform loops again.
// Floating-point contraction is off in this file: every product and sum is rounded on its own, as tests/lens_reference.py rounds it.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

#include "../../include/jaicov_lens.h"
#include "batchcall.h"

#pragma clang fp contract(off)

namespace jaicov {
namespace {

// a camera of the call: interior orientation, r0, its coefficients and where the four that work in pairs lie (-1: absent)
struct LensCam {
    double x0, y0, r0;
    int32_t jb, je, jCx, jCy, jBx, jBy, has_di, has_z;
};

// a coefficient: aux is r0^2e for Ai and Di; n, mi and the terms zb .. ze - 1 of the term table for the Zernike kinds
struct LensCoef {
    double value, aux;
    int32_t kind, order, n, mi, zb, ze;
};

// Math.pow(double, int) for small e >= 0, as rows.hip takes it
__host__ __device__ inline double lens_ipow(double b, int e) {
    double r = 1.0;
    for (int i = 0; i < e; i++) r *= b;
    return r;
}

// MathExtension.binomial (MathExtension.java:53-64)
inline long lens_binomial(int n, int k) {
    if (k < 0 || k > n) return 0;
    if (k > n - k) k = n - k;
    long result = 1;
    for (int i = 1; i <= k; i++) result = result * (n - k + i) / i;
    return result;
}

// sum of the camera's terms at (xs, ys, N) into (sx, sy), and of their chain-rule factors into d[4] = dXxs, dXys, dYxs, dYys.
// Everything but xs, ys, N is the same in every lane that gets here together.
__device__ __forceinline__ void lens_eval(const LensCam &cm, const LensCoef *__restrict__ coef, const int32_t *__restrict__ zt_p,
                                          const double *__restrict__ zt_c, double xs, double ys, double N, double &sx, double &sy,
                                          double *d) {
    sx = 0.0; sy = 0.0;
    d[0] = 0.0; d[1] = 0.0; d[2] = 0.0; d[3] = 0.0;
#define LENS_ADD(deltaX, deltaY, dXxs, dXys, dYxs, dYys)                                  \
    do {                                                                                  \
        sx += (deltaX); sy += (deltaY);                                                   \
        d[0] += (dXxs); d[1] += (dXys); d[2] += (dYxs); d[3] += (dYys);                   \
    } while (0)
    const int jb = cm.jb, je = cm.je;
    const double r0 = cm.r0;
    const double r2 = xs * xs + ys * ys, r02 = r0 * r0;
    const double xxs2 = 2.0 * xs * xs, yys2 = 2.0 * ys * ys, xys2 = 2.0 * xs * ys;
    // ASF:37-81
    if (cm.jCx >= 0 && cm.jCy >= 0) {
        const double cx = coef[cm.jCx].value, cy = coef[cm.jCy].value;
        LENS_ADD(cx * xs + cy * ys, 0.0, cx, cy, 0.0, 0.0);
    }
    // TDF:39-134
    if (cm.jBx >= 0 && cm.jBy >= 0) {
        const double bx = coef[cm.jBx].value, by = coef[cm.jBy].value;
        const double deltaX = bx * (r2 + xxs2) + by * xys2;
        const double deltaY = by * (r2 + yys2) + bx * xys2;
        const double dXxs = 2.0 * (3.0 * bx * xs + by * ys);
        const double dXys = 2.0 * (by * xs + bx * ys);
        const double dYxs = 2.0 * (by * xs + bx * ys);
        const double dYys = 2.0 * (bx * xs + 3.0 * by * ys);
        LENS_ADD(deltaX, deltaY, dXxs, dXys, dYxs, dYys);
        for (int j = jb; j < je; j++) {
            if (coef[j].kind != JAICOV_DIST_TANGENTIAL_BI) continue;
            const double bi = coef[j].value;
            const int e = coef[j].order;
            const double rim1 = lens_ipow(r2, e - 1);
            const double ri = rim1 * r2;
            const double dTani = bi * ri;
            const double constTani = 2.0 * bi * e * rim1;
            const double cX = deltaX * constTani, cY = deltaY * constTani;
            LENS_ADD(deltaX * dTani, deltaY * dTani, dTani * dXxs + xs * cX, dTani * dXys + ys * cX, dTani * dYxs + xs * cY,
                     dTani * dYys + ys * cY);
        }
    }
    // RSF:39-90
    for (int j = jb; j < je; j++) {
        if (coef[j].kind != JAICOV_DIST_RADIAL_AI) continue;
        const double ai = coef[j].value;
        const int e = coef[j].order;
        const double rim1 = lens_ipow(r2, e - 1);
        const double dRi = rim1 * r2 - coef[j].aux;
        const double dRadi = ai * dRi;
        const double constRadi = ai * e * rim1;
        LENS_ADD(xs * dRadi, ys * dRadi, xxs2 * constRadi + dRadi, xys2 * constRadi, xys2 * constRadi, yys2 * constRadi + dRadi);
    }
    // RDF:39-161
    if (cm.has_di)
        for (int j = jb; j < je; j++) {
            if (coef[j].kind != JAICOV_DIST_DISTANCE_DI) continue;
            const double di = coef[j].value;
            const int e = coef[j].order;
            const double rim1 = lens_ipow(r2, e - 1);
            const double dRi = rim1 * r2 - coef[j].aux;
            const double dDisti = (di * dRi) / N;
            const double constRadi = (di * e * rim1) / N;
            LENS_ADD(xs * dDisti, ys * dDisti, xxs2 * constRadi + dDisti, xys2 * constRadi, xys2 * constRadi, yys2 * constRadi + dDisti);
        }
    // ZDF:153-227 (X, Y), then ZDF:41-143 (Gradient), literally -- the integer division of the radial exponents included
    if (cm.has_z) {
        const double xxs = xs * xs, yys = ys * ys, xys = xs * ys;
        const double phi = atan2(ys, xs);
        const double rn2 = r2 / r02;
        const double const2rnr0 = 2.0 / rn2 / r02;
        for (int kind = JAICOV_DIST_ZERNIKE_X; kind <= JAICOV_DIST_ZERNIKE_Z; kind++)
            for (int j = jb; j < je; j++) {
                if (coef[j].kind != kind) continue;
                const double zi = coef[j].value;
                const int mi = coef[j].mi;
                const double m = mi;
                double sinmphi, cosmphi;
                sincos(m * phi, &sinmphi, &cosmphi);
                for (int t = coef[j].zb; t < coef[j].ze; t++) {
                    const int pj = zt_p[t];
                    const double cj = zt_c[t];
                    // rn2^(p/2 - 1) by pow, rn2^(p/2) from it
                    const int ce = pj / 2 - 1;
                    const double pw_lo = pow(rn2, (double)ce), pw_hi = pw_lo * rn2;
                    const double cX = (mi < 0) ? (-pj * xs * sinmphi + m * ys * cosmphi) : (pj * xs * cosmphi + m * ys * sinmphi);
                    const double cY = (mi < 0) ? (-pj * ys * sinmphi - m * xs * cosmphi) : (pj * ys * cosmphi - m * xs * sinmphi);
                    if (kind != JAICOV_DIST_ZERNIKE_Z) {
                        const double constC = cj * pw_hi;
                        const double constZ = zi * cj / r02 * pw_lo;
                        const double az = (mi < 0) ? -constC * sinmphi : constC * cosmphi;
                        const double delta = zi * az;
                        if (kind == JAICOV_DIST_ZERNIKE_X) LENS_ADD(delta, 0.0, constZ * cX, constZ * cY, 0.0, 0.0);
                        else LENS_ADD(0.0, delta, 0.0, 0.0, constZ * cX, constZ * cY);
                    } else {
                        const double constC = cj / r02 * pw_lo;
                        double dXxs, dXys, dYxs, dYys;
                        if (mi < 0) {
                            dXxs = ce * xs * const2rnr0 * cX - pj * sinmphi + m / r2 * (pj * xys * cosmphi + m * yys * sinmphi);
                            dXys = ce * ys * const2rnr0 * cX + m * cosmphi - m / r2 * (pj * xxs * cosmphi + m * xys * sinmphi);
                            dYxs = ce * xs * const2rnr0 * cY - m * cosmphi + m / r2 * (pj * yys * cosmphi - m * xys * sinmphi);
                            dYys = ce * ys * const2rnr0 * cY - pj * sinmphi - m / r2 * (pj * xys * cosmphi - m * xxs * sinmphi);
                        } else {
                            dXxs = ce * xs * const2rnr0 * cX + pj * cosmphi + m / r2 * (pj * xys * sinmphi - m * yys * cosmphi);
                            dXys = ce * ys * const2rnr0 * cX + m * sinmphi - m / r2 * (pj * xxs * sinmphi - m * xys * cosmphi);
                            dYxs = ce * xs * const2rnr0 * cY - m * sinmphi + m / r2 * (pj * yys * sinmphi + m * xys * cosmphi);
                            dYys = ce * ys * const2rnr0 * cY + pj * cosmphi - m / r2 * (pj * xys * sinmphi + m * xxs * cosmphi);
                        }
                        const double zc = zi * constC;
                        LENS_ADD(zc * cX, zc * cY, zc * dXxs, zc * dXys, zc * dYxs, zc * dYys);
                    }
                }
            }
    }
#undef LENS_ADD
}

constexpr int LENS_THREADS = 256;

// CORRECT: measured -> ideal by Newton; otherwise ideal -> measured by one evaluation
template <bool CORRECT>
__global__ __launch_bounds__(LENS_THREADS) void lens_points_kernel(long n, const int32_t *__restrict__ pt_camera,
                                                                   const double *__restrict__ xy, const double *__restrict__ var,
                                                                   const double *__restrict__ depth, const LensCam *__restrict__ cams,
                                                                   const LensCoef *__restrict__ coef, const int32_t *__restrict__ zt_p,
                                                                   const double *__restrict__ zt_c, int max_iter, double tol,
                                                                   double *__restrict__ xy_out, double *__restrict__ var_out,
                                                                   double *__restrict__ jac_out, int32_t *__restrict__ status,
                                                                   int32_t *__restrict__ iterations) {
    const long i = (long)blockIdx.x * LENS_THREADS + threadIdx.x;
    if (i >= n) return;
    const double SQRT_EPS = sqrt(ldexp(1.0, -53));
    const int cam = pt_camera[i];
    const double2 p = reinterpret_cast<const double2 *>(xy)[i];
    const double depth_i = depth ? depth[i] : 1.0;
    double q00 = 1.0, q01 = 0.0, q11 = 1.0;
    if (var_out && var) {
        const double vx = var[3 * i], vy = var[3 * i + 1], rho = var[3 * i + 2];
        q00 = vx; q11 = vy; q01 = rho * sqrt(vx * vy);
    }
    double xs = 0.0, ys = 0.0, ox = 0.0, oy = 0.0, d[4] = {0.0, 0.0, 0.0, 0.0}, det = 1.0;
    int st = JAICOV_LENS_OK, it = 0;
    // the cameras of this wave, one after the other: the lowest lane still waiting names the camera, every lane with that camera
    // works, and inside the camera is the same in every lane at work.  The loop is taken by the whole wave, once per camera.
    unsigned long long pending = __ballot(1);
    while (pending) {
        const int c0 = __builtin_amdgcn_readlane(cam, __ffsll((long long)pending) - 1);
        const bool mine = cam == c0;
        pending &= ~__ballot(mine);
        if (!mine) continue;
        // every lane at work holds c0 in cam; taken from the first of them, the compiler knows it to be the same in all as well
        const LensCam cm = cams[__builtin_amdgcn_readfirstlane(cam)];
        const double mx = p.x - cm.x0, my = p.y - cm.y0;
        xs = mx; ys = my;
        double N = 1.0;
        if (cm.has_di) N = (fabs(depth_i) > 0.0 && fabs(depth_i) < INFINITY) ? depth_i : NAN;   // 0, NaN, Inf: NOT_FINITE below
        st = CORRECT ? JAICOV_LENS_NOT_CONVERGED : JAICOV_LENS_OK;
        bool converged = false;
        for (;;) {
            double sx, sy;
            lens_eval(cm, coef, zt_p, zt_c, xs, ys, N, sx, sy, d);
            d[0] = 1.0 + d[0]; d[3] = 1.0 + d[3];                       // J
            const double z = (xs + ys + sx + sy + d[0] + d[1] + d[2] + d[3]) * 0.0;
            if (z != 0.0) { st = JAICOV_LENS_NOT_FINITE; break; }
            det = d[0] * d[3] - d[1] * d[2];
            if (!(det > SQRT_EPS)) { st = JAICOV_LENS_SINGULAR; break; }
            if (!CORRECT) { ox = (cm.x0 + xs) + sx; oy = (cm.y0 + ys) + sy; break; }
            if (converged || it >= max_iter) { ox = cm.x0 + xs; oy = cm.y0 + ys; break; }
            const double f0 = (mx - xs) - sx, f1 = (my - ys) - sy;
            const double dx = (d[3] * f0 - d[1] * f1) / det, dy = (d[0] * f1 - d[2] * f0) / det;
            it++;
            xs = xs + dx; ys = ys + dy;
            if (fmax(fabs(dx), fabs(dy)) <= tol * fmax(1.0, fmax(fabs(xs), fabs(ys)))) { converged = true; st = JAICOV_LENS_OK; }
        }
    }
    const bool failed = st >= JAICOV_LENS_SINGULAR;
    reinterpret_cast<double2 *>(xy_out)[i] = failed ? make_double2(NAN, NAN) : make_double2(ox, oy);
    status[i] = st;
    if (CORRECT && iterations) iterations[i] = it;
    if (jac_out) {
        reinterpret_cast<double2 *>(jac_out)[2 * i] = failed ? make_double2(NAN, NAN) : make_double2(d[0], d[1]);
        reinterpret_cast<double2 *>(jac_out)[2 * i + 1] = failed ? make_double2(NAN, NAN) : make_double2(d[2], d[3]);
    }
    if (var_out) {
        // M = J^-1 (by the adjugate) or J; Q' = (M Q) M'
        const double m00 = CORRECT ? d[3] / det : d[0], m01 = CORRECT ? -(d[1] / det) : d[1];
        const double m10 = CORRECT ? -(d[2] / det) : d[2], m11 = CORRECT ? d[0] / det : d[3];
        const double b00 = m00 * q00 + m01 * q01, b01 = m00 * q01 + m01 * q11;
        const double b10 = m10 * q00 + m11 * q01, b11 = m10 * q01 + m11 * q11;
        const double p00 = b00 * m00 + b01 * m01, p01 = b00 * m10 + b01 * m11, p11 = b10 * m10 + b11 * m11;
        var_out[3 * i] = failed ? NAN : p00;
        var_out[3 * i + 1] = failed ? NAN : p11;
        var_out[3 * i + 2] = failed ? NAN : p01 / sqrt(p00 * p11);
    }
}

// the tables of a call, as the kernel reads them
struct LensTables {
    std::vector<LensCam> cams;
    std::vector<LensCoef> coef;
    std::vector<int32_t> zt_p;
    std::vector<double> zt_c;
};

// every argument check of the two calls, and the tables.  false: JAICOV_ERR_BAD_ARGUMENT
bool lens_check_and_build(int32_t n_points, const int32_t *pt_camera, const double *xy, const double *var, const double *depth,
                          int32_t n_cameras, const double *cam_io, const double *cam_r0, const int32_t *cam_dist_begin,
                          const int32_t *dist_kind, const int32_t *dist_order, const double *dist_value, const double *xy_out,
                          const int32_t *status, LensTables &t) {
    if (n_points < 0 || n_cameras < 0) return false;
    if (n_points > 0 && (!pt_camera || !xy || !xy_out || !status)) return false;
    if (!cam_dist_begin || (n_cameras > 0 && (!cam_io || !cam_r0))) return false;
    if (!ranges_ok(n_cameras, cam_dist_begin)) return false;
    const int32_t nd = cam_dist_begin[n_cameras];
    if (nd > 0 && (!dist_kind || !dist_order || !dist_value)) return false;
    for (int32_t j = 0; j < nd; j++) {
        const int k = dist_kind[j];
        if (k < JAICOV_DIST_AFFINITY_CX || k > JAICOV_DIST_ZERNIKE_Z) return false;
        const bool has_order = k == JAICOV_DIST_TANGENTIAL_BI || k >= JAICOV_DIST_RADIAL_AI;
        if (has_order && dist_order[j] < 1) return false;
        if (k >= JAICOV_DIST_ZERNIKE_X && dist_order[j] > JAICOV_LENS_MAX_ZERNIKE_ORDER) return false;
    }
    t.cams.resize((size_t)n_cameras);
    t.coef.resize((size_t)nd);
    for (int32_t c = 0; c < n_cameras; c++) {
        const int32_t jb = cam_dist_begin[c], je = cam_dist_begin[c + 1];
        if (je - jb > JAICOV_MAX_DIST_PER_CAMERA) return false;
        if (!(fabs(cam_io[3 * c + 2]) > 0.0)) return false;
        LensCam &cm = t.cams[c];
        cm = LensCam{cam_io[3 * c], cam_io[3 * c + 1], cam_r0[c], jb, je, -1, -1, -1, -1, 0, 0};
        bool needs_r0 = false;
        for (int32_t j = jb; j < je; j++) {
            const int k = dist_kind[j];
            if (k == JAICOV_DIST_AFFINITY_CX) cm.jCx = j;
            else if (k == JAICOV_DIST_AFFINITY_CY) cm.jCy = j;
            else if (k == JAICOV_DIST_TANGENTIAL_BX) cm.jBx = j;
            else if (k == JAICOV_DIST_TANGENTIAL_BY) cm.jBy = j;
            if (k == JAICOV_DIST_DISTANCE_DI) cm.has_di = 1;
            if (k >= JAICOV_DIST_ZERNIKE_X) cm.has_z = 1;
            needs_r0 = needs_r0 || k >= JAICOV_DIST_RADIAL_AI;
        }
        if (needs_r0 && !(cam_r0[c] > 0.0)) return false;
        const double r02 = cam_r0[c] * cam_r0[c];
        for (int32_t j = jb; j < je; j++) {
            LensCoef &cf = t.coef[j];
            cf = LensCoef{dist_value[j], 0.0, dist_kind[j], dist_order[j], 0, 0, 0, 0};
            if (cf.kind == JAICOV_DIST_RADIAL_AI || cf.kind == JAICOV_DIST_DISTANCE_DI) cf.aux = lens_ipow(r02, cf.order);
            if (cf.kind >= JAICOV_DIST_ZERNIKE_X) {
                const int order = cf.order;
                const int n = (int)ceil((-3.0 + sqrt(9.0 + 8.0 * order)) / 2.0);     // ZernikeCoefficient.java:43-44
                const int mi = 2 * order - n * (n + 2);
                const int halfnm = (n - abs(mi)) / 2;
                const double length = sqrt((1 + ((mi != 0) ? 1 : 0)) * (n + 1) / 3.14159265358979323846);
                cf.n = n; cf.mi = mi;
                cf.zb = (int32_t)t.zt_p.size();
                for (int k = 0; k <= halfnm; k++) {
                    t.zt_p.push_back(n - 2 * k);
                    t.zt_c.push_back(length * (double)(((k % 2 == 0) ? 1 : -1) * lens_binomial(n - k, k) * lens_binomial(n - 2 * k, halfnm - k)));
                }
                cf.ze = (int32_t)t.zt_p.size();
            }
        }
    }
    for (int32_t k = 0; k < n_points; k++) {
        if (pt_camera[k] < 0 || pt_camera[k] >= n_cameras) return false;
        if (!depth && t.cams[pt_camera[k]].has_di) return false;
    }
    if (!dispersions_ok(var, n_points)) return false;
    return true;
}

template <bool CORRECT>
int lens_run(int32_t n_points, const int32_t *pt_camera, const double *xy, const double *var, const double *depth, const LensTables &t,
             int32_t max_iterations, double tolerance, double *xy_out, double *var_out, double *jac_out, int32_t *status,
             int32_t *iterations, double *ms_out) {
    if (!device_is_gfx950()) return JAICOV_ERR_NO_DEVICE;
    if (ms_out) *ms_out = 0.0;
    if (n_points == 0) return JAICOV_OK;

    BatchCall call;
    const size_t np = (size_t)n_points;
    const int32_t *d_cam = call.in(pt_camera, np);
    const double *d_xy = call.in(xy, 2 * np), *d_var = call.in(var_out ? var : nullptr, 3 * np), *d_depth = call.in(depth, np);
    const LensCam *d_cams = call.in(t.cams);
    const LensCoef *d_coef = call.in(t.coef);
    const int32_t *d_ztp = call.in(t.zt_p);
    const double *d_ztc = call.in(t.zt_c);
    double *d_xyo = call.alloc<double>(2 * np), *d_varo = var_out ? call.alloc<double>(3 * np) : nullptr,
           *d_jac = jac_out ? call.alloc<double>(4 * np) : nullptr;
    int32_t *d_status = call.alloc<int32_t>(np), *d_it = iterations ? call.alloc<int32_t>(np) : nullptr;   // lens_distort passes none
    const double tol = tolerance > 0.0 ? tolerance : sqrt(ldexp(1.0, -53));
    call.run([&](hipStream_t s) {
        hipLaunchKernelGGL(lens_points_kernel<CORRECT>, dim3((unsigned)((np + LENS_THREADS - 1) / LENS_THREADS)), dim3(LENS_THREADS), 0, s,
                           (long)n_points, d_cam, d_xy, d_var, d_depth, d_cams, d_coef, d_ztp, d_ztc, (int)max_iterations, tol, d_xyo, d_varo,
                           d_jac, d_status, d_it);
    });
    call.out(xy_out, d_xyo, 2 * np);
    call.out(var_out, d_varo, 3 * np);
    call.out(jac_out, d_jac, 4 * np);
    call.out(status, d_status, np);
    call.out(iterations, d_it, np);
    return call.finish(ms_out);
}

}  // namespace
}  // namespace jaicov

using namespace jaicov;

extern "C" int jaicov_lens_correct(int32_t n_points, const int32_t *pt_camera, const double *xy, const double *var, const double *depth,
                                   int32_t n_cameras, const double *cam_io, const double *cam_r0, const int32_t *cam_dist_begin,
                                   const int32_t *dist_kind, const int32_t *dist_order, const double *dist_value, int32_t max_iterations,
                                   double tolerance, double *xy_out, double *var_out, double *jac_out, int32_t *status,
                                   int32_t *iterations, double *ms_out) {
    // argument checks, host only
    LensTables t;
    if (max_iterations < 1 || !(tolerance >= 0.0) || !isfinite(tolerance)) return JAICOV_ERR_BAD_ARGUMENT;
    if (!lens_check_and_build(n_points, pt_camera, xy, var, depth, n_cameras, cam_io, cam_r0, cam_dist_begin, dist_kind, dist_order,
                              dist_value, xy_out, status, t))
        return JAICOV_ERR_BAD_ARGUMENT;
    return lens_run<true>(n_points, pt_camera, xy, var, depth, t, max_iterations, tolerance, xy_out, var_out, jac_out, status, iterations,
                          ms_out);
}

extern "C" int jaicov_lens_distort(int32_t n_points, const int32_t *pt_camera, const double *xy, const double *var, const double *depth,
                                   int32_t n_cameras, const double *cam_io, const double *cam_r0, const int32_t *cam_dist_begin,
                                   const int32_t *dist_kind, const int32_t *dist_order, const double *dist_value, double *xy_out,
                                   double *var_out, double *jac_out, int32_t *status, double *ms_out) {
    // argument checks, host only
    LensTables t;
    if (!lens_check_and_build(n_points, pt_camera, xy, var, depth, n_cameras, cam_io, cam_r0, cam_dist_begin, dist_kind, dist_order,
                              dist_value, xy_out, status, t))
        return JAICOV_ERR_BAD_ARGUMENT;
    return lens_run<false>(n_points, pt_camera, xy, var, depth, t, 1, 0.0, xy_out, var_out, jac_out, status, nullptr, ms_out);
}
