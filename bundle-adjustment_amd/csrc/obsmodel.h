// obsmodel.h -- what the device code knows about an observation row, stated once for everything that assembles normal equations
// from the rows (assemble.hip, schur.hip, densemode.hip, engine_create.hip) or reads the cofactor matrix through them
// (reliability.hip, vce.hip).  predict.hip, calibration.hip, newpoints.hip, transform.hip and pairrows.h hold their own view to it.
// Compact rows (rows.hip): rowsA is [2 KROW][n_ip], local row l of image coordinate r at (2 l + r) n_ip + ip, with
//   l: 0..2 = X,Y,Z of the point; 3..5 = x0,y0,c; 6..11 = X0,Y0,Z0,omega,phi,kappa; 12.. = distortion coefficients   (KROW = 12 + MAXD)
// The shared local columns of an image (everything but its points) are counted
//   c: 0..2 = x0,y0,c; 3..8 = X0,Y0,Z0,omega,phi,kappa; 9.. = distortion coefficients                              (KC_MAX = 9 + MAXD)
// A global column < 0 is a fixed parameter.
// It does not go into one unit with wavealg.h: obs_weight takes the contraction of its first inclusion (both headers refuse).
#pragma once
#ifdef JAICOV_WAVEALG_H
#error "obsmodel.h after wavealg.h: obs_weight would lose the engine's contraction"
#endif
#define JAICOV_OBSMODEL_H
#include "ba_kernels.h"
#include "obsweight.h"

namespace jaicov {

// shared local columns of an image of camera cam
__device__ __forceinline__ int obs_kc(const DevProblem &p, int cam) { return 9 + p.cam_dist_begin[cam + 1] - p.cam_dist_begin[cam]; }
// shared local column c (0..kc) -> local row of the compact rows
__device__ __forceinline__ int obs_shared_row(int c) { return c < 3 ? 3 + c : (c < 9 ? 6 + (c - 3) : 12 + (c - 9)); }
// shared local column c -> global column; jb = cam_dist_begin[cam]
__device__ __forceinline__ int obs_shared_col(const DevProblem &p, int img, int cam, int jb, int c) {
    return c < 3 ? p.io_col[3 * cam + c] : (c < 9 ? p.eo_col[6 * img + (c - 3)] : p.dist_col[jb + (c - 9)]);
}
// local row l of the compact rows -> global column
__device__ __forceinline__ int obs_row_col(const DevProblem &p, int pt, int img, int cam, int jb, int l) {
    return l < 3 ? p.point_col[3 * pt + l]
                 : (l < 6 ? p.io_col[3 * cam + l - 3] : (l < 12 ? p.eo_col[6 * img + l - 6] : p.dist_col[jb + l - 12]));
}
// P = s0 inv(D) of engine image point ip with 2 x 2 weights: p00, p01, p11
__device__ __forceinline__ void obs_weight(const DevProblem &p, int ip, double s0, double &p00, double &p01, double &p11) {
    obs_weight(p.ip_var_x[ip], p.ip_var_y[ip], p.ip_rho[ip], s0, p00, p01, p11);
}
// scale bar s (PDF:210-283): columns and coefficients of its row over the end points a, b, the computed length; the misclosure's sign is the caller's
__device__ __forceinline__ void obs_scalebar_row(const DevProblem &p, const double *vals, int s, int col[6], double ev[6], double &len) {
    const int pa = p.sb_a[s], pb = p.sb_b[s];
    const double *a = vals + 3 * pa, *b = vals + 3 * pb;
    const double dX = b[0] - a[0], dY = b[1] - a[1], dZ = b[2] - a[2];
    len = sqrt(dX * dX + dY * dY + dZ * dZ);
    ev[0] = -dX / len; ev[1] = -dY / len; ev[2] = -dZ / len; ev[3] = dX / len; ev[4] = dY / len; ev[5] = dZ / len;
    for (int t = 0; t < 6; t++) col[t] = t < 3 ? p.point_col[3 * pa + t] : p.point_col[3 * pb + t - 3];
}
// directly observed row (PDF:447-473), row = dg_row_begin[g] + k: its column, and
__device__ __forceinline__ int obs_direct_col(const DevProblem &p, int row) { return p.slot_col[p.dg_slot[row]]; }
// w - A dx = observed - value - dx[col]; dx null or a fixed parameter: observed - value
__device__ __forceinline__ double obs_direct_w(const DevProblem &p, const double *vals, const double *dx, int row, int col) {
    double w = p.dg_obs[row] - vals[p.dg_slot[row]];
    if (dx && col >= 0) w -= dx[col];
    return w;
}
// sum over a workgroup of 256 threads: the LDS tree 128, 64, .., 1; every thread returns the sum
__device__ __forceinline__ double block_sum_256(double *red, double x) {
    red[threadIdx.x] = x;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

}  // namespace jaicov
