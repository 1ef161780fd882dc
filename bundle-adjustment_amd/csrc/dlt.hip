// dlt.hip -- batched direct linear transformation (include/jaicov_dlt.h): DirectLinearTransformation.adjust of the reference
// (dlt/DirectLinearTransformation.java = DT, dlt/DLTPartialDerivativeFactory.java = DPF) for every image of a call in one launch.
//
// One wave (one workgroup of 64 lanes) per image; the whole Gauss-Newton loop of DT:107-165 runs inside it, with no host round
// trip.  The per-image work is a chain of dependent fp64 adds (the normal equations are summed in the reference's observation
// order, so that every run and the restatement in tests/dlt_reference.py give the same bits) and a bordered solve of order <= 16:
// latency, not throughput, bounds it, and many resident single-wave workgroups per SIMD hide that latency better than wider
// workgroups would.
//   Normal equations.  A does not depend on b, so the 66 entries of the upper A'A (DPF:238-344) are summed once per image: lane l
//   owns entry l (lanes 0 and 1 also entries 64 and 65).  A'w depends on b and is summed again before every solve (lanes 0..10).
//   Observations are staged DLT_CHUNK at a time in LDS; an image with at most DLT_CHUNK observations keeps them resident.
//   Solve.  Lane 0 assembles the bordered system (restriction rows DPF:86-236), preconditions it (NES:82-91), and factorises it
//   with the Bunch-Kaufman dsptrf / dsptrs of MathExtension.solve (MX:338-366), LAPACK's reference algorithms.
//   Expansion (DT:185-267) and the 3 x 3 LU of the projection centre run on lane 0 as well.
// Floating-point contraction is off in this file: every product and sum is rounded as the reference rounds it.
#include <hip/hip_runtime.h>

#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/jaicov_dlt.h"
#include "batchcall.h"
#include "dlt.h"

#pragma clang fp contract(off)

namespace jaicov {
namespace {

#define DLT_PK(i, j) ((i) + (j) * ((j) + 1) / 2)   // packed 'U' column-major, i <= j

// A[row][k] of one observation (DPF:274-322): k 0..3 -> (X Y Z 1 | 0), 4..7 -> (0 | X Y Z 1), 8..10 -> (-x P | -y P)
__device__ inline void dlt_a(int k, double x, double y, double X, double Y, double Z, double &a0, double &a1) {
    const int q = k < 8 ? (k & 3) : k - 8;
    const double P = q == 0 ? X : (q == 1 ? Y : (q == 2 ? Z : 1.0));
    if (k < 4) { a0 = P; a1 = 0.0; }
    else if (k < 8) { a0 = 0.0; a1 = P; }
    else { a0 = -x * P; a1 = -y * P; }
}

// dsptrf('U') on a packed matrix in LDS, one lane (LAPACK's reference algorithm, loop for loop).  AP(i) is 1-based.  Returns info (> 0: exactly zero pivot block).
#define AP(i) ap[(i) - 1]
__device__ int dlt_idamax1(int n, const double *x) {
    if (n < 1) return 0;
    int im = 1;
    double dm = fabs(x[0]);
    for (int i = 2; i <= n; i++)
        if (fabs(x[i - 1]) > dm) { im = i; dm = fabs(x[i - 1]); }
    return im;
}

__device__ int dlt_dsptrf(int n, double *ap, int *ipiv) {
    const double alpha = (1.0 + sqrt(17.0)) / 8.0;
    int info = 0;
    int k = n;
    int kc = (n - 1) * n / 2 + 1;
    while (k >= 1) {
        int knc = kc;
        int kstep = 1;
        int kp, kpc = 0, imax = 0, jmax;
        const double absakk = fabs(AP(kc + k - 1));
        double colmax = 0.0;
        if (k > 1) {
            imax = dlt_idamax1(k - 1, &AP(kc));
            colmax = fabs(AP(kc + imax - 1));
        }
        if ((absakk > colmax ? absakk : colmax) == 0.0) {
            if (info == 0) info = k;
            kp = k;
        } else {
            if (absakk >= alpha * colmax) {
                kp = k;
            } else {
                double rowmax = 0.0;
                jmax = imax;
                int kx = imax * (imax + 1) / 2 + imax;
                for (int j = imax + 1; j <= k; j++) {
                    if (fabs(AP(kx)) > rowmax) { rowmax = fabs(AP(kx)); jmax = j; }
                    kx += j;
                }
                kpc = (imax - 1) * imax / 2 + 1;
                if (imax > 1) {
                    jmax = dlt_idamax1(imax - 1, &AP(kpc));
                    const double t = fabs(AP(kpc + jmax - 1));
                    if (t > rowmax) rowmax = t;
                }
                if (absakk >= alpha * colmax * (colmax / rowmax)) kp = k;
                else if (fabs(AP(kpc + imax - 1)) >= alpha * rowmax) kp = imax;
                else { kp = imax; kstep = 2; }
            }
            const int kk = k - kstep + 1;
            if (kstep == 2) knc = knc - k + 1;
            if (kp != kk) {
                kpc = (kp - 1) * kp / 2 + 1;
                for (int i = 0; i < kp - 1; i++) { const double t = AP(knc + i); AP(knc + i) = AP(kpc + i); AP(kpc + i) = t; }
                int kx = kpc + kp - 1;
                for (int j = kp + 1; j <= kk - 1; j++) {
                    kx = kx + j - 1;
                    const double t = AP(knc + j - 1); AP(knc + j - 1) = AP(kx); AP(kx) = t;
                }
                double t = AP(knc + kk - 1); AP(knc + kk - 1) = AP(kpc + kp - 1); AP(kpc + kp - 1) = t;
                if (kstep == 2) { t = AP(kc + k - 2); AP(kc + k - 2) = AP(kc + kp - 1); AP(kc + kp - 1) = t; }
            }
            if (kstep == 1) {
                const double r1 = 1.0 / AP(kc + k - 1);
                int kkx = 1;
                for (int j = 1; j <= k - 1; j++) {
                    const double xj = AP(kc + j - 1);
                    if (xj != 0.0) {
                        const double temp = -r1 * xj;
                        int kq = kkx;
                        for (int i = 1; i <= j; i++) { AP(kq) += AP(kc + i - 1) * temp; kq++; }
                    }
                    kkx += j;
                }
                for (int i = 0; i < k - 1; i++) AP(kc + i) *= r1;
            } else if (k > 2) {
                double d12 = AP(k - 1 + (k - 1) * k / 2);
                const double d22 = AP(k - 1 + (k - 2) * (k - 1) / 2) / d12;
                const double d11 = AP(k + (k - 1) * k / 2) / d12;
                const double t = 1.0 / (d11 * d22 - 1.0);
                d12 = t / d12;
                for (int j = k - 2; j >= 1; j--) {
                    const double wkm1 = d12 * (d11 * AP(j + (k - 2) * (k - 1) / 2) - AP(j + (k - 1) * k / 2));
                    const double wk = d12 * (d22 * AP(j + (k - 1) * k / 2) - AP(j + (k - 2) * (k - 1) / 2));
                    for (int i = j; i >= 1; i--)
                        AP(i + (j - 1) * j / 2) = AP(i + (j - 1) * j / 2) - AP(i + (k - 1) * k / 2) * wk - AP(i + (k - 2) * (k - 1) / 2) * wkm1;
                    AP(j + (k - 1) * k / 2) = wk;
                    AP(j + (k - 2) * (k - 1) / 2) = wkm1;
                }
            }
        }
        if (kstep == 1) ipiv[k - 1] = kp;
        else { ipiv[k - 1] = -kp; ipiv[k - 2] = -kp; }
        k -= kstep;
        kc = knc - k;
    }
    return info;
}

// dsptrs('U', n, nrhs = 1) with the factorisation of dlt_dsptrf
__device__ void dlt_dsptrs(int n, const double *ap, const int *ipiv, double *b) {
#define B(i) b[(i) - 1]
    int k = n;
    int kc = n * (n + 1) / 2 + 1;
    while (k >= 1) {
        kc -= k;
        if (ipiv[k - 1] > 0) {
            const int kp = ipiv[k - 1];
            if (kp != k) { const double t = B(k); B(k) = B(kp); B(kp) = t; }
            for (int i = 1; i <= k - 1; i++) B(i) += -1.0 * AP(kc + i - 1) * B(k);
            B(k) *= 1.0 / AP(kc + k - 1);
            k -= 1;
        } else {
            const int kp = -ipiv[k - 1];
            if (kp != k - 1) { const double t = B(k - 1); B(k - 1) = B(kp); B(kp) = t; }
            for (int i = 1; i <= k - 2; i++) B(i) += -1.0 * AP(kc + i - 1) * B(k);
            for (int i = 1; i <= k - 2; i++) B(i) += -1.0 * AP(kc - (k - 1) + i - 1) * B(k - 1);
            const double akm1k = AP(kc + k - 2);
            const double akm1 = AP(kc - 1) / akm1k;
            const double ak = AP(kc + k - 1) / akm1k;
            const double denom = akm1 * ak - 1.0;
            const double bkm1 = B(k - 1) / akm1k;
            const double bk = B(k) / akm1k;
            B(k - 1) = (ak * bkm1 - bk) / denom;
            B(k) = (akm1 * bk - bkm1) / denom;
            kc = kc - k + 1;
            k -= 2;
        }
    }
    k = 1;
    kc = 1;
    while (k <= n) {
        if (ipiv[k - 1] > 0) {
            double sm = 0.0;
            for (int i = 1; i <= k - 1; i++) sm += AP(kc + i - 1) * B(i);                // dgemv('T')
            B(k) += -1.0 * sm;
            const int kp = ipiv[k - 1];
            if (kp != k) { const double t = B(k); B(k) = B(kp); B(kp) = t; }
            kc += k;
            k += 1;
        } else {
            double sm = 0.0, sm2 = 0.0;
            for (int i = 1; i <= k - 1; i++) sm += AP(kc + i - 1) * B(i);
            B(k) += -1.0 * sm;
            for (int i = 1; i <= k - 1; i++) sm2 += AP(kc + k + i - 1) * B(i);
            B(k + 1) += -1.0 * sm2;
            const int kp = -ipiv[k - 1];
            if (kp != k) { const double t = B(k); B(k) = B(kp); B(kp) = t; }
            kc += 2 * k + 1;
            k += 2;
        }
    }
#undef B
}
#undef AP

// One restriction row (DPF:86-236): row[0..10] of the border and the misclosure, from the current b and the image's io.
__device__ void dlt_restriction(int type, const double *b, double x0, double y0, double c, double *row, double *w) {
    const double b11 = b[0], b12 = b[1], b13 = b[2], b21 = b[4], b22 = b[5], b23 = b[6], b31 = b[8], b32 = b[9], b33 = b[10];
    const double sb11 = b11 * b11, sb12 = b12 * b12, sb13 = b13 * b13;
    const double sb21 = b21 * b21, sb22 = b22 * b22, sb23 = b23 * b23;
    const double sb31 = b31 * b31, sb32 = b32 * b32, sb33 = b33 * b33;
    const double b1 = sb11 + sb12 + sb13, b2 = sb21 + sb22 + sb23, b3 = sb31 + sb32 + sb33;
    const double bx = b11 * b31 + b12 * b32 + b13 * b33, by = b21 * b31 + b22 * b32 + b23 * b33;
    for (int k = 0; k < DLT_NB; k++) row[k] = 0.0;
    switch (type) {
    case JAICOV_DLT_FIXED_PRINCIPAL_POINT_X:
    case JAICOV_DLT_FIXED_PRINCIPAL_POINT_Y: {       // x0 (y0) = bx / b3 (by / b3)
        const bool isx = type == JAICOV_DLT_FIXED_PRINCIPAL_POINT_X;
        const double p1 = isx ? b11 : b21, p2 = isx ? b12 : b22, p3 = isx ? b13 : b23;
        const int o = isx ? 0 : 4;
        row[o + 0] = b31 / b3;
        row[o + 1] = b32 / b3;
        row[o + 2] = b33 / b3;
        row[8] = -(2.0 * b31 * (p2 * b32 + p3 * b33) + p1 * (sb31 - sb32 - sb33)) / b3 / b3;
        row[9] = -(2.0 * b32 * (p1 * b31 + p3 * b33) + p2 * (sb32 - sb31 - sb33)) / b3 / b3;
        row[10] = -(2.0 * b33 * (p1 * b31 + p2 * b32) + p3 * (sb33 - sb32 - sb31)) / b3 / b3;
        *w = isx ? x0 - bx / b3 : y0 - by / b3;
        break;
    }
    case JAICOV_DLT_FIXED_PRINCIPLE_DISTANCE_X:
    case JAICOV_DLT_FIXED_PRINCIPLE_DISTANCE_Y: {    // c^2 = bP / b3 - (bp / b3)^2
        const bool isx = type == JAICOV_DLT_FIXED_PRINCIPLE_DISTANCE_X;
        const double p1 = isx ? b11 : b21, p2 = isx ? b12 : b22, p3 = isx ? b13 : b23;
        const double bP = isx ? b1 : b2, bp = isx ? bx : by;
        const int o = isx ? 0 : 4;
        row[o + 0] = 2.0 * (p1 * (sb32 + sb33) - b31 * (p2 * b32 + p3 * b33)) / b3 / b3;
        row[o + 1] = 2.0 * (p2 * (sb31 + sb33) - b32 * (p1 * b31 + p3 * b33)) / b3 / b3;
        row[o + 2] = 2.0 * (p3 * (sb31 + sb32) - b33 * (p1 * b31 + p2 * b32)) / b3 / b3;
        row[8] = 4.0 * (b31 * bp * bp - 0.5 * b3 * (b31 * bP + bp * p1)) / (b3 * b3 * b3);
        row[9] = 4.0 * (b32 * bp * bp - 0.5 * b3 * (b32 * bP + bp * p2)) / (b3 * b3 * b3);
        row[10] = 4.0 * (b33 * bp * bp - 0.5 * b3 * (b33 * bP + bp * p3)) / (b3 * b3 * b3);
        *w = c * c - bP / b3 + bp * bp / b3 / b3;
        break;
    }
    case JAICOV_DLT_IDENTICAL_PRINCIPLE_DISTANCE:    // cx^2 = cy^2
        row[0] = 2.0 * (b11 * sb32 - b12 * b31 * b32 + b11 * sb33 - b13 * b31 * b33);
        row[1] = 2.0 * (b12 * sb31 - b11 * b32 * b31 + b12 * sb33 - b13 * b32 * b33);
        row[2] = 2.0 * (b13 * sb31 - b11 * b33 * b31 + b13 * sb32 - b12 * b33 * b32);
        row[4] = -2.0 * (b21 * sb32 - b22 * b31 * b32 + b21 * sb33 - b23 * b31 * b33);
        row[5] = -2.0 * (b22 * sb31 - b21 * b32 * b31 + b22 * sb33 - b23 * b32 * b33);
        row[6] = -2.0 * (b23 * sb31 - b21 * b33 * b31 + b23 * sb32 - b22 * b33 * b32);
        row[8] = 2.0 * (b31 * sb12 - b11 * b32 * b12 + b31 * sb13 - b11 * b33 * b13 - b31 * sb22 + b21 * b32 * b22 - b31 * sb23 + b21 * b33 * b23);
        row[9] = 2.0 * (b32 * sb11 - b12 * b31 * b11 + b32 * sb13 - b12 * b33 * b13 - b32 * sb21 + b22 * b31 * b21 - b32 * sb23 + b22 * b33 * b23);
        row[10] = 2.0 * (b33 * sb11 - b13 * b31 * b11 + b33 * sb12 - b13 * b32 * b12 - b33 * sb21 + b23 * b31 * b21 - b33 * sb22 + b23 * b32 * b22);
        *w = -b3 * (b1 - b2) + bx * bx - by * by;
        break;
    case JAICOV_DLT_ROTATION_WITHOUT_SHEAR:          // the rows of R orthogonal
        row[0] = -b21 * sb32 + b22 * b31 * b32 - b21 * sb33 + b23 * b31 * b33;
        row[1] = -b22 * sb31 + b21 * b32 * b31 - b22 * sb33 + b23 * b32 * b33;
        row[2] = -b23 * sb31 + b21 * b33 * b31 - b23 * sb32 + b22 * b33 * b32;
        row[4] = -b11 * sb32 + b12 * b31 * b32 - b11 * sb33 + b13 * b31 * b33;
        row[5] = -b12 * sb31 + b11 * b32 * b31 - b12 * sb33 + b13 * b32 * b33;
        row[6] = -b13 * sb31 + b11 * b33 * b31 - b13 * sb32 + b12 * b33 * b32;
        row[8] = b11 * b22 * b32 + b12 * b21 * b32 - 2.0 * b12 * b22 * b31 + b11 * b23 * b33 + b13 * b21 * b33 - 2.0 * b13 * b23 * b31;
        row[9] = b11 * b22 * b31 - 2.0 * b11 * b21 * b32 + b12 * b21 * b31 + b12 * b23 * b33 + b13 * b22 * b33 - 2.0 * b13 * b23 * b32;
        row[10] = b11 * b23 * b31 - 2.0 * b11 * b21 * b33 + b13 * b21 * b31 - 2.0 * b12 * b22 * b33 + b12 * b23 * b32 + b13 * b22 * b32;
        *w = b3 * (b11 * b21 + b12 * b22 + b13 * b23) - bx * by;
        break;
    }
}

// DT:185-267 on lane 0: b (scaled) -> the 20 output values.  Returns false when the projection centre's LU hits a zero pivot.
__device__ bool dlt_expand(const double *bs, double scale, double x0_io, double y0_io, double c_io, const uint8_t *fixed, double *o) {
    double b[DLT_NB];
    for (int k = 0; k < DLT_NB; k++) b[k] = (k == 3 || k == 7) ? bs[k] : bs[k] / scale;
    const double b11 = b[0], b12 = b[1], b13 = b[2], b14 = b[3], b21 = b[4], b22 = b[5], b23 = b[6], b24 = b[7];
    const double b31 = b[8], b32 = b[9], b33 = b[10];
    const double bb = b31 * b31 + b32 * b32 + b33 * b33;
    const double x0 = (b11 * b31 + b12 * b32 + b13 * b33) / bb;
    const double y0 = (b21 * b31 + b22 * b32 + b23 * b33) / bb;
    const double cx = sqrt((b11 * b11 + b12 * b12 + b13 * b13) / bb - x0 * x0);
    const double cy = sqrt((b21 * b21 + b22 * b22 + b23 * b23) / bb - y0 * y0);
    const double sb = sqrt(bb);
    double r11 = -(x0 * b31 - b11) / sb / cx, r12 = -(y0 * b31 - b21) / sb / cy, r13 = -b31 / sb;
    double r21 = -(x0 * b32 - b12) / sb / cx, r22 = -(y0 * b32 - b22) / sb / cy, r23 = -b32 / sb;
    double r31 = -(x0 * b33 - b13) / sb / cx, r32 = -(y0 * b33 - b23) / sb / cy, r33 = -b33 / sb;
    const double det = r11 * r22 * r33 + r12 * r23 * r31 + r13 * r21 * r32 - r13 * r22 * r31 - r11 * r23 * r32 - r12 * r21 * r33;
    if (det < 0) {
        r11 = -r11; r12 = -r12; r13 = -r13;
        r21 = -r21; r22 = -r22; r23 = -r23;
        r31 = -r31; r32 = -r32; r33 = -r33;
    }
    // F t = (-b14, -b24, -1): dgetf2 + dgetrs (LU with partial pivoting, unit lower L)
    double A[3][3] = {{b11, b12, b13}, {b21, b22, b23}, {b31, b32, b33}};
    double f[3] = {-b14, -b24, -1.0};
    int piv[3];
    for (int j = 0; j < 3; j++) {
        int p = j;
        double amax = fabs(A[j][j]);
        for (int i = j + 1; i < 3; i++)
            if (fabs(A[i][j]) > amax) { p = i; amax = fabs(A[i][j]); }
        piv[j] = p;
        if (A[p][j] == 0.0) return false;
        if (p != j)
            for (int k = 0; k < 3; k++) { const double t = A[j][k]; A[j][k] = A[p][k]; A[p][k] = t; }
        if (fabs(A[j][j]) >= DBL_MIN) {
            const double r = 1.0 / A[j][j];
            for (int i = j + 1; i < 3; i++) A[i][j] *= r;
        } else {
            for (int i = j + 1; i < 3; i++) A[i][j] /= A[j][j];
        }
        for (int k = j + 1; k < 3; k++)
            if (A[j][k] != 0.0) {
                const double temp = -1.0 * A[j][k];
                for (int i = j + 1; i < 3; i++) A[i][k] = A[i][k] + A[i][j] * temp;
            }
    }
    for (int j = 0; j < 3; j++)
        if (piv[j] != j) { const double t = f[j]; f[j] = f[piv[j]]; f[piv[j]] = t; }
    for (int k = 0; k < 3; k++)
        if (f[k] != 0.0)
            for (int i = k + 1; i < 3; i++) f[i] = f[i] - f[k] * A[i][k];
    for (int k = 2; k >= 0; k--)
        if (f[k] != 0.0) {
            f[k] = f[k] / A[k][k];
            for (int i = 0; i < k; i++) f[i] = f[i] - f[k] * A[i][k];
        }
    for (int k = 0; k < DLT_NB; k++) o[k] = b[k];
    o[11] = fixed[0] ? x0_io : x0;              // Q2: a fixed value is the camera's own
    o[12] = fixed[1] ? y0_io : y0;
    o[13] = fixed[2] ? c_io : 0.5 * (cx + cy);
    o[14] = f[0]; o[15] = f[1]; o[16] = f[2];
    o[17] = atan2(-r23, r33);
    o[18] = asin(r13);
    o[19] = atan2(-r12, r11);
    return true;
}

__global__ __launch_bounds__(64) void dlt_adjust_kernel(const int32_t *__restrict__ obs_begin, const double *__restrict__ xy,
                                                        const double *__restrict__ xyz, const double *__restrict__ io,
                                                        const uint8_t *__restrict__ io_fixed, DltRestrictions rs, int max_iter,
                                                        double *__restrict__ out, int32_t *__restrict__ status, int32_t *__restrict__ solves) {
    __shared__ double sx[DLT_CHUNK], sy[DLT_CHUNK], sX[DLT_CHUNK], sY[DLT_CHUNK], sZ[DLT_CHUNK];
    __shared__ double N11[DLT_NB * (DLT_NB + 1) / 2];
    __shared__ double M[DLT_MAX_ORDER * (DLT_MAX_ORDER + 1) / 2];
    __shared__ double rhs[DLT_MAX_ORDER], V[DLT_MAX_ORDER], bv[DLT_NB], sums[2];
    __shared__ int ipiv[DLT_MAX_ORDER];
    __shared__ int ctl[2];
    const int g = blockIdx.x, lane = threadIdx.x;
    const long o0 = obs_begin[g];
    const int m = obs_begin[g + 1] - obs_begin[g];
    double *og = out + (long)JAICOV_DLT_OUT_PER_IMAGE * g;
    if (m < 6) {                                   // DT:96-104
        if (lane < JAICOV_DLT_OUT_PER_IMAGE) og[lane] = NAN;
        if (lane == 0) { status[g] = JAICOV_DLT_TOO_FEW_POINTS; if (solves) solves[g] = 0; }
        return;
    }
    // observations c0 .. c0 + nc - 1 into LDS; `scaled`: object coordinates enter as X / scale (DT:339)
    auto stage = [&](int c0, int nc, double scale, bool scaled) {
        __syncthreads();
        for (int t = lane; t < nc; t += 64) {
            const long q = o0 + c0 + t;
            sx[t] = xy[2 * q]; sy[t] = xy[2 * q + 1];
            const double X = xyz[3 * q], Y = xyz[3 * q + 1], Z = xyz[3 * q + 2];
            sX[t] = scaled ? X / scale : X; sY[t] = scaled ? Y / scale : Y; sZ[t] = scaled ? Z / scale : Z;
        }
        __syncthreads();
    };

    // scale (DT:73-106), sums in observation order
    double acc = 0.0;
    for (int c0 = 0; c0 < m; c0 += DLT_CHUNK) {
        const int nc = min(DLT_CHUNK, m - c0);
        stage(c0, nc, 1.0, false);
        if (lane == 0) for (int t = 0; t < nc; t++) acc += sX[t] * sX[t] + sY[t] * sY[t] + sZ[t] * sZ[t];
        else if (lane == 1) for (int t = 0; t < nc; t++) acc += sx[t] * sx[t] + sy[t] * sy[t];
    }
    if (lane < 2) sums[lane] = acc;
    __syncthreads();
    const double scale = sums[1] > 0 ? sqrt(sums[0] / sums[1]) : 1.0;

    // N = A'A (upper, 66 entries), once: lane l owns entry l, lanes 0 and 1 also 64 and 65
    int ei[2], ej[2];
    for (int s = 0; s < 2; s++) {
        const int e = lane + 64 * s;
        int j = 0;
        while ((j + 1) * (j + 2) / 2 <= e) j++;
        ej[s] = j; ei[s] = e - j * (j + 1) / 2;
    }
    const bool two = lane + 64 < DLT_NB * (DLT_NB + 1) / 2;
    double n0 = 0.0, n1 = 0.0;
    for (int c0 = 0; c0 < m; c0 += DLT_CHUNK) {
        const int nc = min(DLT_CHUNK, m - c0);
        stage(c0, nc, scale, true);
        for (int t = 0; t < nc; t++) {
            double ai0, ai1, aj0, aj1;
            dlt_a(ei[0], sx[t], sy[t], sX[t], sY[t], sZ[t], ai0, ai1);
            dlt_a(ej[0], sx[t], sy[t], sX[t], sY[t], sZ[t], aj0, aj1);
            n0 += ai0 * aj0;
            n0 += ai1 * aj1;
        }
        if (two)
            for (int t = 0; t < nc; t++) {
                double ai0, ai1, aj0, aj1;
                dlt_a(ei[1], sx[t], sy[t], sX[t], sY[t], sZ[t], ai0, ai1);
                dlt_a(ej[1], sx[t], sy[t], sX[t], sY[t], sZ[t], aj0, aj1);
                n1 += ai0 * aj0;
                n1 += ai1 * aj1;
            }
    }
    N11[lane] = n0;
    if (two) N11[lane + 64] = n1;
    if (lane < DLT_NB) bv[lane] = 0.0;             // DT:280-303: every unknown starts at 0
    const bool resident = m <= DLT_CHUNK;          // the last staged chunk is the whole image

    const double x0_io = io[3L * g], y0_io = io[3L * g + 1], c_io = io[3L * g + 2];
    uint8_t fixed[3] = {0, 0, 0};
    if (io_fixed) for (int k = 0; k < 3; k++) fixed[k] = io_fixed[3L * g + k];
    const double EPS = ldexp(1.0, -53), SQRT_EPS = sqrt(EPS);     // Constant.EPS (Constant.java:68-75)
    const int nr = rs.n;
    // loop state, meaningful on lane 0 (DT:107-113)
    int runs = max_iter - 1, nsolve = 0, st = JAICOV_DLT_CONVERGED;
    bool isEstimated = max_iter == 0, include = false, isConverge = true;
    for (;;) {
        __syncthreads();
        // n = A'w at the current b (DPF:325-333), lanes 0..10
        double b[DLT_NB];
        for (int k = 0; k < DLT_NB; k++) b[k] = bv[k];
        double na = 0.0;
        for (int c0 = 0; c0 < m; c0 += DLT_CHUNK) {
            const int nc = min(DLT_CHUNK, m - c0);
            if (!resident) stage(c0, nc, scale, true);
            if (lane < DLT_NB)
                for (int t = 0; t < nc; t++) {
                    const double x = sx[t], y = sy[t], X = sX[t], Y = sY[t], Z = sZ[t];
                    const double w0 = x - (X * b[0] + Y * b[1] + Z * b[2] + b[3] - x * X * b[8] - x * Y * b[9] - x * Z * b[10]);
                    const double w1 = y - (X * b[4] + Y * b[5] + Z * b[6] + b[7] - y * X * b[8] - y * Y * b[9] - y * Z * b[10]);
                    double a0, a1;
                    dlt_a(lane, x, y, X, Y, Z, a0, a1);
                    na += a0 * w0;
                    na += a1 * w1;
                }
        }
        if (lane < DLT_NB) rhs[lane] = na;
        __syncthreads();
        if (lane == 0) {
            const bool ecm = isEstimated || nr == 0;                // estimateCompleteModel, DT:130
            const int ord = include ? DLT_NB + nr : DLT_NB;
            for (int q = 0; q < DLT_NB * (DLT_NB + 1) / 2; q++) M[q] = N11[q];
            for (int q = DLT_NB * (DLT_NB + 1) / 2; q < ord * (ord + 1) / 2; q++) M[q] = 0.0;
            if (include)
                for (int r = 0; r < nr; r++) {
                    double row[DLT_NB], w = 0.0;
                    dlt_restriction(rs.id[r], b, x0_io, y0_io, c_io, row, &w);
                    for (int k = 0; k < DLT_NB; k++) M[DLT_PK(k, DLT_NB + r)] = row[k];
                    rhs[DLT_NB + r] = w;
                }
            for (int q = 0; q < ord; q++) {                         // DT:345-348
                const double v = M[DLT_PK(q, q)];
                V[q] = v > EPS ? 1.0 / sqrt(v) : 1.0;
            }
            for (int r = 0; r < ord; r++) {                         // NES:82-91
                rhs[r] = V[r] * rhs[r];
                for (int q = r; q < ord; q++) M[DLT_PK(r, q)] = V[q] * M[DLT_PK(r, q)] * V[r];
            }
            nsolve++;
            bool go = false;
            if (dlt_dsptrf(ord, M, ipiv) != 0) {
                st = JAICOV_DLT_SINGULAR;
            } else {
                dlt_dsptrs(ord, M, ipiv, rhs);
                double maxAbsDx = 0.0;
                bool finite = true;
                for (int k = 0; k < DLT_NB; k++) {                  // DT:171-183 after NES:82-91 on dx
                    const double d = V[k] * rhs[k];
                    if (!isfinite(d)) finite = false;
                    maxAbsDx = fmax(fabs(d), maxAbsDx);
                    bv[k] = b[k] + d;
                }
                include = true;
                if (!finite) {
                    st = JAICOV_DLT_NOT_FINITE;
                } else {
                    if (maxAbsDx <= SQRT_EPS && runs > 0) {
                        isEstimated = true;
                    } else if (runs-- <= 1) {
                        if (ecm) isConverge = false;
                        isEstimated = true;
                    }
                    go = !ecm;
                    if (!go) st = isConverge ? JAICOV_DLT_CONVERGED : JAICOV_DLT_NOT_CONVERGED;
                }
            }
            ctl[0] = go;
            ctl[1] = st;
        }
        __syncthreads();
        if (!ctl[0]) break;
    }
    if (lane == 0) {
        st = ctl[1];
        double o[JAICOV_DLT_OUT_PER_IMAGE];
        if (st == JAICOV_DLT_CONVERGED || st == JAICOV_DLT_NOT_CONVERGED) {
            if (!dlt_expand(bv, scale, x0_io, y0_io, c_io, fixed, o)) st = JAICOV_DLT_SINGULAR;
        }
        if (st != JAICOV_DLT_CONVERGED && st != JAICOV_DLT_NOT_CONVERGED)
            for (int k = 0; k < JAICOV_DLT_OUT_PER_IMAGE; k++) o[k] = NAN;       // Q3
        for (int k = 0; k < JAICOV_DLT_OUT_PER_IMAGE; k++) og[k] = o[k];
        status[g] = st;
        if (solves) solves[g] = nsolve;
    }
}

}  // namespace
}  // namespace jaicov

using namespace jaicov;

extern "C" int jaicov_dlt_adjust(int32_t n_images, const int32_t *obs_begin, const double *xy, const double *xyz, const double *io,
                                 const uint8_t *io_fixed, const int32_t *restrictions, int32_t n_restrictions, int32_t max_iterations,
                                 double *out, int32_t *status, int32_t *solves, double *ms_out) {
    // argument checks, host only
    if (n_images < 0 || n_restrictions < 0 || max_iterations < 0 || !obs_begin) return JAICOV_ERR_BAD_ARGUMENT;
    if (n_restrictions > 0 && !restrictions) return JAICOV_ERR_BAD_ARGUMENT;
    if (n_images > 0 && (!io || !out || !status)) return JAICOV_ERR_BAD_ARGUMENT;
    if (!ranges_ok(n_images, obs_begin)) return JAICOV_ERR_BAD_ARGUMENT;
    const long n_obs = obs_begin[n_images];
    if (n_obs > 0 && (!xy || !xyz)) return JAICOV_ERR_BAD_ARGUMENT;
    // DT:269-278: duplicates dropped in first-seen order, IDENTICAL dropped when both FIXED_PRINCIPLE_DISTANCE_* are present
    bool seen[DLT_TYPES] = {false, false, false, false, false, false};
    int order[DLT_TYPES], nu = 0;
    for (int32_t r = 0; r < n_restrictions; r++) {
        const int32_t id = restrictions[r];
        if (id < 0 || id >= DLT_TYPES) return JAICOV_ERR_BAD_ARGUMENT;
        if (!seen[id]) { seen[id] = true; order[nu++] = id; }
    }
    DltRestrictions rs;
    rs.n = 0;
    const bool drop_identical = seen[JAICOV_DLT_FIXED_PRINCIPLE_DISTANCE_X] && seen[JAICOV_DLT_FIXED_PRINCIPLE_DISTANCE_Y];
    for (int r = 0; r < nu; r++)
        if (!(drop_identical && order[r] == JAICOV_DLT_IDENTICAL_PRINCIPLE_DISTANCE)) rs.id[rs.n++] = order[r];
    for (int r = rs.n; r < DLT_MAX_RESTR; r++) rs.id[r] = 0;

    if (!device_is_gfx950()) return JAICOV_ERR_NO_DEVICE;
    if (ms_out) *ms_out = 0.0;
    if (n_images == 0) return JAICOV_OK;

    BatchCall call;
    const size_t ni = (size_t)n_images, no = (size_t)n_obs;
    const int32_t *d_begin = call.in(obs_begin, ni + 1);
    const double *d_xy = call.in(xy, 2 * no), *d_xyz = call.in(xyz, 3 * no), *d_io = call.in(io, 3 * ni);
    const uint8_t *d_fixed = call.in(io_fixed, 3 * ni);
    double *d_out = call.alloc<double>(JAICOV_DLT_OUT_PER_IMAGE * ni);
    int32_t *d_status = call.alloc<int32_t>(ni), *d_solves = solves ? call.alloc<int32_t>(ni) : nullptr;
    call.run([&](hipStream_t s) {
        hipLaunchKernelGGL(dlt_adjust_kernel, dim3(n_images), dim3(64), 0, s, d_begin, d_xy, d_xyz, d_io, d_fixed, rs, (int)max_iterations,
                           d_out, d_status, d_solves);
    });
    call.out(out, d_out, JAICOV_DLT_OUT_PER_IMAGE * ni);
    call.out(status, d_status, ni);
    call.out(solves, d_solves, ni);
    return call.finish(ms_out);
}
