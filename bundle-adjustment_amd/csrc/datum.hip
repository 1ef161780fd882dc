// Baarda's S-transformation of the cofactor matrix on the device (include/jaicov_datum.h).
//
// The cofactor matrix Q (order n, border rows 0 .. d-1, lower part of a row-major square) is read twice and written once:
//   1. sym_y_tile_kernel + sym_y_reduce_kernel (symtile.h, shared with precision.hip): Y = Q B'' over the lower triangle, rows and
//      columns [d, n).  Each 128 x 128 tile serves its rows and, transposed, its columns; the partial sums go to a [block row][slot]
//      table and are added in slot order, so two runs give the same bits.
//   2. the d x d algebra on the host: G^ (the unknowns x border block, n d doubles), C = (B' G^)^-1, Z = G^ C, W = B' Y,
//      Y~ = Y - Z W / 2.
//   3. datum_update_kernel: Q' = Q - Z Y~' - Y~ Z' on the unknowns block, Z in the border block, 0 in the border x border block,
//      one read and one write of the lower triangle.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/jaicov_datum.h"
#include "datum.h"
#include "qview.h"
#include "small_inverse.h"
#include "status.h"
#include "symtile.h"

namespace jaicov {

void datum_state_invalidate(DatumState *s) {
    if (s) s->valid = false;
}

// Q'[i][j], j <= i < n: 0 (i < d), Z[i][j] (j < d <= i), Q[i][j] - sum_a (Z[i][a] Y~[j][a] + Y~[i][a] Z[j][a]) otherwise.
// ZY: [row][Z (D) | Y~ (D)].  One workgroup: 256 columns x 32 rows; the column operands stay in registers.
template <int D>
__global__ __launch_bounds__(256) void datum_update_kernel(double *__restrict__ Q, long ld, int n, int d, const double *__restrict__ ZY) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i0 = blockIdx.y * 32;
    if (blockIdx.x * 256 > i0 + 31) return;          // the whole workgroup lies above the diagonal
    double zj[D], yj[D];
#pragma unroll
    for (int a = 0; a < D; a++) {
        zj[a] = j < n ? ZY[(size_t)j * 2 * D + a] : 0.0;
        yj[a] = j < n ? ZY[(size_t)j * 2 * D + D + a] : 0.0;
    }
    for (int r = 0; r < 32; r++) {
        const int i = i0 + r;
        if (i >= n) break;
        if (j > i || j >= n) continue;
        const double *zyi = ZY + (size_t)i * 2 * D;
        double *q = Q + (long)i * ld + j;
        if (i < d) {
            *q = 0.0;
        } else if (j < d) {
            *q = zyi[j];
        } else {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < D; a++) {
                s = fma(zyi[a], yj[a], s);
                s = fma(zyi[D + a], zj[a], s);
            }
            *q = *q - s;
        }
    }
}

template <int D>
static hipError_t launch_update(hipStream_t st, double *Q, long ld, int n, int d, const double *ZY) {
    hipLaunchKernelGGL(datum_update_kernel<D>, dim3((n + 255) / 256, (n + 31) / 32), dim3(256), 0, st, Q, ld, n, d, ZY);
    return hipGetLastError();
}

static hipError_t launch_y_d(int D, hipStream_t st, const double *Q, long ld, int n, const double *Bt, int np, int nbk, double *P, double *Y) {
    switch (D) {
    case 1: return launch_sym_y<1>(st, Q, ld, n, D, Bt, np, nbk, P, Y);
    case 2: return launch_sym_y<2>(st, Q, ld, n, D, Bt, np, nbk, P, Y);
    case 3: return launch_sym_y<3>(st, Q, ld, n, D, Bt, np, nbk, P, Y);
    case 4: return launch_sym_y<4>(st, Q, ld, n, D, Bt, np, nbk, P, Y);
    case 5: return launch_sym_y<5>(st, Q, ld, n, D, Bt, np, nbk, P, Y);
    case 6: return launch_sym_y<6>(st, Q, ld, n, D, Bt, np, nbk, P, Y);
    default: return launch_sym_y<7>(st, Q, ld, n, D, Bt, np, nbk, P, Y);
    }
}

static hipError_t launch_update_d(int D, hipStream_t st, double *Q, long ld, int n, const double *ZY) {
    switch (D) {
    case 1: return launch_update<1>(st, Q, ld, n, D, ZY);
    case 2: return launch_update<2>(st, Q, ld, n, D, ZY);
    case 3: return launch_update<3>(st, Q, ld, n, D, ZY);
    case 4: return launch_update<4>(st, Q, ld, n, D, ZY);
    case 5: return launch_update<5>(st, Q, ld, n, D, ZY);
    case 6: return launch_update<6>(st, Q, ld, n, D, ZY);
    default: return launch_update<7>(st, Q, ld, n, D, ZY);
    }
}

}  // namespace jaicov

using namespace jaicov;

extern "C" int jaicov_datum_transform(jaicov_engine *e, const uint8_t *point_datum, int32_t n_points) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    if (v.d == 0) FAIL(*v.err, JAICOV_ERR_UNSUPPORTED, "datum transformation: the network has no datum defect (d = 0)");
    TRY(q_guard(v, "datum transformation on a sharded engine"));
    if (!point_datum || n_points != v.n_points) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "point_datum must hold one flag per object point");
    const int n = v.order, d = v.d, nbk = (n + 127) / 128, np = nbk * 128;
    std::vector<double> B;
    int rc = engine_datum_rows(e, point_datum, B, np);
    if (rc) return rc;
    HIPE(*v.err, hipSetDevice(v.device));
    // G^: the unknowns x border block (rows d .. n-1, columns 0 .. d-1)
    std::vector<double> G((size_t)n * d, 0.0);
    HIPE(*v.err, hipMemcpy2DAsync(G.data() + (size_t)d * d, d * sizeof(double), v.Q + (long)d * v.ld, v.ld * sizeof(double),
                             d * sizeof(double), n - d, hipMemcpyDeviceToHost, v.stream));
    HIPE(*v.err, hipStreamSynchronize(v.stream));
    // C = (B' G^)^-1, Z = G^ C
    double M[49], Cm[49];
    for (int a = 0; a < d; a++)
        for (int b = 0; b < d; b++) {
            double s = 0.0;
            for (int i = d; i < n; i++) s += B[(size_t)a * np + i] * G[(size_t)i * d + b];
            M[a * d + b] = s;
        }
    if (!datum_small_inverse(d, M, Cm)) FAIL(*v.err, JAICOV_ERR_SINGULAR, "the new datum points do not fix the frame (B' G^ is singular)");
    std::vector<double> Z((size_t)n * d, 0.0);
    for (int i = d; i < n; i++)
        for (int a = 0; a < d; a++) {
            double s = 0.0;
            for (int b = 0; b < d; b++) s += G[(size_t)i * d + b] * Cm[b * d + a];
            Z[(size_t)i * d + a] = s;
        }
    // work buffers, kept with the engine
    DatumState *st = q_state(v.slot->datum);
    HIPE(*v.err, st->work.reserve((size_t)d * np * 4 + (size_t)nbk * nbk * 128 * d));
    double *dB = st->work.get(), *dY = dB + (size_t)d * np, *dZY = dY + (size_t)d * np, *dP = dZY + (size_t)2 * d * np;
    HIPE(*v.err, hipMemcpyAsync(dB, B.data(), (size_t)d * np * sizeof(double), hipMemcpyHostToDevice, v.stream));
    HIPE(*v.err, launch_y_d(d, v.stream, v.Q, v.ld, n, dB, np, nbk, dP, dY));
    std::vector<double> Y((size_t)np * d);
    TRY(q_download(v, {{Y.data(), dY, Y.size() * sizeof(double)}}));
    // W = B' Y (symmetric: its two triangles averaged), Y~ = Y - Z W / 2
    double W[49];
    for (int a = 0; a < d; a++)
        for (int b = 0; b < d; b++) {
            double s = 0.0;
            for (int i = d; i < n; i++) s += B[(size_t)a * np + i] * Y[(size_t)i * d + b];
            W[a * d + b] = s;
        }
    for (int a = 0; a < d; a++)
        for (int b = 0; b < a; b++) W[a * d + b] = W[b * d + a] = 0.5 * (W[a * d + b] + W[b * d + a]);
    std::vector<double> ZY((size_t)np * 2 * d, 0.0);
    for (int i = d; i < n; i++)
        for (int a = 0; a < d; a++) {
            double s = 0.0;
            for (int b = 0; b < d; b++) s += Z[(size_t)i * d + b] * W[b * d + a];
            ZY[(size_t)i * 2 * d + a] = Z[(size_t)i * d + a];
            ZY[(size_t)i * 2 * d + d + a] = Y[(size_t)i * d + a] - 0.5 * s;
        }
    HIPE(*v.err, hipMemcpyAsync(dZY, ZY.data(), ZY.size() * sizeof(double), hipMemcpyHostToDevice, v.stream));
    st->valid = false;      // from here on Q changes: the S of an earlier transform no longer applies to it
    HIPE(*v.err, launch_update_d(d, v.stream, v.Q, v.ld, n, dZY));
    HIPE(*v.err, hipStreamSynchronize(v.stream));
    // S = I - Z B' for jaicov_datum_apply
    st->order = n;
    st->d = d;
    st->Z.swap(Z);
    st->B.assign((size_t)d * n, 0.0);
    for (int a = 0; a < d; a++) std::copy(B.begin() + (size_t)a * np, B.begin() + (size_t)a * np + n, st->B.begin() + (size_t)a * n);
    st->valid = true;
    return JAICOV_OK;
}

extern "C" int jaicov_datum_apply(jaicov_engine *e, const double *x, double *out, int32_t n) {
    if (!e || !x || !out) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    const DatumState *st = v.slot->datum.get();
    if (!st || !st->valid) FAIL(*v.err, JAICOV_ERR_BAD_STATE, "no datum transformation since the last inverting solve");
    if (n != st->order) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "n must be the order of the transformed cofactor matrix");
    const int d = st->d;
    double t[7];
    for (int a = 0; a < d; a++) {
        double s = 0.0;
        for (int i = d; i < n; i++) s += st->B[(size_t)a * n + i] * x[i];
        t[a] = s;
    }
    for (int i = 0; i < d; i++) out[i] = 0.0;
    for (int i = d; i < n; i++) {
        double s = 0.0;
        for (int a = 0; a < d; a++) s += st->Z[(size_t)i * d + a] * t[a];
        out[i] = x[i] - s;
    }
    return JAICOV_OK;
}
