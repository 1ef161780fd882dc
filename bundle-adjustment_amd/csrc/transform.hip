// Coordinate transformation into the frame of a reference image with covariance propagation (include/jaicov_transform.h):
// CoordinateTransformationExteriorOrientation.transform (CTEO) on the device, next to the cofactor matrix.  gfx950 only.
//
//   xform_rows_kernel   one lane per transformed point: X_T = X0_T + R_T R_S' (X - X0_S), its 3 x 15 Jacobian and the 15 columns
//   xform_cov_kernel    C = sigma2 J Q J', one workgroup per pair of row chunks (lower triangle), straight into the packed output
//   xform_sub_kernel    C[rows, rows] gathered from the packed output
//   xform_blocks_kernel every 3 x 3 diagonal block of the packed output
//
// The product.  Rows are cut into chunks of at most XF_TP transformed points of ONE (ref, src) pair, in the caller's row order
// (rows are enumerated pair-major, so a pair's points are contiguous).  The points of a chunk share their 12 exterior-orientation
// columns, so a chunk touches at most 3 XF_TP + 12 columns of Q.  For chunks A (rows) and B (columns) the workgroup stages
// Q[cols(A), cols(B)] in LDS (60 x 60), forms Z = J_A Q[cols(A), cols(B)] (15 terms per entry), overwrites the staging with Z and
// writes C[A, B] = sigma2 Z J_B' (15 terms per entry).  Q is the solver's lower-row-major square: an entry with row column < column
// column is read from the mirrored position, in a second pass whose lanes run along the row index so that those reads are
// coalesced as well.  No atomics: every output entry is one fixed-order sum, so two runs give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/jaicov_transform.h"
#include "qview.h"
#include "rotation.h"
#include "status.h"
#include "transform.h"

namespace jaicov {

constexpr int XF_TP = 16;                 // transformed points per chunk
constexpr int XF_PR = 3 * XF_TP;          // point rows / columns of a chunk (48)
constexpr int XF_NC = XF_PR + 12;         // + the 6 + 6 exterior-orientation columns (60)
constexpr int XF_NT = 256;                // threads per workgroup of the product
constexpr int XF_ZPT = (XF_PR * XF_NC + XF_NT - 1) / XF_NT;   // Z entries per thread (12)

// R(omega, phi, kappa) of the collinearity rows (rows.hip, PDF:125-135), row-major, and its derivatives by omega, phi, kappa
__device__ __forceinline__ void xf_rotation(const double *eo, double R[9], double dR[3][9]) {
    double so, co, sp, cp, sk, ck;
    sincos(eo[3], &so, &co);
    sincos(eo[4], &sp, &cp);
    sincos(eo[5], &sk, &ck);
    rotation_opk(so, co, sk, ck, sp, cp, R);
    // d/domega: the first row does not depend on omega; row 2' = -row 3, row 3' = row 2
    dR[0][0] = 0.0;   dR[0][1] = 0.0;   dR[0][2] = 0.0;
    dR[0][3] = -R[6]; dR[0][4] = -R[7]; dR[0][5] = -R[8];
    dR[0][6] = R[3];  dR[0][7] = R[4];  dR[0][8] = R[5];
    // d/dphi
    dR[1][0] = -sp * ck;      dR[1][1] = sp * sk;       dR[1][2] = cp;
    dR[1][3] = so * cp * ck;  dR[1][4] = -so * cp * sk; dR[1][5] = so * sp;
    dR[1][6] = -co * cp * ck; dR[1][7] = co * cp * sk;  dR[1][8] = -co * sp;
    // d/dkappa: column 1' = column 2, column 2' = -column 1, column 3' = 0
    for (int r = 0; r < 3; r++) { dR[2][3 * r] = R[3 * r + 1]; dR[2][3 * r + 1] = -R[3 * r]; dR[2][3 * r + 2] = 0.0; }
}

// tp[3t..3t+2] = (point, src image, ref image).  Columns per transformed point: 0-2 X, Y, Z of the point; 3-8 X0, Y0, Z0, omega,
// phi, kappa of src; 9-14 the same of ref.  A fixed parameter (or an exterior orientation of a src == ref row) gets column -1 and 0.
__global__ __launch_bounds__(256) void xform_rows_kernel(DevProblem p, const double *__restrict__ vals, const int32_t *__restrict__ tp, int nT,
                                                         double *__restrict__ xyz, double *__restrict__ Jv, int32_t *__restrict__ Jc) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nT) return;
    const int pt = tp[3 * t], src = tp[3 * t + 1], ref = tp[3 * t + 2];
    const int sp = 3 * pt, ss = slot_eo(p, src), sr = slot_eo(p, ref);
    double J[3][15];
    int col[15];
    for (int k = 0; k < 3; k++) col[k] = p.slot_col[sp + k];
    for (int k = 0; k < 6; k++) { col[3 + k] = p.slot_col[ss + k]; col[9 + k] = p.slot_col[sr + k]; }
    double X[3];
    if (src == ref) {           // CTEO:149-158: the point itself, identity on its columns
        for (int c = 0; c < 3; c++) {
            X[c] = vals[sp + c];
            for (int k = 0; k < 15; k++) J[c][k] = (k == c) ? 1.0 : 0.0;
        }
        for (int k = 3; k < 15; k++) col[k] = -1;
    } else {
        double eoS[6], eoT[6], RS[9], RT[9], dRS[3][9], dRT[3][9];
        for (int k = 0; k < 6; k++) { eoS[k] = vals[ss + k]; eoT[k] = vals[sr + k]; }
        xf_rotation(eoS, RS, dRS);
        xf_rotation(eoT, RT, dRT);
        const double d[3] = {vals[sp] - eoS[0], vals[sp + 1] - eoS[1], vals[sp + 2] - eoS[2]};
        double u[3], M[9];
        for (int i = 0; i < 3; i++) u[i] = RS[i] * d[0] + RS[3 + i] * d[1] + RS[6 + i] * d[2];          // u = R_S' d
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) M[3 * i + j] = RT[3 * i] * RS[3 * j] + RT[3 * i + 1] * RS[3 * j + 1] + RT[3 * i + 2] * RS[3 * j + 2];   // R_T R_S'
        for (int c = 0; c < 3; c++) {
            X[c] = eoT[c] + (RT[3 * c] * u[0] + RT[3 * c + 1] * u[1] + RT[3 * c + 2] * u[2]);
            for (int k = 0; k < 3; k++) {
                J[c][k] = M[3 * c + k];                     // dX_T / dX
                J[c][3 + k] = -M[3 * c + k];                // dX_T / dX0_S
                J[c][9 + k] = (c == k) ? 1.0 : 0.0;         // dX_T / dX0_T
            }
            for (int a = 0; a < 3; a++) {
                // dX_T / d(angle a of S) = R_T (dR_S/da)' d ;  dX_T / d(angle a of T) = (dR_T/da) u
                double w[3];
                for (int i = 0; i < 3; i++) w[i] = dRS[a][i] * d[0] + dRS[a][3 + i] * d[1] + dRS[a][6 + i] * d[2];
                J[c][6 + a] = RT[3 * c] * w[0] + RT[3 * c + 1] * w[1] + RT[3 * c + 2] * w[2];
                J[c][12 + a] = dRT[a][3 * c] * u[0] + dRT[a][3 * c + 1] * u[1] + dRT[a][3 * c + 2] * u[2];
            }
        }
    }
    for (int k = 0; k < 15; k++) {
        if (col[k] < 0) { col[k] = -1; for (int c = 0; c < 3; c++) J[c][k] = 0.0; }
        Jc[15 * (long)t + k] = col[k];
    }
    for (int c = 0; c < 3; c++) {
        xyz[3 * (long)t + c] = X[c];
        for (int k = 0; k < 15; k++) Jv[(3 * (long)t + c) * 15 + k] = J[c][k];
    }
}

// chunks[i] = (first transformed point, points).  One workgroup per tile (a, b), b <= a, of the chunk triangle.
__global__ __launch_bounds__(XF_NT) void xform_cov_kernel(const double *__restrict__ Q, long ld, const int2 *__restrict__ chunks, long tiles,
                                                          const double *__restrict__ Jv, const int32_t *__restrict__ Jc, double sigma2,
                                                          double *__restrict__ ap) {
    __shared__ double sQ[XF_PR * XF_NC > XF_NC * XF_NC ? XF_PR * XF_NC : XF_NC * XF_NC];   // Q[cols(A), cols(B)], then Z (48 x 60)
    __shared__ double sJA[XF_PR * 15], sJB[XF_PR * 15];
    __shared__ int colA[XF_NC], colB[XF_NC];
    const int tid = threadIdx.x;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        long a = (long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
        while (a * (a + 1) / 2 > t) a--;
        while ((a + 1) * (a + 2) / 2 <= t) a++;
        const long b = t - a * (a + 1) / 2;
        const int2 ca = chunks[a], cb = chunks[b];
        const int rA = 3 * ca.y, rB = 3 * cb.y;
        if (tid < XF_NC) {
            colA[tid] = tid < XF_PR ? (tid < rA ? Jc[15 * (long)(ca.x + tid / 3) + tid % 3] : -1) : Jc[15 * (long)ca.x + 3 + (tid - XF_PR)];
            colB[tid] = tid < XF_PR ? (tid < rB ? Jc[15 * (long)(cb.x + tid / 3) + tid % 3] : -1) : Jc[15 * (long)cb.x + 3 + (tid - XF_PR)];
        }
        for (int i = tid; i < XF_PR * 15; i += XF_NT) {
            sJA[i] = i < rA * 15 ? Jv[45 * (long)ca.x + i] : 0.0;
            sJB[i] = i < rB * 15 ? Jv[45 * (long)cb.x + i] : 0.0;
        }
        __syncthreads();
        // stage Q[cols(A), cols(B)]: lower entries along the column index, mirrored ones along the row index
        for (int i = tid; i < XF_NC * XF_NC; i += XF_NT) {
            const int r = i / XF_NC, c = i - r * XF_NC;
            const int qr = colA[r], qc = colB[c];
            if (qr < 0 || qc < 0) sQ[i] = 0.0;
            else if (qr >= qc) sQ[i] = Q[(long)qr * ld + qc];
        }
        for (int i = tid; i < XF_NC * XF_NC; i += XF_NT) {
            const int c = i / XF_NC, r = i - c * XF_NC;
            const int qr = colA[r], qc = colB[c];
            if (qr >= 0 && qc >= 0 && qr < qc) sQ[r * XF_NC + c] = Q[(long)qc * ld + qr];
        }
        __syncthreads();
        // Z = J_A Q[cols(A), cols(B)]: row r of chunk A has its 3 point columns at 3 (r / 3) .. + 2 and the EO columns at 48 .. 59
        double z[XF_ZPT];
#pragma unroll
        for (int m = 0; m < XF_ZPT; m++) {
            const int i = tid + m * XF_NT, r = i / XF_NC, c = i - r * XF_NC;
            double acc = 0.0;
            if (r < rA) {
                const double *j = sJA + 15 * r;
                const double *q = sQ + 3 * (r / 3) * XF_NC + c;
                acc = fma(j[0], q[0], acc);
                acc = fma(j[1], q[XF_NC], acc);
                acc = fma(j[2], q[2 * XF_NC], acc);
                const double *qe = sQ + XF_PR * XF_NC + c;
#pragma unroll
                for (int e = 0; e < 12; e++) acc = fma(j[3 + e], qe[e * XF_NC], acc);
            }
            z[m] = acc;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < XF_ZPT; m++) {
            const int i = tid + m * XF_NT;
            if (i < XF_PR * XF_NC) sQ[i] = z[m];
        }
        __syncthreads();
        // C[A, B] = sigma2 Z J_B', lower part only on the diagonal tile; packed 'U' column-major == lower row-major packed
        const long g0 = 3 * (long)ca.x, h0 = 3 * (long)cb.x;
        for (int i = tid; i < rA * rB; i += XF_NT) {
            const int r = i / rB, c = i - r * rB;
            const long gi = g0 + r, gj = h0 + c;
            if (gj > gi) continue;
            const double *zr = sQ + r * XF_NC, *j = sJB + 15 * c;
            const int pc = 3 * (c / 3);
            double acc = 0.0;
            acc = fma(zr[pc], j[0], acc);
            acc = fma(zr[pc + 1], j[1], acc);
            acc = fma(zr[pc + 2], j[2], acc);
#pragma unroll
            for (int e = 0; e < 12; e++) acc = fma(zr[XF_PR + e], j[3 + e], acc);
            ap[(size_t)gi * (gi + 1) / 2 + gj] = sigma2 * acc;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void xform_sub_kernel(const double *__restrict__ ap, const int32_t *__restrict__ rows, int k, double *__restrict__ out) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)k * k) return;
    const int a = (int)(t / k), b = (int)(t - (long)a * k);
    const long i = rows[a], j = rows[b];
    const long hi = i > j ? i : j, lo = i > j ? j : i;
    out[t] = ap[(size_t)hi * (hi + 1) / 2 + lo];
}

// out[9 t + 3 a + b] = C[3 t + a, 3 t + b]
__global__ __launch_bounds__(256) void xform_blocks_kernel(const double *__restrict__ ap, long nT, double *__restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 9 * nT) return;
    const long t = i / 9, a = (i - 9 * t) / 3, b = i - 9 * t - 3 * a;
    const long r = 3 * t + a, c = 3 * t + b;
    const long hi = r > c ? r : c, lo = r > c ? c : r;
    out[i] = ap[(size_t)hi * (hi + 1) / 2 + lo];
}

}  // namespace jaicov

using namespace jaicov;

static int xform_run_impl(const QView &v, XformState *s, double sigma2) {
    const DevProblem &p = *v.p;
    const int nT = s->nT;
    if (nT == 0) return JAICOV_OK;
    const size_t packed = (size_t)s->R * (s->R + 1) / 2;
    // chunks of at most XF_TP points of one pair, in row order
    std::vector<int2> chunks;
    for (int t = 0; t < nT;) {
        int n = 1;
        while (t + n < nT && n < XF_TP && s->ids[3 * (t + n) + 1] == s->ids[3 * t + 1] && s->ids[3 * (t + n) + 2] == s->ids[3 * t + 2])
            n++;
        chunks.push_back(make_int2(t, n));
        t += n;
    }
    s->n_chunks = (int)chunks.size();
    HIPE(*v.err, s->tp.reserve(3 * (size_t)nT));
    HIPE(*v.err, s->xyz.reserve(3 * (size_t)nT));
    HIPE(*v.err, s->Jv.reserve(45 * (size_t)nT));
    HIPE(*v.err, s->Jc.reserve(15 * (size_t)nT));
    HIPE(*v.err, s->chunks.reserve(chunks.size()));
    HIPE(*v.err, s->ap.reserve(packed));
    HIPE(*v.err, hipMemcpyAsync(s->tp.get(), s->ids.data(), 3 * (size_t)nT * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    HIPE(*v.err, hipMemcpyAsync(s->chunks.get(), chunks.data(), chunks.size() * sizeof(int2), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(xform_rows_kernel, dim3((nT + 255) / 256), dim3(256), 0, v.stream, p, v.d_vals, s->tp.get(), nT, s->xyz.get(), s->Jv.get(), s->Jc.get());
    HIPE(*v.err, hipGetLastError());
    const long nc = (long)chunks.size(), tiles = nc * (nc + 1) / 2;
    const unsigned grid = (unsigned)std::min<long>(tiles, 1L << 24);
    hipLaunchKernelGGL(xform_cov_kernel, dim3(grid), dim3(XF_NT), 0, v.stream, v.Q, v.ld, s->chunks.get(), tiles, s->Jv.get(), s->Jc.get(), sigma2, s->ap.get());
    HIPE(*v.err, hipGetLastError());
    HIPE(*v.err, hipStreamSynchronize(v.stream));
    return JAICOV_OK;
}

extern "C" int jaicov_xform_run(jaicov_engine *e, const int32_t *points, int32_t n_points, const int32_t *pair_ref, const int32_t *pair_src,
                                int32_t n_pairs, double sigma2, int32_t *n_transformed) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    if (!v.full_q)
        FAIL(*v.err, JAICOV_ERR_BAD_STATE, "no full cofactor matrix: solve with JAICOV_INVERT_FULL or JAICOV_INVERT_FULL_EXPANDED first");
    const DevProblem &p = *v.p;
    if (n_points < 0 || n_pairs < 0 || (n_points > 0 && !points) || (n_pairs > 0 && (!pair_ref || !pair_src)))
        FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "point / pair arrays missing or negative counts");
    if (!std::isfinite(sigma2)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "sigma2 must be finite");
    std::vector<uint8_t> seen(p.n_points, 0);
    for (int i = 0; i < n_points; i++) {
        if (points[i] < 0 || points[i] >= p.n_points) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "point index out of range");
        if (seen[points[i]]) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "duplicate point (the reference takes a Set)");
        seen[points[i]] = 1;
    }
    for (int k = 0; k < n_pairs; k++)
        if (pair_ref[k] < 0 || pair_ref[k] >= p.n_images || pair_src[k] < 0 || pair_src[k] >= p.n_images)
            FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "image index out of range");
    // which points each source image observes (CTEO:83 image.get(point) != null): CSR over the problem's image points
    std::vector<int32_t> ip_image(p.n_ip), ip_point(p.n_ip);
    const size_t ip_bytes = (size_t)p.n_ip * sizeof(int32_t);
    TRY(q_download(v, {{ip_image.data(), p.ip_image, ip_bytes}, {ip_point.data(), p.ip_point, ip_bytes}}));
    std::vector<int32_t> img_begin(p.n_images + 1, 0), img_pts(p.n_ip);
    for (int q = 0; q < p.n_ip; q++) img_begin[ip_image[q] + 1]++;
    for (int i = 0; i < p.n_images; i++) img_begin[i + 1] += img_begin[i];
    {
        std::vector<int32_t> fill(img_begin.begin(), img_begin.end() - 1);
        for (int q = 0; q < p.n_ip; q++) img_pts[fill[ip_image[q]]++] = ip_point[q];
    }
    std::vector<int32_t> stamp(p.n_points, -1), ids;
    for (int k = 0; k < n_pairs; k++) {
        const int S = pair_src[k], T = pair_ref[k];
        for (int q = img_begin[S]; q < img_begin[S + 1]; q++) stamp[img_pts[q]] = k;
        for (int i = 0; i < n_points; i++)
            if (stamp[points[i]] == k) { ids.push_back(points[i]); ids.push_back(S); ids.push_back(T); }
    }
    // the arguments are accepted: the previous result goes
    v.slot->xform.reset();
    std::unique_ptr<XformState> s(new XformState());
    s->ids = std::move(ids);
    s->nT = (int)(s->ids.size() / 3);
    s->R = 3 * (long)s->nT;
    const int rc = xform_run_impl(v, s.get(), sigma2);
    if (rc != JAICOV_OK) {
        hipStreamSynchronize(v.stream);
        return rc;
    }
    if (n_transformed) *n_transformed = s->nT;
    v.slot->xform = std::move(s);
    return JAICOV_OK;
}

static const char XF_NONE[] = "no transformation result: call jaicov_xform_run first";

extern "C" int jaicov_xform_get_coordinates(jaicov_engine *e, double *xyz, int32_t *ids, int32_t n) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    XformState *s = q_result(v, v.slot->xform, XF_NONE);
    if (!s) return JAICOV_ERR_BAD_STATE;
    if (n != s->nT) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "n must equal the number of transformed points");
    if (ids && n > 0) memcpy(ids, s->ids.data(), 3 * (size_t)n * sizeof(int32_t));
    if (xyz && n > 0) TRY(q_download(v, {{xyz, s->xyz.get(), 3 * (size_t)n * sizeof(double)}}));
    return JAICOV_OK;
}

extern "C" int jaicov_xform_get_covariance(jaicov_engine *e, double *packed, size_t len) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    XformState *s = q_result(v, v.slot->xform, XF_NONE);
    if (!s) return JAICOV_ERR_BAD_STATE;
    const size_t want = (size_t)s->R * (s->R + 1) / 2;
    if (len != want) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "covariance buffer length must be R(R+1)/2");
    if (want == 0) return JAICOV_OK;
    if (!packed) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "covariance buffer missing");
    return q_download(v, {{packed, s->ap.get(), want * sizeof(double)}});
}

extern "C" int jaicov_xform_get_covariance_sub(jaicov_engine *e, const int32_t *rows, int32_t k, double *out) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    XformState *s = q_result(v, v.slot->xform, XF_NONE);
    if (!s) return JAICOV_ERR_BAD_STATE;
    if (!rows || !out || k <= 0) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "rows / out missing or k <= 0");
    for (int i = 0; i < k; i++)
        if (rows[i] < 0 || rows[i] >= s->R) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "row index out of range");
    HIPE(*v.err, hipSetDevice(v.device));
    DevBuf<int32_t> d_rows;
    DevBuf<double> d_out;
    HIPE(*v.err, d_rows.reserve((size_t)k));
    HIPE(*v.err, d_out.reserve((size_t)k * k));
    HIPE(*v.err, hipMemcpyAsync(d_rows.get(), rows, (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    hipLaunchKernelGGL(xform_sub_kernel, dim3((unsigned)(((size_t)k * k + 255) / 256)), dim3(256), 0, v.stream, s->ap.get(), d_rows.get(), k, d_out.get());
    HIPE(*v.err, hipMemcpyAsync(out, d_out.get(), (size_t)k * k * sizeof(double), hipMemcpyDeviceToHost, v.stream));
    HIPE(*v.err, hipStreamSynchronize(v.stream));
    return JAICOV_OK;
}

extern "C" int jaicov_xform_get_point_blocks(jaicov_engine *e, double *out, int32_t n) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    XformState *s = q_result(v, v.slot->xform, XF_NONE);
    if (!s) return JAICOV_ERR_BAD_STATE;
    if (n != s->nT) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "n must equal the number of transformed points");
    if (n == 0) return JAICOV_OK;
    if (!out) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "out missing");
    HIPE(*v.err, hipSetDevice(v.device));
    DevBuf<double> d_out;
    HIPE(*v.err, d_out.reserve(9 * (size_t)n));
    hipLaunchKernelGGL(xform_blocks_kernel, dim3((unsigned)((9 * (size_t)n + 255) / 256)), dim3(256), 0, v.stream, s->ap.get(), (long)n, d_out.get());
    HIPE(*v.err, hipMemcpyAsync(out, d_out.get(), 9 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, v.stream));
    HIPE(*v.err, hipStreamSynchronize(v.stream));
    return JAICOV_OK;
}

extern "C" int jaicov_xform_release(jaicov_engine *e) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    q_release(v, v.slot->xform);
    return JAICOV_OK;
}
