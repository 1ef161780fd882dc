// Camera calibration in image space (include/jaicov_calibration.h): the distortion field of a camera with its covariance from the
// camera's own block of the cofactor matrix, and the difference field of two calibrations with a summary formed on the device.
// gfx950 only, wave64.
//
//   rows                  J and w of every node come from the adjustment's own rows (pairrows.h) on a SYNTHETIC problem: the nodes are
//                         its object points, it has one image per camera with six zero exterior orientation values (R = I), and a
//                         private slot vector [3 n node points | io | coefficients | zeros].  rows.hip is used as it is.
//   calib_nodes_kernel    node (xs, ys, N) -> the point (-xs N / c, -ys N / c, N) and the measurement (x0 + xs, y0 + ys), at the
//                         current x0, y0, c of side A's camera on the device
//   calib_cov_kernel      C = J_s Q[s, s] J_s' of every node, or C_d of a comparison.  The host sorts the nodes of a field by camera
//                         (stable); a workgroup of one wave takes up to 64 nodes of ONE camera (one camera pair in a comparison),
//                         stages the column list and Q[s, s] through q_at once in LDS (<= 23 columns, <= 46 in a comparison), and lane
//                         i reads the J of node i from the SoA rows block, coalesced.  J lies in LDS, one column of 64 words per lane,
//                         so the sums over s index it at run time without a register array.
//   calib_summary_kernel  one workgroup over the nodes of a comparison in the caller's order: thread t takes the nodes t, t + 256, ..,
//                         the 64 lanes of a wave meet in an xor butterfly, the four waves are added in the order 0, 1, 2, 3.  Sums are
//                         carried with their rounding error (two-sum), maxima take the smaller index on a tie.  No atomics.
// Nothing here writes to the cofactor matrix or to any other state of the engine but the buffers of CalibState.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/jaicov_calibration.h"
#include "ba_kernels.h"
#include "calibration.h"
#include "pairrows.h"
#include "qview.h"
#include "status.h"

namespace jaicov {

constexpr int CAL_K = JAICOV_CALIB_MAX_COLUMNS;     // the camera's own columns: io (3), dist (<= 20)
constexpr int CAL_WG = 64;                          // nodes of one workgroup of calib_cov_kernel, one lane each
constexpr int CAL_NT = 256;                         // threads of calib_summary_kernel
constexpr int CAL_WAVES = CAL_NT / 64;
static_assert(CAL_K == 3 + MAXD, "x0, y0, c and the coefficients of one camera");
static_assert(2 * CAL_K <= CAL_WG, "one lane per staged column");

// local column l of the camera (x0, y0, c, coefficients) in the local row layout of rows.hip
__device__ __forceinline__ int cal_local(int l) { return l < 3 ? 3 + l : 9 + l; }

// Node i (sorted order) of camera cam[i]: nodes = xs [n] | ys [n] | depth [n] (depth null: N = -c).  The point goes into both private
// slot vectors (valsB may be null), the measurement into x, y.  io0: offset of the first camera's x0 in a private slot vector.
__global__ __launch_bounds__(256) void calib_nodes_kernel(const int32_t *__restrict__ cam, const double *__restrict__ xs, const double *__restrict__ ys,
                                                          const double *__restrict__ depth, int n, long io0, double *__restrict__ valsA,
                                                          double *__restrict__ valsB, double *__restrict__ x, double *__restrict__ y) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double *io = valsA + io0 + 3 * (long)cam[i];
    const double x0 = io[0], y0 = io[1], c = io[2];
    const double N = depth ? depth[i] : -c;
    const double X = -xs[i] * N / c, Y = -ys[i] * N / c;
    valsA[3 * i] = X; valsA[3 * i + 1] = Y; valsA[3 * i + 2] = N;
    if (valsB) { valsB[3 * i] = X; valsB[3 * i + 1] = Y; valsB[3 * i + 2] = N; }
    x[i] = x0 + xs[i];
    y[i] = y0 + ys[i];
}

// J_a M[a, b] J_b' (2 x 2) of one lane: a over a0 .. a0 + na, b over b0 .. b0 + nb, both ascending.  Ms [NS][NS], Js [2 NS][64] in LDS.
template <int NS>
__device__ __forceinline__ void cal_block(const double *Ms, const double (*Js)[CAL_WG], int lane, int a0, int na, int b0, int nb, double &xx,
                                          double &xy, double &yx, double &yy) {
    xx = 0.0; xy = 0.0; yx = 0.0; yy = 0.0;
    for (int a = a0; a < a0 + na; a++) {
        double tx = 0.0, ty = 0.0;
        for (int b = b0; b < b0 + nb; b++) {
            const double q = Ms[a * NS + b];
            tx += q * Js[2 * b][lane];
            ty += q * Js[2 * b + 1][lane];
        }
        const double ax = Js[2 * a][lane], ay = Js[2 * a + 1][lane];
        xx += ax * tx; xy += ax * ty; yx += ay * tx; yy += ay * ty;
    }
}

// Workgroup w: the nodes first[w] .. first[w] + count[w] (<= 64, sorted order) of one camera.  cols [rows][CAL_K]: the matrix column of
// every local column of a camera (-1: fixed, not selected, or behind its K), ktab / ptab: K and the PARTIAL bit of every row of cols.
// Field: row cam[node] of cols, sa = sigma2, sb = k2, out rows of 14, jac (may be null) [n][2][CAL_K] zeroed by the host.
// COMPARE: side A is row 0 and side B row 1 of cols; sa = s0, sb = sigma2_post, out rows of 8.  ref != 0: side B has no columns in the
// matrix: its block is refcov / s0 (refcov null: zero) and there is no cross block.  ioA, ioB: x0, y0 of the two sides when the
// positions are relative to them, else null.
template <bool COMPARE>
__global__ __launch_bounds__(CAL_WG) void calib_cov_kernel(const double *__restrict__ Q, long ld, const int32_t *__restrict__ cam,
                                                           const int32_t *__restrict__ first, const int32_t *__restrict__ count,
                                                           const int32_t *__restrict__ cols, const int32_t *__restrict__ ktab,
                                                           const int32_t *__restrict__ ptab, int n, const double *__restrict__ JA,
                                                           const double *__restrict__ wA, const double *__restrict__ JB,
                                                           const double *__restrict__ wB, const double *__restrict__ nodes, int ref,
                                                           const double *__restrict__ refcov, const double *__restrict__ ioA,
                                                           const double *__restrict__ ioB, double sa, double sb, double *__restrict__ out,
                                                           double *__restrict__ jac, int32_t *__restrict__ status) {
    constexpr int NS = COMPARE ? 2 * CAL_K : CAL_K;
    __shared__ double Ms[NS * NS];
    __shared__ double Js[2 * NS][CAL_WG];
    __shared__ int scol[NS];
    const int lane = threadIdx.x, w = blockIdx.x;
    const int g0 = first[w], cnt = count[w];
    const int row = COMPARE ? 0 : cam[g0];
    const int ka = ktab[row], kb = COMPARE ? ktab[1] : 0, kt = ka + kb;
    if (lane < NS) scol[lane] = lane < CAL_K ? (lane < ka ? cols[CAL_K * row + lane] : -1) : (lane - CAL_K < kb ? cols[lane] : -1);
    __syncthreads();
    // the staged matrix: side A at 0 .., side B at CAL_K ..
    for (int e = lane; e < kt * kt; e += CAL_WG) {
        const int a = e / kt, b = e - a * kt;
        const int pa = a < ka ? a : CAL_K + a - ka, pb = b < ka ? b : CAL_K + b - ka;
        double q;
        if (COMPARE && ref && (a >= ka || b >= ka)) {
            q = 0.0;
            if (a >= ka && b >= ka && refcov && scol[pa] >= 0 && scol[pb] >= 0) {
                const int i = a - ka, j = b - ka;
                q = refcov[(i > j ? i : j) * kb + (i > j ? j : i)] / sa;
            }
        } else {
            q = q_at(Q, ld, scol[pa], scol[pb]);
        }
        Ms[pa * NS + pb] = q;
    }
    const bool on = lane < cnt;
    const int gi = g0 + (on ? lane : 0);
    double z = 0.0;                                    // NaN unless every row entry of the node is finite
    for (int l = 0; l < ka; l++) {
        const int loc = cal_local(l);
        const double vx = JA[(size_t)(2 * loc) * n + gi], vy = JA[(size_t)(2 * loc + 1) * n + gi];
        z += vx * 0.0 + vy * 0.0;
        if (!COMPARE && jac && on) {
            jac[(size_t)gi * 2 * CAL_K + l] = vx;
            jac[(size_t)gi * 2 * CAL_K + CAL_K + l] = vy;
        }
        const bool keep = scol[l] >= 0;
        Js[2 * l][lane] = keep ? vx : 0.0;
        Js[2 * l + 1][lane] = keep ? vy : 0.0;
    }
    if (COMPARE)
        for (int l = 0; l < kb; l++) {
            const int loc = cal_local(l);
            const double vx = JB[(size_t)(2 * loc) * n + gi], vy = JB[(size_t)(2 * loc + 1) * n + gi];
            z += vx * 0.0 + vy * 0.0;
            const bool keep = scol[CAL_K + l] >= 0;
            Js[2 * (CAL_K + l)][lane] = keep ? vx : 0.0;
            Js[2 * (CAL_K + l) + 1][lane] = keep ? vy : 0.0;
        }
    const double a0 = wA[gi], a1 = wA[(size_t)n + gi];
    __syncthreads();
    double cxx, cxy, cyx, cyy;
    cal_block<NS>(Ms, Js, lane, 0, ka, 0, ka, cxx, cxy, cyx, cyy);
    double d0 = -a0, d1 = -a1;
    int st = ptab[row];
    if (COMPARE) {
        double bxx = 0.0, bxy = 0.0, byx = 0.0, byy = 0.0, xxx = 0.0, xxy = 0.0, xyx = 0.0, xyy = 0.0;
        if (!ref) cal_block<NS>(Ms, Js, lane, 0, ka, CAL_K, kb, xxx, xxy, xyx, xyy);
        cal_block<NS>(Ms, Js, lane, CAL_K, kb, CAL_K, kb, bxx, bxy, byx, byy);
        // aa - ab - ba + bb from left to right; ba is the transpose of ab
        cxx = ((cxx - xxx) - xxx) + bxx;
        cxy = ((cxy - xxy) - xyx) + bxy;
        cyy = ((cyy - xyy) - xyy) + byy;
        d0 = wB[gi] - a0; d1 = wB[(size_t)n + gi] - a1;
        if (ioA) { d0 += ioB[0] - ioA[0]; d1 += ioB[1] - ioA[1]; }
        st |= ptab[1];
    }
    if (!on) return;
    constexpr int NC = COMPARE ? JAICOV_CALIB_COMPARE_COLUMNS : JAICOV_CALIB_FIELD_COLUMNS;
    double *o = out + (size_t)NC * gi;
    const double fin = z + (((cxx + cxy) + cyy) + (d0 + d1) + (sa + sb));
    if (!isfinite(fin)) {
#pragma unroll
        for (int k = 0; k < NC; k++) o[k] = NAN;
        status[gi] = st | JAICOV_CALIB_NOT_FINITE;
        return;
    }
    const double hm = 0.5 * (cxx + cyy), hd = 0.5 * (cxx - cyy), hw = hypot(hd, cxy);
    if (hm - hw < -1e-12 * (cxx + cyy)) st |= JAICOV_CALIB_NEGATIVE;
    if (COMPARE) {
        const double det = cxx * cyy - cxy * cxy;
        double q = NAN;
        if (det > 0.0 && cxx > 0.0) q = ((cyy * d0 * d0 - 2.0 * cxy * d0 * d1) + cxx * d1 * d1) / det;
        else st |= JAICOV_CALIB_SINGULAR;
        o[0] = d0; o[1] = d1; o[2] = cxx; o[3] = cxy; o[4] = cyy; o[5] = q;
        o[6] = q / (2.0 * sa); o[7] = q / (2.0 * sb);
    } else {
        o[0] = d0; o[1] = d1; o[2] = cxx; o[3] = cxy; o[4] = cyy;
        o[5] = sqrt(sa * fmax(cxx, 0.0)); o[6] = sqrt(sa * fmax(cyy, 0.0));
        o[7] = sb * sqrt(sa * fmax(hm + hw, 0.0));
        o[8] = sb * sqrt(sa * fmax(hm - hw, 0.0));
        double dir = 0.5 * atan2(2.0 * cxy, cxx - cyy);
        if (dir < 0.0) dir += M_PI;
        if (dir >= M_PI) dir = 0.0;
        o[9] = dir;
        const double xs = nodes[gi], ys = nodes[(size_t)n + gi];
        const double r = hypot(xs, ys);
        if (r > 0.0) {
            const double r2 = r * r;
            const double qrr = ((xs * xs * cxx + 2.0 * xs * ys * cxy) + ys * ys * cyy) / r2;
            const double qtt = ((ys * ys * cxx - 2.0 * xs * ys * cxy) + xs * xs * cyy) / r2;
            o[10] = (xs * d0 + ys * d1) / r;
            o[11] = (-ys * d0 + xs * d1) / r;
            o[12] = sqrt(sa * fmax(qrr, 0.0));
            o[13] = sqrt(sa * fmax(qtt, 0.0));
        } else {
            o[10] = NAN; o[11] = NAN; o[12] = NAN; o[13] = NAN;
        }
    }
    status[gi] = st;
}

// A sum carried with its rounding error (Knuth's two-sum), as vce.hip carries the sums of its groups.  Sums only, no products: nothing
// here can be contracted.
struct CalPair {
    double hi, lo;
};
__device__ __forceinline__ void cal_pair_add(CalPair &a, double x) {
    const double s = a.hi + x, b = s - a.hi;
    a.lo += (a.hi - (s - b)) + (x - b);
    a.hi = s;
}
// a += b, b a pair
__device__ __forceinline__ void cal_pair_join(CalPair &a, double bhi, double blo) {
    cal_pair_add(a, bhi);
    a.lo += blo;
}
// the same pair in every lane: both partners add the larger lane's pair to the smaller lane's, in that order
__device__ __forceinline__ CalPair cal_pair_wave(CalPair a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double h = __shfl_xor(a.hi, off, 64), l = __shfl_xor(a.lo, off, 64);
        const bool upper = (threadIdx.x & off) != 0;
        CalPair x{upper ? h : a.hi, upper ? l : a.lo};
        cal_pair_join(x, upper ? a.hi : h, upper ? a.lo : l);
        a = x;
    }
    return a;
}
// a maximum with its node: the larger value, on a tie the smaller node; node < 0: none yet
struct CalMax {
    double v;
    int i;
};
__device__ __forceinline__ void cal_max_join(CalMax &a, double v, int i) {
    if (i < 0) return;
    if (a.i < 0 || v > a.v || (v == a.v && i < a.i)) { a.v = v; a.i = i; }
}
__device__ __forceinline__ CalMax cal_max_wave(CalMax a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double v = __shfl_xor(a.v, off, 64);
        const int i = __shfl_xor(a.i, off, 64);
        cal_max_join(a, v, i);
    }
    return a;
}
__device__ __forceinline__ int cal_int_wave(int x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// out [n][8] and status [n] of a comparison in the caller's order -> summary [8].  One workgroup.
__global__ __launch_bounds__(CAL_NT) void calib_summary_kernel(const double *__restrict__ out, const int32_t *__restrict__ status, int n, double s0,
                                                               double *__restrict__ summary) {
    __shared__ double sd[CAL_WAVES][6];
    __shared__ int si[CAL_WAVES][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int nf = 0, ns = 0;
    CalPair d2{0.0, 0.0}, tr{0.0, 0.0};
    CalMax md{0.0, -1}, mt{0.0, -1};
    for (int i = tid; i < n; i += CAL_NT) {
        const int st = status[i];
        if (st & JAICOV_CALIB_SINGULAR) ns++;
        if (st & JAICOV_CALIB_NOT_FINITE) continue;
        const double *o = out + (size_t)JAICOV_CALIB_COMPARE_COLUMNS * i;
        nf++;
        const double q = __dadd_rn(__dmul_rn(o[0], o[0]), __dmul_rn(o[1], o[1]));      // each operation rounded on its own
        cal_pair_add(d2, q);
        cal_pair_add(tr, __dadd_rn(o[2], o[4]));
        cal_max_join(md, q, i);
        if (!(st & JAICOV_CALIB_SINGULAR)) cal_max_join(mt, o[6], i);
    }
    nf = cal_int_wave(nf); ns = cal_int_wave(ns);
    d2 = cal_pair_wave(d2); tr = cal_pair_wave(tr);
    md = cal_max_wave(md); mt = cal_max_wave(mt);
    if (lane == 0) {
        sd[wave][0] = d2.hi; sd[wave][1] = d2.lo; sd[wave][2] = tr.hi; sd[wave][3] = tr.lo; sd[wave][4] = md.v; sd[wave][5] = mt.v;
        si[wave][0] = nf; si[wave][1] = ns; si[wave][2] = md.i; si[wave][3] = mt.i;
    }
    __syncthreads();
    if (tid != 0) return;
    for (int k = 1; k < CAL_WAVES; k++) {
        nf += si[k][0]; ns += si[k][1];
        cal_pair_join(d2, sd[k][0], sd[k][1]);
        cal_pair_join(tr, sd[k][2], sd[k][3]);
        cal_max_join(md, sd[k][4], si[k][2]);
        cal_max_join(mt, sd[k][5], si[k][3]);
    }
    const double nan = (double)NAN;
    summary[0] = (double)nf;
    summary[1] = nf > 0 ? sqrt((d2.hi + d2.lo) / (double)nf) : nan;
    summary[2] = nf > 0 ? sqrt(s0 * (tr.hi + tr.lo) / (double)nf) : nan;
    summary[3] = md.i >= 0 ? sqrt(md.v) : nan;
    summary[4] = (double)md.i;
    summary[5] = mt.i >= 0 ? mt.v : nan;
    summary[6] = (double)mt.i;
    summary[7] = (double)ns;
}

// the camera tables of the problem, read from the device once per engine
static int calib_tables(const QView &v, CalibState *st) {
    if (st->have_tables) return JAICOV_OK;
    st->cam_dist_begin.resize((size_t)v.p->n_cameras + 1);
    st->dist_kind.resize((size_t)v.p->n_dist);
    TRY(q_download(v, {{st->cam_dist_begin.data(), v.p->cam_dist_begin, st->cam_dist_begin.size() * sizeof(int32_t)},
                       {st->dist_kind.data(), v.p->dist_kind, st->dist_kind.size() * sizeof(int32_t)}}));
    st->have_tables = true;
    return JAICOV_OK;
}

static bool all_finite(const double *a, size_t n) {
    for (size_t k = 0; k < n; k++)
        if (!std::isfinite(a[k])) return false;
    return true;
}

struct CalibCall {
    bool compare = false;
    double sa = 0.0, sb = 0.0;                      // field: sigma2, k2; compare: s0, sigma2_post
    uint32_t columns = JAICOV_CALIB_ALL, flags = 0;
    const int32_t *cams = nullptr;                  // field
    int32_t cam_a = 0, cam_b = 0;                   // compare
    const double *ref_values = nullptr, *ref_cov = nullptr;
    const double *xy = nullptr, *depth = nullptr;
    int32_t n = 0;
    double *out = nullptr, *jac = nullptr, *summary = nullptr;
    int32_t *status = nullptr;
};

static int calib_run(jaicov_engine *e, CalibCall c) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    TRY(q_guard(v, "the calibration in image space on a sharded engine"));
    const DevProblem &p = *v.p;
    const int n = c.n, nc = p.n_cameras;
    if (c.compare) {
        c.sa = v.sigma2;
        const char *what = "calibration comparison: NULL xy, a negative count, a camera out of range or unknown flags";
        if (n < 0 || (n > 0 && !c.xy) || c.cam_a < 0 || c.cam_a >= nc || c.cam_b < 0 || c.cam_b >= nc || (c.flags & ~(uint32_t)JAICOV_CALIB_RELATIVE))
            FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, what);
        if (!c.ref_values && (c.cam_a == c.cam_b || c.ref_cov))
            FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "calibration comparison: without ref_values side B is another camera of the engine, and there is no ref_cov");
        if (!(c.sb > 0.0) || !std::isfinite(c.sb)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "calibration comparison: sigma2_post must be positive");
    } else {
        if (n < 0 || (n > 0 && (!c.cams || !c.xy || !c.out || !c.status)))
            FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "calibration field: NULL argument or a negative count");
        if (!(c.sa >= 0.0) || !(c.sb >= 0.0)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "calibration field: sigma2 and k2 must not be negative");
        if (c.columns == 0 || (c.columns & ~(uint32_t)JAICOV_CALIB_ALL)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "calibration field: no column selected, or an unknown bit");
        for (int i = 0; i < n; i++)
            if (c.cams[i] < 0 || c.cams[i] >= nc) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "calibration field: camera index out of range");
    }
    CalibState *st = q_state(v.slot->calib);
    TRY(calib_tables(v, st));
    const std::vector<int32_t> &cdb = st->cam_dist_begin;
    auto n_dist_of = [&](int k) { return cdb[k + 1] - cdb[k]; };
    auto has_di = [&](int k) {
        for (int j = cdb[k]; j < cdb[k + 1]; j++)
            if (st->dist_kind[j] == JAICOV_DIST_DISTANCE_DI) return true;
        return false;
    };
    // the cameras of the call; a field counts its nodes per camera on the way (a stable counting sort follows)
    std::vector<int32_t> begin((size_t)nc + 1, 0);
    if (c.compare) {
        begin[(size_t)c.cam_a + 1] = n;
    } else {
        for (int i = 0; i < n; i++) begin[(size_t)c.cams[i] + 1]++;
    }
    std::vector<uint8_t> used(nc, 0);
    for (int k = 0; k < nc; k++) used[k] = begin[k + 1] > 0;
    if (c.compare) used[c.cam_a] = used[c.cam_b] = 1;
    for (int k = 0; k < nc; k++) {
        if (!used[k]) continue;
        if (n_dist_of(k) > MAXD) FAIL(*v.err, JAICOV_ERR_UNSUPPORTED, "a camera with more coefficients than JAICOV_MAX_DIST_PER_CAMERA");
        if (n > 0 && !c.depth && has_di(k))
            FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "depth == NULL, but a camera of the call has a distance-dependent coefficient D_i");
    }
    const int Kb = c.compare ? 3 + n_dist_of(c.cam_b) : 0;
    if (c.ref_values && !all_finite(c.ref_values, (size_t)Kb)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "calibration comparison: a ref_values entry is not finite");
    if (c.ref_cov)
        for (int i = 0; i < Kb; i++)
            if (!all_finite(c.ref_cov + (size_t)i * Kb, (size_t)i + 1)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "calibration comparison: a ref_cov entry is not finite");
    // the matrix column of every local column of the cameras' rows: rows of cols by camera (field), or side A and side B (compare)
    const size_t s_io = 3 * (size_t)p.n_points, s_dist = s_io + 3 * (size_t)nc;
    const bool ref = c.ref_values != nullptr;
    const int n_rows = c.compare ? 2 : nc;
    std::vector<int32_t> cols((size_t)n_rows * CAL_K, -1), ktab(n_rows, 0), ptab(n_rows, 0);
    for (int r = 0; r < n_rows; r++) {
        const int k = c.compare ? (r == 0 ? c.cam_a : c.cam_b) : r;
        if (!used[k]) continue;
        ktab[r] = 3 + n_dist_of(k);
        for (int l = 0; l < ktab[r]; l++) {
            const uint32_t bit = l < 2 ? JAICOV_CALIB_PRINCIPAL_POINT : l == 2 ? JAICOV_CALIB_PRINCIPAL_DISTANCE
                                                                               : 1u << (JAICOV_CALIB_KIND_SHIFT + st->dist_kind[cdb[k] + l - 3]);
            const bool selected = c.compare ? !(l < 2 && (c.flags & JAICOV_CALIB_RELATIVE)) : (c.columns & bit) != 0;
            if (!selected) continue;
            if (c.compare && r == 1 && ref) {       // a reference set has no columns in the matrix: every selected one counts
                cols[(size_t)r * CAL_K + l] = 0;
                continue;
            }
            int col = -1;
            TRY(q_column(v, l < 3 ? s_io + 3 * (size_t)k + l : s_dist + (size_t)cdb[k] + l - 3, "a camera's column lies outside the cofactor matrix", &col));
            if (col < 0) ptab[r] = JAICOV_CALIB_PARTIAL;
            cols[(size_t)r * CAL_K + l] = col;
        }
    }
    const double nan = NAN;
    if (n == 0) {
        if (c.compare && c.summary) {
            const double empty[JAICOV_CALIB_SUMMARY_COLUMNS] = {0.0, nan, nan, nan, -1.0, nan, -1.0, 0.0};
            std::copy(empty, empty + JAICOV_CALIB_SUMMARY_COLUMNS, c.summary);
        }
        return JAICOV_OK;
    }
    HIPE(*v.err, hipSetDevice(v.device));

    // a stable counting sort by camera: order[s] = the caller's index of sorted position s (a comparison has one camera: the identity)
    for (int k = 0; k < nc; k++) begin[k + 1] += begin[k];
    std::vector<int32_t> order(n);
    if (c.compare) {
        for (int i = 0; i < n; i++) order[i] = i;
    } else {
        std::vector<int32_t> next(begin.begin(), begin.end() - 1);
        for (int i = 0; i < n; i++) order[next[c.cams[i]]++] = i;
    }
    size_t W = 0;
    for (int k = 0; k < nc; k++) W += (size_t)(begin[k + 1] - begin[k] + CAL_WG - 1) / CAL_WG;
    const size_t N = (size_t)n, R = (size_t)n_rows;
    // tab: camera A [n] | camera B [n] | point [n] | image_camera [nc] | first [W] | count [W] | cols [R CAL_K] | K [R] | PARTIAL [R] || status [n]
    const size_t o_camb = N, o_pt = 2 * N, o_ic = 3 * N, o_first = o_ic + (size_t)nc, o_count = o_first + W, o_cols = o_count + W,
                 o_k = o_cols + R * CAL_K, o_p = o_k + R, n_up = o_p + R, o_status = n_up, n_tab = o_status + N;
    std::vector<int32_t> tab(n_up, 0);
    for (size_t s = 0; s < N; s++) {
        tab[s] = c.compare ? c.cam_a : c.cams[order[s]];
        tab[o_camb + s] = c.cam_b;
        tab[o_pt + s] = (int32_t)s;
    }
    for (int k = 0; k < nc; k++) tab[o_ic + k] = k;
    {
        size_t w = 0;
        for (int k = 0; k < nc; k++)
            for (int s = begin[k]; s < begin[k + 1]; s += CAL_WG, w++) {
                tab[o_first + w] = s;
                tab[o_count + w] = std::min(CAL_WG, begin[k + 1] - s);
            }
    }
    std::copy(cols.begin(), cols.end(), tab.begin() + o_cols);
    std::copy(ktab.begin(), ktab.end(), tab.begin() + o_k);
    std::copy(ptab.begin(), ptab.end(), tab.begin() + o_p);
    // out: xs [n] | ys [n] | depth [n] | out [NC n] | jac [2 CAL_K n] | ref_cov [Kb Kb] | summary [8]
    const int NC = c.compare ? JAICOV_CALIB_COMPARE_COLUMNS : JAICOV_CALIB_FIELD_COLUMNS;
    const size_t n_jac = c.jac ? 2 * CAL_K * N : 0, n_cov = c.ref_cov ? (size_t)Kb * Kb : 0;
    const size_t o_out = 3 * N, o_jac = o_out + (size_t)NC * N, o_cov = o_jac + n_jac, o_sum = o_cov + n_cov, n_out = o_sum + JAICOV_CALIB_SUMMARY_COLUMNS;
    std::vector<double> nodes(3 * N + n_cov, 0.0);
    for (size_t s = 0; s < N; s++) {
        const size_t i = (size_t)order[s];
        nodes[s] = c.xy[2 * i]; nodes[N + s] = c.xy[2 * i + 1];
        if (c.depth) nodes[2 * N + s] = c.depth[i];
    }
    if (n_cov) std::copy(c.ref_cov, c.ref_cov + n_cov, nodes.begin() + 3 * N);
    // the private slot vectors: node points [3 n] | io [3 nc] | coefficients [n_dist] | zeros [6 nc]
    const size_t n_cam = 3 * (size_t)nc + (size_t)p.n_dist, n_vals = 3 * N + n_cam + 6 * (size_t)nc;
    const int sides = c.compare ? 2 : 1;
    PairRows prA(N), prB(N);
    HIPE(*v.err, st->tab.reserve(n_tab));
    HIPE(*v.err, st->rows.reserve(prA.size * sides));
    HIPE(*v.err, st->vals.reserve(n_vals * sides));
    HIPE(*v.err, st->out.reserve(n_out));
    int32_t *d_tab = st->tab.get();
    double *d_o = st->out.get(), *d_valsA = st->vals.get(), *d_valsB = c.compare ? d_valsA + n_vals : nullptr;
    double *d_out = d_o + o_out, *d_jac = c.jac ? d_o + o_jac : nullptr, *d_cov = n_cov ? d_o + o_cov : nullptr, *d_sum = d_o + o_sum;
    prA.bind(st->rows.get());
    prB.bind(st->rows.get() + (c.compare ? prA.size : 0));
    const hipStream_t s = v.stream;
    HIPE(*v.err, hipMemcpyAsync(d_tab, tab.data(), n_up * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPE(*v.err, hipMemcpyAsync(d_o, nodes.data(), 3 * N * sizeof(double), hipMemcpyHostToDevice, s));
    if (n_cov) HIPE(*v.err, hipMemcpyAsync(d_cov, nodes.data() + 3 * N, n_cov * sizeof(double), hipMemcpyHostToDevice, s));
    if (d_jac) HIPE(*v.err, hipMemsetAsync(d_jac, 0, n_jac * sizeof(double), s));
    for (int side = 0; side < sides; side++) {
        double *vals = side ? d_valsB : d_valsA;
        const PairRows &pr = side ? prB : prA;
        HIPE(*v.err, hipMemcpyAsync(vals + 3 * N, v.d_vals + s_io, n_cam * sizeof(double), hipMemcpyDeviceToDevice, s));
        HIPE(*v.err, hipMemsetAsync(vals + 3 * N + n_cam, 0, 6 * (size_t)nc * sizeof(double), s));
        // the rows are zeroed first: rows_kernel writes no column of a family that the camera lacks
        HIPE(*v.err, hipMemsetAsync(pr.J, 0, pr.o_w * sizeof(double), s));
    }
    if (ref) {
        HIPE(*v.err, hipMemcpyAsync(d_valsB + 3 * N + 3 * (size_t)c.cam_b, c.ref_values, 3 * sizeof(double), hipMemcpyHostToDevice, s));
        if (Kb > 3)
            HIPE(*v.err, hipMemcpyAsync(d_valsB + 3 * N + 3 * (size_t)nc + (size_t)cdb[c.cam_b], c.ref_values + 3, (size_t)(Kb - 3) * sizeof(double),
                                        hipMemcpyHostToDevice, s));
    }
    QTimer<4> timer(s);
    HIPE(*v.err, timer.arm(st->timing));
    HIPE(*v.err, timer.mark(0));
    hipLaunchKernelGGL(calib_nodes_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, d_tab, d_o, d_o + N, c.depth ? d_o + 2 * N : nullptr, n,
                       (long)(3 * N), d_valsA, d_valsB, prA.x, prA.y);
    HIPE(*v.err, hipGetLastError());
    // the synthetic problem: the nodes are its points, camera k has the image k with R = I
    DevProblem qa = prA.problem(p, d_tab, d_tab + o_pt);
    qa.n_points = n; qa.n_images = nc; qa.n_slots = (int)n_vals; qa.image_camera = d_tab + o_ic;
    HIPE(*v.err, prA.rows(s, qa, d_valsA));
    if (c.compare) {
        DevProblem qb = qa;
        qb.ip_image = d_tab + o_camb;
        HIPE(*v.err, launch_rows(s, qb, d_valsB, 0, n, prB.J, prB.w));
    }
    HIPE(*v.err, timer.mark(1));
    const bool relative = c.compare && (c.flags & JAICOV_CALIB_RELATIVE);
    if (c.compare)
        hipLaunchKernelGGL(calib_cov_kernel<true>, dim3((unsigned)W), dim3(CAL_WG), 0, s, v.Q, v.ld, d_tab, d_tab + o_first, d_tab + o_count,
                           d_tab + o_cols, d_tab + o_k, d_tab + o_p, n, prA.J, prA.w, prB.J, prB.w, d_o, ref ? 1 : 0, d_cov,
                           relative ? d_valsA + 3 * N + 3 * (size_t)c.cam_a : nullptr, relative ? d_valsB + 3 * N + 3 * (size_t)c.cam_b : nullptr,
                           c.sa, c.sb, d_out, d_jac, d_tab + o_status);
    else
        hipLaunchKernelGGL(calib_cov_kernel<false>, dim3((unsigned)W), dim3(CAL_WG), 0, s, v.Q, v.ld, d_tab, d_tab + o_first, d_tab + o_count,
                           d_tab + o_cols, d_tab + o_k, d_tab + o_p, n, prA.J, prA.w, prA.J, prA.w, d_o, 0, d_cov, nullptr, nullptr, c.sa, c.sb,
                           d_out, d_jac, d_tab + o_status);
    HIPE(*v.err, hipGetLastError());
    HIPE(*v.err, timer.mark(2));
    if (c.compare && c.summary) {
        hipLaunchKernelGGL(calib_summary_kernel, dim3(1), dim3(CAL_NT), 0, s, d_out, d_tab + o_status, n, c.sa, d_sum);
        HIPE(*v.err, hipGetLastError());
    }
    HIPE(*v.err, timer.mark(3));
    if (c.compare) {             // the caller's order is the device's
        TRY(q_download(v, {{c.out, d_out, (size_t)NC * N * sizeof(double)},
                           {c.status, d_tab + o_status, N * sizeof(int32_t)},
                           {c.summary, d_sum, JAICOV_CALIB_SUMMARY_COLUMNS * sizeof(double)}}));
        HIPE(*v.err, timer.read(st->ms));
        return JAICOV_OK;
    }
    std::vector<double> h_out((size_t)NC * N), h_jac(n_jac);
    std::vector<int32_t> h_status(N);
    TRY(q_download(v, {{h_out.data(), d_out, h_out.size() * sizeof(double)},
                       {h_status.data(), d_tab + o_status, N * sizeof(int32_t)},
                       {h_jac.data(), d_jac, n_jac * sizeof(double)}}));
    HIPE(*v.err, timer.read(st->ms));
    for (size_t q = 0; q < N; q++) {             // back into the caller's order
        const size_t i = (size_t)order[q];
        std::copy(h_out.begin() + NC * q, h_out.begin() + NC * (q + 1), c.out + (size_t)NC * i);
        c.status[i] = h_status[q];
        if (c.jac) std::copy(h_jac.begin() + 2 * CAL_K * q, h_jac.begin() + 2 * CAL_K * (q + 1), c.jac + 2 * CAL_K * i);
    }
    return JAICOV_OK;
}

}  // namespace jaicov

using namespace jaicov;

extern "C" int jaicov_calib_field(jaicov_engine *e, double sigma2, double k2, uint32_t columns, const int32_t *cams, const double *xy,
                                  const double *depth, int32_t n, double *out, double *jac_out, int32_t *status) {
    CalibCall c;
    c.sa = sigma2; c.sb = k2; c.columns = columns; c.cams = cams; c.xy = xy; c.depth = depth; c.n = n; c.out = out; c.jac = jac_out; c.status = status;
    return calib_run(e, c);
}

extern "C" int jaicov_calib_compare(jaicov_engine *e, double sigma2_post, int32_t cam_a, int32_t cam_b, const double *ref_values,
                                    const double *ref_cov, uint32_t flags, const double *xy, const double *depth, int32_t n, double *out,
                                    int32_t *status, double *summary) {
    CalibCall c;
    c.compare = true;
    c.sb = sigma2_post; c.cam_a = cam_a; c.cam_b = cam_b; c.ref_values = ref_values; c.ref_cov = ref_cov; c.flags = flags; c.xy = xy; c.depth = depth;
    c.n = n; c.out = out; c.status = status; c.summary = summary;
    return calib_run(e, c);
}

extern "C" int jaicov_calib_release(jaicov_engine *e) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    q_release(v, v.slot->calib);
    return JAICOV_OK;
}

// The hook of scripts/calib_bench.py: on != 0 makes the following calls time their kernels by events on the engine's stream;
// ms[0 .. 2]: what the node and rows kernels, calib_cov_kernel and calib_summary_kernel of the last call took.
extern "C" int jaicov_debug_calib_timing(jaicov_engine *e, int on, float *ms) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    CalibState *st = on ? q_state(v.slot->calib) : v.slot->calib.get();       // asking an engine that never ran the call allocates nothing
    if (st) st->timing = on != 0;
    if (ms)
        for (int k = 0; k < 3; k++) ms[k] = st ? st->ms[k] : 0.f;
    return JAICOV_OK;
}
