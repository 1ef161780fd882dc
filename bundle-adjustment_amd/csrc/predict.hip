// Image-space readers of the cofactor matrix on the device (include/jaicov_predict.h): predicted image points with their
// confidence ellipses, and the test of check measurements pair by pair and in groups.
//
//   rows               J and w of every pair come from the adjustment's own rows (pairrows.h): the collinearity and distortion formulas
//                      are written once.  The row buffers are the state's own.
//   pred_cov_kernel    C = J Qxx J' of every pair.  The host sorts the pairs by image (stable); a workgroup of one wave takes up to 64
//                      pairs of ONE image, stages Q[S, S] of that image's camera and EO columns S (<= 29) once in LDS, and lane i
//                      gathers for pair i only the 3 x |S| strip and the 3 x 3 block of its point.  J lies in LDS, one column of 64
//                      words per lane, so the sums over S index it at run time without a register array.
//   pred_group_kernel  one wave per group of m <= 32 pairs: M_G (2m x 2m, packed upper in LDS) block by block, every block gathered by
//                      the 64 lanes and reduced by an xor butterfly, then the scaling, the lane-parallel Cholesky factor and the
//                      forward substitution of wavealg.h.
// Nothing here writes to the cofactor matrix or to any other state of the engine but the buffers of PredictState.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/jaicov_predict.h"
#include "ba_kernels.h"
#include "pairrows.h"
#include "predict.h"
#include "qview.h"
#include "status.h"
#include "wavealg.h"

namespace jaicov {

constexpr int PRED_S = KC_MAX;                               // camera and EO columns of one image: io (3), eo (6), dist (<= 20)
constexpr int PRED_WG = 64;                                  // pairs of one workgroup of pred_cov_kernel, one lane each
constexpr int PRED_STAGE = (PRED_S * PRED_S + PRED_WG - 1) / PRED_WG;
constexpr int PRED_R = 2 * JAICOV_PRED_MAX_GROUP;            // largest order of M_G
constexpr int PRED_TRI = PRED_R * (PRED_R + 1) / 2;
static_assert(PRED_S == KROW - 3, "the local columns behind X, Y, Z are the image's shared columns");
static_assert(PRED_R == 64, "one lane per row of M_G");

// Workgroup w: the pairs first[w] .. first[w] + count[w] (<= 64, sorted order) of one image.  rowsA [2 KROW][n], rowsW [2][n] and
// disp [3][n] run over the sorted pairs.  CHECK: sa = s0, sb = sigma2_post, out rows of 8; otherwise sa = sigma2, sb = k2, rows of 10.
template <bool CHECK>
__global__ __launch_bounds__(PRED_WG) void pred_cov_kernel(const double *__restrict__ Q, long ld, DevProblem p, const int32_t *__restrict__ img,
                                                           const int32_t *__restrict__ pt, const int32_t *__restrict__ first,
                                                           const int32_t *__restrict__ count, int n, const double *__restrict__ rowsA,
                                                           const double *__restrict__ rowsW, const double *__restrict__ disp, double sa,
                                                           double sb, double *__restrict__ out, int32_t *__restrict__ status) {
    __shared__ double Qs[PRED_S * PRED_S];
    __shared__ double Js[2 * KROW][PRED_WG];
    __shared__ int scol[PRED_S];
    const int lane = threadIdx.x, w = blockIdx.x;
    const int g0 = first[w], cnt = count[w];
    const int image = img[g0], cam = p.image_camera[image];
    const int jb = p.cam_dist_begin[cam], ns = 9 + (p.cam_dist_begin[cam + 1] - jb);
    int myc = -1;
    if (lane < ns) myc = lane < 3 ? p.io_col[3 * cam + lane] : lane < 9 ? p.eo_col[6 * image + lane - 3] : p.dist_col[jb + lane - 9];
    if (lane < PRED_S) scol[lane] = myc;
    const bool s_fixed = __any(lane < ns && myc < 0) != 0;
    const bool on = lane < cnt;
    const int gi = g0 + (on ? lane : 0);
    const int point = pt[gi];
    int pc[3];
#pragma unroll
    for (int a = 0; a < 3; a++) pc[a] = p.point_col[3 * point + a];
    __syncthreads();
    // every load of the lane is issued before the first of them is used: Q[S, S], the point's block, its strip, its rows
    double stq[PRED_STAGE];
#pragma unroll
    for (int t = 0; t < PRED_STAGE; t++) {
        const int e = lane + PRED_WG * t, a = e / ns, b = e - a * ns;
        stq[t] = e < ns * ns ? q_at(Q, ld, scol[a], scol[b]) : 0.0;
    }
    double qpp[3][3], q3[3][PRED_S];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b <= a; b++) qpp[a][b] = qpp[b][a] = q_at(Q, ld, pc[a], pc[b]);
#pragma unroll
    for (int b = 0; b < PRED_S; b++) {
        const int cb = scol[b];                    // -1 behind the camera's coefficients
#pragma unroll
        for (int a = 0; a < 3; a++) q3[a][b] = q_at(Q, ld, pc[a], cb);
    }
#pragma unroll
    for (int l = 0; l < 2 * KROW; l++) {
        const double v = rowsA[(size_t)l * n + gi];
        const bool fixed = (l >> 1) < 3 ? pc[(l >> 1) % 3] < 0 : scol[(l >> 1) - 3] < 0;
        Js[l][lane] = fixed ? 0.0 : v;
    }
    const double w0 = rowsW[gi], w1 = rowsW[(size_t)n + gi];
#pragma unroll
    for (int t = 0; t < PRED_STAGE; t++) {
        const int e = lane + PRED_WG * t, a = e / ns, b = e - a * ns;
        if (e < ns * ns) Qs[a * PRED_S + b] = stq[t];
    }
    __syncthreads();
    // the point's rows against its own block and against the strip
    double jx[3], jy[3], ppx[3], ppy[3], wx[3] = {0.0, 0.0, 0.0}, wy[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 3; a++) { jx[a] = Js[2 * a][lane]; jy[a] = Js[2 * a + 1][lane]; }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        ppx[a] = (qpp[a][0] * jx[0] + qpp[a][1] * jx[1]) + qpp[a][2] * jx[2];
        ppy[a] = (qpp[a][0] * jy[0] + qpp[a][1] * jy[1]) + qpp[a][2] * jy[2];
    }
#pragma unroll
    for (int b = 0; b < PRED_S; b++) {
        const double bx = Js[2 * (b + 3)][lane], by = Js[2 * (b + 3) + 1][lane];
#pragma unroll
        for (int a = 0; a < 3; a++) { wx[a] += q3[a][b] * bx; wy[a] += q3[a][b] * by; }
    }
    // the shared columns against Q[S, S]
    double sxx = 0.0, sxy = 0.0, syy = 0.0;
    for (int a = 0; a < ns; a++) {
        double tx = 0.0, ty = 0.0;
        for (int b = 0; b < ns; b++) {
            const double q = Qs[a * PRED_S + b];
            tx += q * Js[2 * (b + 3)][lane];
            ty += q * Js[2 * (b + 3) + 1][lane];
        }
        const double ax = Js[2 * (a + 3)][lane], ay = Js[2 * (a + 3) + 1][lane];
        sxx += ax * tx; sxy += ax * ty; syy += ay * ty;
    }
    double cxx = 0.0, cxy = 0.0, cyy = 0.0, uxx = 0.0, uxy = 0.0, uyy = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        cxx += jx[a] * (ppx[a] + wx[a]); cxy += jx[a] * (ppy[a] + wy[a]); cyy += jy[a] * (ppy[a] + wy[a]);
        uxx += jx[a] * wx[a]; uxy += jy[a] * wx[a]; uyy += jy[a] * wy[a];
    }
    cxx = (cxx + uxx) + sxx; cxy = (cxy + uxy) + sxy; cyy = (cyy + uyy) + syy;
    if (!on) return;
    int st = (s_fixed || pc[0] < 0 || pc[1] < 0 || pc[2] < 0) ? JAICOV_PRED_PARTIAL : 0;
    constexpr int NC = CHECK ? JAICOV_PRED_CHECK_COLUMNS : JAICOV_PRED_POINT_COLUMNS;
    double *o = out + (size_t)NC * gi;
    double fin = ((cxx + cxy) + cyy) + (w0 + w1) + (sa + sb);
    double vx = 0.0, vy = 0.0, rho = 0.0;
    if (CHECK) {
        vx = disp[3 * (size_t)gi]; vy = disp[3 * (size_t)gi + 1]; rho = disp[3 * (size_t)gi + 2];
        fin += (vx + vy) + rho;
    }
    if (!isfinite(fin)) {
#pragma unroll
        for (int k = 0; k < NC; k++) o[k] = NAN;
        status[gi] = st | JAICOV_PRED_NOT_FINITE;
        return;
    }
    const double hm = 0.5 * (cxx + cyy), hd = 0.5 * (cxx - cyy), hw = hypot(hd, cxy);
    if (hm - hw < -1e-12 * (cxx + cyy)) st |= JAICOV_PRED_NEGATIVE;
    if (CHECK) {
        const double mxx = vx / sa + cxx, mxy = rho * sqrt(vx * vy) / sa + cxy, myy = vy / sa + cyy;
        const double det = mxx * myy - mxy * mxy;
        double q = NAN;
        if (det > 0.0 && mxx > 0.0) q = ((myy * w0 * w0 - 2.0 * mxy * w0 * w1) + mxx * w1 * w1) / det;
        else st |= JAICOV_PRED_SINGULAR;
        o[0] = w0; o[1] = w1; o[2] = mxx; o[3] = mxy; o[4] = myy; o[5] = q;
        o[6] = q / (2.0 * sa); o[7] = q / (2.0 * sb);
    } else {
        o[0] = -w0; o[1] = -w1; o[2] = cxx; o[3] = cxy; o[4] = cyy;
        o[5] = sqrt(sa * fmax(cxx, 0.0)); o[6] = sqrt(sa * fmax(cyy, 0.0));
        o[7] = sb * sqrt(sa * fmax(hm + hw, 0.0));
        o[8] = sb * sqrt(sa * fmax(hm - hw, 0.0));
        double dir = 0.5 * atan2(2.0 * cxy, cxx - cyy);
        if (dir < 0.0) dir += M_PI;
        if (dir >= M_PI) dir = 0.0;
        o[9] = dir;
    }
    status[gi] = st;
}

// Group g: the members gbegin[g] .. gbegin[g + 1] (caller's order), member k at the sorted position gpos[k].  One wave per workgroup:
// the precondition of the LDS routines of wavealg.h.
__global__ __launch_bounds__(64) void pred_group_kernel(const double *__restrict__ Q, long ld, DevProblem p, const int32_t *__restrict__ img,
                                                        const int32_t *__restrict__ pt, int n, const double *__restrict__ rowsA,
                                                        const double *__restrict__ rowsW, const double *__restrict__ disp,
                                                        const int32_t *__restrict__ gbegin, const int32_t *__restrict__ gpos, double s0,
                                                        double s2post, double *__restrict__ gout, int32_t *__restrict__ gstatus) {
    __shared__ double U[PRED_TRI];
    __shared__ double Jg[JAICOV_PRED_MAX_GROUP][2][KROW];
    __shared__ double dv[PRED_R], Sc[PRED_R], Sv[PRED_R];
    __shared__ int col[JAICOV_PRED_MAX_GROUP][KROW];
    __shared__ int kk[JAICOV_PRED_MAX_GROUP], pos[JAICOV_PRED_MAX_GROUP];
    const int g = blockIdx.x, lane = threadIdx.x;
    const int m0 = wave_uniform(gbegin[g]), m = wave_uniform(gbegin[g + 1]) - m0, n2 = 2 * m;
    auto ix = [n2](int i, int j) { return tri_ix_n(n2, i, j); };
    if (lane < m) {
        const int gi = gpos[m0 + lane];
        const int cam = p.image_camera[img[gi]];
        pos[lane] = gi;
        kk[lane] = 12 + (p.cam_dist_begin[cam + 1] - p.cam_dist_begin[cam]);
    }
    __syncthreads();
    // the members' local columns and rows; a fixed column carries a zero row entry
    int partial = 0;
    for (int t = lane; t < m * KROW; t += 64) {
        const int i = t / KROW, l = t - i * KROW, gi = pos[i];
        const int image = img[gi], cam = p.image_camera[image];
        int c = -1;
        if (l < 3) c = p.point_col[3 * pt[gi] + l];
        else if (l < 6) c = p.io_col[3 * cam + l - 3];
        else if (l < 12) c = p.eo_col[6 * image + l - 6];
        else if (l < kk[i]) c = p.dist_col[p.cam_dist_begin[cam] + l - 12];
        if (l < kk[i] && c < 0) partial = 1;
        col[i][l] = c;
        const double ax = rowsA[(size_t)(2 * l) * n + gi], ay = rowsA[(size_t)(2 * l + 1) * n + gi];
        Jg[i][0][l] = c < 0 ? 0.0 : ax;
        Jg[i][1][l] = c < 0 ? 0.0 : ay;
    }
    if (lane < n2) dv[lane] = rowsW[(size_t)(lane & 1) * n + pos[lane >> 1]];
    __syncthreads();
    int st = wave_uniform(__any(partial) != 0) ? JAICOV_PRED_PARTIAL : 0;
    // M_G block by block: lane t takes the entries e = t, t + 64, .. of Q[cols_i, cols_j] in order, the lanes' sums meet in a butterfly
    for (int i = 0; i < m; i++)
        for (int j = i; j < m; j++) {
            const int kj = kk[j], cnt = kk[i] * kj;
            double xx = 0.0, xy = 0.0, yx = 0.0, yy = 0.0;
            for (int e = lane; e < cnt; e += 64) {
                const int a = e / kj, b = e - a * kj;
                const double q = q_at(Q, ld, col[i][a], col[j][b]);
                const double qx = q * Jg[j][0][b], qy = q * Jg[j][1][b];
                xx += Jg[i][0][a] * qx; xy += Jg[i][0][a] * qy; yx += Jg[i][1][a] * qx; yy += Jg[i][1][a] * qy;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                xx += __shfl_xor(xx, off); xy += __shfl_xor(xy, off); yx += __shfl_xor(yx, off); yy += __shfl_xor(yy, off);
            }
            if (lane == 0) {
                if (i == j) {
                    const double vx = disp[3 * (size_t)pos[i]], vy = disp[3 * (size_t)pos[i] + 1], rho = disp[3 * (size_t)pos[i] + 2];
                    U[ix(2 * i, 2 * i)] = vx / s0 + xx;
                    U[ix(2 * i, 2 * i + 1)] = rho * sqrt(vx * vy) / s0 + xy;
                    U[ix(2 * i + 1, 2 * i + 1)] = vy / s0 + yy;
                } else {
                    U[ix(2 * i, 2 * j)] = xx; U[ix(2 * i, 2 * j + 1)] = xy;
                    U[ix(2 * i + 1, 2 * j)] = yx; U[ix(2 * i + 1, 2 * j + 1)] = yy;
                }
            }
        }
    __syncthreads();
    auto fail = [&](int bit) {
        if (lane < 3) gout[(size_t)JAICOV_PRED_GROUP_COLUMNS * g + lane] = NAN;
        if (lane == 3) gout[(size_t)JAICOV_PRED_GROUP_COLUMNS * g + 3] = (double)n2;
        if (lane == 0) gstatus[g] = st | bit;
    };
    // NaN in z unless every value is finite
    double z = (s0 + s2post) * 0.0;
    if (lane < n2) z += dv[lane] * 0.0;
    wave_equilibrate_lds(n2, U, Sc, Sv, z, lane);
    if (wave_uniform(__any(!(z == 0.0)) != 0)) { fail(JAICOV_PRED_NOT_FINITE); return; }
    if (wave_chol_lds(n2, U, lane) != WAVE_OK) { fail(JAICOV_PRED_SINGULAR); return; }
    // q_G = |U^-T (S d)|^2, the squares added in row order
    double zz[1] = {lane < n2 ? (Sc[lane] * Sv[lane]) * dv[lane] : 0.0};
    wave_forward_lds<1>(n2, U, zz, lane);
    __syncthreads();
    if (lane < n2) dv[lane] = zz[0];
    __syncthreads();
    double q = 0.0;
    for (int r = 0; r < n2; r++) q += dv[r] * dv[r];
    if (lane == 0) {
        double *o = gout + (size_t)JAICOV_PRED_GROUP_COLUMNS * g;
        o[0] = q; o[1] = q / ((double)n2 * s0); o[2] = q / ((double)n2 * s2post); o[3] = (double)n2;
        gstatus[g] = st;
    }
}

// the image points of the problem as sorted keys, read from the device tables once per engine
static int pred_observed(const QView &v, PredictState *st) {
    if (st->have_observed) return JAICOV_OK;
    const size_t n_ip = (size_t)v.p->n_ip;
    std::vector<int32_t> hi(n_ip), hp(n_ip);
    TRY(q_download(v, {{hi.data(), v.p->ip_image, n_ip * sizeof(int32_t)}, {hp.data(), v.p->ip_point, n_ip * sizeof(int32_t)}}));
    st->observed.resize(n_ip);
    for (size_t k = 0; k < n_ip; k++) st->observed[k] = (uint64_t)(uint32_t)hi[k] << 32 | (uint32_t)hp[k];
    std::sort(st->observed.begin(), st->observed.end());
    st->have_observed = true;
    return JAICOV_OK;
}

static int pred_run(jaicov_engine *e, bool check, double sa, double sb, const int32_t *images, const int32_t *points, const double *xy,
                    const double *disp, int32_t n, const int32_t *group_begin, int32_t n_groups, double *out, int32_t *status, double *gout,
                    int32_t *gstatus) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    TRY(q_guard(v, "image predictions on a sharded engine",
                "image predictions need all of Qxx on the device: solve with invert FULL or FULL_EXPANDED first"));
    const DevProblem &p = *v.p;
    const char *what = check ? "check measurements: NULL argument, a negative count or a malformed group table"
                             : "image predictions: NULL argument or a negative count";
    if (n < 0 || n_groups < 0) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, what);
    if (n > 0 && (!images || !points || !out || !status || (check && (!xy || !disp)))) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, what);
    if (n_groups > 0 && (!group_begin || !gout || !gstatus)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, what);
    if (check) {
        if (!(sb > 0.0) || !std::isfinite(sb)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "check measurements: sigma2_post must be positive");
    } else if (!(sa >= 0.0) || !(sb >= 0.0)) {
        FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "image predictions: sigma2 and k2 must not be negative");
    }
    for (int i = 0; i < n; i++)
        if (images[i] < 0 || images[i] >= p.n_images || points[i] < 0 || points[i] >= p.n_points)
            FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "image predictions: image or point index out of range");
    if (check && !dispersions_ok(disp, n)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "check measurements: var must be positive and |rho| below 1");
    if (n_groups > 0) {
        if (group_begin[0] != 0 || group_begin[n_groups] != n) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "check measurements: group_begin must run from 0 to n");
        for (int g = 0; g < n_groups; g++) {
            const long m = (long)group_begin[g + 1] - group_begin[g];
            if (m < 1 || m > JAICOV_PRED_MAX_GROUP) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "check measurements: a group holds 1 .. 32 pairs");
        }
    }
    if (n == 0) return JAICOV_OK;
    HIPE(*v.err, hipSetDevice(v.device));
    PredictState *st = q_state(v.slot->pred);
    TRY(pred_observed(v, st));

    // a stable counting sort by image: order[s] = the caller's index of sorted position s, inv its inverse
    std::vector<int32_t> begin((size_t)p.n_images + 1, 0), order(n), inv(n);
    for (int i = 0; i < n; i++) begin[(size_t)images[i] + 1]++;
    for (int k = 0; k < p.n_images; k++) begin[k + 1] += begin[k];
    {
        std::vector<int32_t> next(begin.begin(), begin.end() - 1);
        for (int i = 0; i < n; i++) { const int s = next[images[i]]++; order[s] = i; inv[i] = s; }
    }
    size_t W = 0;
    for (int k = 0; k < p.n_images; k++) W += (size_t)(begin[k + 1] - begin[k] + PRED_WG - 1) / PRED_WG;
    const size_t G = (size_t)n_groups, N = (size_t)n;
    const size_t o_pt = N, o_first = 2 * N, o_count = o_first + W, o_gbegin = o_count + W, o_gpos = o_gbegin + G + 1, n_up = o_gpos + N,
                 o_status = n_up, o_gstatus = o_status + N, n_tab = o_gstatus + G;
    std::vector<int32_t> tab(n_up, 0);
    for (int s = 0; s < n; s++) { tab[s] = images[order[s]]; tab[o_pt + s] = points[order[s]]; }
    {
        size_t w = 0;
        for (int k = 0; k < p.n_images; k++)
            for (int s = begin[k]; s < begin[k + 1]; s += PRED_WG, w++) {
                tab[o_first + w] = s;
                tab[o_count + w] = std::min(PRED_WG, begin[k + 1] - s);
            }
    }
    for (size_t g = 0; g <= G; g++) tab[o_gbegin + g] = G ? group_begin[g] : 0;
    for (int i = 0; i < n; i++) tab[o_gpos + i] = inv[i];
    const int NC = check ? JAICOV_PRED_CHECK_COLUMNS : JAICOV_PRED_POINT_COLUMNS;
    PairRows pr(N);
    HIPE(*v.err, st->tab.reserve(n_tab));
    HIPE(*v.err, st->rows.reserve(pr.size));
    HIPE(*v.err, st->out.reserve((size_t)NC * N + JAICOV_PRED_GROUP_COLUMNS * G));
    int32_t *d_tab = st->tab.get();
    double *d_out = st->out.get(), *d_gout = d_out + (size_t)NC * N;
    pr.bind(st->rows.get());
    HIPE(*v.err, hipMemcpyAsync(d_tab, tab.data(), n_up * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
    // the rows are zeroed first: rows_kernel writes no column behind the camera's coefficients; x = y = 0 for a prediction
    HIPE(*v.err, hipMemsetAsync(pr.J, 0, pr.o_disp * sizeof(double), v.stream));
    HIPE(*v.err, pr.stage(v.stream, xy, disp, order.data()));
    QTimer<4> timer(v.stream);
    HIPE(*v.err, timer.arm(st->timing));
    HIPE(*v.err, timer.mark(0));
    HIPE(*v.err, pr.rows(v.stream, pr.problem(p, d_tab, d_tab + o_pt), v.d_vals));
    HIPE(*v.err, timer.mark(1));
    if (check)
        hipLaunchKernelGGL(pred_cov_kernel<true>, dim3((unsigned)W), dim3(PRED_WG), 0, v.stream, v.Q, v.ld, p, d_tab, d_tab + o_pt, d_tab + o_first,
                           d_tab + o_count, n, pr.J, pr.w, pr.disp, sa, sb, d_out, d_tab + o_status);
    else
        hipLaunchKernelGGL(pred_cov_kernel<false>, dim3((unsigned)W), dim3(PRED_WG), 0, v.stream, v.Q, v.ld, p, d_tab, d_tab + o_pt, d_tab + o_first,
                           d_tab + o_count, n, pr.J, pr.w, pr.disp, sa, sb, d_out, d_tab + o_status);
    HIPE(*v.err, hipGetLastError());
    HIPE(*v.err, timer.mark(2));
    if (G > 0) {
        hipLaunchKernelGGL(pred_group_kernel, dim3((unsigned)G), dim3(64), 0, v.stream, v.Q, v.ld, p, d_tab, d_tab + o_pt, n, pr.J, pr.w,
                           pr.disp, d_tab + o_gbegin, d_tab + o_gpos, sa, sb, d_gout, d_tab + o_gstatus);
        HIPE(*v.err, hipGetLastError());
    }
    HIPE(*v.err, timer.mark(3));
    std::vector<double> h_out((size_t)NC * N), h_gout(JAICOV_PRED_GROUP_COLUMNS * G);
    std::vector<int32_t> h_status(N), h_gstatus(G);
    TRY(q_download(v, {{h_out.data(), d_out, h_out.size() * sizeof(double)},
                       {h_status.data(), d_tab + o_status, N * sizeof(int32_t)},
                       {h_gout.data(), d_gout, h_gout.size() * sizeof(double)},
                       {h_gstatus.data(), d_tab + o_gstatus, G * sizeof(int32_t)}}));
    HIPE(*v.err, timer.read(st->ms));
    // back into the caller's order, with the one bit the host knows
    for (int i = 0; i < n; i++) {
        const size_t s = (size_t)inv[i];
        std::copy(h_out.begin() + NC * s, h_out.begin() + NC * (s + 1), out + (size_t)NC * i);
        const uint64_t key = (uint64_t)(uint32_t)images[i] << 32 | (uint32_t)points[i];
        status[i] = h_status[s] | (std::binary_search(st->observed.begin(), st->observed.end(), key) ? JAICOV_PRED_OBSERVED : 0);
    }
    std::copy(h_gout.begin(), h_gout.end(), gout);
    std::copy(h_gstatus.begin(), h_gstatus.end(), gstatus);
    return JAICOV_OK;
}

}  // namespace jaicov

using namespace jaicov;

extern "C" int jaicov_pred_points(jaicov_engine *e, double sigma2, double k2, const int32_t *images, const int32_t *points, int32_t n, double *out,
                                  int32_t *status) {
    return pred_run(e, false, sigma2, k2, images, points, nullptr, nullptr, n, nullptr, 0, out, status, nullptr, nullptr);
}

extern "C" int jaicov_pred_check(jaicov_engine *e, double sigma2_post, const int32_t *images, const int32_t *points, const double *xy,
                                 const double *disp, int32_t n, const int32_t *group_begin, int32_t n_groups, double *out, int32_t *status,
                                 double *gout, int32_t *gstatus) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    return pred_run(e, true, q_view(e).sigma2, sigma2_post, images, points, xy, disp, n, group_begin, n_groups, out, status, gout, gstatus);
}

// The hook of scripts/predict_bench.py: on != 0 makes the following calls time their kernels by events on the engine's stream;
// ms[0 .. 2]: what the rows, pred_cov_kernel and pred_group_kernel of the last call took.
extern "C" int jaicov_debug_pred_timing(jaicov_engine *e, int on, float *ms) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    PredictState *st = q_state(q_view(e).slot->pred);
    st->timing = on != 0;
    if (ms)
        for (int k = 0; k < 3; k++) ms[k] = st->ms[k];
    return JAICOV_OK;
}
