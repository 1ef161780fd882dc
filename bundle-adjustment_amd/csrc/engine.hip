// C ABI of the normal-equation engine (include/jaicov_neq.h): host control + small glue kernels.  gfx950 only.
// There is NO CPU fallback here: every entry point fails with JAICOV_ERR_NO_DEVICE / JAICOV_ERR_DEVICE when HIP is
// unusable.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/jaicov_dense.h"
#include "../../include/jaicov_neq.h"
#include "ba_kernels.h"
#include "batchinv.h"
#include "create_plan.h"
#include "datum.h"
#include "dense.h"
#include "devbuf.h"
#include "forms.h"
#include "predict.h"
#include "newpoints.h"
#include "vce.h"
#include "calibration.h"
#include "gemm_f64.h"
#include "parameters.h"
#include "precision.h"
#include "qview.h"
#include "reliability.h"
#include "status.h"
#include "transform.h"

namespace jaicov {
hipError_t launch_rows(hipStream_t, const DevProblem &, const double *, int, int, double *, double *);
hipError_t launch_assemble_small(hipStream_t, const DevProblem &, const int32_t *, const int32_t *, int, const double *,
                                 const double *, double, double *, double *);
hipError_t launch_assemble_blocks(hipStream_t, const DevProblem &, const int32_t *, int, int, const int32_t *, int,
                                  const double *, const double *, double *, double, double *, double *, const PPGather &,
                                  const SchurBufs &, double *, hipStream_t, hipEvent_t, hipEvent_t);
hipError_t launch_schur_backsub(hipStream_t, const DevProblem &, const int32_t *, int, const double *, const double *,
                                const double *, double *);
hipError_t launch_shared_groups(hipStream_t, const DevProblem &, const double *, double, double *, double *,
                                const double *, double *);
hipError_t launch_schur_expand_f(hipStream_t, const DevProblem &, const int32_t *, int, const double *, const double *, const double *,
                                 const double *, double *, long);
hipError_t launch_omega(hipStream_t, const DevProblem &, const uint8_t *, int, int, const int32_t *, int, int,
                        const double *, const double *, const double *, double, double *, double *);
struct RefineBorder { double kappa[7]; double rk[7]; };
hipError_t launch_residual_dd(hipStream_t, const double *, long, int, int, int, const double *, const double *, const double *,
                              const double *, const double *, long, const RefineBorder &, double *, double *);
}  // namespace jaicov
using namespace jaicov;

static const double EPS53 = 1.1102230246251565e-16;   // Constant.EPS = 2^-53 (Constant.java:68-75)

// ---------------------------------------------------------------------------------------------------------------
// glue kernels
// ---------------------------------------------------------------------------------------------------------------
// BA:814-828: damping on unknown columns, then V = 1/sqrt(diag) where diag > EPS (V = 1 on the border, whose
// diagonal is zero); padded rows get V = 1
__global__ void damp_and_precond_kernel(double *N, long ld, int U, int Upad, int d, double lambda, double *V,
                                        const double *diagcorr) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Upad) return;
    double v = 1.0;
    if (c >= d && c < U) {
        double diag = N[(long)c * ld + c];
        if (lambda > 0.0) {
            // the reference damps the diagonal of the UNREDUCED normal matrix; diagcorr = what the EO elimination took
            diag += lambda * (diag + (diagcorr ? diagcorr[c] : 0.0));
            N[(long)c * ld + c] = diag;
        }
        v = diag > 1.1102230246251565e-16 ? 1.0 / sqrt(diag) : 1.0;
    }
    V[c] = v;
}

// zero the lower triangle (row r: columns 0 .. r, rounded up to 4) of the leading `rows` rows; grid (ceil(rows/1024), rows)
// rows skip_lo..skip_hi (the point rows the gather stores itself, PPGather::plain): only the columns before skip_lo
__global__ __launch_bounds__(256) void zero_lower_kernel(double *__restrict__ N, long ld, int rows, int skip_lo, int skip_hi, int row0) {
    const int r = row0 + blockIdx.y, c = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (c > r || r >= rows) return;
    if (r >= skip_lo && r <= skip_hi) {
        if (c >= skip_lo) return;
        if (c + 4 > skip_lo) {           // the quad straddles the first stored column
            for (int k = c; k < skip_lo; k++) N[(long)r * ld + k] = 0.0;
            return;
        }
    }
    *reinterpret_cast<d4_t *>(N + (long)r * ld + c) = (d4_t){0.0, 0.0, 0.0, 0.0};
}

// M = V N V + Bh' Bh on the unknown block (lower part), identity on border and padding.  Bh: [d][bstride]
__global__ __launch_bounds__(256) void scale_copy_kernel(const double *__restrict__ N, long ldN, double *__restrict__ M,
                                                         long ld, int U, int Upad, int d, const double *__restrict__ V,
                                                         const double *__restrict__ Bh, int bstride, int c_begin, int c_end) {
    const int j = c_begin + blockIdx.x * 256 + threadIdx.x;   // columns [c_begin, c_end)
    const int i = blockIdx.y;
    if (j > i || j >= c_end) return;
    double v;
    if (i < d || i >= U || j < d) v = (i == j) ? 1.0 : 0.0;
    else {
        v = V[i] * N[(long)i * ldN + j] * V[j];
        for (int a = 0; a < d; a++) v += Bh[(long)a * bstride + i] * Bh[(long)a * bstride + j];
    }
    M[(long)i * ld + j] = v;
}

__global__ void scale_vec_kernel(const double *n, const double *V, double *out, int U, int Upad, int d) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Upad) return;
    out[c] = (c >= d && c < U) ? V[c] * n[c] : 0.0;
}

// final cofactor: Qxx[i][j] = V_i V_j (Q[i][j] - sum_a G[a][i] H[a][j]) on the unknown block, border from F, E.
// G: [d][gs]; H, F: [d][Upad]; E: [d][d].  Lower part (j <= i) of the leading `order` rows only.
__global__ __launch_bounds__(256) void qfix_kernel(double *__restrict__ Q, long ld, int U, int Upad, int d,
                                                   const double *__restrict__ V, const double *__restrict__ G, long gs,
                                                   const double *__restrict__ H, const double *__restrict__ F,
                                                   const double *__restrict__ E, int order) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j > i || j >= order) return;
    double v;
    if (i >= U) v = 0.0;
    else if (i < d) v = E[i * d + j];
    else if (j < d) v = F[(long)j * Upad + i];
    else {
        v = Q[(long)i * ld + j];
        for (int a = 0; a < d; a++) v -= G[(long)a * gs + i] * H[(long)a * Upad + j];
        v *= V[i] * V[j];
    }
    Q[(long)i * ld + j] = v;
}

// Full cofactor matrix from the inverse of the EO-reduced system (JAICOV_INVERT_FULL_EXPANDED):
//   rows / columns < e0        Qr (the reduced inverse, final: unscaled, border included)
//   EO row e0 + r, column < e0   T1[r][c] = -(F Q_RR)[r][c]
//   EO row, EO column            T2 = -(T1 F') (lower) + N_EE^-1 on the 6 x 6 diagonal blocks, N_EE^-1 = L_E^-T L_E^-1
// lower part (j <= i) of the leading U rows of Qf.
__global__ __launch_bounds__(256) void expand_cofactor_kernel(double *__restrict__ Qf, long ldf, int U, int e0,
                                                              const double *__restrict__ Qr, long ldr,
                                                              const double *__restrict__ T1, long ld1,
                                                              const double *__restrict__ T2, long ld2,
                                                              const double *__restrict__ Linv) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j > i || i >= U) return;
    double v;
    if (i < e0) v = Qr[(long)i * ldr + j];
    else if (j < e0) v = T1[(long)(i - e0) * ld1 + j];
    else {
        const int ri = i - e0, rj = j - e0;
        v = T2[(long)ri * ld2 + rj];
        if (ri / 6 == rj / 6) {
            const double *Li = Linv + (long)(ri / 6) * 36;
            const int a = ri % 6, b = rj % 6;
            for (int m = a > b ? a : b; m < 6; m++) v += Li[6 * m + a] * Li[6 * m + b];
        }
    }
    Qf[(long)i * ldf + j] = v;
}

// row-major lower square <-> packed ('U' column-major == row-major lower packed)
__global__ __launch_bounds__(256) void pack_kernel(const double *__restrict__ M, long ld, int U, double *__restrict__ ap) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j > i || i >= U) return;
    ap[(size_t)i * (i + 1) / 2 + j] = M[(long)i * ld + j];
}
__global__ __launch_bounds__(256) void unpack_kernel(const double *__restrict__ ap, long ld, int U, double *__restrict__ M) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j > i || i >= U) return;
    M[(long)i * ld + j] = ap[(size_t)i * (i + 1) / 2 + j];
}
__global__ void gather_sub_kernel(const double *__restrict__ Q, long ld, const int32_t *idx, int k, double *out, double scale) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k * k) return;
    const int a = t / k, b = t - a * k;
    const int i = idx[a], j = idx[b];
    out[t] = scale * (i >= j ? Q[(long)i * ld + j] : Q[(long)j * ld + i]);
}
// dense dispersion (row-major m x m) -> padded lower square with identity padding
// perm (optional): engine point position -> caller's point position inside the block (rows 2q, 2q+1 move together)
__global__ void load_disp_kernel(const double *__restrict__ D, int m, double *__restrict__ L, long ld, int mp,
                                 const int32_t *__restrict__ perm) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= mp) return;
    double v = (i == j) ? 1.0 : 0.0;
    if (i < m && j < m) {
        const int si = perm ? 2 * perm[i >> 1] + (i & 1) : i, sj = perm ? 2 * perm[j >> 1] + (j & 1) : j;
        v = D[(long)si * m + sj];
    }
    L[(long)i * ld + j] = v;
}
__global__ void store_inv_kernel(const double *__restrict__ Q, long ld, int m, double *__restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= m) return;
    out[(long)i * m + j] = i >= j ? Q[(long)i * ld + j] : Q[(long)j * ld + i];
}

struct jaicov_engine {
    std::string err = "";
    int device = 0;
    // The engine's stream.  Declared before, so destroyed after, every member that synchronises or frees on it: both solvers, dm, the
    // bag, the events and the states below.  jaicov_neq_destroy relies on that order.
    StreamLease stream_lease;
    hipStream_t stream = nullptr;   // ... as every launch names it
    int flow_retries = 0;      // dataflow factorisations that were abandoned and repeated (solve)
    DevBuf<double> ns_work;    // three squares of the inverse's Newton-Schulz step (orders <= 8192, option inverse_refinement)
    int refine_steps = 1;      // iterative refinement of the step (refine.hip): engine option `refinement` / JAICOV_REFINE
    double *d_Braw = nullptr, *d_ref = nullptr;   // unscaled datum rows; rhs | tmp | delta
    DevBuf<double> refP;       // partial-sum table of the refinement's residual
    double last_refine_correction = 0.0;   // max |correction| / max |dx| of the last refinement step (diagnostics)
    DevEvent ev_fork, ev_join;      // assembly: camera-side kernels on a side stream (assemble.hip)
    DevProblem p{};
    DevBag bag;                     // every device buffer that lives as long as the engine; the raw pointers below and in p, pp, sb are views of it
    // host copies
    jaicov_engine_options opts{};
    int U = 0, Upad = 0, d = 0, datum_flags = 0, n_slots = 0;
    std::vector<int32_t> h_slot_col;        // column of every slot [3P | 3C | n_dist | 6I]
    std::vector<uint8_t> h_point_datum;
    std::vector<double> h_vals, h_V;
    int n_points = 0;
    // image range handled by this engine
    int ip0 = 0, ip_count = 0;
    // assembly tables
    int n_seg = 0, n_blk_list = 0, max_m = 0, n_blk_ip = 0;
    int32_t *d_seg_begin = nullptr, *d_seg_end = nullptr, *d_blk_list = nullptr, *d_blk_ip_list = nullptr;
    uint8_t *d_in_block = nullptr;
    PPGather pp;
    // EO pre-elimination (schur.hip)
    bool schur_ok = false, schur_active = false;
    DenseMode dm;                    // assembly_mode = 1
    bool dense_mode = false;
    double dm_flops_per_pass = 0.0, dm_stat_passes = 0.0, dm_stat_ms = 0.0, dm_stat_flops = 0.0;
    int inverse_mode_next = 0;       // JAICOV_INVERT_* announced for the solve after the next build
    bool all_images = true;          // this engine accumulates every image (not a shard): FULL_EXPANDED needs every image's F band and L_E ...
    DevBuf<double> expF;             // ... a shard's caller sums them over the ranks: [F (6 images padded x reduced order padded) | Linv (36 per image)]
    size_t expF_len = 0;             // the length in use (the allocation only grows)
    bool exp_ready = false;          // d_expF belongs to the system accumulated last and has been handed out (jaicov_neq_expansion_buffer)
    std::vector<int> h_blk_images;   // image of every block handled by this engine
    std::vector<int32_t> h_caller_block; // internal image block -> the caller's block index (-1: an ordinary image served as a block); empty: identity
    std::vector<int32_t> h_perm_local;   // per image point of a dense block: engine position -> caller's position inside the block (empty: identity)
    std::vector<int64_t> h_blk_w_off;    // offset of every image block's weight in p.blk_w
    std::vector<int32_t> h_blk_ip_begin; // blk_ip_begin of the effective description (CreatePlan::D)
    std::vector<uint8_t> h_blk_mine;     // this engine holds the block's weight
    std::vector<int32_t> ip_old2new; // empty, or: engine position of the caller's observation (dense blocks are column-sorted)
    int e0 = 0;                   // first EO column == order of the reduced system
    SchurBufs sb;
    double *d_xE = nullptr;
    DenseSolver solverS;
    bool solverS_ready = false;
    double lambda_acc = 0.0;
    // device state
    double *d_vals = nullptr, *d_rowsA = nullptr, *d_rowsW = nullptr, *d_T = nullptr, *d_vbuf = nullptr;
    double *d_N = nullptr, *d_n = nullptr;          // one allocation: N (Upad x Upad) followed by n (Upad)
    double *d_packed = nullptr;                     // reduce buffer: packed N (U(U+1)/2) + n (U)
    double *d_V = nullptr, *d_B = nullptr, *d_dx = nullptr;
    double *d_cc_partial = nullptr;                 // [blocks of this engine][16 parts][KC_MAX (KC_MAX + 1)] partial camera blocks (assemble.hip)
    double *d_omega = nullptr, *d_G = nullptr, *d_H = nullptr, *d_F = nullptr, *d_E = nullptr;
    int32_t *d_idx = nullptr;
    DenseSolver solver;
    enum { ST_NEW, ST_PARAMS, ST_ACCUMULATED, ST_BUILT, ST_SOLVED } state = ST_NEW;
    bool rows_valid = false, reduced = false;
    bool deterministic = true;   // engine option `deterministic` (default on): fixed summation order in the assembly of the image groups
    std::atomic<int> cancel{0};  // BundleAdjustment.interrupt() (BA:1455): polled by estimate() where the reference polls (BA:240, 320)
    bool sim_built = false;      // the system at hand was built with simulation != 0: the right-hand side is zero for ALL unknowns (BA:830-831)
    double lambda_used = 0.0;
    std::vector<double> hB;      // [d][Upad] datum rows (unscaled), host
    double timings[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double create_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // jaicov_neq_create: [0] whole call, [1] host time in the dispersion uploads, [2] dispersions -> weights (wall),
                                                      // [3] validation + tables (the plan, create_plan.h) + structure upload, [4] work buffers + full-order solver, [5] EO pre-elimination buffers + reduced solver
    DevEvent ev[10];
    bool pp_plain_ok = false;   // the point x point gather may store its strips (see PPGather::plain)
    DevEvent ev_first, ev_all;   // solve(): first panel's columns / whole matrix copied into the solver
    DevEvent ev_r0, ev_r1;       // solve(): device part of a refinement step
    const double *d_ll_diag = nullptr;                 // [2 n_ip + n_dg_rows]: diag(D) of every image coordinate (engine order) and direct row
    double sigma2_acc = 0.0;                           // sigma0^2 of the last accumulate
    // What an inverting solve leaves: Solve::finish records all of it at once and withdraws the S of an earlier datum transformation
    // with it; accumulate withdraws `valid` alone (the matrix's buffer is the next factorisation's to use), the rest waits for the
    // next inverting solve to overwrite it.
    struct Cofactor {
        bool valid = false;
        int order = 0;                   // U, or e0 for the inverse of the EO-reduced system
        bool reduced = false;            // ... which lies in solverS.Q, every other one in solver.Q
        double sigma2 = 0.0, lambda = 0.0;   // sigma0^2 and damping of the build whose system the matrix inverts
        std::vector<double> vals;        // slot values of that build: the datum rows of jaicov_datum_transform (datum.hip)
    } q;
    DenseSolver &q_solver() { return q.reduced ? solverS : solver; }   // the solver that holds the matrix
    // What the consumers of the matrix keep (qview.h).  A result of jaicov_xform_run or jaicov_rel_run outlives a later inverting
    // solve; only the datum state is invalidated by one.  Their buffers free on the stream: they stay declared after stream_lease.
    jaicov::QSlots slot;
};

template <typename T, typename P>      // P: T or const T
static int upload(jaicov_engine *e, const T *src, size_t count, P **dst) {
    *dst = nullptr;
    if (count == 0) return JAICOV_OK;
    T *ptr = nullptr;
    HIPE(e->err, e->bag.alloc(&ptr, count));
    HIPE(e->err, hipMemcpy(ptr, src, count * sizeof(T), hipMemcpyHostToDevice));
    *dst = ptr;
    return JAICOV_OK;
}
template <typename T>
static int dalloc(jaicov_engine *e, size_t count, T **dst, bool zero = false) {
    if (count == 0) count = 1;
    HIPE(e->err, e->bag.alloc(dst, count));
    if (zero) HIPE(e->err, hipMemset(*dst, 0, count * sizeof(T)));
    return JAICOV_OK;
}

static int check_device(std::string &err) {
    int count = 0;
    hipError_t r = hipGetDeviceCount(&count);
    if (r != hipSuccess || count <= 0) {
        err = "no HIP device available (this engine has no CPU fallback)";
        return JAICOV_ERR_NO_DEVICE;
    }
    return JAICOV_OK;
}

// ---- dense dispersions -> weights, all groups of one padded order together (batchinv.hip) ------------------------------------
struct DispItem { const double *host; double *dst; const int32_t *perm; int m; };   // dst, perm: device pointers
struct DispDesc { const double *src; double *dst; const int32_t *perm; int m; int pad; };
// dense dispersion (row-major m x m, in the staging buffer) -> padded square with identity padding, in the engine's point order
// perm (optional): engine point position -> caller's point position inside the block (rows 2q, 2q+1 move together)
__global__ void load_disp_batched_kernel(const DispDesc *__restrict__ desc, double *__restrict__ Lb, double *__restrict__ Db, long ld, long msz, int mp) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= mp) return;
    const DispDesc dd = desc[blockIdx.z];
    double v = (i == j) ? 1.0 : 0.0;
    if (i < dd.m && j < dd.m) {
        const int si = dd.perm ? 2 * dd.perm[i >> 1] + (i & 1) : i, sj = dd.perm ? 2 * dd.perm[j >> 1] + (j & 1) : j;
        // the LOWER triangle of the caller's array, mirrored (dpptrf / the per-matrix path of rounds 1-3 read nothing else: a caller that fills
        // one triangle only, or a slightly asymmetric matrix, must not reach the Newton-Schulz step as a non-symmetric D)
        v = si >= sj ? dd.src[(long)si * dd.m + sj] : dd.src[(long)sj * dd.m + si];
    }
    Lb[(long)blockIdx.z * msz + (long)i * ld + j] = v;
    if (Db) Db[(long)blockIdx.z * msz + (long)i * ld + j] = v;      // the refinement of the inverse reads the matrix once more
}
__global__ void store_inv_batched_kernel(const DispDesc *__restrict__ desc, const double *__restrict__ Qb, long ld, long msz) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    const DispDesc dd = desc[blockIdx.z];
    if (i >= dd.m || j >= dd.m) return;
    dd.dst[(long)i * dd.m + j] = Qb[(long)blockIdx.z * msz + (long)i * ld + j];
}

// The same weights in compact form (DevProblem::ip_w3): (w00, w01, w11) per image point, nothing else stored -- an ordinary image with m
// rows then costs 1.5 m doubles instead of m^2, and T = inv(D) [A_c | w] two multiplications per entry instead of a dense product.
__global__ void fill_ip_w3_kernel(const double *__restrict__ vx, const double *__restrict__ vy, const double *__restrict__ rho, int n_ip,
                                  double *__restrict__ out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_ip) return;
    const double x = vx[q], y = vy[q], c = rho[q];
    double w00, w01, w11;
    if (c == 0.0) { w00 = 1.0 / x; w01 = 0.0; w11 = 1.0 / y; }
    else {
        const double inv_det = 1.0 / ((1.0 - c * c) * x * y);
        w00 = inv_det * y; w01 = -inv_det * c * sqrt(x * y); w11 = inv_det * x;
    }
    out[3 * (long)q] = w00; out[3 * (long)q + 1] = w01; out[3 * (long)q + 2] = w11;
}

// inv(D) of an ordinary image served as a block: 2 x 2 blocks [[vx, rho s], [rho s, vy]]^-1, s = sqrt(vx vy), on the diagonal
// (PDF:313-319 divided by sigma0^2; rho == 0: 1 / vx, 1 / vy as PDF:308-312), zeros elsewhere.  One workgroup per row.
__global__ void fill_diag_weight_kernel(const double *__restrict__ vx, const double *__restrict__ vy, const double *__restrict__ rho, int ipb, int m,
                                        double *__restrict__ out) {
    const int i = blockIdx.x, q = i >> 1, r = i & 1;
    const double x = vx[ipb + q], y = vy[ipb + q], c = rho[ipb + q];
    double w0, w1;   // entries (i, 2q), (i, 2q + 1)
    if (c == 0.0) { w0 = r == 0 ? 1.0 / x : 0.0; w1 = r == 0 ? 0.0 : 1.0 / y; }
    else {
        const double inv_det = 1.0 / ((1.0 - c * c) * x * y), off = -inv_det * c * sqrt(x * y);
        w0 = r == 0 ? inv_det * y : off;
        w1 = r == 0 ? off : inv_det * x;
    }
    double *o = out + (long)i * m;
    for (int j = threadIdx.x; j < m; j += blockDim.x) o[j] = j == 2 * q ? w0 : (j == 2 * q + 1 ? w1 : 0.0);
}

// DOPG:82-86 for every jointly dispersed group of the problem: items of one padded order are inverted in chunks (one set of
// batched launches per chunk); the upload of chunk c + 1 runs on a copy stream beside the inversion of chunk c.
// Timings (ms) are left in e->create_ms: [1] host time spent in the uploads, [2] everything (wall).
static int invert_dispersions(jaicov_engine *e, std::vector<DispItem> &items) {
    if (items.empty()) return JAICOV_OK;
    const auto t_all = std::chrono::steady_clock::now();
    double up_ms = 0.0;
    std::stable_sort(items.begin(), items.end(), [](const DispItem &a, const DispItem &b) { return (a.m + 127) / 128 < (b.m + 127) / 128; });
    StreamLease copy_lease(jaicov::STREAM_PLAIN);      // (goes back to the pool, synchronised, on every way out; so do the events)
    const hipStream_t cstream = copy_lease.get();
    if (!cstream) FAIL(e->err, JAICOV_ERR_DEVICE, "no stream for the dispersion uploads");
    DevEvent ev_up[2], ev_free[2];
    int status = JAICOV_OK;
    std::string msg;
    for (int b = 0; b < 2 && status == JAICOV_OK; b++)
        if (ev_up[b].create(hipEventDisableTiming) != hipSuccess || ev_free[b].create(hipEventDisableTiming) != hipSuccess) {
            status = JAICOV_ERR_DEVICE; msg = "inversion of the dispersion matrices: no events";
        }
    for (size_t g0 = 0; g0 < items.size() && status == JAICOV_OK;) {
        const int mp = ((items[g0].m + 127) / 128) * 128;
        size_t g1 = g0;
        int mmax = 0;
        while (g1 < items.size() && ((items[g1].m + 127) / 128) * 128 == mp) { mmax = std::max(mmax, items[g1].m); g1++; }
        const int count = (int)(g1 - g0);
        const size_t msz = (size_t)mp * mp, mm = (size_t)mmax * mmax;
        // chunk: <= 64 matrices and <= ~4 GB of workspace (3 squares per matrix, 6 with the refinement) -- 8 chunks at config 4, the first upload (0.5 GB)
        // is the only one that nothing overlaps
        const bool refine = e->opts.dispersion_refinement >= 0;
        int cap = (int)std::max<size_t>(1, std::min<size_t>(64, ((size_t)4 << 30) / ((refine ? 6 : 3) * msz * sizeof(double))));
        cap = std::min(cap, count);
        BatchedSpdInverse bi;             // (its buffers and the bag's are freed at the end of this pass of the loop, both streams synchronised)
        DevBag stage;
        double *d_stage[2] = {nullptr, nullptr};
        DispDesc *d_desc = nullptr;
        std::vector<DispDesc> desc(count);
        hipError_t he = bi.init(e->stream, mp, cap, refine);
        for (int b = 0; b < 2 && he == hipSuccess; b++) he = stage.alloc(&d_stage[b], (size_t)cap * mm);
        if (he == hipSuccess) he = stage.alloc(&d_desc, (size_t)count);
        if (he == hipSuccess) {
            for (int t = 0; t < count; t++) {
                const int c = t / cap, b = c & 1;
                desc[t] = DispDesc{d_stage[b] + (size_t)(t - c * cap) * mm, items[g0 + t].dst, items[g0 + t].perm, items[g0 + t].m, 0};
            }
            he = hipMemcpyAsync(d_desc, desc.data(), (size_t)count * sizeof(DispDesc), hipMemcpyHostToDevice, e->stream);
        }
        for (int c = 0; he == hipSuccess && c * cap < count; c++) {
            const int b = c & 1, first = c * cap, cnt = std::min(cap, count - first);
            if (c >= 2) he = hipStreamWaitEvent(cstream, ev_free[b].get(), 0);      // the load kernel of chunk c - 2 has consumed this buffer
            const auto t_up = std::chrono::steady_clock::now();
            for (int t = 0; t < cnt && he == hipSuccess; t++) {
                const DispItem &it = items[g0 + first + t];
                he = hipMemcpyAsync(d_stage[b] + (size_t)t * mm, it.host, (size_t)it.m * it.m * sizeof(double), hipMemcpyHostToDevice, cstream);
            }
            up_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_up).count();
            if (he == hipSuccess) he = hipEventRecord(ev_up[b].get(), cstream);
            if (he == hipSuccess) he = hipStreamWaitEvent(e->stream, ev_up[b].get(), 0);
            if (he != hipSuccess) break;
            hipLaunchKernelGGL(load_disp_batched_kernel, dim3((mp + 255) / 256, mp, cnt), dim3(256), 0, e->stream, d_desc + first, bi.Lb, bi.refine ? bi.Db : (double *)nullptr, bi.ld, bi.msz, mp);
            he = hipEventRecord(ev_free[b].get(), e->stream);
            if (he == hipSuccess) he = bi.run(cnt);
            if (he != hipSuccess) break;
            hipLaunchKernelGGL(store_inv_batched_kernel, dim3((mmax + 255) / 256, mmax, cnt), dim3(256), 0, e->stream, d_desc + first, bi.Qb, bi.ld, bi.msz);
        }
        int info = 0;
        if (he == hipSuccess) he = hipMemcpyAsync(&info, bi.d_info, sizeof(int), hipMemcpyDeviceToHost, e->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
        hipStreamSynchronize(cstream);
        if (he != hipSuccess) { status = he == hipErrorOutOfMemory ? JAICOV_ERR_OUT_OF_MEMORY : JAICOV_ERR_DEVICE; msg = std::string("inversion of the dispersion matrices: ") + hipGetErrorString(he); }
        else if (info != 0) { status = JAICOV_ERR_SINGULAR; msg = "dispersion matrix is not positive definite (MatrixNotSPDException, DOPG:85-86)"; }
        g0 = g1;
    }
    e->create_ms[1] = up_ms;
    e->create_ms[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_all).count();
    if (status != JAICOV_OK) FAIL(e->err, status, msg);
    return JAICOV_OK;
}

extern "C" int jaicov_neq_abi_version(void) { return JAICOV_NEQ_ABI_VERSION; }

extern "C" const char *jaicov_neq_last_error(const jaicov_engine *e) { return e ? e->err.c_str() : "null engine"; }

extern "C" void jaicov_neq_destroy(jaicov_engine *e) {
    if (!e) return;
    hipSetDevice(e->device);
    if (e->stream) hipStreamSynchronize(e->stream);
    delete e;      // every member frees what it holds; the stream's lease goes last (see the member)
}

// ---- engine creation, second stage: what happens on the device.  The first stage, every decision and table that needs
//      no device, is the plan (create_plan.h); each function here takes the engine and the finished plan. ---------------------
static int acquire_stream_and_events(jaicov_engine *e) {
    e->stream_lease = StreamLease(jaicov::STREAM_PLAIN);
    e->stream = e->stream_lease.get();
    if (!e->stream) FAIL(e->err, JAICOV_ERR_DEVICE, "no stream");
    for (auto &evt : e->ev) HIPE(e->err, evt.create());
    for (DevEvent *evt : {&e->ev_first, &e->ev_fork, &e->ev_join, &e->ev_all}) HIPE(e->err, evt->create(hipEventDisableTiming));
    HIPE(e->err, e->ev_r0.create());
    HIPE(e->err, e->ev_r1.create());
    return JAICOV_OK;
}

// the sizes and decisions of the plan that the engine's other entry points read
static void adopt_decisions(jaicov_engine *e, const CreatePlan &pl) {
    const jaicov_problem_desc *D = &pl.D;
    e->U = pl.U; e->d = pl.d; e->datum_flags = D->datum_flags; e->Upad = pl.Upad;
    e->n_points = D->n_points; e->n_slots = pl.n_slots;
    e->all_images = pl.ib == 0 && pl.ie == D->n_images;
    e->ip0 = pl.ip0; e->ip_count = pl.ip_count;
    e->max_m = pl.max_m;
    e->n_seg = (int)pl.seg_b.size();
    e->n_blk_list = (int)pl.blk_list.size();
    e->n_blk_ip = (int)pl.blk_ip_list.size();
    e->pp_plain_ok = pl.plain_ok;
    e->dm_flops_per_pass = pl.dm_flops_per_pass;
    DevProblem &p = e->p;
    p.U = pl.U; p.Upad = pl.Upad; p.d = pl.d; p.ld = pl.Upad;
    p.n_points = D->n_points; p.n_cameras = D->n_cameras; p.n_images = D->n_images; p.n_dist = D->n_dist;
    p.n_ip = D->n_image_points; p.n_blocks = D->n_image_blocks; p.n_sb = D->n_scale_bars; p.n_dg = D->n_direct_groups;
    p.n_dg_rows = D->n_direct_rows; p.n_slots = pl.n_slots;
}

static int upload_structure(jaicov_engine *e, const CreatePlan &pl) {
    const jaicov_problem_desc *D = &pl.D;
    DevProblem &p = e->p;
    TRY(upload(e, D->point_col, (size_t)3 * D->n_points, &p.point_col));
    TRY(upload(e, D->io_col, (size_t)3 * D->n_cameras, &p.io_col));
    TRY(upload(e, D->cam_dist_begin, (size_t)D->n_cameras + 1, &p.cam_dist_begin));
    TRY(upload(e, D->dist_kind, (size_t)D->n_dist, &p.dist_kind));
    TRY(upload(e, D->dist_order, (size_t)D->n_dist, &p.dist_order));
    TRY(upload(e, D->dist_col, (size_t)D->n_dist, &p.dist_col));
    TRY(upload(e, D->image_camera, (size_t)D->n_images, &p.image_camera));
    TRY(upload(e, D->eo_col, (size_t)6 * D->n_images, &p.eo_col));
    TRY(upload(e, D->cam_r0, (size_t)D->n_cameras, &p.cam_r0));
    TRY(upload(e, D->ip_image, (size_t)D->n_image_points, &p.ip_image));
    TRY(upload(e, D->ip_point, (size_t)D->n_image_points, &p.ip_point));
    TRY(upload(e, D->ip_x, (size_t)D->n_image_points, &p.ip_x));
    TRY(upload(e, D->ip_y, (size_t)D->n_image_points, &p.ip_y));
    TRY(upload(e, D->ip_var_x, (size_t)D->n_image_points, &p.ip_var_x));
    TRY(upload(e, D->ip_var_y, (size_t)D->n_image_points, &p.ip_var_y));
    TRY(upload(e, D->ip_rho, (size_t)D->n_image_points, &p.ip_rho));
    TRY(upload(e, D->blk_ip_begin, (size_t)D->n_image_blocks + 1, &p.blk_ip_begin));
    TRY(upload(e, pl.blk_w_off.data(), (size_t)D->n_image_blocks, &p.blk_w_offset));
    TRY(upload(e, D->sb_point_a, (size_t)D->n_scale_bars, &p.sb_a));
    TRY(upload(e, D->sb_point_b, (size_t)D->n_scale_bars, &p.sb_b));
    TRY(upload(e, D->sb_length, (size_t)D->n_scale_bars, &p.sb_len));
    TRY(upload(e, D->sb_var, (size_t)D->n_scale_bars, &p.sb_var));
    TRY(upload(e, D->dg_row_begin, (size_t)D->n_direct_groups + 1, &p.dg_row_begin));
    TRY(upload(e, D->dg_slot, (size_t)D->n_direct_rows, &p.dg_slot));
    TRY(upload(e, D->dg_obs, (size_t)D->n_direct_rows, &p.dg_obs));
    TRY(upload(e, D->dg_var, (size_t)D->n_direct_rows, &p.dg_var));
    TRY(upload(e, pl.slot_col.data(), (size_t)pl.n_slots, &p.slot_col));
    TRY(upload(e, pl.seg_b.data(), pl.seg_b.size(), &e->d_seg_begin));
    TRY(upload(e, pl.seg_e.data(), pl.seg_e.size(), &e->d_seg_end));
    TRY(upload(e, pl.blk_list.data(), pl.blk_list.size(), &e->d_blk_list));
    TRY(upload(e, pl.blk_ip_list.data(), pl.blk_ip_list.size(), &e->d_blk_ip_list));
    TRY(upload(e, pl.in_block.data(), pl.in_block.size(), &e->d_in_block));
    if (!pl.gather) return JAICOV_OK;
    // XCD-partitioned block order (assemble.hip): measured no faster (3.24 vs 3.26 ms at 960 columns, slower where the chunks
    // do not divide evenly over eight XCDs) and FETCH_SIZE fell by 6 % only: the partner records are not what the kernel waits for
    e->pp.xcd_map = 0;
    e->pp.cw = pl.cw;
    TRY(upload(e, pl.pt_ip_begin.data(), pl.pt_ip_begin.size(), &e->pp.pt_ip_begin));
    TRY(upload(e, pl.recs.data(), pl.recs.size(), &e->pp.recs));
    TRY(upload(e, pl.ipcol.data(), pl.ipcol.size(), &e->pp.ipcol));
    TRY(upload(e, pl.range.data(), pl.range.size(), &e->pp.range));
    e->pp.det = e->deterministic ? 1 : 0;
    e->pp.cmin = pl.cmin;
    e->pp.n_chunks = pl.n_chunks;
    e->pp.cmax = pl.cmax;
    return JAICOV_OK;
}

// diag(D) of every image coordinate in engine order (the variances, or the diagonal of the block's dispersion), then of every
// directly observed row (dg_var, or the diagonal of the group's dispersion): Q_ll of jaicov_rel_run
static int upload_ll_diag(jaicov_engine *e, const CreatePlan &pl) {
    const jaicov_problem_desc *D = &pl.D;
    std::vector<double> lld(2 * (size_t)D->n_image_points + D->n_direct_rows);
    for (int ip = 0; ip < D->n_image_points; ip++) { lld[2 * (size_t)ip] = D->ip_var_x[ip]; lld[2 * (size_t)ip + 1] = D->ip_var_y[ip]; }
    for (int g : pl.blk_list) {
        if (D->blk_disp_offset[g] < 0) continue;
        const int b = D->blk_ip_begin[g];
        const int64_t m = 2 * (int64_t)(D->blk_ip_begin[g + 1] - b);
        const double *Dg = D->blk_disp + D->blk_disp_offset[g];
        for (int ip = b; ip < D->blk_ip_begin[g + 1]; ip++) {
            const int64_t lp = pl.perm_local.empty() ? ip - b : pl.perm_local[ip];
            for (int c = 0; c < 2; c++) lld[2 * (size_t)ip + c] = Dg[(2 * lp + c) * m + 2 * lp + c];
        }
    }
    for (int g = 0; g < D->n_direct_groups; g++) {
        const int b = D->dg_row_begin[g], m = D->dg_row_begin[g + 1] - b;
        const bool dense = D->dg_disp_offset && D->dg_disp_offset[g] >= 0;
        for (int r = 0; r < m; r++)
            lld[2 * (size_t)D->n_image_points + b + r] = dense ? D->dg_disp[D->dg_disp_offset[g] + (int64_t)r * m + r] : D->dg_var[b + r];
    }
    return upload(e, lld.data(), lld.size(), &e->d_ll_diag);
}

// dense dispersions -> D^-1 on the device (DOPG:82-86: dpptrf + dpptri once, cached); closed-form weights of ordinary images
static int create_weights(jaicov_engine *e, const CreatePlan &pl) {
    const jaicov_problem_desc *D = &pl.D;
    DevProblem &p = e->p;
    double *d_w = nullptr;
    TRY(dalloc(e, (size_t)pl.w_total, &d_w));
    p.blk_w = d_w;
    std::vector<int64_t> dg_w_off(D->n_direct_groups + 1, -1);
    int64_t dg_total = 0;
    if (e->opts.apply_shared)
        for (int g = 0; g < D->n_direct_groups; g++) {
            const int m = D->dg_row_begin[g + 1] - D->dg_row_begin[g];
            if (D->dg_disp_offset && D->dg_disp_offset[g] >= 0 && m > 0) {
                dg_w_off[g] = dg_total;
                dg_total += (int64_t)m * m;
            }
        }
    double *d_dgw = nullptr;
    TRY(dalloc(e, (size_t)dg_total, &d_dgw));
    p.dg_w = d_dgw;
    TRY(upload(e, dg_w_off.data(), (size_t)D->n_direct_groups, &p.dg_w_offset));
    std::vector<DispItem> items;
    const int32_t *d_perm_local = nullptr;
    TRY(upload(e, pl.perm_local.data(), pl.perm_local.size(), &d_perm_local));
    for (int g : pl.blk_list) {
        const int m = 2 * (D->blk_ip_begin[g + 1] - D->blk_ip_begin[g]);
        if (D->blk_disp_offset[g] < 0 && pl.blk_w_off[g] < 0) continue;      // compact form: filled below for all image points at once
        if (D->blk_disp_offset[g] < 0) {      // an ordinary image: inv(D) = diag of 2 x 2 blocks in closed form, engine order (PDF:296-319)
            hipLaunchKernelGGL(fill_diag_weight_kernel, dim3(m), dim3(256), 0, e->stream, p.ip_var_x, p.ip_var_y, p.ip_rho,
                               D->blk_ip_begin[g], m, d_w + pl.blk_w_off[g]);
            continue;
        }
        items.push_back(DispItem{D->blk_disp + D->blk_disp_offset[g], d_w + pl.blk_w_off[g], d_perm_local ? d_perm_local + D->blk_ip_begin[g] : nullptr, m});
    }
    for (int g = 0; g < D->n_direct_groups; g++) {
        if (dg_w_off[g] < 0) continue;
        items.push_back(DispItem{D->dg_disp + D->dg_disp_offset[g], d_dgw + dg_w_off[g], nullptr, D->dg_row_begin[g + 1] - D->dg_row_begin[g]});
    }
    if (pl.compact_blocks) {
        double *d_w3 = nullptr;
        TRY(dalloc(e, (size_t)3 * D->n_image_points, &d_w3));
        hipLaunchKernelGGL(fill_ip_w3_kernel, dim3((D->n_image_points + 255) / 256), dim3(256), 0, e->stream, p.ip_var_x, p.ip_var_y, p.ip_rho,
                           D->n_image_points, d_w3);
        p.ip_w3 = d_w3;
    }
    TRY(invert_dispersions(e, items));
    return upload_ll_diag(e, pl);
}

static int alloc_work_buffers(jaicov_engine *e, const CreatePlan &pl) {
    const size_t sq = (size_t)e->Upad * e->Upad, n_ip = (size_t)std::max(1, pl.D.n_image_points);
    TRY(dalloc(e, (size_t)e->n_slots, &e->d_vals));
    TRY(dalloc(e, 2 * KROW * n_ip, &e->d_rowsA, true));
    TRY(dalloc(e, 2 * n_ip, &e->d_rowsW, true));
    TRY(dalloc(e, 2 * n_ip * KC_LD, &e->d_T));
    TRY(dalloc(e, 2 * n_ip, &e->d_vbuf));
    TRY(dalloc(e, sq + e->Upad, &e->d_N));
    e->d_n = e->d_N + sq;
    TRY(dalloc(e, (size_t)e->Upad, &e->d_V));
    TRY(dalloc(e, (size_t)8 * e->Upad, &e->d_B, true));
    TRY(dalloc(e, (size_t)e->Upad, &e->d_dx, true));
    TRY(dalloc(e, (size_t)8 * e->Upad, &e->d_G, true));
    TRY(dalloc(e, (size_t)8 * e->Upad, &e->d_Braw, true));
    TRY(dalloc(e, (size_t)3 * e->Upad, &e->d_ref, true));
    TRY(dalloc(e, (size_t)8 * e->Upad, &e->d_H, true));
    TRY(dalloc(e, (size_t)8 * e->Upad, &e->d_F, true));
    TRY(dalloc(e, (size_t)64, &e->d_E, true));
    TRY(dalloc(e, (size_t)1, &e->d_omega, true));
    TRY(dalloc(e, (size_t)std::max(1, e->n_blk_list) * 16 * KC_MAX * (KC_MAX + 1), &e->d_cc_partial));
    HIPE(e->err, e->solver.init(e->stream, e->Upad, false, true));
    return JAICOV_OK;
}

// buffers of the EO pre-elimination (schur.hip) and the solver of the reduced system
static int init_elimination(jaicov_engine *e, const CreatePlan &pl) {
    const jaicov_problem_desc *D = &pl.D;
    const size_t n_ip = (size_t)std::max(1, D->n_image_points);
    TRY(dalloc(e, 16 * n_ip, &e->sb.U, true));
    TRY(dalloc(e, 12 * n_ip, &e->sb.Ug, true));   // U again, in the gather's layout
    TRY(dalloc(e, (size_t)36 * D->n_images, &e->sb.Linv, true));
    TRY(dalloc(e, (size_t)6 * SCHUR_GLD * D->n_images, &e->sb.G, true));
    // P' = sigma2 Dinv - U U' is formed inside the point x point gather; a copy in memory (4 GB at config 4) only on request
    e->sb.materialise = assembly_form() == ASSEMBLY_MATERIALISE ? 1 : 0;     // test hook (JAICOV_ASSEMBLY_FORM, assemble.hip)
    if (e->sb.materialise) TRY(dalloc(e, (size_t)std::max<int64_t>(pl.w_total, 1), &e->sb.Pp));
    TRY(dalloc(e, (size_t)6 * D->n_images, &e->d_xE, true));
    if (e->opts.reduced_reference_quirk) TRY(dalloc(e, (size_t)6 * D->n_images, &e->sb.xq, true));
    TRY(dalloc(e, (size_t)1, &e->sb.info, true));
    TRY(dalloc(e, (size_t)e->Upad, &e->sb.diagcorr, true));
    e->schur_ok = true;
    e->e0 = pl.e0;
    // the solver of the reduced system is created here, with its streams, not at the first solve: stream creation
    // order matters when the host also runs RCCL (bench.py: communicator after the engine)
    HIPE(e->err, e->solverS.init(e->stream, ((pl.e0 + 127) / 128) * 128, false, true, &e->solver));      // never at work beside the full-order solver: shares its side streams
    e->solverS_ready = true;
    return JAICOV_OK;
}

// the plan's tables that the engine reads after creation change owner; nothing is copied
static void keep_host_tables(jaicov_engine *e, CreatePlan &pl) {
    e->h_slot_col = std::move(pl.slot_col);
    e->h_point_datum = std::move(pl.point_datum);
    e->h_caller_block = std::move(pl.caller_block);
    e->h_blk_images = std::move(pl.blk_images);
    e->h_perm_local = std::move(pl.perm_local);
    e->h_blk_w_off = std::move(pl.blk_w_off);
    e->h_blk_ip_begin = std::move(pl.blk_ip_begin);
    e->h_blk_mine = std::move(pl.blk_mine);
    e->ip_old2new = std::move(pl.ip_old2new);
    e->h_vals.assign(e->n_slots, 0.0);
    e->h_V.assign(e->Upad, 1.0);
    e->hB.assign((size_t)8 * e->Upad, 0.0);
}

static double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

static int create_impl(jaicov_engine *e, const jaicov_problem_desc *desc) {
    HIPE(e->err, hipSetDevice(e->device));
    e->deterministic = e->opts.deterministic >= 0;      // 0 = default = ON since round 4 (costs 0.3 ms per pass at config 4); < 0: arrival-order sums
    e->refine_steps = e->opts.refinement == 0 ? 1 : (e->opts.refinement < 0 ? 0 : std::min(e->opts.refinement, 4));
    hipDeviceProp_t prop;
    HIPE(e->err, hipGetDeviceProperties(&prop, e->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        FAIL(e->err, JAICOV_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    auto t = std::chrono::steady_clock::now();
    CreatePlan pl;
    if (!build_create_plan(pl, *desc, e->opts, assembly_form())) FAIL(e->err, pl.status, pl.err);
    adopt_decisions(e, pl);
    TRY(acquire_stream_and_events(e));      // a refused description has created nothing on the device
    TRY(upload_structure(e, pl));
    e->create_ms[3] = ms_since(t);
    TRY(create_weights(e, pl));
    t = std::chrono::steady_clock::now();
    TRY(alloc_work_buffers(e, pl));
    e->create_ms[4] = ms_since(t);
    t = std::chrono::steady_clock::now();
    if (pl.dense_mode) {
        HIPE(e->err, e->dm.init(pl.max_m, pl.max_k1, e->n_blk_list, e->opts.assembly_mode == 2));
        e->dense_mode = true;
    } else if (pl.schur_ok)
        TRY(init_elimination(e, pl));
    e->create_ms[5] = ms_since(t);
    keep_host_tables(e, pl);
    HIPE(e->err, hipStreamSynchronize(e->stream));
    return JAICOV_OK;
}

static jaicov_engine_options default_options() {
    jaicov_engine_options o{};
    o.image_begin = o.image_end = -1;
    o.apply_shared = 1;
    return o;
}

extern "C" int jaicov_neq_create(const jaicov_problem_desc *desc, const jaicov_engine_options *opts, jaicov_engine **out) {
    if (!out) return JAICOV_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (!desc || desc->struct_size != sizeof(jaicov_problem_desc)) return JAICOV_ERR_BAD_ARGUMENT;
    std::string err;
    int rc = check_device(err);
    if (rc != JAICOV_OK) return rc;
    if (opts && opts->struct_size != sizeof(jaicov_engine_options)) return JAICOV_ERR_BAD_ARGUMENT;
    jaicov_engine *e = new jaicov_engine();
    e->opts = opts ? *opts : default_options();
    e->device = e->opts.device;
    *out = e;     // returned even on failure so that the caller can read jaicov_neq_last_error(); destroy() frees it
    const auto t0 = std::chrono::steady_clock::now();
    rc = create_impl(e, desc);
    e->create_ms[0] = ms_since(t0);
    return rc;
}

extern "C" size_t jaicov_neq_num_slots(const jaicov_engine *e) { return e ? (size_t)e->n_slots : 0; }
extern "C" size_t jaicov_neq_packed_length(const jaicov_engine *e) { return e ? (size_t)e->U * (e->U + 1) / 2 : 0; }

extern "C" int jaicov_neq_set_parameters(jaicov_engine *e, const double *slots, size_t n) {
    if (!e || !slots || n != (size_t)e->n_slots) return JAICOV_ERR_BAD_ARGUMENT;
    HIPE(e->err, hipSetDevice(e->device));
    memcpy(e->h_vals.data(), slots, n * sizeof(double));
    HIPE(e->err, hipMemcpyAsync(e->d_vals, e->h_vals.data(), n * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    e->rows_valid = false;
    if (e->state == jaicov_engine::ST_NEW) e->state = jaicov_engine::ST_PARAMS;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_get_parameters(jaicov_engine *e, double *slots, size_t n) {
    if (!e || !slots || n != (size_t)e->n_slots) return JAICOV_ERR_BAD_ARGUMENT;
    memcpy(slots, e->h_vals.data(), n * sizeof(double));
    return JAICOV_OK;
}

int jaicov::engine_ensure_rows(jaicov_engine *e) {
    if (e->rows_valid) return JAICOV_OK;
    HIPE(e->err, launch_rows(e->stream, e->p, e->d_vals, e->ip0, e->ip_count, e->d_rowsA, e->d_rowsW));
    e->rows_valid = true;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_accumulate(jaicov_engine *e, double sigma2) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state == jaicov_engine::ST_NEW) FAIL(e->err, JAICOV_ERR_BAD_STATE, "set_parameters first");
    if (!(sigma2 > 0)) FAIL(e->err, JAICOV_ERR_BAD_ARGUMENT, "variance of unit weight must be positive (DOPG:68-69)");
    HIPE(e->err, hipSetDevice(e->device));
    e->reduced = false;          // a packed buffer of an earlier accumulate must not be unpacked over this one
    e->sigma2_acc = sigma2;
    const size_t sq = (size_t)e->Upad * e->Upad;
    HIPE(e->err, hipEventRecord(e->ev[0].get(), e->stream));
    TRY(engine_ensure_rows(e));
    HIPE(e->err, hipEventRecord(e->ev[1].get(), e->stream));
    e->schur_active = e->schur_ok && e->inverse_mode_next != JAICOV_INVERT_FULL;
    // The point x point gather owns every entry of rows cmin..cmax from column cmin on: when it runs before everything
    // else that adds into that region it stores its strips, and the region needs neither zeroing nor reading back.
    const bool plain = e->pp_plain_ok && !e->dense_mode && e->pp.pt_ip_begin != nullptr && e->n_blk_list > 0;
    {   // only the lower triangle of N is ever written or read (nadd, pack, scale_copy); the reduced system has e0 rows
        const int rows = e->schur_active ? std::min(e->Upad, ((e->e0 + 127) / 128) * 128) : e->Upad;
        // three launches, each over the rows and columns that need zeroing only (one launch over the whole square spent 60 us at
        // config 4 dispatching 226 000 workgroups of which 99.9 % returned at once): rows above the stored strips, the stored rows'
        // columns before the first stored column (nothing when the points come first and there is no datum border), rows below
        const int slo = plain ? e->pp.cmin : rows, shi = plain ? e->pp.cmax : -1;
        auto zero_rows = [&](int r0, int r1, int cols) {
            if (r1 > r0 && cols > 0)
                hipLaunchKernelGGL(zero_lower_kernel, dim3((cols + 1023) / 1024, r1 - r0), dim3(256), 0, e->stream, e->d_N, (long)e->Upad, rows, slo, shi, r0);
        };
        zero_rows(0, std::min(slo, rows), std::min(slo, rows));
        if (plain) {
            zero_rows(slo, std::min(shi + 1, rows), slo);
            zero_rows(std::min(shi + 1, rows), rows, rows);
        }
        HIPE(e->err, hipMemsetAsync(e->d_N + sq, 0, (size_t)e->Upad * sizeof(double), e->stream));
    }
    if (!plain)
        HIPE(e->err, launch_assemble_small(e->stream, e->p, e->d_seg_begin, e->d_seg_end, e->n_seg, e->d_rowsA, e->d_rowsW, sigma2, e->d_N, e->d_n));
    SchurBufs sb = e->sb;
    sb.active = e->schur_active;
    sb.lambda = e->lambda_acc;
    if (e->schur_active) {
        HIPE(e->err, hipMemsetAsync(e->sb.info, 0, sizeof(int), e->stream));
        HIPE(e->err, hipMemsetAsync(e->sb.diagcorr, 0, (size_t)e->Upad * sizeof(double), e->stream));
    }
    if (e->dense_mode) {
        float ms = 0.f;
        HIPE(e->err, e->dm.assemble(e->stream, e->p, e->d_blk_list, e->n_blk_list, e->d_rowsA, e->d_rowsW, sigma2, e->d_N, e->d_n,
                               e->solver.profile ? &ms : nullptr));
        if (e->solver.profile) { e->dm_stat_passes += 1.0; e->dm_stat_ms += ms; e->dm_stat_flops += e->dm_flops_per_pass; }
    } else {
        PPGather ppg = e->pp;
        ppg.plain = plain ? 1 : 0;
        ppg.ug = sb.active ? sb.Ug : nullptr;
        HIPE(e->err, launch_assemble_blocks(e->stream, e->p, e->d_blk_list, e->n_blk_list, e->max_m, e->d_blk_ip_list, e->n_blk_ip,
                                       e->d_rowsA, e->d_rowsW, e->d_T, sigma2, e->d_N, e->d_n, ppg, sb, e->d_cc_partial,
                                       e->solver.pstream, e->ev_fork.get(), e->ev_join.get()));   // side stream: the solver's (idle during the assembly)
    }
    if (plain)   // the images outside the dense blocks come after the stores
        HIPE(e->err, launch_assemble_small(e->stream, e->p, e->d_seg_begin, e->d_seg_end, e->n_seg, e->d_rowsA, e->d_rowsW, sigma2, e->d_N, e->d_n));
    if (e->opts.apply_shared) HIPE(e->err, launch_shared_groups(e->stream, e->p, e->d_vals, sigma2, e->d_N, e->d_n, nullptr, nullptr));
    HIPE(e->err, hipEventRecord(e->ev[2].get(), e->stream));
    e->exp_ready = false;            // the expansion buffer of an earlier pass is stale now
    e->state = jaicov_engine::ST_ACCUMULATED;
    e->q.valid = false;
    return JAICOV_OK;
}

// datum rows (BA:493-635) of the point mask at the slot values `vals`: B [d][stride] (columns >= stride are not stored)
static int datum_rows(jaicov_engine *e, const uint8_t *mask, const double *vals, std::vector<double> &hB, int stride) {
    const int d = e->d;
    std::fill(hB.begin(), hB.end(), 0.0);
    if (d == 0) return JAICOV_OK;
    double x0 = 0, y0 = 0, z0 = 0;
    int count = 0;
    for (int pt = 0; pt < e->n_points; pt++) {
        const int32_t *c = &e->h_slot_col[3 * pt];
        if (!mask[pt] || c[0] < 0 || c[1] < 0 || c[2] < 0) continue;
        x0 += vals[3 * pt]; y0 += vals[3 * pt + 1]; z0 += vals[3 * pt + 2];
        count++;
    }
    if (count < 3) FAIL(e->err, JAICOV_ERR_BAD_ARGUMENT, "not enough object points to realise the frame datum (BA:515-516)");
    x0 /= (double)count; y0 /= (double)count; z0 /= (double)count;
    int row = 0;
    const int f = e->datum_flags;
    const int tx = (f & JAICOV_DATUM_TX) ? row++ : -1, ty = (f & JAICOV_DATUM_TY) ? row++ : -1, tz = (f & JAICOV_DATUM_TZ) ? row++ : -1;
    const int rx = (f & JAICOV_DATUM_RX) ? row++ : -1, ry = (f & JAICOV_DATUM_RY) ? row++ : -1, rz = (f & JAICOV_DATUM_RZ) ? row++ : -1;
    const int ms = (f & JAICOV_DATUM_SCALE) ? row++ : -1;
    double norm[7] = {0, 0, 0, 0, 0, 0, 0};
    double sink = 0.0;
    auto B = [&](int r, int c) -> double & { return c < stride ? hB[(size_t)r * stride + c] : sink; };
    for (int pt = 0; pt < e->n_points; pt++) {
        const int32_t *c = &e->h_slot_col[3 * pt];
        if (!mask[pt] || c[0] < 0 || c[1] < 0 || c[2] < 0) continue;
        const double x = vals[3 * pt] - x0, y = vals[3 * pt + 1] - y0, z = vals[3 * pt + 2] - z0;
        if (tx >= 0) { B(tx, c[0]) = 1.0; norm[tx] += 1.0; }
        if (ty >= 0) { B(ty, c[1]) = 1.0; norm[ty] += 1.0; }
        if (tz >= 0) { B(tz, c[2]) = 1.0; norm[tz] += 1.0; }
        if (rx >= 0) { B(rx, c[1]) = z; B(rx, c[2]) = -y; norm[rx] += z * z + y * y; }
        if (ry >= 0) { B(ry, c[0]) = -z; B(ry, c[2]) = x; norm[ry] += z * z + x * x; }
        if (rz >= 0) { B(rz, c[0]) = y; B(rz, c[1]) = -x; norm[rz] += x * x + y * y; }
        if (ms >= 0) { B(ms, c[0]) = x; B(ms, c[1]) = y; B(ms, c[2]) = z; norm[ms] += x * x + y * y + z * z; }
    }
    const int cend = std::min(e->U, stride);
    for (int r = 0; r < d; r++) {
        const double s = sqrt(norm[r]);
        for (int c = 0; c < cend; c++)
            if (hB[(size_t)r * stride + c] != 0.0) hB[(size_t)r * stride + c] = hB[(size_t)r * stride + c] / s;
    }
    return JAICOV_OK;
}

// datum rows of the build from the host copy of the parameter values
static int datum_rows_host(jaicov_engine *e) {
    return datum_rows(e, e->h_point_datum.data(), e->h_vals.data(), e->hB, e->Upad);
}

extern "C" int jaicov_neq_finalize(jaicov_engine *e, double sigma2, double lambda, int simulation) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    (void)sigma2;
    if (e->state != jaicov_engine::ST_ACCUMULATED) FAIL(e->err, JAICOV_ERR_BAD_STATE, "accumulate first");
    HIPE(e->err, hipSetDevice(e->device));
    TRY(datum_rows_host(e));
    if (e->reduced) {   // the host has summed the packed buffer over ranks: bring it back into the square
        const int Ua = e->schur_active ? e->e0 : e->U;
        const size_t len = (size_t)Ua * (Ua + 1) / 2;
        hipLaunchKernelGGL(unpack_kernel, dim3((Ua + 255) / 256, std::max(Ua, 1)), dim3(256), 0, e->stream, e->d_packed, (long)e->Upad, Ua, e->d_N);
        HIPE(e->err, hipMemcpyAsync(e->d_n, e->d_packed + len, (size_t)Ua * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        if (e->schur_active)   // what the EO elimination took from the diagonal, summed over the ranks like N itself (LM damping)
            HIPE(e->err, hipMemcpyAsync(e->sb.diagcorr, e->d_packed + len + Ua, (size_t)Ua * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        e->reduced = false;
    }
    if (e->schur_active && lambda != e->lambda_acc && (lambda > 0 || e->lambda_acc > 0))
        FAIL(e->err, JAICOV_ERR_BAD_ARGUMENT, "EO pre-elimination: pass the damping value to accumulate2()/build() as well");
    hipLaunchKernelGGL(damp_and_precond_kernel, dim3((e->Upad + 255) / 256), dim3(256), 0, e->stream, e->d_N, (long)e->Upad,
                       e->schur_active ? e->e0 : e->U, e->Upad, e->d, lambda > 0 ? lambda : 0.0, e->d_V,
                       e->schur_active ? e->sb.diagcorr : nullptr);
    if (simulation) HIPE(e->err, hipMemsetAsync(e->d_n, 0, e->Upad * sizeof(double), e->stream));   // BA:830-831
    e->sim_built = simulation != 0;
    HIPE(e->err, hipEventRecord(e->ev[3].get(), e->stream));
    e->lambda_used = lambda;
    e->state = jaicov_engine::ST_BUILT;
    return JAICOV_OK;
}

// buffers of the inverse (W = L^-1 and Q, two squares of the solver's order) of the solver that factorises; for the effective mode
// FULL_EXPANDED also the Q of the full-order solver, where the expanded matrix lives
static int ensure_inverse_buffers(jaicov_engine *e, bool reduced_system, int mode) {
    HIPE(e->err, (reduced_system ? e->solverS : e->solver).reserve_inverse(true));
    if (mode == JAICOV_INVERT_FULL_EXPANDED) HIPE(e->err, e->solver.reserve_inverse(false));
    return JAICOV_OK;
}

// the expansion's workspace is the reduced solver's W square: F and T1 ([6 images, padded] x order) and T2 must fit (they do
// unless the exterior orientations outnumber the other unknowns several times over: then the literal route is taken)
// *I6p: EO unknowns of all images, padded; *Up: padded order of the reduced system
static bool expansion_fits(const jaicov_engine *e, size_t *I6p, size_t *Up) {
    *I6p = ((size_t)6 * e->p.n_images + 127) / 128 * 128;
    *Up = (size_t)e->solverS.nfact;
    return *I6p * (2 * *Up + *I6p) <= (size_t)e->solverS.n * e->solverS.ld;
}

// FULL_EXPANDED is FULL wherever the expansion cannot be done: no EO pre-elimination, or an engine that sees a shard of the images
// and whose caller has not promised to sum the expansion's inputs over the ranks (engine option expansion_exchange)
static int effective_invert(const jaicov_engine *e, int invert) {
    if (invert != JAICOV_INVERT_FULL_EXPANDED) return invert;
    if (!(e->schur_ok && (e->all_images || e->opts.expansion_exchange != 0) && e->solverS_ready)) return JAICOV_INVERT_FULL;
    size_t I6p, Up;
    return expansion_fits(e, &I6p, &Up) ? invert : JAICOV_INVERT_FULL;
}

extern "C" int jaicov_neq_prepare_inverse(jaicov_engine *e, int inverse_follows) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    if (inverse_follows < 0 || inverse_follows > JAICOV_INVERT_FULL_EXPANDED) return JAICOV_ERR_BAD_ARGUMENT;
    inverse_follows = effective_invert(e, inverse_follows);
    e->inverse_mode_next = inverse_follows;
    // the inverse's buffers are allocated HERE, when the final pass is announced (BA:250: known before the build), not inside
    // the solve: hipMalloc of 2 x 1.8 .. 2.6 GB cost the first inverting solve 45 ms at config 4
    if (inverse_follows == JAICOV_INVERT_NONE) return JAICOV_OK;
    HIPE(e->err, hipSetDevice(e->device));
    const bool reduced = e->schur_ok && (inverse_follows == JAICOV_INVERT_REDUCED || inverse_follows == JAICOV_INVERT_FULL_EXPANDED) && e->solverS_ready;
    return ensure_inverse_buffers(e, reduced, inverse_follows);
}

extern "C" int jaicov_neq_cofactor_order(const jaicov_engine *e) {
    if (!e || !e->q.valid) return -1;
    return e->q.order;
}

extern "C" int jaicov_neq_reduced_order(const jaicov_engine *e) {
    if (!e) return -1;
    return e->schur_active ? e->e0 : e->U;
}

extern "C" int jaicov_neq_accumulate2(jaicov_engine *e, double sigma2, double lambda) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    e->lambda_acc = lambda > 0 ? lambda : 0.0;
    return jaicov_neq_accumulate(e, sigma2);
}

extern "C" int jaicov_neq_build(jaicov_engine *e, double sigma2, double lambda, int simulation) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    e->lambda_acc = lambda > 0 ? lambda : 0.0;
    TRY(jaicov_neq_accumulate(e, sigma2));
    return jaicov_neq_finalize(e, sigma2, lambda, simulation);
}

static int reduce_buffer_impl(jaicov_engine *e, void **device_ptr, size_t *count, bool sync) {
    if (!e || !device_ptr || !count) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state != jaicov_engine::ST_ACCUMULATED) FAIL(e->err, JAICOV_ERR_BAD_STATE, "accumulate first");
    HIPE(e->err, hipSetDevice(e->device));
    // packed lower triangle (== UPLO='U' packed) followed by n: one contiguous array the collective sums as it is.
    // With the EO pre-elimination only the reduced system (order e0) exists.
    const int Ua = e->schur_active ? e->e0 : e->U;
    const size_t len = (size_t)Ua * (Ua + 1) / 2;
    if (!e->d_packed) TRY(dalloc(e, (size_t)e->U * (e->U + 1) / 2 + 2 * (size_t)e->U, &e->d_packed));
    hipLaunchKernelGGL(pack_kernel, dim3((Ua + 255) / 256, std::max(Ua, 1)), dim3(256), 0, e->stream, e->d_N, (long)e->Upad, Ua, e->d_packed);
    HIPE(e->err, hipMemcpyAsync(e->d_packed + len, e->d_n, (size_t)Ua * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    // with the EO pre-elimination the LM damping needs diag(N) - diag(N_reduced), also a sum over the ranks' images
    if (e->schur_active)
        HIPE(e->err, hipMemcpyAsync(e->d_packed + len + Ua, e->sb.diagcorr, (size_t)Ua * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    if (sync) HIPE(e->err, hipStreamSynchronize(e->stream));   // the caller's collective runs on its own stream
    e->reduced = true;
    *device_ptr = e->d_packed;
    *count = len + Ua + (e->schur_active ? (size_t)Ua : 0);
    return JAICOV_OK;
}

extern "C" int jaicov_neq_reduce_buffer(jaicov_engine *e, void **device_ptr, size_t *count) {
    return reduce_buffer_impl(e, device_ptr, count, true);
}

extern "C" int jaicov_neq_reduce_buffer_async(jaicov_engine *e, void **device_ptr, size_t *count, void **stream) {
    if (!stream) return JAICOV_ERR_BAD_ARGUMENT;
    const int rc = reduce_buffer_impl(e, device_ptr, count, false);
    if (rc == JAICOV_OK) *stream = (void *)e->stream;
    return rc;
}

// small dense helpers on the host (d <= 7)
static bool small_inverse(int d, const double *S, double *Sinv) {
    double a[7][14];
    for (int i = 0; i < d; i++)
        for (int j = 0; j < d; j++) { a[i][j] = S[i * d + j]; a[i][d + j] = i == j ? 1.0 : 0.0; }
    for (int c = 0; c < d; c++) {
        int piv = c;
        for (int r = c + 1; r < d; r++)
            if (fabs(a[r][c]) > fabs(a[piv][c])) piv = r;
        if (a[piv][c] == 0.0) return false;
        if (piv != c)
            for (int j = 0; j < 2 * d; j++) std::swap(a[c][j], a[piv][j]);
        const double inv = 1.0 / a[c][c];
        for (int j = 0; j < 2 * d; j++) a[c][j] *= inv;
        for (int r = 0; r < d; r++) {
            if (r == c) continue;
            const double f = a[r][c];
            if (f != 0.0)
                for (int j = 0; j < 2 * d; j++) a[r][j] -= f * a[c][j];
        }
    }
    for (int i = 0; i < d; i++)
        for (int j = 0; j < d; j++) Sinv[i * d + j] = a[i][d + j];
    return true;
}

// ---- one call of jaicov_neq_solve: what its stages share, then the stages in the order they run ------------------------------
struct Solve {
    jaicov_engine *const e;
    const bool schur;                   // the EO-reduced system is at hand
    const int U, d, Upad;               // order of the system that is factorised (reduced: points, IO, distortion; or full); rank of the datum border; ld of N, V, B, rhs
    DenseSolver &slv;
    const int Up, vs;                   // padded order of the factorised system == stride between the solution vectors (the solver's order)
    const long ld;
    int invert = 0;                     // the effective mode
    bool expand = false;                // ... is FULL_EXPANDED: all of Qxx from the reduced inverse
    std::vector<double> Bh, X, delta0;  // datum rows R B V [8][Upad]; y~ and G^ [d + 1][vs]; the correction of the device's own refinement step
    double R[7] = {1, 1, 1, 1, 1, 1, 1}, Sinv[49];
    bool fast_refined = false;          // d = 0: the first refinement step went out behind the substitution, without the host
    float refine_ms = 0.f;
    explicit Solve(jaicov_engine *eng)
        : e(eng), schur(e->schur_active), U(schur ? e->e0 : e->U), d(e->d), Upad(e->Upad), slv(schur ? e->solverS : e->solver),
          Up(slv.nfact), vs(Up), ld(slv.ld) {}

    double border_dot(int a, const double *v) const {      // Bh[a] . v over the unknowns
        double s = 0.0;
        for (int c = d; c < U; c++) s += Bh[(size_t)a * Upad + c] * v[c];
        return s;
    }
    void border_multipliers(const double *v, const double *rk, double *k) const {      // k = S^-1 (Bh v - rk)
        double t[7];
        for (int a = 0; a < d; a++) t[a] = border_dot(a, v) - rk[a];
        for (int a = 0; a < d; a++) {
            double s = 0.0;
            for (int b = 0; b < d; b++) s += Sinv[a * d + b] * t[b];
            k[a] = s;
        }
    }

    int solve_mode(int requested) {
        invert = effective_invert(e, requested);
        if (invert == JAICOV_INVERT_FULL_EXPANDED && !schur) invert = JAICOV_INVERT_FULL;     // the system at hand was assembled unreduced
        expand = invert == JAICOV_INVERT_FULL_EXPANDED;
        if (schur && invert == JAICOV_INVERT_FULL)
            FAIL(e->err, JAICOV_ERR_BAD_STATE, "the normal equations were assembled with the EO blocks pre-eliminated: call "
                                          "jaicov_neq_prepare_inverse(e, JAICOV_INVERT_FULL) before the build whose solve shall invert");
        slv.profile = e->solver.profile;
        slv.flops_order = (double)U;
        // normally done by prepare_inverse(); a host that did not announce the final pass pays the allocation here
        return invert ? ensure_inverse_buffers(e, schur, invert) : JAICOV_OK;
    }
    // V to the host, scaled + row-normalised datum rows Bh = R B V (NES:82-91 scaling of the border)
    // This round trip stays even where nothing of it is needed before the factorisation (d = 0): with the host running ahead of
    // the assembly -- enqueuing the factorisation and spinning in its residency handshake while the assembly kernels still run --
    // every pass was 0.6 ms SLOWER (assembly +0.19, factorisation +0.4; measured A/B in round 3).
    // What d = 0 does save is the round trip between the substitution and the first refinement step (factor_and_substitute).
    int border_rows() {
        int hinfo = 0;   // status of the per-image EO eliminations, fetched in the same round trip
        HIPE(e->err, hipMemcpyAsync(e->h_V.data(), e->d_V, Upad * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        if (schur) HIPE(e->err, hipMemcpyAsync(&hinfo, e->sb.info, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        HIPE(e->err, hipStreamSynchronize(e->stream));
        if (hinfo != 0) FAIL(e->err, JAICOV_ERR_SINGULAR, "exterior orientation block of image " + std::to_string(hinfo - 1000000) + " is not positive definite");
        Bh.assign((size_t)8 * Upad, 0.0);
        for (int a = 0; a < d; a++) {
            double s = 0.0;
            for (int c = d; c < U; c++) {
                const double v = e->hB[(size_t)a * Upad + c] * e->h_V[c];
                Bh[(size_t)a * Upad + c] = v;
                s += v * v;
            }
            if (!(s > 0.0)) FAIL(e->err, JAICOV_ERR_SINGULAR, "empty datum condition row");
            R[a] = 1.0 / sqrt(s);
            for (int c = d; c < U; c++) Bh[(size_t)a * Upad + c] *= R[a];
        }
        if (d > 0) HIPE(e->err, hipMemcpyAsync(e->d_B, Bh.data(), (size_t)d * Upad * sizeof(double), hipMemcpyHostToDevice, e->stream));
        HIPE(e->err, hipEventRecord(e->ev[4].get(), e->stream));
        return JAICOV_OK;
    }
    // ---- iterative refinement (refine.hip): residual of the unscaled bordered system in two-fold precision, one forward and
    // one backward substitution with the factor at hand per step.  The correction of the border follows the same rank-d
    // algebra as the step itself with r_y = V rho_x, r_k = R rho_kappa:  delta0 = M^-1 (r_y + Bh' r_k),
    // dk = S^-1 (Bh delta0 - r_k),  dy = delta0 - G^ dk.
    // The device's part of a step: refine_begin, then whatever gives d_dx its value, then refine_step.
    int refine_begin() {
        const int nbk = Up / 128;
        HIPE(e->err, e->refP.reserve((size_t)nbk * nbk * 256));      // ahead of the event: an allocation is no part of the step's time
        HIPE(e->err, hipEventRecord(e->ev_r0.get(), e->stream));
        return JAICOV_OK;
    }
    // residual of d_dx, delta = M^-1 residual, and delta on its way to the host (complete once the stream has been synchronised)
    int refine_step(const RefineBorder &bd, std::vector<double> &delta) {
        double *d_rhs = e->d_ref, *d_tmp = e->d_ref + Upad, *d_delta = e->d_ref + 2 * (size_t)Upad;
        HIPE(e->err, launch_residual_dd(e->stream, e->d_N, (long)Upad, U, d, Up, e->d_dx, e->d_n, e->d_V, e->d_Braw, e->d_B, (long)Upad,
                                   bd, e->refP.get(), d_rhs));
        HIPE(e->err, slv.solve_rhs(d_rhs, d_tmp, d_delta));
        HIPE(e->err, hipEventRecord(e->ev_r1.get(), e->stream));
        delta.assign((size_t)Up, 0.0);
        HIPE(e->err, hipMemcpyAsync(delta.data(), d_delta, delta.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        return JAICOV_OK;
    }
    // a completed step: its time, dx += the correction that belongs to delta (d = 0: V delta), max |correction| / max |dx|
    int apply_correction(const RefineBorder &bd, const std::vector<double> &dl, double *dx_out) {
        float ms1 = 0.f;
        hipEventElapsedTime(&ms1, e->ev_r0.get(), e->ev_r1.get());
        refine_ms += ms1;
        double dk[7] = {0, 0, 0, 0, 0, 0, 0};
        border_multipliers(dl.data(), bd.rk, dk);
        double cmax = 0.0, xmax = 0.0;
        for (int c = d; c < U; c++) {
            double dy = dl[c];
            for (int a = 0; a < d; a++) dy -= X[(size_t)(1 + a) * vs + c] * dk[a];
            const double corr = e->h_V[c] * dy;
            if (!std::isfinite(corr)) FAIL(e->err, JAICOV_ERR_NOT_FINITE, "non-finite refinement step");
            dx_out[c] += corr;
            cmax = std::max(cmax, fabs(corr)); xmax = std::max(xmax, fabs(dx_out[c]));
        }
        for (int a = 0; a < d; a++) dx_out[a] += R[a] * dk[a];
        e->last_refine_correction = xmax > 0.0 ? cmax / xmax : 0.0;
        return JAICOV_OK;
    }
    // right-hand sides: row 0 = V n, rows 1..d = Bh.  They are the extra rows below the matrix, so the factorisation
    // itself carries out the forward substitution (dense.hip).
    // dataflow factorisation: the tile kernel reads N itself and scales on the fly (no copy of the matrix at all);
    // stream-scheduled one: the columns of the first panel go first, together with the right-hand sides; the panel then
    // factors on its stream while the rest of the matrix is still being scaled and copied (0.4 ms at config 4).
    // (in a loop: a dataflow factorisation that was abandoned -- cholflow.hip, "Visibility": a wait ran into its time limit, seen
    // about once in 1 000 factorisations at config 4 -- is repeated; N, V and the datum rows are untouched by it)
    int factor_and_substitute() {
        const int nrhs = d + 1;
        const bool fused = slv.flow.ready();
        const int c1 = std::min(slv.first_panel_cols(), Up);
        int info = 0;
        for (int attempt = 0;; attempt++) {
            HIPE(e->err, slv.begin_refactor());      // the side stream's premultiply of the last pass may still read the old factor: nothing writes L before this
            if (!fused)
                hipLaunchKernelGGL(scale_copy_kernel, dim3((c1 + 255) / 256, Up), dim3(256), 0, e->stream, e->d_N, (long)Upad, slv.L, ld, U,
                                   Up, d, e->d_V, e->d_B, Upad, 0, c1);
            HIPE(e->err, hipMemsetAsync(slv.rhs_row(0), 0, (size_t)128 * ld * sizeof(double), e->stream));
            hipLaunchKernelGGL(scale_vec_kernel, dim3((Up + 255) / 256), dim3(256), 0, e->stream, e->d_n, e->d_V, slv.rhs_row(0), U, Up, d);
            if (d > 0)
                HIPE(e->err, hipMemcpy2DAsync(slv.rhs_row(1), (size_t)ld * sizeof(double), e->d_B, (size_t)Upad * sizeof(double),
                                         (size_t)Up * sizeof(double), (size_t)d, hipMemcpyDeviceToDevice, e->stream));
            HIPE(e->err, hipEventRecord(e->ev_first.get(), e->stream));
            if (!fused && c1 < Up)
                hipLaunchKernelGGL(scale_copy_kernel, dim3((Up - c1 + 255) / 256, Up), dim3(256), 0, e->stream, e->d_N, (long)Upad, slv.L,
                                   ld, U, Up, d, e->d_V, e->d_B, Upad, c1, Up);
            HIPE(e->err, hipEventRecord(e->ev_all.get(), e->stream));
            if (fused) slv.flow.set_source(e->d_N, (long)Upad, e->d_V, e->d_B, Upad, d, U);
            HIPE(e->err, slv.potrf(e->ev_first.get(), e->ev_all.get()));
            HIPE(e->err, hipEventRecord(e->ev[5].get(), e->stream));
            HIPE(e->err, slv.backsolve_aug(e->d_G, vs, nrhs));           // G <- L^-T (L^-1 Y)   (row 0: y~, rows 1..d: G^)
            HIPE(e->err, hipEventRecord(e->ev[6].get(), e->stream));
            X.assign((size_t)nrhs * vs, 0.0);
            HIPE(e->err, hipMemcpyAsync(X.data(), e->d_G, X.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
            fast_refined = false;
            if (d == 0 && e->refine_steps >= 1 && !e->sim_built) {
                // first refinement step without the host: dx = V y on the device, residual of the unscaled system in two-fold precision,
                // forward + backward substitution (refine.hip, dense.hip); the correction comes back together with y
                TRY(refine_begin());
                hipLaunchKernelGGL(scale_vec_kernel, dim3((Up + 255) / 256), dim3(256), 0, e->stream, e->d_G, e->d_V, e->d_dx, U, Up, 0);   // dx = V y
                TRY(refine_step(RefineBorder{}, delta0));
                fast_refined = true;
            }
            info = slv.fetch_info();
            if (info == -9 && attempt < 2) {
                ++e->flow_retries;
                fprintf(stderr, "jaicov: factorisation abandoned on the device (a wait ran into its time limit); repeating it (%d)\n", attempt + 1);
                continue;
            }
            break;
        }
        if (info < 0) FAIL(e->err, JAICOV_ERR_DEVICE, "factorisation did not complete on the device (code " + std::to_string(info) + ")");
        if (info != 0) FAIL(e->err, JAICOV_ERR_SINGULAR, "normal-equation matrix is singular / not positive definite at pivot " + std::to_string(info));
        return JAICOV_OK;
    }
    // ---- rank-d border algebra on the host ---------------------------------------------------------------------
    int border_step(double *dx_out) {
        double Sm[49], kh[7];
        std::vector<double> y(X.begin(), X.begin() + vs);
        if (d > 0) {
            for (int a = 0; a < d; a++)
                for (int b = 0; b < d; b++) Sm[a * d + b] = border_dot(a, &X[(size_t)(1 + b) * vs]);
            if (!small_inverse(d, Sm, Sinv)) FAIL(e->err, JAICOV_ERR_SINGULAR, "datum conditions are linearly dependent");
            const double no_rk[7] = {0, 0, 0, 0, 0, 0, 0};
            border_multipliers(X.data(), no_rk, kh);
            for (int c = d; c < U; c++) {
                double s = 0.0;
                for (int a = 0; a < d; a++) s += X[(size_t)(1 + a) * vs + c] * kh[a];
                y[c] -= s;
            }
        }
        for (int c = 0; c < U; c++) dx_out[c] = c < d ? R[c] * kh[c] : e->h_V[c] * y[c];
        for (int c = 0; c < U; c++)
            if (!std::isfinite(dx_out[c])) FAIL(e->err, JAICOV_ERR_NOT_FINITE, "non-finite step");
        return JAICOV_OK;
    }
    // the step the device took on its own (d = 0: no border algebra), then the others with the host in between
    int refine(double *dx_out) {
        e->last_refine_correction = 0.0;
        if (fast_refined) TRY(apply_correction(RefineBorder{}, delta0, dx_out));
        for (int step = fast_refined ? 1 : 0; step < e->refine_steps && !e->sim_built; step++) {
            RefineBorder bd{};
            for (int a = 0; a < d; a++) {
                long double sacc = 0.0L;
                for (int c = d; c < U; c++) sacc += (long double)e->hB[(size_t)a * Upad + c] * (long double)dx_out[c];
                bd.kappa[a] = dx_out[a];
                bd.rk[a] = (double)(-(long double)R[a] * sacc);
            }
            TRY(refine_begin());
            if (d > 0 && step == 0)
                HIPE(e->err, hipMemcpyAsync(e->d_Braw, e->hB.data(), (size_t)d * Upad * sizeof(double), hipMemcpyHostToDevice, e->stream));
            HIPE(e->err, hipMemcpyAsync(e->d_dx, dx_out, (size_t)U * sizeof(double), hipMemcpyHostToDevice, e->stream));
            std::vector<double> dl;
            TRY(refine_step(bd, dl));
            HIPE(e->err, hipStreamSynchronize(e->stream));
            TRY(apply_correction(bd, dl, dx_out));
        }
        return JAICOV_OK;
    }
    // EO step of every image of this engine: dx_E = L_E^-T U' (w - A_r dx_R), from d_dx into d_xE   (schur.hip)
    int eo_backsub() {
        HIPE(e->err, launch_omega(e->stream, e->p, e->d_in_block, e->ip0, e->ip_count, e->d_blk_list, 0, e->max_m, e->d_rowsA,
                             e->d_rowsW, e->d_dx, 1.0, e->d_vbuf, e->d_omega));
        HIPE(e->err, launch_schur_backsub(e->stream, e->p, e->d_blk_list, e->n_blk_list, e->sb.U, e->sb.Linv, e->d_vbuf, e->d_xE));
        return JAICOV_OK;
    }
    // Round 5: once in ~10 runs of the GPU test-suite a solve returned an EO step of EXACT zeros for every image (N, n and the reduced
    // step correct; 1 200 solves of the same scene alone: never).  The back-substitution kernel cannot produce that from finite
    // operands, so the copy is checked: all zeros -> read again with a blocking copy after a device-wide wait, and say so.
    int eo_zero_step_guard(std::vector<double> &xE) {
        bool all_zero = !e->h_blk_images.empty();
        for (int img : e->h_blk_images)
            for (int k = 0; k < 6 && all_zero; k++) all_zero = xE[(size_t)6 * img + k] == 0.0;
        if (!all_zero) return JAICOV_OK;
        HIPE(e->err, hipDeviceSynchronize());
        HIPE(e->err, hipMemcpy(xE.data(), e->d_xE, xE.size() * sizeof(double), hipMemcpyDeviceToHost));
        bool still = true;
        for (int img : e->h_blk_images)
            for (int k = 0; k < 6 && still; k++) still = xE[(size_t)6 * img + k] == 0.0;
        if (still) {      // the kernel itself left zeros: run the two kernels once more
            TRY(eo_backsub());
            HIPE(e->err, hipStreamSynchronize(e->stream));
            HIPE(e->err, hipMemcpy(xE.data(), e->d_xE, xE.size() * sizeof(double), hipMemcpyDeviceToHost));
        }
        fprintf(stderr, "jaicov: the exterior-orientation step came back as exact zeros; %s\n",
                still ? "the back-substitution was run again" : "a second, blocking copy had the values (the first copy returned before the data)");
        return JAICOV_OK;
    }
    // the EO entries of the step, which the reduced system does not hold
    int eo_entries(double *dx_out) {
        const bool quirk = e->opts.reduced_reference_quirk && invert == JAICOV_INVERT_REDUCED;
        if (schur)
            for (int c = U; c < e->U; c++) dx_out[c] = 0.0;
        // SIMULATION zeroes the right-hand side of the WHOLE system (BA:830-831 `n.zero()`): the eliminated exterior
        // orientations get no step either (their back substitution would use the real misclosures)
        if (schur && e->sim_built) return JAICOV_OK;
        if (schur && quirk) {
            // what the reference's last pass leaves in the EO entries of dx under MatrixInversion.REDUCED (quirk Q1): V_c^2 n_c
            std::vector<double> xq((size_t)6 * e->p.n_images);
            HIPE(e->err, hipMemcpyAsync(xq.data(), e->sb.xq, xq.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
            HIPE(e->err, hipStreamSynchronize(e->stream));
            for (int img : e->h_blk_images)
                for (int k = 0; k < 6; k++) dx_out[e->e0 + 6 * img + k] = xq[(size_t)6 * img + k];
        } else if (schur) {
            HIPE(e->err, hipMemcpyAsync(e->d_dx, dx_out, (size_t)e->U * sizeof(double), hipMemcpyHostToDevice, e->stream));
            TRY(eo_backsub());
            std::vector<double> xE((size_t)6 * e->p.n_images);
            HIPE(e->err, hipMemcpyAsync(xE.data(), e->d_xE, xE.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
            HIPE(e->err, hipStreamSynchronize(e->stream));
            TRY(eo_zero_step_guard(xE));
            for (int img : e->h_blk_images)
                for (int k = 0; k < 6; k++) {
                    dx_out[e->e0 + 6 * img + k] = xE[(size_t)6 * img + k];
                    if (!std::isfinite(xE[(size_t)6 * img + k])) FAIL(e->err, JAICOV_ERR_NOT_FINITE, "non-finite step");
                }
        } else if (quirk) {
            // full-order path (no EO pre-elimination possible): the same quirk from the assembled right-hand side, V_c^2 n_c
            std::vector<double> hn((size_t)e->U);
            HIPE(e->err, hipMemcpyAsync(hn.data(), e->d_n, hn.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
            HIPE(e->err, hipStreamSynchronize(e->stream));
            const int ns = e->n_slots, s_eo = ns - 6 * e->p.n_images;
            for (int sl = s_eo; sl < ns; sl++) {
                const int c = e->h_slot_col[sl];
                if (c >= 0) dx_out[c] = e->h_V[c] * e->h_V[c] * hn[c];
            }
        }
        return JAICOV_OK;
    }
    // FULL: Qxx of all unknowns.  REDUCED on a pre-eliminated system: the inverse of the reduced normal equations,
    // which IS the block of Qxx that belongs to the datum border, points, interior orientation and distortion
    // (MatrixInversion.REDUCED / PRE_ELIMINATION, BA:261-267: solve(N, n, numRows, true) on the reduced system).
    int invert_and_expand() {
        HIPE(e->err, slv.trtri());
        HIPE(e->err, slv.lauum());
        if (e->opts.inverse_refinement >= 0 && Up <= 8192) {
            // One Newton-Schulz step on Q = inv(M) with the residual I - M Q formed exactly (batchinv.hip): M is materialised once more
            // (scaled, with the datum border's term; the factor in slv.L is not needed again before the next factorisation), W is free
            // after lauum(), three more squares are kept with the engine.
            const size_t sq = (size_t)Up * ld;
            HIPE(e->err, e->ns_work.reserve(3 * sq));
            double *ns = e->ns_work.get();
            HIPE(e->err, slv.begin_refactor());
            HIPE(e->err, slv.symmetrize(slv.Q));
            hipLaunchKernelGGL(scale_copy_kernel, dim3((Up + 255) / 256, Up), dim3(256), 0, e->stream, e->d_N, (long)Upad, slv.L, ld, U,
                               Up, d, e->d_V, e->d_B, Upad, 0, Up);
            HIPE(e->err, slv.symmetrize(slv.L));
            HIPE(e->err, newton_schulz_exact(e->stream, Up, ld, slv.L, slv.Q, slv.W, ns, ns + sq, ns + 2 * sq));
        }
        // H = Sinv G^ ; F = R (Sinv G^) V ; E = R (I - Sinv) R
        std::vector<double> H((size_t)8 * Upad, 0.0), F((size_t)8 * Upad, 0.0);
        double E[49];
        for (int a = 0; a < d; a++) {
            for (int c = d; c < U; c++) {
                double s = 0.0;
                for (int b = 0; b < d; b++) s += Sinv[a * d + b] * X[(size_t)(1 + b) * vs + c];
                H[(size_t)a * Upad + c] = s;
                F[(size_t)a * Upad + c] = R[a] * s * e->h_V[c];
            }
            for (int b = 0; b < d; b++) E[a * d + b] = R[a] * ((a == b ? 1.0 : 0.0) - Sinv[a * d + b]) * R[b];
        }
        if (d > 0) {
            HIPE(e->err, hipMemcpyAsync(e->d_H, H.data(), (size_t)d * Upad * sizeof(double), hipMemcpyHostToDevice, e->stream));
            HIPE(e->err, hipMemcpyAsync(e->d_F, F.data(), (size_t)d * Upad * sizeof(double), hipMemcpyHostToDevice, e->stream));
            HIPE(e->err, hipMemcpyAsync(e->d_E, E, (size_t)d * d * sizeof(double), hipMemcpyHostToDevice, e->stream));
        }
        hipLaunchKernelGGL(qfix_kernel, dim3((Up + 255) / 256, Up), dim3(256), 0, e->stream, slv.Q, ld, U, Upad, d,
                           e->d_V, e->d_G + vs, (long)vs, e->d_H, e->d_F, e->d_E, Up);
        return expand ? expand_cofactor() : JAICOV_OK;
    }
    // ---- the full cofactor matrix from the reduced one (schur.hip, blk_expand_f_kernel): workspace = W of the reduced
    //      solver, free again after lauum():  F [6I pad][Up] | T1 = -F Q_RR [6I pad][Up] | T2 = -T1 F' [6I pad][6I pad]
    int expand_cofactor() {
        size_t I6, UpS;
        if (!expansion_fits(e, &I6, &UpS))
            FAIL(e->err, JAICOV_ERR_UNSUPPORTED, "FULL_EXPANDED: more exterior orientations than the workspace holds; use JAICOV_INVERT_FULL");
        const int I6p = (int)I6;
        double *Fm = slv.W, *T1 = Fm + (size_t)I6p * Up, *T2 = T1 + (size_t)I6p * Up;
        const double *LinvAll = e->sb.Linv;
        if (e->all_images) {
            HIPE(e->err, hipMemsetAsync(Fm, 0, (size_t)I6p * Up * sizeof(double), e->stream));
            HIPE(e->err, launch_schur_expand_f(e->stream, e->p, e->d_blk_list, e->n_blk_list, e->d_rowsA, e->sb.U, e->sb.Linv, e->sb.G, Fm, (long)Up));
        } else {      // a shard: F and L_E^-1 of EVERY image, summed over the ranks by the caller (jaicov_neq_expansion_buffer)
            if (!e->exp_ready || e->expF_len != (size_t)I6p * Up + (size_t)36 * e->p.n_images)
                FAIL(e->err, JAICOV_ERR_BAD_STATE, "FULL_EXPANDED on a sharded engine: all-reduce jaicov_neq_expansion_buffer() between accumulate and solve");
            HIPE(e->err, hipMemcpyAsync(Fm, e->expF.get(), (size_t)I6p * Up * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
            // the summed L_E^-1 records are READ from the buffer, never copied over sb.Linv: that array must keep zeros for the
            // foreign images, or the next pass's expansion buffer would carry their stale records into the sum (ADVICE r4, high:
            // a second sharded FULL_EXPANDED pass gave R times the EO cofactors)
            LinvAll = e->expF.get() + (size_t)I6p * Up;
        }
        HIPE(e->err, slv.symmetrize(slv.Q));
        GemmArgs g1{};
        g1.A = Fm; g1.lda = Up; g1.B = slv.Q; g1.ldb = ld; g1.C = T1; g1.ldc = Up;
        g1.M = I6p; g1.N = Up; g1.K = Up; g1.alpha = -1.0; g1.beta = 0.0; g1.kmode = KMODE_FULL;
        HIPE(e->err, gemm_f64(e->stream, LAY_KC, LAY_KC, g1));             // Q_RR symmetric: F Q_RR = F Q_RR'
        GemmArgs g2{};
        g2.A = T1; g2.lda = Up; g2.B = Fm; g2.ldb = Up; g2.C = T2; g2.ldc = I6p;
        g2.M = I6p; g2.N = I6p; g2.K = Up; g2.alpha = -1.0; g2.beta = 0.0; g2.kmode = KMODE_FULL; g2.lower_only = 1;
        HIPE(e->err, gemm_f64(e->stream, LAY_KC, LAY_KC, g2));
        hipLaunchKernelGGL(expand_cofactor_kernel, dim3((e->U + 255) / 256, e->U), dim3(256), 0, e->stream, e->solver.Q, e->solver.ld,
                           e->U, e->e0, slv.Q, ld, T1, (long)Up, T2, (long)I6p, LinvAll);
        return JAICOV_OK;
    }
    // end of the device's work, what the cofactor matrix at hand is, the timings
    int finish() {
        HIPE(e->err, hipEventRecord(e->ev[7].get(), e->stream));
        HIPE(e->err, hipStreamSynchronize(e->stream));
        if (invert) {
            e->q.valid = true;
            e->q.sigma2 = e->sigma2_acc;
            e->q.lambda = e->lambda_used;
            e->q.vals = e->h_vals;
            jaicov::datum_state_invalidate(e->slot.datum.get());
            e->q.reduced = schur && !expand;
            e->q.order = expand ? e->U : U;
        }
        slv.prof_collect();
        if (schur) {
            e->solver.stat_launches += slv.stat_launches; e->solver.stat_ms += slv.stat_ms; e->solver.stat_flops += slv.stat_flops;
            slv.stat_launches = slv.stat_ms = slv.stat_flops = 0.0;
        }
        float ms;
        hipEventElapsedTime(&ms, e->ev[0].get(), e->ev[1].get()); e->timings[0] = ms;
        hipEventElapsedTime(&ms, e->ev[1].get(), e->ev[2].get()); e->timings[1] = ms;
        hipEventElapsedTime(&ms, e->ev[2].get(), e->ev[3].get()); e->timings[2] = ms;
        hipEventElapsedTime(&ms, e->ev[4].get(), e->ev[5].get()); e->timings[3] = ms;
        hipEventElapsedTime(&ms, e->ev[5].get(), e->ev[6].get()); e->timings[4] = ms + refine_ms;   // substitution + refinement steps
        hipEventElapsedTime(&ms, e->ev[6].get(), e->ev[7].get()); e->timings[5] = std::max(0.f, ms - refine_ms);   // the refinement sits between these events: counted under [4]
        hipEventElapsedTime(&ms, e->ev[0].get(), e->ev[7].get()); e->timings[7] = ms;
        e->state = jaicov_engine::ST_SOLVED;
        return JAICOV_OK;
    }
};

extern "C" int jaicov_neq_solve(jaicov_engine *e, int invert, double *dx_out) {
    if (!e || !dx_out) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state != jaicov_engine::ST_BUILT) FAIL(e->err, JAICOV_ERR_BAD_STATE, "build first");
    HIPE(e->err, hipSetDevice(e->device));
    if (invert < 0 || invert > JAICOV_INVERT_FULL_EXPANDED) return JAICOV_ERR_BAD_ARGUMENT;
    Solve s(e);
    TRY(s.solve_mode(invert));
    TRY(s.border_rows());
    TRY(s.factor_and_substitute());
    TRY(s.border_step(dx_out));
    TRY(s.refine(dx_out));
    TRY(s.eo_entries(dx_out));
    if (s.invert) TRY(s.invert_and_expand());
    return s.finish();
}

extern "C" int jaicov_neq_expansion_buffer(jaicov_engine *e, void **device_ptr, size_t *count) {
    if (!e || !device_ptr || !count) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state != jaicov_engine::ST_ACCUMULATED || !e->schur_active || !e->solverS_ready)
        FAIL(e->err, JAICOV_ERR_BAD_STATE, "expansion buffer: accumulate a pre-eliminated system first (prepare_inverse(JAICOV_INVERT_FULL_EXPANDED))");
    HIPE(e->err, hipSetDevice(e->device));
    size_t I6p, Up;
    expansion_fits(e, &I6p, &Up);
    const size_t len = I6p * Up + (size_t)36 * e->p.n_images;
    HIPE(e->err, e->expF.reserve(len));
    e->expF_len = len;
    double *d_expF = e->expF.get();
    TRY(engine_ensure_rows(e));
    HIPE(e->err, hipMemsetAsync(d_expF, 0, I6p * Up * sizeof(double), e->stream));       // foreign images' bands: zero
    HIPE(e->err, launch_schur_expand_f(e->stream, e->p, e->d_blk_list, e->n_blk_list, e->d_rowsA, e->sb.U, e->sb.Linv, e->sb.G, d_expF, (long)Up));
    // L_E^-1: written for this engine's images only (blk_elim_kernel), zero elsewhere since create
    HIPE(e->err, hipMemcpyAsync(d_expF + I6p * Up, e->sb.Linv, (size_t)36 * e->p.n_images * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    e->exp_ready = true;
    *device_ptr = d_expF;
    *count = len;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_eo_step_buffer(jaicov_engine *e, void **device_ptr, size_t *count) {
    if (!e || !device_ptr || !count) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state != jaicov_engine::ST_SOLVED || !e->schur_active || !e->d_xE) FAIL(e->err, JAICOV_ERR_BAD_STATE, "no pre-eliminated exterior orientations: solve a reduced system first");
    *device_ptr = e->d_xE;
    *count = (size_t)6 * e->p.n_images;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_omega(jaicov_engine *e, double sigma2, const double *dx, double *omega) {
    if (!e || !dx || !omega) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state == jaicov_engine::ST_NEW) FAIL(e->err, JAICOV_ERR_BAD_STATE, "set_parameters first");
    HIPE(e->err, hipSetDevice(e->device));
    TRY(engine_ensure_rows(e));
    hipEvent_t t0 = e->ev[8].get(), t1 = e->ev[9].get();
    HIPE(e->err, hipEventRecord(t0, e->stream));
    HIPE(e->err, hipMemcpyAsync(e->d_dx, dx, (size_t)e->U * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPE(e->err, hipMemsetAsync(e->d_omega, 0, sizeof(double), e->stream));
    HIPE(e->err, launch_omega(e->stream, e->p, e->d_in_block, e->ip0, e->ip_count, e->d_blk_list, e->n_blk_list, e->max_m,
                         e->d_rowsA, e->d_rowsW, e->d_dx, sigma2, e->d_vbuf, e->d_omega));
    if (e->opts.apply_shared) HIPE(e->err, launch_shared_groups(e->stream, e->p, e->d_vals, sigma2, nullptr, nullptr, e->d_dx, e->d_omega));
    HIPE(e->err, hipEventRecord(t1, e->stream));
    HIPE(e->err, hipMemcpyAsync(omega, e->d_omega, sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    float ms;
    hipEventElapsedTime(&ms, t0, t1);
    e->timings[6] = ms;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_update(jaicov_engine *e, const double *dx, double *max_abs_dx) {
    if (!e || !dx) return JAICOV_ERR_BAD_ARGUMENT;
    HIPE(e->err, hipSetDevice(e->device));
    double mx = 0.0;
    for (int s = 0; s < e->n_slots; s++) {
        const int c = e->h_slot_col[s];
        if (c >= 0) {
            const double dv = dx[c];
            mx = std::max(mx, fabs(dv));
            e->h_vals[s] = e->h_vals[s] + dv;
        }
    }
    if (max_abs_dx) *max_abs_dx = mx;
    HIPE(e->err, hipMemcpyAsync(e->d_vals, e->h_vals.data(), (size_t)e->n_slots * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    e->rows_valid = false;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_get_normal(jaicov_engine *e, double *N_packed, size_t len, double *n, size_t Ulen) {
    if (!e || !N_packed || !n) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state != jaicov_engine::ST_BUILT && e->state != jaicov_engine::ST_SOLVED && e->state != jaicov_engine::ST_ACCUMULATED)
        FAIL(e->err, JAICOV_ERR_BAD_STATE, "build first");
    const int U = e->U;
    if (len != (size_t)U * (U + 1) / 2 || Ulen != (size_t)U) return JAICOV_ERR_BAD_ARGUMENT;
    HIPE(e->err, hipSetDevice(e->device));
    // with the exterior orientations pre-eliminated only the reduced system (order e0) was assembled: the rows from e0 on
    // of the square are neither zeroed nor written in such a pass.  The header's contract: reduced system in the leading
    // e0 rows / columns, zeros elsewhere.
    const int Ua = e->schur_active ? e->e0 : U;
    const size_t lenA = (size_t)Ua * (Ua + 1) / 2;
    DevBuf<double> ap;
    HIPE(e->err, ap.reserve(std::max<size_t>(lenA, 1)));
    hipLaunchKernelGGL(pack_kernel, dim3((Ua + 255) / 256, std::max(Ua, 1)), dim3(256), 0, e->stream, e->d_N, (long)e->Upad, Ua, ap.get());
    HIPE(e->err, hipMemcpyAsync(N_packed, ap.get(), lenA * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPE(e->err, hipMemcpyAsync(n, e->d_n, Ua * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    if (lenA < len) memset(N_packed + lenA, 0, (len - lenA) * sizeof(double));
    for (int c = Ua; c < U; c++) n[c] = 0.0;
    // the datum border lives on the host (rows 0..d-1): K[r][c] = B[r][c]  (BA:548-593), packed index r + c(c+1)/2
    if (e->state != jaicov_engine::ST_ACCUMULATED)
        for (int r = 0; r < e->d; r++)
            for (int c = e->d; c < Ua; c++) N_packed[(size_t)r + (size_t)c * (c + 1) / 2] = e->hB[(size_t)r * e->Upad + c];
    return JAICOV_OK;
}

extern "C" int jaicov_neq_get_cofactor(jaicov_engine *e, double *Q_packed, size_t len) {
    if (!e || !Q_packed) return JAICOV_ERR_BAD_ARGUMENT;
    if (!e->q.valid) FAIL(e->err, JAICOV_ERR_BAD_STATE, "no cofactor matrix: solve with invert != 0 first (MatrixInversion.NONE, BA:1177)");
    const int U = e->q.order;
    if (len != (size_t)U * (U + 1) / 2) FAIL(e->err, JAICOV_ERR_BAD_ARGUMENT, "cofactor buffer length must be order(order+1)/2 with order = jaicov_neq_cofactor_order()");
    HIPE(e->err, hipSetDevice(e->device));
    const DenseSolver &qs = e->q_solver();
    DevBuf<double> ap;
    HIPE(e->err, ap.reserve(std::max<size_t>(len, 1)));
    hipLaunchKernelGGL(pack_kernel, dim3((U + 255) / 256, std::max(U, 1)), dim3(256), 0, e->stream, qs.Q, qs.ld, U, ap.get());
    HIPE(e->err, hipMemcpyAsync(Q_packed, ap.get(), len * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    return JAICOV_OK;
}

// every consumer of the cofactor matrix sees the engine through this view (qview.h)
void jaicov::engine_q_view(jaicov_engine *e, QView *v) {
    DenseSolver &qs = e->q_solver();
    v->device = e->device;
    v->stream = e->stream;
    v->Q = qs.Q;
    v->ld = qs.ld;
    v->order = e->q.order;
    v->U = e->U;
    v->d = e->d;
    v->n_points = e->n_points;
    v->have_q = e->q.valid;
    v->reduced = e->q.reduced;
    v->full_q = e->q.valid && !e->q.reduced && e->q.order == e->U;
    v->sharded = !e->all_images || !e->opts.apply_shared || e->ip0 != 0 || e->ip_count != e->p.n_ip;
    v->sigma2 = e->q.sigma2;
    v->lambda = e->q.lambda;
    v->p = &e->p;
    v->d_vals = e->d_vals;
    v->rowsA = e->d_rowsA;
    v->rowsW = e->d_rowsW;
    v->ll_diag = e->d_ll_diag;
    v->slot_col = &e->h_slot_col;
    v->ip_old2new = &e->ip_old2new;
    v->blk_ip_begin = &e->h_blk_ip_begin;
    v->blk_w_off = &e->h_blk_w_off;
    v->caller_block = &e->h_caller_block;
    v->slot = &e->slot;
    v->err = &e->err;
}

int jaicov::engine_datum_rows(jaicov_engine *e, const uint8_t *mask, std::vector<double> &B, int stride) {
    if (e->q.vals.size() != (size_t)e->n_slots) FAIL(e->err, JAICOV_ERR_BAD_STATE, "no inverting solve has recorded its parameter values");
    B.assign((size_t)e->d * stride, 0.0);
    return datum_rows(e, mask, e->q.vals.data(), B, stride);
}

static int cofactor_sub_impl(jaicov_engine *e, const int32_t *idx, int32_t k, double scale, double *out) {
    if (!e || !idx || !out || k <= 0) return JAICOV_ERR_BAD_ARGUMENT;
    if (!e->q.valid) FAIL(e->err, JAICOV_ERR_BAD_STATE, "no cofactor matrix: solve with invert != 0 first");
    for (int i = 0; i < k; i++)
        if (idx[i] < 0 || idx[i] >= e->q.order) return JAICOV_ERR_BAD_ARGUMENT;
    const DenseSolver &qs = e->q_solver();
    HIPE(e->err, hipSetDevice(e->device));
    DevBuf<int32_t> d_idx;
    DevBuf<double> d_out;
    HIPE(e->err, d_idx.reserve((size_t)k));
    HIPE(e->err, d_out.reserve((size_t)k * k));
    HIPE(e->err, hipMemcpyAsync(d_idx.get(), idx, (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(gather_sub_kernel, dim3(((size_t)k * k + 255) / 256), dim3(256), 0, e->stream, qs.Q, qs.ld, d_idx.get(), k, d_out.get(), scale);
    HIPE(e->err, hipMemcpyAsync(out, d_out.get(), (size_t)k * k * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    return JAICOV_OK;
}

extern "C" int jaicov_neq_get_cofactor_sub(jaicov_engine *e, const int32_t *idx, int32_t k, double *out) {
    return cofactor_sub_impl(e, idx, k, 1.0, out);
}

extern "C" int jaicov_neq_get_dispersion_sub(jaicov_engine *e, double sigma2_aposteriori, const int32_t *idx, int32_t k, double *out) {
    return cofactor_sub_impl(e, idx, k, sigma2_aposteriori, out);
}

extern "C" int jaicov_neq_get_rows(jaicov_engine *e, int32_t ip_begin, int32_t ip_count, double *w, double *A) {
    if (!e || !w || !A || ip_begin < e->ip0 || ip_count < 0 || ip_begin + ip_count > e->ip0 + e->ip_count) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state == jaicov_engine::ST_NEW) FAIL(e->err, JAICOV_ERR_BAD_STATE, "set_parameters first");
    HIPE(e->err, hipSetDevice(e->device));
    TRY(engine_ensure_rows(e));
    const size_t S = (size_t)e->p.n_ip;
    std::vector<double> hA((size_t)2 * KROW * S), hW(2 * S);
    HIPE(e->err, hipMemcpyAsync(hA.data(), e->d_rowsA, hA.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPE(e->err, hipMemcpyAsync(hW.data(), e->d_rowsW, hW.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    for (int i = 0; i < ip_count; i++) {
        const size_t ip = e->ip_old2new.empty() ? (size_t)ip_begin + i : (size_t)e->ip_old2new[(size_t)ip_begin + i];
        w[2 * i] = hW[ip]; w[2 * i + 1] = hW[S + ip];
        for (int r = 0; r < 2; r++)
            for (int l = 0; l < KROW; l++) A[((size_t)2 * i + r) * KROW + l] = hA[(size_t)(2 * l + r) * S + ip];
    }
    return JAICOV_OK;
}

extern "C" int jaicov_neq_set_profiling(jaicov_engine *e, int enable) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    e->solver.profile = enable != 0;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_kernel_stats(jaicov_engine *e, double *stats, int32_t n, int reset) {
    if (!e || !stats || n < 3) return JAICOV_ERR_BAD_ARGUMENT;
    stats[0] = e->solver.stat_launches; stats[1] = e->solver.stat_ms; stats[2] = e->solver.stat_flops;
    if (n >= 6) { stats[3] = e->dm_stat_passes; stats[4] = e->dm_stat_ms; stats[5] = e->dm_stat_flops; }
    if (n >= 10) {   // health of the dataflow factorisation since create (never reset): see jaicov_neq.h
        stats[6] = (double)e->flow_retries;
        const FlowCounters &c = e->solver.flow.counters(), &cS = e->solverS.flow.counters();
        stats[7] = (double)(c.stale_events + cS.stale_events);
        stats[8] = (double)(c.stale_confirmed + cS.stale_confirmed);
        stats[9] = (double)(c.rescued + cS.rescued);
    }
    if (n >= 11) stats[10] = e->last_refine_correction;
    if (n >= 12) stats[11] = (double)e->refine_steps;      // refinement steps per solve the engine actually runs (option `refinement`, clamped)
    if (n >= 13) stats[12] = (double)e->pp.cw;             // columns of one LDS strip of the point x point gather (chosen at create from the scene)
    if (reset) e->solver.stat_launches = e->solver.stat_ms = e->solver.stat_flops = e->dm_stat_passes = e->dm_stat_ms = e->dm_stat_flops = 0.0;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_create_timings(jaicov_engine *e, double *ms, int32_t n) {
    if (!e || !ms) return JAICOV_ERR_BAD_ARGUMENT;
    for (int i = 0; i < n && i < 8; i++) ms[i] = e->create_ms[i];
    return JAICOV_OK;
}

// diagnostic / parity hook: the cached inverse dispersion inv(D) of image block `block` (DOPG:82-86 caches sigma0^2 inv(D / sigma0^2),
// which is sigma0^2 times this), m x m row-major in the CALLER's order of the block's observations
extern "C" int jaicov_neq_get_block_weight(jaicov_engine *e, int32_t block, double *out, size_t len) {
    if (!e || !out) return JAICOV_ERR_BAD_ARGUMENT;
    if (!e->h_caller_block.empty()) {      // the engine's internal blocks are the images; find the caller's
        int internal = -1;
        for (size_t g = 0; g < e->h_caller_block.size(); g++)
            if (e->h_caller_block[g] == block) internal = (int)g;
        block = internal;
    }
    if (block < 0 || block >= (int)e->h_blk_mine.size() || !e->h_blk_mine[block]) FAIL(e->err, JAICOV_ERR_BAD_ARGUMENT, "no such image block on this engine");
    const int b = e->h_blk_ip_begin[block], mpts = e->h_blk_ip_begin[block + 1] - b, m = 2 * mpts;
    if (len != (size_t)m * m) FAIL(e->err, JAICOV_ERR_BAD_ARGUMENT, "len must be (2 * points of the block)^2");
    HIPE(e->err, hipSetDevice(e->device));
    if (e->h_blk_w_off[block] < 0) FAIL(e->err, JAICOV_ERR_BAD_ARGUMENT, "this block has no dispersion of its own");
    std::vector<double> w((size_t)m * m);
    HIPE(e->err, hipMemcpy(w.data(), e->p.blk_w + e->h_blk_w_off[block], w.size() * sizeof(double), hipMemcpyDeviceToHost));
    const int32_t *perm = e->h_perm_local.empty() ? nullptr : e->h_perm_local.data() + b;
    for (int i = 0; i < m; i++) {
        const int si = perm ? 2 * perm[i >> 1] + (i & 1) : i;
        for (int j = 0; j < m; j++) {
            const int sj = perm ? 2 * perm[j >> 1] + (j & 1) : j;
            out[(size_t)si * m + sj] = w[(size_t)i * m + j];
        }
    }
    return JAICOV_OK;
}

extern "C" int jaicov_neq_last_timings(jaicov_engine *e, double *ms, int32_t n) {
    if (!e || !ms) return JAICOV_ERR_BAD_ARGUMENT;
    for (int i = 0; i < n && i < 8; i++) ms[i] = e->timings[i];
    return JAICOV_OK;
}

// BA.estimateModel (BA:203-387) + updateModel (BA:389-442); inversion modes NONE / FULL / REDUCED (PRE_ELIMINATION = REDUCED:
// the engine pre-eliminates the exterior orientations in every pass whenever the problem allows it)
extern "C" int jaicov_neq_estimate(jaicov_engine *e, const jaicov_estimate_options *o, jaicov_estimate_result *res) {
    if (!e || !o || !res || o->struct_size != sizeof(jaicov_estimate_options)) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state == jaicov_engine::ST_NEW) FAIL(e->err, JAICOV_ERR_BAD_STATE, "set_parameters first");
    const double SQRT_EPS = sqrt(EPS53);
    if (o->invert < 0 || o->invert > JAICOV_INVERT_FULL_EXPANDED) return JAICOV_ERR_BAD_ARGUMENT;
    // MatrixInversion.FULL: all of Qxx, computed from the EO-reduced system where the engine can (jaicov_neq.h, FULL_EXPANDED)
    const int inv_mode = o->invert == JAICOV_INVERT_FULL ? JAICOV_INVERT_FULL_EXPANDED : o->invert;
    const int max_iter = o->max_iterations;
    auto t0 = std::chrono::steady_clock::now();
    bool deriveFirst = o->lambda0 > 0;
    double adapted = 0.0;
    const double damping = fabs(o->lambda0);
    double maxAbsDx = 0.0, lastValid = 0.0, omega = 0.0;
    int runs = max_iter - 1;
    bool isEstimated = false, complete = false, isConverge = true;
    if (max_iter == 0) { complete = isEstimated = true; adapted = 0; }
    const double sigma2 = o->sigma2apriori > 0 ? o->sigma2apriori : 1.0;
    std::vector<double> dx(e->U > 0 ? e->U : 1);
    int state = 0, iter = 0, rc = JAICOV_OK;
    do {
        auto tp = std::chrono::steady_clock::now();
        maxAbsDx = 0.0;
        iter = max_iter - runs;
        if (deriveFirst) { adapted = damping; deriveFirst = false; }
        jaicov_neq_prepare_inverse(e, isEstimated ? inv_mode : JAICOV_INVERT_NONE);
        rc = jaicov_neq_build(e, sigma2, adapted, o->simulation);
        if (rc == JAICOV_ERR_OUT_OF_MEMORY) { state = -7; break; }
        if (rc) { state = rc == JAICOV_ERR_BAD_ARGUMENT || rc > 0 ? -2 : -1; break; }
        if (e->cancel.exchange(0)) { state = -1; rc = JAICOV_OK; break; }       // BA:240-245: INTERRUPT, flag cleared
        complete = isEstimated;
        rc = jaicov_neq_solve(e, complete ? inv_mode : JAICOV_INVERT_NONE, dx.data());
        if (rc == JAICOV_ERR_OUT_OF_MEMORY) { state = -7; break; }
        if (rc) { state = (rc > 0 || rc == JAICOV_ERR_BAD_ARGUMENT) ? -2 : -1; break; }
        bool rejected = false;
        if (adapted > 0) {
            double alpha = 0.25 * pow(adapted, -0.05);
            alpha = std::min(alpha, 0.75);
            for (auto &v : dx) v *= alpha;
            double prevOmega = omega, curOmega = 0.0;
            if ((rc = jaicov_neq_omega(e, sigma2, dx.data(), &curOmega))) { state = -1; break; }
            prevOmega = prevOmega <= 0 ? 1.7976931348623157e308 : prevOmega;
            const bool lmaConverge = prevOmega >= curOmega;
            omega = curOmega;
            if (lmaConverge) adapted *= 0.2;
            else {
                adapted *= 5.0;
                if (adapted > 1.0 / SQRT_EPS) { adapted = 1.0 / SQRT_EPS; omega = 0.0; }
            }
            if (!lmaConverge) { maxAbsDx = lastValid; rejected = true; }
        }
        if (!rejected) {
            if (complete) {
                if (o->simulation) omega = 0.0;
                else if ((rc = jaicov_neq_omega(e, sigma2, dx.data(), &omega))) { state = -1; break; }
            }
            if ((rc = jaicov_neq_update(e, dx.data(), &maxAbsDx))) { state = -1; break; }
            lastValid = maxAbsDx;
        }
        res->seconds_last_pass = std::chrono::duration<double>(std::chrono::steady_clock::now() - tp).count();
        if (e->cancel.exchange(0)) { state = -1; rc = JAICOV_OK; break; }       // BA:320-325
        if (std::isinf(maxAbsDx) || std::isnan(maxAbsDx)) { state = -2; break; }
        else if (maxAbsDx <= SQRT_EPS && runs > 0 && adapted == 0) isEstimated = true;
        else if (runs-- <= 1) {
            if (complete) isConverge = false;
            isEstimated = true;
        }
        if (isEstimated || adapted <= SQRT_EPS || runs < max_iter * 0.5 + 1) adapted = 0.0;
    } while (!complete);
    if (state == 0) state = isConverge ? 1 : -4;
    res->state = state;
    res->iterations = iter;
    res->omega = omega;
    res->max_abs_dx = maxAbsDx;
    res->final_lambda = adapted;
    res->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return (state == 1 || state == -4 || state == -2 || state == -1) ? (state == -1 && rc ? rc : JAICOV_OK) : rc;
}

// BundleAdjustment.interrupt() (BA:1455-1457): may be called from another thread while estimate() runs
extern "C" int jaicov_neq_cancel(jaicov_engine *e) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    e->cancel.store(1);
    return JAICOV_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// jaicov_dense.h: stand-alone dense SPD solve / inverse (MX.solve / MX.inv on UpperSPDPackMatrix, MX:239-264,304-324)
// ---------------------------------------------------------------------------------------------------------------
extern "C" int jaicov_dense_spd_solve_packed(int32_t n, double *ap, double *b, int32_t nrhs, int32_t invert, double *ms_out) {
    if (n <= 0 || !ap || nrhs < 0 || nrhs > DENSE_MAX_RHS || (nrhs > 0 && !b)) return JAICOV_ERR_BAD_ARGUMENT;
    std::string err;
    int rc = check_device(err);
    if (rc) return rc;
    DevStream stream;                  // first, so that the solver and the buffers go before the stream does
    if (stream.create() != hipSuccess) return JAICOV_ERR_DEVICE;
    const hipStream_t s = stream.get();
    const int np = ((n + 127) / 128) * 128;
    DenseSolver ds;
    DevBuf<double> ap_store, Y_store;
    DevEvent ev0, ev1;
    const size_t len = (size_t)n * (n + 1) / 2;
    if (ev0.create() != hipSuccess || ev1.create() != hipSuccess) return JAICOV_ERR_DEVICE;
    const hipEvent_t e0 = ev0.get(), e1 = ev1.get();
    if (ds.init(s, np, invert != 0, true) != hipSuccess || ap_store.reserve(len) != hipSuccess ||
        Y_store.reserve((size_t)DENSE_MAX_RHS * np) != hipSuccess)
        return JAICOV_ERR_OUT_OF_MEMORY;
    double *d_ap = ap_store.get(), *d_Y = Y_store.get();
    hipMemcpyAsync(d_ap, ap, len * sizeof(double), hipMemcpyHostToDevice, s);
    int info = 0;
    for (int attempt = 0;; attempt++) {      // an abandoned dataflow factorisation (-9) is repeated: the packed input is still there
        // identity padding, then unpack the lower triangle
        hipLaunchKernelGGL(load_disp_kernel, dim3((np + 255) / 256, np), dim3(256), 0, s, (const double *)nullptr, 0, ds.L, ds.ld, np, (const int32_t *)nullptr);
        hipLaunchKernelGGL(unpack_kernel, dim3((n + 255) / 256, n), dim3(256), 0, s, d_ap, ds.ld, n, ds.L);
        hipMemsetAsync(ds.rhs_row(0), 0, (size_t)128 * ds.ld * sizeof(double), s);
        for (int q = 0; q < nrhs; q++) hipMemcpyAsync(ds.rhs_row(q), b + (size_t)q * n, n * sizeof(double), hipMemcpyHostToDevice, s);
        hipEventRecord(e0, s);
        if (ds.potrf() != hipSuccess) { info = -1; break; }
        if (nrhs > 0) ds.backsolve_aug(d_Y, np, nrhs);
        if (invert) {
            ds.trtri();
            ds.lauum();
        }
        hipEventRecord(e1, s);
        info = ds.fetch_info();
        if (info == -9 && attempt < 2) {
            fprintf(stderr, "jaicov: factorisation abandoned on the device (a wait ran into its time limit); repeating it (%d)\n", attempt + 1);
            continue;
        }
        break;
    }
    if (info < 0) return JAICOV_ERR_DEVICE;
    if (info != 0) return JAICOV_ERR_SINGULAR;
    for (int q = 0; q < nrhs; q++) hipMemcpyAsync(b + (size_t)q * n, d_Y + (size_t)q * np, n * sizeof(double), hipMemcpyDeviceToHost, s);
    if (invert) {
        hipLaunchKernelGGL(pack_kernel, dim3((n + 255) / 256, n), dim3(256), 0, s, ds.Q, ds.ld, n, d_ap);
        hipMemcpyAsync(ap, d_ap, len * sizeof(double), hipMemcpyDeviceToHost, s);
    }
    const bool ok = hipStreamSynchronize(s) == hipSuccess;
    if (ms_out) { float ms = 0; hipEventElapsedTime(&ms, e0, e1); *ms_out = ms; }
    return ok ? JAICOV_OK : JAICOV_ERR_DEVICE;
}

namespace jaicov { hipError_t diag_kernel_bench(int dbg, int iters, float *ms_out); hipError_t mfma_peak_bench(int, int, float *, double *); }
namespace jaicov { hipError_t cumask_bench(const uint32_t *, int, int, float *, double *); }
// Per-workgroup timeline of one trailing-update shaped GEMM (C -= A A', K columns): out[8 * tiles]
// The plan of jaicov_neq_create alone (create_plan.h): no device is looked for and nothing is created on one.  Returns the plan's status,
// leaves its text in err and its decisions in summary: {blocks of the effective description, synthesized, compact, permuted, n_seg,
// n_blk_list, n_blk_ip, max_m, w_total (saturated), schur_ok, e0, cw, n_chunks, cmin, cmax, plain_ok}.  tests/test_create_plan.py
extern "C" int jaicov_debug_create_plan(const jaicov_problem_desc *desc, const jaicov_engine_options *opts, int assembly_form, int32_t *summary,
                                        int n_summary, char *err, int err_cap) {
    if (!desc || desc->struct_size != sizeof(jaicov_problem_desc) || (opts && opts->struct_size != sizeof(jaicov_engine_options))) return JAICOV_ERR_BAD_ARGUMENT;
    CreatePlan pl;
    build_create_plan(pl, *desc, opts ? *opts : default_options(), assembly_form);
    if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "%s", pl.err.c_str());
    const int64_t s[16] = {pl.D.n_image_blocks, pl.synthesized, pl.compact_blocks, !pl.ip_old2new.empty(), (int64_t)pl.seg_b.size(),
                           (int64_t)pl.blk_list.size(), (int64_t)pl.blk_ip_list.size(), pl.max_m, std::min<int64_t>(pl.w_total, INT32_MAX),
                           pl.schur_ok, pl.e0, pl.cw, pl.n_chunks, pl.cmin, pl.cmax, pl.plain_ok};
    for (int i = 0; summary && pl.status == JAICOV_OK && i < n_summary && i < 16; i++) summary[i] = (int32_t)s[i];
    return pl.status;
}

// One table of the same plan.  which: 0 ip_old2new, 1 seg_b, 2 seg_e, 3 blk_list, 4 range, 5 the gather's records as (ipb, mp, lp),
// 6 blk_ip_begin of the effective description.  Returns the number of entries (out == NULL: nothing else), or the plan's status (< 0).
extern "C" int jaicov_debug_create_plan_table(const jaicov_problem_desc *desc, const jaicov_engine_options *opts, int assembly_form, int which,
                                              int32_t *out, int cap) {
    if (!desc || desc->struct_size != sizeof(jaicov_problem_desc) || (opts && opts->struct_size != sizeof(jaicov_engine_options))) return JAICOV_ERR_BAD_ARGUMENT;
    CreatePlan pl;
    if (!build_create_plan(pl, *desc, opts ? *opts : default_options(), assembly_form)) return pl.status;
    std::vector<int32_t> recs;
    for (const PPRecord &r : pl.recs) recs.insert(recs.end(), {r.ipb, r.mp, r.lp});
    const std::vector<int32_t> *tables[7] = {&pl.ip_old2new, &pl.seg_b, &pl.seg_e, &pl.blk_list, &pl.range, &recs, &pl.blk_ip_begin};
    if (which < 0 || which >= 7) return JAICOV_ERR_BAD_ARGUMENT;
    const std::vector<int32_t> &t = *tables[which];
    if (out) std::copy(t.begin(), t.begin() + std::min<size_t>(t.size(), (size_t)std::max(cap, 0)), out);
    return (int)t.size();
}

extern "C" int jaicov_debug_gemm_trace(int M, int K, int lower_only, long long *out) {
    std::string err;
    if (check_device(err)) return JAICOV_ERR_NO_DEVICE;
    const int tm = M / 128, tiles = lower_only ? tm * (tm + 1) / 2 : tm * tm;
    DevBuf<double> A_store, C_store;
    DevBuf<long long> T_store;
    if (A_store.reserve((size_t)M * K) != hipSuccess || C_store.reserve((size_t)M * M) != hipSuccess || T_store.reserve((size_t)tiles * 8) != hipSuccess)
        return JAICOV_ERR_OUT_OF_MEMORY;
    double *dA = A_store.get(), *dC = C_store.get(); long long *dT = T_store.get();
    hipMemset(dC, 0, (size_t)M * M * 8); hipMemset(dT, 0, (size_t)tiles * 64);
    {   // random operands (the matrix pipe draws more power on them than on zeros) and a warm chip
        std::vector<double> h((size_t)M * K);
        uint64_t x = 88172645463325252ull;
        for (auto &v : h) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; v = (double)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5; }
        hipMemcpy(dA, h.data(), h.size() * 8, hipMemcpyHostToDevice);
    }
    GemmArgs g{};
    g.A = dA; g.B = dA; g.C = dC; g.lda = K; g.ldb = K; g.ldc = M; g.M = M; g.N = M; g.K = K;
    g.alpha = -1e-3; g.beta = 1.0; g.lower_only = lower_only; g.kmode = KMODE_FULL;
    int warm = 40;
    if (const char *e = getenv("JAICOV_TRACE_WARM")) warm = atoi(e);
    const int tag = getenv("JAICOV_TRACE_TAG") ? atoi(getenv("JAICOV_TRACE_TAG")) : 0;
    for (int i = 0; i < warm; i++) gemm_f64(nullptr, LAY_KC, LAY_KC, g, 1, 0, tag);
    g.trace = dT;
    hipError_t he = gemm_f64(nullptr, LAY_KC, LAY_KC, g, 1, 0, tag);
    he = he == hipSuccess ? hipDeviceSynchronize() : he;
    hipMemcpy(out, dT, (size_t)tiles * 64, hipMemcpyDeviceToHost);
    return he == hipSuccess ? JAICOV_OK : JAICOV_ERR_DEVICE;
}

extern "C" int jaicov_debug_cumask(const uint32_t *mask, int blocks, int iters, double *ms_out, double *tflops) {
    float ms = 0;
    hipError_t he = jaicov::cumask_bench(mask, blocks, iters, &ms, tflops);
    *ms_out = ms;
    return he == hipSuccess ? 0 : (int)he;
}
extern "C" int jaicov_debug_mfma_peak(int blocks, int iters, double *ms_out, double *tflops) {
    float ms = 0;
    hipError_t he = jaicov::mfma_peak_bench(blocks, iters, &ms, tflops);
    *ms_out = ms;
    return he == hipSuccess ? 0 : -5;
}
extern "C" int jaicov_debug_diag_bench(int dbg, int iters, double *ms_out) {
    float ms = 0;
    hipError_t he = jaicov::diag_kernel_bench(dbg, iters, &ms);
    *ms_out = ms;
    return he == hipSuccess ? 0 : -5;
}

// Stand-alone timing of the factorisation on a synthetic SPD matrix of order n (multiple of 128): M = R + n I, R uniform in
// (-0.5, 0.5), right-hand-side rows random.  ms_out[r] = device time of repetition r (HIP events on the solver's stream).
// trace_out (optional, dataflow factorisation only): [tasks][8] of the LAST repetition, see cholflow.hip; tasks_out = task count.
__global__ void fill_spd_kernel(double *L, long ld, int n, int nfact) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j > i || i >= n) return;
    unsigned long long x = 0x9E3779B97F4A7C15ull * ((unsigned long long)i * 65537ull + (unsigned long long)j + 1ull);
    x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
    double v = (double)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5;
    if (i == j && i < nfact) v += (double)nfact;
    L[(long)i * ld + j] = v;
}
extern "C" int jaicov_debug_potrf_bench(int n, int reps, double *ms_out, long long *trace_out, long long trace_cap, int *tasks_out) {
    std::string err;
    if (check_device(err)) return JAICOV_ERR_NO_DEVICE;
    if (n <= 0 || n % 128 || reps < 1 || !ms_out) return JAICOV_ERR_BAD_ARGUMENT;
    DevStream stream;                  // first, so that the solver goes before the stream does
    if (stream.create(hipStreamNonBlocking) != hipSuccess) return JAICOV_ERR_DEVICE;
    const hipStream_t s = stream.get();
    DenseSolver ds;
    DevEvent ev0, ev1;
    if (ev0.create() != hipSuccess || ev1.create() != hipSuccess) return JAICOV_ERR_DEVICE;
    const hipEvent_t e0 = ev0.get(), e1 = ev1.get();
    if (ds.init(s, n, false, true) != hipSuccess) return JAICOV_ERR_OUT_OF_MEMORY;
    if (trace_out && ds.flow.ready()) ds.flow.enable_trace(true);
    for (int r = 0; r < reps; r++) {
        hipLaunchKernelGGL(fill_spd_kernel, dim3((ds.n + 255) / 256, ds.n), dim3(256), 0, s, ds.L, ds.ld, ds.n, n);
        hipEventRecord(e0, s);
        const hipError_t pe = ds.potrf();
        if (pe != hipSuccess) { fprintf(stderr, "potrf: %s\n", hipGetErrorString(pe)); return JAICOV_ERR_DEVICE; }
        hipEventRecord(e1, s);
        const int info = ds.fetch_info();
        if (info < 0) fprintf(stderr, "potrf: info %d (flow_ready %d)\n", info, (int)ds.flow.ready());
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        ms_out[r] = ms;
        if (info < 0) return JAICOV_ERR_DEVICE;
        if (info != 0) return JAICOV_ERR_SINGULAR;
    }
    if (trace_out && ds.flow.trace()) {
        const long long cnt = std::min<long long>(trace_cap, (long long)ds.flow.trace_words());   // per task, then per block column (chain kernel)
        hipMemcpy(trace_out, ds.flow.trace(), (size_t)cnt * sizeof(long long), hipMemcpyDeviceToHost);
    }
    if (tasks_out) *tasks_out = ds.flow.ready() ? ds.flow.n_tasks() : 0;
    hipStreamSynchronize(s);
    return JAICOV_OK;
}

// debug: factor a host matrix (n x n row-major, lower part used, n a multiple of 128) with DenseSolver::potrf and return the
// factor (lower part, row-major n x n) -- scripts/flow_small_check.py compares it tile by tile with LAPACK
extern "C" int jaicov_debug_potrf_factor(int n, const double *A, double *L_out) {
    std::string err;
    if (check_device(err)) return JAICOV_ERR_NO_DEVICE;
    if (n <= 0 || n % 128 || !A || !L_out) return JAICOV_ERR_BAD_ARGUMENT;
    DevStream stream;                  // first, so that the solver goes before the stream does
    if (stream.create(hipStreamNonBlocking) != hipSuccess) return JAICOV_ERR_DEVICE;
    const hipStream_t s = stream.get();
    DenseSolver ds;
    if (ds.init(s, n, false, true) != hipSuccess) return JAICOV_ERR_OUT_OF_MEMORY;
    hipLaunchKernelGGL(fill_spd_kernel, dim3((ds.n + 255) / 256, ds.n), dim3(256), 0, s, ds.L, ds.ld, ds.n, n);   // incl. the right-hand-side rows
    if (hipMemcpy2DAsync(ds.L, ds.ld * sizeof(double), A, (size_t)n * sizeof(double), (size_t)n * sizeof(double), n, hipMemcpyHostToDevice, s) != hipSuccess) return JAICOV_ERR_DEVICE;
    if (ds.potrf() != hipSuccess) return JAICOV_ERR_DEVICE;
    const int info = ds.fetch_info();
    if (info < 0) return JAICOV_ERR_DEVICE;
    if (info > 0) return JAICOV_ERR_SINGULAR;
    const bool copied = hipMemcpy2DAsync(L_out, (size_t)n * sizeof(double), ds.L, ds.ld * sizeof(double), (size_t)n * sizeof(double), n, hipMemcpyDeviceToHost, s) == hipSuccess;
    hipStreamSynchronize(s);
    return copied ? JAICOV_OK : JAICOV_ERR_DEVICE;
}

// debug: one step of newton_schulz_exact (batchinv.hip) on host matrices: M and Q0 full symmetric squares, n x n row-major, n a multiple
// of 128 up to 8192.  On the device they stand with the leading dimension the solver gives them (n + 128, its right-hand-side rows beside the
// factor, filled with NaN here), not n.  Q_out = the refined inverse; R_out (optional) = the residual square I - M Q0 as the step formed it, before the product
// Q0 R -- tests/test_gpu_inverse_refinement.py holds both
extern "C" int jaicov_debug_newton_schulz(int n, const double *M, const double *Q0, double *Q_out, double *R_out) {
    std::string err;
    if (check_device(err)) return JAICOV_ERR_NO_DEVICE;
    if (n <= 0 || n % 128 || n > 8192 || !M || !Q0 || !Q_out) return JAICOV_ERR_BAD_ARGUMENT;
    DevStream stream;                  // first, so that the buffer goes before the stream does
    if (stream.create(hipStreamNonBlocking) != hipSuccess) return JAICOV_ERR_DEVICE;
    const hipStream_t s = stream.get();
    const long ld = (long)n + 128;
    const size_t sq = (size_t)n * ld, row = (size_t)n * sizeof(double);
    DevBuf<double> store;                                // M, Q, W, T1, T2, T3
    if (store.reserve(6 * sq) != hipSuccess) return JAICOV_ERR_OUT_OF_MEMORY;
    double *buf = store.get();
    double *dM = buf, *dQ = buf + sq, *dW = buf + 2 * sq, *T1 = buf + 3 * sq, *T2 = buf + 4 * sq, *T3 = buf + 5 * sq;
    // M and Q start as NaN (all bits set) and the work squares as zero: the columns n .. n + 127, where the solver keeps its right-hand-side
    // rows, then hold NaN beside both operands, and a slice or product that read up to ld instead of n would show in every entry
    if (hipMemsetAsync(buf, 0xFF, 2 * sq * sizeof(double), s) != hipSuccess ||
        hipMemsetAsync(buf + 2 * sq, 0, 4 * sq * sizeof(double), s) != hipSuccess ||
        hipMemcpy2DAsync(dM, ld * sizeof(double), M, row, row, n, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpy2DAsync(dQ, ld * sizeof(double), Q0, row, row, n, hipMemcpyHostToDevice, s) != hipSuccess ||
        newton_schulz_exact(s, n, ld, dM, dQ, dW, T1, T2, T3) != hipSuccess ||
        hipMemcpy2DAsync(Q_out, row, dQ, ld * sizeof(double), row, n, hipMemcpyDeviceToHost, s) != hipSuccess ||
        (R_out && hipMemcpy2DAsync(R_out, row, T3, ld * sizeof(double), row, n, hipMemcpyDeviceToHost, s) != hipSuccess))   // (the product Q0 R went to T1)
        return JAICOV_ERR_DEVICE;
    return hipStreamSynchronize(s) == hipSuccess ? JAICOV_OK : JAICOV_ERR_DEVICE;
}

// C (M x N row-major) = alpha * op(A) op(B) + beta * C on the device, host buffers in/out (kernel parity + timing)
extern "C" int jaicov_dense_gemm(int32_t alay, int32_t blay, int32_t M, int32_t N, int32_t K, double alpha, const double *A,
                                 int64_t lda, const double *B, int64_t ldb, double beta, double *C, int64_t ldc,
                                 int32_t lower_only, int32_t kmode, int32_t repeats, double *ms_out) {

    if (M % 128 || N % 128 || K % 16 || M <= 0 || N <= 0 || K <= 0 || !A || !B || !C) return JAICOV_ERR_BAD_ARGUMENT;
    if (alpha == 0.0) return JAICOV_ERR_BAD_ARGUMENT;      // gemm_f64_plan refuses it: the kernel forms (beta/alpha) C
    std::string err;
    int rc = check_device(err);
    if (rc) return rc;
    const size_t sa = (size_t)(alay == LAY_KC ? M : K) * lda, sb = (size_t)(blay == LAY_KC ? N : K) * ldb, sc = (size_t)M * ldc;
    DevBuf<double> A_store, B_store, C_store;
    DevEvent ev0, ev1;
    if (A_store.reserve(sa) != hipSuccess || B_store.reserve(sb) != hipSuccess || C_store.reserve(sc) != hipSuccess) return JAICOV_ERR_OUT_OF_MEMORY;
    if (ev0.create() != hipSuccess || ev1.create() != hipSuccess) return JAICOV_ERR_DEVICE;
    double *dA = A_store.get(), *dB = B_store.get(), *dC = C_store.get();
    const hipEvent_t e0 = ev0.get(), e1 = ev1.get();
    hipMemcpy(dA, A, sa * 8, hipMemcpyHostToDevice);
    hipMemcpy(dB, B, sb * 8, hipMemcpyHostToDevice);
    hipMemcpy(dC, C, sc * 8, hipMemcpyHostToDevice);
    GemmArgs g{};
    g.A = dA; g.B = dB; g.C = dC; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.alpha = alpha; g.beta = beta; g.lower_only = lower_only; g.kmode = kmode;
    hipError_t he = gemm_f64(nullptr, alay, blay, g);
    hipMemcpy(C, dC, sc * 8, hipMemcpyDeviceToHost);
    if (repeats > 0) {
        hipEventRecord(e0, nullptr);
        for (int r = 0; r < repeats; r++) gemm_f64(nullptr, alay, blay, g);
        hipEventRecord(e1, nullptr);
        hipEventSynchronize(e1);
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        if (ms_out) *ms_out = ms / repeats;
    }
    he = he == hipSuccess ? hipDeviceSynchronize() : he;
    return he == hipSuccess ? JAICOV_OK : JAICOV_ERR_DEVICE;
}

// debug: ONE launch of gemm_f64() with every argument of the launcher in the caller's hand (tests/test_gpu_gemm_family.py), and the plan
// of that launch without a device (plan_only, tests/test_gemm_plan.py).  Not declared under include/: no product calls it.
//   A, B, C: host buffers of n_A, n_B, n_C doubles.  c_alias 1 / 2: C is A / B -- one device buffer holds the operand's n_A / n_B doubles,
//   the launch gets the same pointer twice, and the whole buffer comes back in C (n_C must equal that count).  A == B with n_A == n_B: one
//   buffer, the same pointer for both operands.  tile_map: n_map (row, col) pairs, row < 0 = no tile.
//   plan_out[7] = {hipError_t of the plan, TM, TN, tag, grid x, y, z}; filled whenever the arguments themselves are in order.
// Refused with JAICOV_ERR_BAD_ARGUMENT, before anything is uploaded: what the plan refuses (alpha == 0, in place with more than one
// column tile), tag >= 2 (the timing experiments: wrong results on purpose), and every extent, leading dimension, stride, count or map
// entry with which an access of the launch could leave the uploaded buffers.  The test of that is the full rectangle of each operand in
// every batch of the batch rectangle (batch_sum_limit only removes batches), so it does not depend on the k ranges or the map.
struct jaicov_debug_gemm_args {
    uint32_t struct_size;
    int32_t alay, blay, M, N, K;
    double alpha, beta;
    const double *A; int64_t n_A;
    const double *B; int64_t n_B;
    double *C; int64_t n_C;
    int64_t lda, ldb, ldc;
    int32_t c_alias, lower_only, kmode, batch, batch2;
    int64_t strideA, strideB, strideC, strideA2, strideB2, strideC2;
    int32_t batch_sum_limit, small_tiles, tag;
    const int32_t *tile_map; int32_t n_map;
    int32_t plan_only;
    int32_t *plan_out;
};
extern "C" int jaicov_debug_gemm(const jaicov_debug_gemm_args *a) {
    if (!a || a->struct_size != sizeof(jaicov_debug_gemm_args)) return JAICOV_ERR_BAD_ARGUMENT;
    if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->M % 128 || a->N % 128 || a->K % 16 || a->M > 32768 || a->N > 32768 || a->K > 32768) return JAICOV_ERR_BAD_ARGUMENT;
    if ((a->alay != LAY_KC && a->alay != LAY_XC) || (a->blay != LAY_KC && a->blay != LAY_XC) || a->kmode < KMODE_FULL || a->kmode > KMODE_GE_COL) return JAICOV_ERR_BAD_ARGUMENT;
    if (a->c_alias < 0 || a->c_alias > 2 || a->batch < 1 || a->batch2 < 1 || a->batch > 1024 || a->batch2 > 1024 || a->batch_sum_limit < 0) return JAICOV_ERR_BAD_ARGUMENT;
    if (a->tag < 0 || a->tag >= 2 || a->n_map < 0 || (a->n_map > 0 && !a->tile_map) || a->n_map > (1 << 22)) return JAICOV_ERR_BAD_ARGUMENT;
    if (a->lower_only && a->M != a->N) return JAICOV_ERR_BAD_ARGUMENT;
    const bool same_ab = a->A == a->B && a->n_A == a->n_B;
    // the plan sees the aliasing through pointer equality alone: stand-ins with the same equalities as the device pointers will have
    static const double stand_in[3] = {0, 0, 0};
    GemmArgs g{};
    g.A = stand_in; g.B = same_ab ? stand_in : stand_in + 1;
    g.C = const_cast<double *>(a->c_alias == 1 ? g.A : a->c_alias == 2 ? g.B : stand_in + 2);
    g.lda = a->lda; g.ldb = a->ldb; g.ldc = a->ldc; g.M = a->M; g.N = a->N; g.K = a->K; g.alpha = a->alpha; g.beta = a->beta;
    g.lower_only = a->lower_only != 0; g.kmode = a->kmode;
    g.strideA = a->strideA; g.strideB = a->strideB; g.strideC = a->strideC;
    g.strideA2 = a->strideA2; g.strideB2 = a->strideB2; g.strideC2 = a->strideC2;
    g.batch_sum_limit = a->batch_sum_limit;
    g.tile_map = a->n_map > 0 ? reinterpret_cast<const int2 *>(stand_in) : nullptr; g.n_map = a->n_map;
    const GemmPlan p = gemm_f64_plan(a->alay, a->blay, g, a->batch, a->small_tiles, a->tag, a->batch2);
    if (a->plan_out) {
        const int32_t out[7] = {(int32_t)p.status, p.TM, p.TN, p.tag, (int32_t)p.grid_x, (int32_t)p.grid_y, (int32_t)p.grid_z};
        std::copy(out, out + 7, a->plan_out);
    }
    if (p.status != hipSuccess || p.TM == 0) return JAICOV_ERR_BAD_ARGUMENT;
    if (a->plan_only) return JAICOV_OK;

    // ---- every access of the launch stays inside the buffers: decided here, on the host -------------------------------------------------
    if (!a->A || !a->B || !a->C) return JAICOV_ERR_BAD_ARGUMENT;
    const int64_t a_rows = a->alay == LAY_KC ? a->M : a->K, a_cols = a->alay == LAY_KC ? a->K : a->M;
    const int64_t b_rows = a->blay == LAY_KC ? a->N : a->K, b_cols = a->blay == LAY_KC ? a->K : a->N;
    auto inside = [&](int64_t rows, int64_t cols, int64_t ld, int64_t s1, int64_t s2, int64_t count) {   // all factors are bounded above: no overflow
        if (ld < cols || ld > (1 << 20) || ld % 2 || s1 % 2 || s2 % 2 ||       // (even: the kernel loads the operands in pairs of doubles)
            s1 < 0 || s2 < 0 || s1 > ((int64_t)1 << 32) || s2 > ((int64_t)1 << 32) || count <= 0) return false;
        return (a->batch - 1) * s1 + (a->batch2 - 1) * s2 + (rows - 1) * ld + cols <= count;
    };
    const int64_t count_c = a->c_alias == 1 ? a->n_A : a->c_alias == 2 ? a->n_B : a->n_C;
    if (!inside(a_rows, a_cols, a->lda, a->strideA, a->strideA2, a->n_A) || !inside(b_rows, b_cols, a->ldb, a->strideB, a->strideB2, a->n_B) ||
        !inside(a->M, a->N, a->ldc, a->strideC, a->strideC2, count_c) || a->n_C != count_c)
        return JAICOV_ERR_BAD_ARGUMENT;
    if (p.use_map) {       // in tiles of the plan's instance; the lower grid takes what the map says, so the map decides what is written
        if ((int64_t)p.grid_x != a->n_map) return JAICOV_ERR_BAD_ARGUMENT;
        for (int i = 0; i < a->n_map; i++) {
            const int r = a->tile_map[2 * i], c = a->tile_map[2 * i + 1];
            if (r >= 0 && (r >= a->M / p.TM || c < 0 || c >= a->N / p.TN)) return JAICOV_ERR_BAD_ARGUMENT;
        }
    }
    std::string err;
    const int rc = check_device(err);
    if (rc) return rc;
    {
        DevBuf<double> A_store, B_store, C_store;
        DevBuf<int2> map_store;
        if (A_store.reserve((size_t)a->n_A) != hipSuccess || (!same_ab && B_store.reserve((size_t)a->n_B) != hipSuccess) ||
            (a->c_alias == 0 && C_store.reserve((size_t)a->n_C) != hipSuccess) || (p.use_map && map_store.reserve((size_t)a->n_map) != hipSuccess))
            return JAICOV_ERR_OUT_OF_MEMORY;
        double *dA = A_store.get(), *dB = same_ab ? dA : B_store.get();
        double *dC = a->c_alias == 1 ? dA : a->c_alias == 2 ? dB : C_store.get();
        if (hipMemcpy(dA, a->A, (size_t)a->n_A * 8, hipMemcpyHostToDevice) != hipSuccess ||
            (!same_ab && hipMemcpy(dB, a->B, (size_t)a->n_B * 8, hipMemcpyHostToDevice) != hipSuccess) ||
            (a->c_alias == 0 && hipMemcpy(dC, a->C, (size_t)a->n_C * 8, hipMemcpyHostToDevice) != hipSuccess) ||
            (p.use_map && hipMemcpy(map_store.get(), a->tile_map, (size_t)a->n_map * sizeof(int2), hipMemcpyHostToDevice) != hipSuccess))
            return JAICOV_ERR_DEVICE;
        g.A = dA; g.B = dB; g.C = dC;
        g.tile_map = p.use_map ? map_store.get() : nullptr; g.n_map = p.use_map ? a->n_map : 0;
        const GemmPlan q = gemm_f64_plan(a->alay, a->blay, g, a->batch, a->small_tiles, a->tag, a->batch2);   // the device pointers alias as the stand-ins did
        if (q.status != p.status || q.TM != p.TM || q.TN != p.TN || q.tag != p.tag || q.grid_x != p.grid_x || q.use_map != p.use_map) return JAICOV_ERR_BAD_STATE;
        hipError_t he = gemm_f64(nullptr, a->alay, a->blay, g, a->batch, a->small_tiles, a->tag, a->batch2);
        he = he == hipSuccess ? hipDeviceSynchronize() : he;
        if (he != hipSuccess) return JAICOV_ERR_DEVICE;
        if (hipMemcpy(a->C, dC, (size_t)a->n_C * 8, hipMemcpyDeviceToHost) != hipSuccess) return JAICOV_ERR_DEVICE;
    }
    return JAICOV_OK;
}

// debug: xcd_tile_map(T) of gemm_f64.h as (row, col) pairs; returns the number of pairs (out == NULL or cap too small: nothing else)
extern "C" int jaicov_debug_xcd_tile_map(int T, int32_t *out, int cap) {
    if (T < 1 || T > 4096) return JAICOV_ERR_BAD_ARGUMENT;
    const std::vector<int2> m = xcd_tile_map(T);
    if (out && cap >= (int)m.size())
        for (size_t i = 0; i < m.size(); i++) { out[2 * i] = m[i].x; out[2 * i + 1] = m[i].y; }
    return (int)m.size();
}
