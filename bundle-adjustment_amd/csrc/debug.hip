// jaicov_debug_*: the bench, trace and parity hooks that scripts and tests call and no product does.  None of them touches an engine.
// gfx950 only.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "batchinv.h"
#include "create_plan.h"
#include "dense.h"
#include "gemm_f64.h"
#include "launchers.h"
#include "status.h"

using namespace jaicov;

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

// Per-workgroup timeline of one trailing-update shaped GEMM (C -= A A', K columns): out[8 * tiles]
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
