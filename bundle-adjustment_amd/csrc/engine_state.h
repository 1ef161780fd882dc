// engine_state.h -- struct jaicov_engine and what the engine's own translation units share: engine.hip (lifecycle, accumulate /
// finalize / build, getters), engine_create.hip (the device stage of creation) and engine_solve.hip (solve, estimate).  Private to
// those three: whatever reads the cofactor matrix goes through qview.h / engine_q_view and never sees a field.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/jaicov_neq.h"
#include "ba_kernels.h"
#include "dense.h"
#include "devbuf.h"
#include "qview.h"
#include "status.h"

using namespace jaicov;      // (a header of three .hip files that all say so themselves)

// ev[] of the engine: marks on the engine's stream, in the order a pass records them
enum EvSlot {
    EV_ACC_BEGIN, EV_ROWS, EV_ASSEMBLED,      // accumulate: its start, the compact rows, the normal equations
    EV_BUILT,                                 // finalize
    EV_BORDER, EV_FACTORED, EV_SUBSTITUTED,   // solve: the datum rows are up, the factor, the step
    EV_SOLVED,                                // ... its end
    EV_OMEGA_BEGIN, EV_OMEGA_END,             // jaicov_neq_omega
    EV_COUNT
};
// jaicov_engine::timings[] as jaicov_neq_last_timings hands them out (ms, between the marks above)
enum TimingSlot { T_ROWS, T_ASSEMBLY, T_FINALIZE, T_FACTOR, T_SOLVE /* substitution + refinement */, T_INVERSE, T_OMEGA, T_TOTAL, T_COUNT };
// jaicov_engine::create_ms[] as jaicov_neq_create_timings hands them out (ms, host wall clock)
enum CreateSlot {
    CREATE_TOTAL,         // the whole call
    CREATE_DISP_UPLOAD,   // host time in the dispersion uploads
    CREATE_WEIGHTS,       // dispersions -> weights
    CREATE_STRUCTURE,     // validation + tables (the plan, create_plan.h) + structure upload
    CREATE_WORK,          // work buffers + full-order solver
    CREATE_ELIMINATION,   // EO pre-elimination buffers + reduced solver
    CREATE_COUNT = 8
};

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
    double timings[T_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};          // TimingSlot
    double create_ms[CREATE_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};   // CreateSlot
    DevEvent ev[EV_COUNT];                               // EvSlot
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
    QSlots slot;
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

static inline double ms_since(std::chrono::steady_clock::time_point t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

namespace jaicov {
// engine_create.hip: everything jaicov_neq_create does once the engine object exists
int engine_create_impl(jaicov_engine *e, const jaicov_problem_desc *desc);
// engine_solve.hip, also asked by jaicov_neq_prepare_inverse and jaicov_neq_expansion_buffer (engine.hip)
int ensure_inverse_buffers(jaicov_engine *e, bool reduced_system, int mode);
bool expansion_fits(const jaicov_engine *e, size_t *I6p, size_t *Up);
int effective_invert(const jaicov_engine *e, int invert);
}  // namespace jaicov
