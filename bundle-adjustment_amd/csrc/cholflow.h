// Host side of the dataflow Cholesky (cholflow.hip): which form of the factorisation a solver uses (a pure function of the order, of
// what the host can do and of the test hooks), where its flag words lie, and the object that owns everything the factorisation needs
// beyond the solver's own matrix.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stddef.h>

#include <vector>

#include "devbuf.h"

namespace jaicov {

// ---- hooks and decision ---------------------------------------------------------------------------------------------------------------
// JAICOV_FACTOR_FORM = streams | two_step | one_kernel | chain2 | chain3: the forms of the factorisation other than the default (dataflow, chain
// form), each named by a case of tests/test_gpu_parity.py (test_factor_tile_by_tile, test_config3_step_against_oracle).
enum { FACTOR_DEFAULT = 0, FACTOR_STREAMS = 1, FACTOR_TWO_STEP = 2, FACTOR_ONE_KERNEL = 3, FACTOR_CHAIN2 = 4, FACTOR_CHAIN3 = 5 };

// Every environment hook of the solver, parsed by flow_hooks() and nowhere else.  WHEN a hook takes effect is up to who calls flow_hooks():
// a solver keeps the hooks it was initialised under (form, min_blocks, split, trace_on, chain_trace: the tests switch them between engines of
// one process) and asks again at every factorisation for timeout_ms and verbose, at every substitution for chain8_min_nb (chains.h,
// chain_decide): the tests set those around single calls.
constexpr int HOOK_UNSET = INT_MIN;
struct FlowHooks {
    int form = FACTOR_DEFAULT;     // JAICOV_FACTOR_FORM
    int min_blocks = HOOK_UNSET;   // JAICOV_FLOW_MIN_BLOCKS (the tests lower it)
    int split_m = 0, split_from = 0;   // JAICOV_FLOW_SPLIT="m:from" (0 pieces: not set)
    int timeout_ms = HOOK_UNSET;   // JAICOV_FLOW_TIMEOUT_MS (the tests set 0)
    bool trace_on = false;         // JAICOV_FLOW_TRACE_ON: per-task timestamps, read by FlowFactor::report_stall
    int chain8_min_nb = HOOK_UNSET;   // JAICOV_CHAIN8_MIN_NB (the tests lower it)
    bool chain_trace = false;      // JAICOV_CHAIN_TRACE: development, link times of the backward chain on stderr
    bool verbose = false;          // JAICOV_VERBOSE
};
FlowHooks flow_hooks();

struct FlowDecision {
    bool use_flow;       // the dataflow factorisation (else dense.hip's stream-scheduled one)
    bool one_kernel;     // ... as ONE kernel with inline diagonal blocks (kernels cannot run side by side on this host)
    bool chain;          // ... with potrf_chain_kernel as companion (else potrf_diag_chain_kernel, "two_step")
    int second;          // third chain workgroup: 0 = none, 2 = it finishes tile (c+2, c) and subtracts it from (c+2, c+1)
    int split_m, split_from;   // update ranges of the tasks of the block columns >= split_from are cut into split_m pieces (1: none)
};
// nb block columns to factorise; `kernels_overlap`: two kernels of this process can run at the same time (does not bear on use_flow)
FlowDecision flow_decide(int nb, bool kernels_overlap, const FlowHooks &h);

// ---- flag words -----------------------------------------------------------------------------------------------------------------------
// control words
enum { FLOW_TICKET = 0, FLOW_ABORT = 1, FLOW_DIAG_NEXT = 2, FLOW_CHAIN_AT = 3, FLOW_STALE = 4, FLOW_STALE_CONFIRMED = 5, FLOW_RESCUED = 6, FLOW_WG_OFF = 7, FLOW_CTRL_WORDS = 16 };   // RESCUED: hits of the read-modify-write poll after > 1 ms of waiting   // CHAIN_AT: column << 4 | stage of the chain workgroup
constexpr int FLOW_MAX_GRID = 1024;      // most workgroups the tile kernel is launched with: one state word each, and one more for the snapshot

// Offsets (in words) of the regions of the flag allocation, in this order, and its length.
struct FlowLayout {
    size_t done;         // [row blocks][nb]  after the FLOW_CTRL_WORDS control words
    size_t applied;      // [row blocks][nb]
    size_t diag_ready;   // [nb]
    size_t factored;     // [nb]
    size_t wgstate;      // [FLOW_MAX_GRID] one state word per workgroup ...
    size_t wgsnap;       // [FLOW_MAX_GRID] ... and their copy at the moment a wait ran out (flow_give_up)
    size_t pflag;        // [partials]
    size_t words;
};
FlowLayout flow_layout(int nb, int row_blocks, int partials);

// ---- the factorisation ----------------------------------------------------------------------------------------------------------------
// What FlowFactor uses and does not own: the solver's matrix and streams.  Handed over once, at init; the solver outlives its FlowFactor.
struct FlowView {
    double *L;           // n x ld, the matrix / the factor
    long ld;
    double *invd;        // inverses of the diagonal blocks
    int *d_info;         // first failing pivot
    int nfact, n;        // order that is factorised; rows of L (the right-hand-side rows included)
    hipStream_t stream;  // the tile kernel, and everything the caller orders around the factorisation
    hipStream_t pstream; // a stream that is never behind a kernel of the factorisation (to reach the abort word), may be null
    hipStream_t dstream; // the companion kernel: the reserved CUs
};

struct FlowCounters { long long stale_events = 0, stale_confirmed = 0, rescued = 0; };   // flags that only the read-modify-write poll saw

class FlowFactor {     // move-only (its owners are)
  public:
    // the hooks' form, split and trace_on decide here; a failure leaves the object as it was (empty)
    hipError_t init(const FlowView &view, const FlowHooks &hooks);
    bool ready() const { return ready_; }
    // source of the NEXT factor(): M = V N V + Bh' Bh read straight from N by the tile kernel (no scaled copy into L first)
    void set_source(const double *N, long ldN, const double *V, const double *Bh, int bstride, int d, int U) {
        src_ = N; src_ld_ = ldN; V_ = V; Bh_ = Bh; bstride_ = bstride; d_ = d; U_ = U;
    }
    hipError_t factor(hipEvent_t all_ready, bool profile);
    const int *abort_word() const { return ready_ ? flags_.get() + FLOW_ABORT : nullptr; }   // kernels behind an abandoned factorisation leave at once
    hipError_t read_ctrl(int (&cw)[8]) const;      // enqueues the copy of the first control words on the stream ...
    bool collect(const int (&cw)[8]);              // ... and once the stream has been synchronised: counts; true = the factorisation was abandoned
    void report_stall() const;                     // one report on stderr: how far the abandoned factorisation got
    bool elapsed_ms(float *ms);                    // device time of the last profiled factor(), once (after the stream has been synchronised)
    hipError_t enable_trace(bool on);              // debug: per-task timeline of the next factorisations (scripts/flow_trace.py)
    const long long *trace() const { return trace_.get(); }      // [n_tasks][8], then [nb][8] of the chain kernel (device memory)
    size_t trace_words() const { return ((size_t)n_tasks() + v_.nfact / 128) * 8; }
    int n_tasks() const { return (int)tasks_host_.size(); }
    const FlowCounters &counters() const { return counters_; }

  private:
    FlowView v_{};
    bool ready_ = false, timed_ = false;
    bool one_kernel_ = false, chain_ = false;
    int second_ = 0;
    int grid_ = 0;
    int keep_ = 0;                       // blocks >= this on an XCD that hosts a chain workgroup take no ticket (measured at init)
    int partials_ = 0;                   // 128 x 128 buffers for the partial sums of split update ranges
    FlowLayout lay_{};
    int wg_off_ = 0;                     // lay_.wgstate as the device reads it (FLOW_WG_OFF)
    std::vector<int4> tasks_host_;       // the task list (report_stall)
    DevBuf<int4> tasks_;
    DevBuf<int> flags_;                  // fine-grained device memory where there is any
    DevBuf<double> scratch_;             // one-kernel form: [grid][128 x 128]; then 64 zeros (every form)
    DevBuf<double> partial_;
    DevBuf<long long> trace_;
    DevBuf<double> diag_scratch_;        // one-kernel form: work arrays of the inline diagonal blocks
    HostMapped<int> alive_;              // sequence number of the last companion kernel that has started, per workgroup
    int seq_ = 0;
    DevEvent e0_, e1_, t0_, t1_;
    const double *src_ = nullptr, *V_ = nullptr, *Bh_ = nullptr;
    long src_ld_ = 0;
    int d_ = 0, U_ = 0, bstride_ = 0;
    FlowCounters counters_;
};

}  // namespace jaicov
