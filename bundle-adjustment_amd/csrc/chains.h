// Host side of the substitution chains (chains.hip): which form of the chain a call runs (a pure function of the block columns, the
// right-hand sides, the compute units and the test hooks), and the object that owns everything the chains need beyond the solver's
// factor: the pre-multiplied blocks, the exchange vector of the split chains, and the protocol between the two streams they run on.
#pragma once
#include <hip/hip_runtime.h>

#include "cholflow.h"
#include "devbuf.h"

namespace jaicov {

// ---- decision -------------------------------------------------------------------------------------------------------------------------
struct ChainDecision {
    bool polling_wave;   // ONE right-hand side in the polling-wave form (backsolve_chain8_kernel; pre-multiplied blocks), else backsolve_chain_kernel<nr>
    int workgroups;      // ... with this many workgroups per block column / row (1 or 2; 2: the whole grid is resident at once)
    int nr;              // right-hand sides the chain kernel carries: the smallest of 1, 2, 4, 8 that holds nrhs
};
int chain8_min_blocks(const FlowHooks &h);     // the polling-wave chains: from this many block columns on
// nb block columns, nrhs right-hand sides (1 .. 8), `cus` compute units (0: could not be asked); `have_buffers`: the pre-multiplied
// blocks and the exchange vector exist.  chain8_min_nb is a hook the tests set around single calls: ask with flow_hooks() at every call.
ChainDecision chain_decide(int nb, int nrhs, int cus, bool have_buffers, const FlowHooks &h);

// ---- the chains -----------------------------------------------------------------------------------------------------------------------
// What SolveChains uses and does not own: the solver's factor and streams.  Handed over once, at init; the solver outlives its chains.
struct ChainView {
    const double *L;     // the factor (lower), leading dimension ld
    long ld;
    const double *invd;  // inverses of its diagonal blocks
    int nfact;           // order that was factorised
    int cus;             // compute units of the device (0: could not be asked)
    hipStream_t stream;  // the chains, and the P half of premultiply()
    hipStream_t pstream; // the Ft half of premultiply(), beside the first backward chain; may be null
};

class SolveChains {     // move-only (its owners are)
  public:
    // the hooks' chain_trace decides here; a failure leaves the object empty
    hipError_t init(const ChainView &view, const FlowHooks &hooks);
    // Before the first WRITE into L for a new factorisation: the pre-multiplied blocks are no longer the factor's, and the Ft half of
    // the last premultiply() may still be reading the old factor on pstream (`stream` waits for it if it has not yet)
    hipError_t factor_changes();
    // L' X = Z for nrhs <= 8 right-hand sides: rows of Z have stride zs, rows of X stride xs (X is preset here)
    hipError_t backward(const double *Z, long zs, double *X, long xs, int nrhs, const int *abort_word);
    // X = (L L')^-1 b, one right-hand side: forward chain into `tmp`, backward chain into X (length nfact; b, tmp, X distinct)
    hipError_t solve(const double *b, double *tmp, double *X, const int *abort_word);

  private:
    ChainView v_{};
    DevBuf<double> pm_;        // 2 x CH_PM x nb x 128 x 128 : the pre-multiplied blocks P_1 .. P_5, then Ft_1 .. Ft_5 (premultiply())
    DevBuf<double> xch_;       // nfact : the two workgroups of a block column / row pass their halves of v through this
    bool pm_ready_ = false;    // pm_ belongs to the factor at hand (factor_changes() clears it)
    DevEvent pm_e0_, pm_done_; // the Ft half of premultiply() runs on pstream
    bool pm_wait_ = false;     // ... and `stream` has not waited for it yet
    bool trace_ = false;       // JAICOV_CHAIN_TRACE as it was at init
    ChainDecision decide(int nrhs) const;
    hipError_t preset(double *p, size_t count);      // "not yet published": what a chain polls has to hold this before its launch
    hipError_t wait_premultiplied();
    hipError_t premultiply();
    hipError_t launch_backward8(const ChainDecision &d, const double *Z, double *X, const int *abort_word, long long *trace);
    hipError_t launch_backward(const ChainDecision &d, const double *Z, long zs, double *X, long xs, int nrhs, const int *abort_word);
    hipError_t launch_forward(const ChainDecision &d, const double *b, double *Z);
    hipError_t dump_trace(const long long *trace);
};

}  // namespace jaicov
