// Dense fp64 SPD machinery on the device: blocked Cholesky, multi-rhs substitution, triangular inverse, L^-T L^-1.
// Storage: row-major, LOWER triangle, order n (multiple of 128), leading dimension ld.  The same memory read
// column-major is LAPACK's UPLO='U' -- which is how MTJ's UpperSymmPackMatrix (packed) maps onto it.
// Replaces the arithmetic of MathExtension.solve / MathExtension.inv (MathExtension.java:239-264,304-324,338-366),
// i.e. netlib dppsv/dpptrf/dpptri and (through the bordered formulation in engine.hip) dspsv/dsptri.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <vector>

#include "chains.h"
#include "cholflow.h"
#include "devbuf.h"

namespace jaicov {

struct GemmArgs;

constexpr int DENSE_NB = 128;      // diagonal block handled by one workgroup in LDS
constexpr int DENSE_MAX_RHS = 8;   // rhs vectors the substitution kernels carry at once
constexpr int DENSE_PANEL = 512;   // outer panel width of the stream-scheduled factorisation (multiple of 128)

// Streams are kept for the life of the process (dense.hip): creating one costs 12-35 ms on this stack (a hardware queue is set up), destroying
// one 5 ms, and an engine needs eight -- 100 ms of the 225 ms an engine creation took at BASELINE config 4.  stream_acquire hands out a
// stream nobody else holds (a cached one if there is one of that kind for the current device, else a new one; nullptr if it cannot
// be created); stream_release synchronises it and puts it back.  CU-masked streams are the exception to "kept": each is a hardware queue
// of its own, idle or not, and a process that holds more than ~16 has ALL its queues time-sliced (round 5: 94 block columns 19.5 ms with 8
// idle ones beside the solver's, 28.8 with 16, 58 with 32; scripts/queue_count_probe.py) -- at most STREAM_MASKED_IDLE_MAX of a kind stay
// in the pool, the rest are destroyed on release.
enum { STREAM_PLAIN = 0, STREAM_HIGH_PRIORITY = 1, STREAM_UPDATE_CUS = 2, STREAM_DIAGONAL_CUS = 3, STREAM_KINDS = 4 };
constexpr int STREAM_MASKED_IDLE_MAX = 2;
hipStream_t stream_acquire(int kind);
void stream_release(int kind, hipStream_t s);
int device_cu_count();     // compute units of the current device; 0 if it cannot be asked
// A stream out of that pool for as long as the lease lives (move-only; get() is null if none could be had)
class StreamLease {
    int kind_ = STREAM_PLAIN;
    hipStream_t stream_ = nullptr;
  public:
    StreamLease() = default;
    explicit StreamLease(int kind) : kind_(kind), stream_(stream_acquire(kind)) {}
    StreamLease(StreamLease &&o) noexcept : kind_(o.kind_), stream_(o.stream_) { o.stream_ = nullptr; }
    StreamLease &operator=(StreamLease &&o) noexcept { std::swap(kind_, o.kind_); std::swap(stream_, o.stream_); return *this; }
    ~StreamLease() { stream_release(kind_, stream_); }
    hipStream_t get() const { return stream_; }
};

struct DenseSolver {     // not copyable: it holds owners
    hipStream_t stream = nullptr;
    int n = 0;                 // rows of the storage, multiple of 128: nfact, plus 128 right-hand-side rows if `aug`
    int nfact = 0;             // padded order of the matrix that is factorised
    bool aug = false;          // right-hand sides are carried through the factorisation as rows nfact.. of L
    long ld = 0;
    int cus = 0;               // compute units of the device (0: could not be asked)
    // the streams this solver launches on (factor panel s+1 on `pstream` while the rest of trailing update s runs) ...
    hipStream_t pstream = nullptr;   // panel GEMMs (high priority)
    hipStream_t ustream = nullptr;   // trailing updates: all CUs except the reserved ones (CU mask)
    hipStream_t dstream = nullptr;   // diagonal-block kernel: the reserved CUs
    StreamLease pstream_lease, ustream_lease, dstream_lease;   // ... and those of them it acquired itself (the others are init's `share` solver's)
    std::vector<DevEvent> sync_ev;
    size_t ev_used = 0;
    hipEvent_t next_event();
    std::map<int, std::pair<int2 *, int>> tile_maps;   // XCD-aware tile order of the trailing update, by tile rows
    DevBuf<int2> tile_map_store;
    std::map<long, DevBuf<int2>> trtri_maps;   // tile orders of the triangular inverse's products, longest k-range first (dense.hip)
    const int2 *trtri_tile_order(int tm, int tn, int kind);
    double *L = nullptr;       // n x ld : input SPD matrix (lower) -> Cholesky factor (lower)
    double *invd = nullptr;    // (n/128) x 128 x 128 : inverses of the diagonal blocks of L
    double *W = nullptr;       // n x ld : L^-1 (lower), only for the inverse
    double *Q = nullptr;       // n x ld : (L L')^-1 (lower tiles valid; symmetrize() fills the rest); workspace of trtri()
    int *d_info = nullptr;     // first failing pivot (1-based), 0 = ok
    struct Store { DevBuf<double> L, invd, W, Q; DevBuf<int> info; } store;   // the owners of the buffers above
    SolveChains chains;        // the substitution chains (chains.hip) and what they own beyond the factor
    FlowHooks hooks;           // the environment's test hooks as they were at init()
    // optional per-launch profiling of the trailing update (HIP events on `stream`)
    bool profile = false;
    std::vector<DevEvent> prof_ev;       // pairs
    std::vector<double> prof_flops;
    size_t prof_used = 0;
    double stat_launches = 0, stat_ms = 0, stat_flops = 0;
    void prof_collect();                 // call after the stream has been synchronised
    double flops_order = 0;              // real (unpadded) order of the matrix, for the algorithmic flop count n^3/3; 0 = nfact

    FlowFactor flow;                     // the dataflow factorisation (cholflow.hip), ready() if this solver factorises by it
    hipError_t potrf_streams(hipEvent_t first_ready, hipEvent_t all_ready);   // the stream / event scheduled factorisation

    // `share`: a solver of the same engine that is never at work at the same time (the full-order and the EO-reduced solver of an engine):
    // its side streams are used instead of streams of this solver's own -- a CU-masked stream is a HARDWARE QUEUE, and beyond ~16 of them
    // in a process the scheduler time-slices the queues, persistent kernels included ("Hardware queues")
    // A failure leaves nothing behind.
    hipError_t init(hipStream_t s, int n_padded, bool with_inverse, bool with_rhs_rows = false, const DenseSolver *share = nullptr);
    hipError_t acquire(bool with_inverse, const DenseSolver *share);      // init's body
    // the inverse's squares, two allocations of the solver's order: Q, and with want_W also W.  What is there already stays (engine.hip
    // reserves them before the solve that needs them, jaicov_neq_prepare_inverse)
    hipError_t reserve_inverse(bool want_W);
    ~DenseSolver() { release(); }
    double *rhs_row(int q) const { return L + (long)(nfact + q) * ld; }   // row q of the right-hand sides / of Z = Y L^-T
    void release();            // everything goes back: buffers, events, the leased streams (synchronised by stream_release)
    hipError_t panel(hipStream_t st, int K0, int K1);
    hipError_t timed_gemm(hipStream_t st, const GemmArgs &u, double flops, int small = 0);
    // L <- chol(L); info via fetch_info().  first_ready / all_ready (optional, events on `stream`): the first panel's
    // columns [0, first_panel_cols()) resp. the whole matrix are in place -- the first panel then factors while the
    // caller is still filling the rest.
    hipError_t potrf(hipEvent_t first_ready = nullptr, hipEvent_t all_ready = nullptr);
    hipError_t begin_refactor();                            // before the first write into L for a new factorisation (waits for the side stream's readers of the old one)
    int first_panel_cols() const;
    hipError_t backsolve_aug(double *X, long xs, int nrhs);  // L' X = Z, Z = the rhs rows after potrf(); X rows have stride xs
    hipError_t solve_rhs(const double *b, double *tmp, double *X);   // X = (L L')^-1 b, one right-hand side (forward + backward chain)
    hipError_t trtri();                                     // W <- L^-1
    hipError_t lauum();                                     // Q <- W' W (lower tiles)
    hipError_t symmetrize(double *M);                       // copy lower -> upper
    int fetch_info();                                       // synchronises the stream; > 0 failing pivot, -9 dataflow stalled
};

}  // namespace jaicov
