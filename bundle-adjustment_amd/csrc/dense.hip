// Dense fp64 SPD solver kernels + drivers (see dense.h).  gfx950 only.
#include "dense.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "gemm_f64.h"
#include "launchers.h"
#include "potrf_diag.h"
#include "status.h"

namespace jaicov {

__global__ __launch_bounds__(256) void potrf_diag_kernel(double *A, long ld, double *inv_out, int *info, int blk, int dbg) {
    __shared__ double S[128 * DP];
    __shared__ double Wd[8 * 16 * WDP];
    potrf_diag_body(A, ld, inv_out, info, blk, dbg, S, Wd);
}

__global__ void copy_diag_blocks_kernel(const double *invd, double *W, long ld) {
    const int k = blockIdx.x;
    for (int idx = threadIdx.x; idx < 128 * 128; idx += blockDim.x) {
        const int r = idx >> 7, c = idx & 127;
        W[(long)(k * 128 + r) * ld + k * 128 + c] = invd[(long)k * 16384 + idx];
    }
}

// M[c][r] = M[r][c] for c < r, tile by tile through LDS
__global__ __launch_bounds__(256) void symmetrize_kernel(double *M, long ld, int nt) {
    __shared__ double tile[32][33];
    // lower-triangle tile index
    const int t = blockIdx.x;
    int tr = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((long)(tr + 1) * (tr + 2) / 2 <= t) ++tr;
    while ((long)tr * (tr + 1) / 2 > t) --tr;
    const int tc = t - tr * (tr + 1) / 2;
    (void)nt;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int y = ty; y < 32; y += 8) tile[y][tx] = M[(long)(tr * 32 + y) * ld + tc * 32 + tx];
    __syncthreads();
    for (int y = ty; y < 32; y += 8) {
        const int r = tc * 32 + y, c = tr * 32 + tx;   // transposed position
        if (c > r) M[(long)r * ld + c] = tile[tx][y];
    }
}

namespace {
std::mutex g_stream_mutex;
std::map<std::pair<int, int>, std::vector<hipStream_t>> g_stream_pool;      // (device, kind) -> idle streams
// The idle streams are destroyed when this library's static objects are (at exit, BEFORE those of the HIP runtime it depends on and before
// a profiler's finalisation: under rocprofv3 a process that left streams to the runtime's own teardown ended in a segmentation fault
// inside __cxa_finalize, after the tool had written its output).
std::vector<hipStream_t> g_all_streams;       // every stream stream_acquire has created and nobody has destroyed: idle ones and those of live (or leaked) engines
std::map<hipStream_t, int> g_stream_kind;      // ... its kind (census below)
std::map<hipStream_t, int> g_stream_device;    // ... and the device each belongs to (a stream is filed under ITS device whatever the caller's current one is)
struct StreamPoolCleanup {
    ~StreamPoolCleanup() {
        std::lock_guard<std::mutex> lock(g_stream_mutex);
        for (hipStream_t s : g_all_streams) (void)hipStreamDestroy(s);
        g_all_streams.clear();
        g_stream_device.clear();
        g_stream_kind.clear();
        g_stream_pool.clear();
    }
} g_stream_pool_cleanup;
}

hipStream_t stream_acquire(int kind) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    {
        std::lock_guard<std::mutex> lock(g_stream_mutex);
        std::vector<hipStream_t> &idle = g_stream_pool[{dev, kind}];
        if (!idle.empty()) {
            hipStream_t s = idle.back();
            idle.pop_back();
            return s;
        }
    }
    hipStream_t s = nullptr;
    hipError_t err = hipSuccess;
    if (kind == STREAM_PLAIN) {
        err = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    } else if (kind == STREAM_HIGH_PRIORITY) {
        int least = 0, greatest = 0;
        err = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (err == hipSuccess) err = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest);
    } else {
        // CU reservation (measured on MI355X/ROCm 7.2: bit i of the 256-bit mask is CU i/8 of XCD i%8): the trailing
        // updates get CUs 0..30 of every XCD, the diagonal-block kernel CU 31 of every XCD.  (Reserving fewer CUs was
        // measured: one or two reserved CUs cost 5 ms per factorisation at config 4, eight cost the update 3 % of the chip.)
        uint32_t mask[8];
        for (int w = 0; w < 8; w++) mask[w] = kind == STREAM_UPDATE_CUS ? 0xFFFFFFFFu : 0u;
        mask[7] = kind == STREAM_UPDATE_CUS ? 0x00FFFFFFu : 0xFF000000u;
        err = hipExtStreamCreateWithCUMask(&s, 8, mask);
    }
    if (err != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    std::lock_guard<std::mutex> lock(g_stream_mutex);
    g_all_streams.push_back(s);
    g_stream_device[s] = dev;
    g_stream_kind[s] = kind;
    return s;
}

void stream_release(int kind, hipStream_t s) {
    if (!s) return;
    if (hipStreamSynchronize(s) != hipSuccess) {      // a stream in an error state is not worth keeping
        (void)hipGetLastError();
        {
            std::lock_guard<std::mutex> lock(g_stream_mutex);
            g_all_streams.erase(std::remove(g_all_streams.begin(), g_all_streams.end(), s), g_all_streams.end());
            g_stream_device.erase(s);
            g_stream_kind.erase(s);
        }
        hipStreamDestroy(s);
        return;
    }
    {
        std::lock_guard<std::mutex> lock(g_stream_mutex);
        const auto it = g_stream_device.find(s);
        std::vector<hipStream_t> &idle = g_stream_pool[{it == g_stream_device.end() ? 0 : it->second, kind}];
        const bool masked = kind == STREAM_UPDATE_CUS || kind == STREAM_DIAGONAL_CUS;
        if (!masked || (int)idle.size() < STREAM_MASKED_IDLE_MAX) {
            idle.push_back(s);
            return;
        }
        // a CU-masked stream beyond the few that are kept: its hardware queue goes back to the device (dense.h)
        g_all_streams.erase(std::remove(g_all_streams.begin(), g_all_streams.end(), s), g_all_streams.end());
        g_stream_device.erase(s);
        g_stream_kind.erase(s);
    }
    (void)hipStreamDestroy(s);
}

// tests / DESIGN.md: streams of this library in the process, [kind] alive (held by solvers or idle) and [4 + kind] idle in the pool;
// kinds: 0 plain, 1 high priority, 2 CU-masked (trailing updates), 3 CU-masked (diagonal blocks) -- the masked ones are hardware queues
extern "C" void jaicov_debug_stream_census(int *out8) {
    std::lock_guard<std::mutex> lock(g_stream_mutex);
    for (int i = 0; i < 8; i++) out8[i] = 0;
    for (const auto &kv : g_stream_kind)
        if (kv.second >= 0 && kv.second < 4) out8[kv.second]++;
    for (const auto &kv : g_stream_pool)
        if (kv.first.second >= 0 && kv.first.second < 4) out8[4 + kv.first.second] += (int)kv.second.size();
}

// tests / DESIGN.md: device memory that the library's owners (devbuf.h) hold in this process: [0] bytes, [1] allocations.  Complete, since
// nothing else in the library allocates
extern "C" void jaicov_debug_device_census(long long *out2) {
    out2[0] = device_live[0].load();
    out2[1] = device_live[1].load();
}

int device_cu_count() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) return cus;
    (void)hipGetLastError();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
hipError_t DenseSolver::init(hipStream_t s, int n_padded, bool with_inverse, bool with_rhs_rows, const DenseSolver *share) {
    stream = s;
    aug = with_rhs_rows;
    nfact = n_padded;
    n = n_padded + (aug ? 128 : 0);
    ld = n;
    const hipError_t err = acquire(with_inverse, share);
    if (err != hipSuccess) release();
    return err;
}

hipError_t DenseSolver::acquire(bool with_inverse, const DenseSolver *share) {
    const size_t sq = (size_t)n * ld, nbq = (size_t)(nfact / 128) * 16384;
    HIPCHK(store.L.reserve(sq));
    HIPCHK(store.invd.reserve(nbq));
    HIPCHK(hipMemset(store.invd.get(), 0, nbq * sizeof(double)));
    L = store.L.get(); invd = store.invd.get();

    cus = device_cu_count();
    hooks = flow_hooks();
    const bool flow_wanted = flow_decide(nfact / 128, true, hooks).use_flow;      // (whether kernels overlap is asked once the streams are there: it does not bear on this)
    // the side streams of `share` where it holds them itself, streams of this solver's own otherwise
    const bool borrowed = share != nullptr && share->pstream_lease.get() != nullptr;
    if (borrowed) {
        pstream = share->pstream;
    } else {
        pstream_lease = StreamLease(STREAM_HIGH_PRIORITY);
        pstream = pstream_lease.get();
        if (!pstream) return hipErrorUnknown;
    }
    HIPCHK(chains.init(ChainView{L, ld, invd, nfact, cus, stream, pstream}, hooks));
    HIPCHK(store.info.reserve(1));
    d_info = store.info.get();
    // reserved CUs: CU 31 of every XCD for the diagonal blocks, the other 31 for the trailing updates (stream_acquire).  The masked
    // stream of the trailing updates is only held by a solver that factorises by the stream-scheduled form: the dataflow form
    // (flow_wanted) launches its tile kernel on the ordinary stream, and every CU-masked stream is a hardware queue (dense.h).
    // A masked stream the other solver of the engine holds is used (only where this solver needs one); what it does not hold is
    // acquired here and is then this solver's own to release.
    auto masked = [&](hipStream_t theirs, StreamLease &own, int kind) {
        if (theirs) return theirs;
        own = StreamLease(kind);
        return own.get();
    };
    if (nfact >= 2048 || flow_wanted) {
        dstream = masked(borrowed ? share->dstream : nullptr, dstream_lease, STREAM_DIAGONAL_CUS);
        if (!flow_wanted) ustream = masked(borrowed ? share->ustream : nullptr, ustream_lease, STREAM_UPDATE_CUS);
        if (!dstream || (!flow_wanted && !ustream)) {
            ustream_lease = StreamLease();
            dstream_lease = StreamLease();
            ustream = dstream = nullptr;
        }
    }
    // XCD-aware tile orders of every trailing-update size this solver can launch (one allocation, built here so that the
    // first factorisation does not stop for host work)
    if (n / 128 >= 24) {
        std::vector<int2> all;
        std::vector<std::pair<int, std::pair<size_t, int>>> where;
        for (int T = 24; T <= n / 128; T++) {
            const std::vector<int2> m = xcd_tile_map(T);
            where.push_back({T, {all.size(), (int)m.size()}});
            all.insert(all.end(), m.begin(), m.end());
        }
        HIPCHK(tile_map_store.reserve(all.size()));
        HIPCHK(hipMemcpy(tile_map_store.get(), all.data(), all.size() * sizeof(int2), hipMemcpyHostToDevice));
        for (auto &w : where) tile_maps.emplace(w.first, std::make_pair(tile_map_store.get() + w.second.first, w.second.second));
    }
    if (with_inverse) HIPCHK(reserve_inverse(true));
    if (flow_wanted && dstream && flow.init(FlowView{L, ld, invd, d_info, nfact, n, stream, pstream, dstream}, hooks) != hipSuccess) {
        // the stream-scheduled factorisation remains: it wants the masked stream of the trailing updates after all
        (void)hipGetLastError();
        ustream = masked(ustream, ustream_lease, STREAM_UPDATE_CUS);
    }
    return hipSuccess;
}

hipError_t DenseSolver::reserve_inverse(bool want_W) {
    const size_t sq = (size_t)n * ld;
    if (want_W) HIPCHK(store.W.reserve(sq));
    HIPCHK(store.Q.reserve(sq));
    W = store.W.get(); Q = store.Q.get();
    return hipSuccess;
}

void DenseSolver::release() {
    flow = FlowFactor();
    store = Store();
    chains = SolveChains();
    tile_map_store.reset();
    trtri_maps.clear();
    tile_maps.clear();
    prof_ev.clear();
    sync_ev.clear();
    pstream_lease = StreamLease();
    ustream_lease = StreamLease();
    dstream_lease = StreamLease();
    pstream = ustream = dstream = nullptr;
    L = invd = W = Q = nullptr;
    d_info = nullptr;
}

// Two-level right-looking Cholesky with one-panel look-ahead.
// Outer panels of DENSE_PANEL columns (trailing update with K = DENSE_PANEL: enough flops per byte of C to be MFMA-bound); inside a
// panel a left-looking sweep over 128-column blocks:
//   block column kk -= L[kk:n, k0:kk] L[kk:kk+128, k0:kk]'     (fp64 MFMA GEMM, K grows to DENSE_PANEL-128)
//   diagonal block factor + inverse (one workgroup, LDS)        L21 = A21 inv(L11)'  (GEMM with the inverse)
// Look-ahead: the trailing update of panel s is split into (a) the columns of panel s+1 and (b) the rest; panel s+1 is
// factored on a second, high-priority stream as soon as (a) is done, while (b) keeps the chip busy.
hipEvent_t DenseSolver::next_event() {
    if (ev_used >= sync_ev.size()) {
        DevEvent e;
        if (e.create(hipEventDisableTiming) != hipSuccess) return nullptr;
        sync_ev.push_back(std::move(e));
    }
    return sync_ev[ev_used++].get();
}

// Panel factorisation of block columns [K0,K1).  GEMMs go to `st`; when a reserved-CU stream exists the diagonal-block
// kernel (which needs a whole CU's LDS and would otherwise starve behind the trailing update's workgroups) runs there,
// chained with events.
hipError_t DenseSolver::panel(hipStream_t st, int K0, int K1) {
    // In the tail (short trailing updates, the panel chain is the critical path) the diagonal kernel stays on the panel
    // stream: the two event hops per block cost more than the contention they avoid.
    constexpr int tail_rows = 6144;
    for (int k = K0; k < K1; k++) {
        double *Akk = L + (long)(k * 128) * ld + k * 128;
        const int rows_k = n - k * 128;
        // ... except for the first block of a panel: it becomes ready at the moment the trailing update is launched, and a
        // workgroup that wants a whole CU's LDS then waits for the update's first tiles to retire (130 us instead of 49)
        // (only while the update still has more workgroups than the chip has slots: 31 tile rows = 496 tiles)
        const bool split = dstream != nullptr && st == pstream && (rows_k > tail_rows || (k == K0 && rows_k > 4096));
        // While the trailing update still hides the panel (many rows left) the panel GEMMs take the 128-tile: it costs
        // the update fewer CU slots per flop than the 64-tile latency variant, which is for the critical-path regime.
        constexpr int bulk_rows = 9216;
        // in between (the update still shares the chip) the 64-tile; the 32-tile only once the panel runs alone
        const int small = (st == pstream && rows_k > bulk_rows) ? 0 : ((st == pstream && rows_k > tail_rows) ? 1 : -1);
        if (k > K0) {
            GemmArgs c{};
            c.A = L + (long)(k * 128) * ld + K0 * 128; c.lda = ld;      // L[k*128:n, K0*128 : k*128]
            c.B = c.A; c.ldb = ld;                                       // first 128 rows of the same strip
            c.C = Akk; c.ldc = ld; c.M = rows_k; c.N = 128; c.K = (k - K0) * 128;
            c.alpha = -1.0; c.beta = 1.0; c.lower_only = 0; c.kmode = KMODE_FULL;
            HIPCHK(gemm_f64(st, LAY_KC, LAY_KC, c, 1, small));
        }
        hipStream_t ds = st;
        if (split) {
            hipEvent_t e = next_event();
            HIPCHK(hipEventRecord(e, st));
            HIPCHK(hipStreamWaitEvent(dstream, e, 0));
            ds = dstream;
        }
        hipLaunchKernelGGL(potrf_diag_kernel, dim3(1), dim3(256), 0, ds, Akk, ld, invd + (long)k * 16384, d_info, k, 0);
        if (split) {
            hipEvent_t e = next_event();
            HIPCHK(hipEventRecord(e, dstream));
            HIPCHK(hipStreamWaitEvent(st, e, 0));
        }
        const int rows = rows_k - 128;
        if (rows <= 0) break;
        double *A21 = L + (long)((k + 1) * 128) * ld + k * 128;
        GemmArgs g{};
        // L21 = A21 * inv(L11)'   (in place: one column tile, every workgroup reads and writes only its own rows)
        g.A = A21; g.lda = ld; g.B = invd + (long)k * 16384; g.ldb = 128; g.C = A21; g.ldc = ld;
        g.M = rows; g.N = 128; g.K = 128; g.alpha = 1.0; g.beta = 0.0; g.lower_only = 0; g.kmode = KMODE_FULL;
        HIPCHK(gemm_f64(st, LAY_KC, LAY_KC, g, 1, small));
    }
    return hipGetLastError();
}

hipError_t DenseSolver::timed_gemm(hipStream_t st, const GemmArgs &u, double flops, int small) {
    if (profile) {
        if (prof_used + 2 > prof_ev.size()) {
            DevEvent a, b;
            HIPCHK(a.create()); HIPCHK(b.create());
            prof_ev.push_back(std::move(a)); prof_ev.push_back(std::move(b));
        }
        HIPCHK(hipEventRecord(prof_ev[prof_used].get(), st));
    }
    HIPCHK(gemm_f64(st, LAY_KC, LAY_KC, u, 1, small, 1));   // own kernel symbol: gemm_f64_kernel<0, 0, 128, 128, 1> (64, 64 in the tail)
    if (profile) {
        HIPCHK(hipEventRecord(prof_ev[prof_used + 1].get(), st));
        prof_flops.push_back(flops);
        prof_used += 2;
    }
    return hipSuccess;
}

int DenseSolver::first_panel_cols() const {
    const int nb = nfact / 128;
    return 128 * std::min(DENSE_PANEL / 128, nb);
}

// Call before the first WRITE into L for a new factorisation (the engine's scaled copy, a dispersion load): the chains' side stream
// may still be reading the old factor (chains.h).  potrf() does the same for callers that fill L through potrf's own first tile load
// (FlowFactor::set_source), where nothing writes L earlier.
hipError_t DenseSolver::begin_refactor() { return chains.factor_changes(); }

hipError_t DenseSolver::potrf(hipEvent_t first_ready, hipEvent_t all_ready) {
    HIPCHK(begin_refactor());
    if (flow.ready()) return flow.factor(all_ready, profile);
    return potrf_streams(first_ready, all_ready);
}

hipError_t DenseSolver::potrf_streams(hipEvent_t first_ready, hipEvent_t all_ready) {
    const int nb = nfact / 128;   // diagonal blocks; rows run to n (the right-hand-side rows below the matrix included)
    // Panel width: one width for the whole factorisation (wide panels while many rows remain, narrow ones in the tail: measured
    // flat +- 0.3 ms at config 4, DESIGN_HISTORY.md)
    constexpr int bo = DENSE_PANEL / 128;
    const bool la = pstream != nullptr && nb > bo;            // look-ahead: panel s+1 on pstream beside the rest of trailing update s
    ev_used = 0;
    hipStream_t sp = la ? pstream : stream;                 // panel GEMMs
    hipStream_t su = la && ustream ? ustream : stream;      // trailing updates (all CUs but the reserved ones)
    hipEvent_t e_start = next_event();
    if (la) {
        if (first_ready && all_ready) {                     // the caller is still filling the columns behind the first panel
            HIPCHK(hipStreamWaitEvent(sp, first_ready, 0));
            if (su != stream) HIPCHK(hipStreamWaitEvent(su, all_ready, 0));
        } else {
            HIPCHK(hipEventRecord(e_start, stream));
            HIPCHK(hipStreamWaitEvent(sp, e_start, 0));
            if (su != stream) HIPCHK(hipStreamWaitEvent(su, e_start, 0));
        }
    }
    HIPCHK(hipMemsetAsync(d_info, 0, sizeof(int), sp));    // before the first diagonal kernel, which runs on sp or behind it
    int K0 = 0, K1 = std::min(bo, nb);
    HIPCHK(panel(sp, 0, K1));
    hipEvent_t e_panel = next_event();
    if (la) HIPCHK(hipEventRecord(e_panel, sp));
    while (K1 < nb) {
        const int K2 = std::min(K1 + bo, nb);     // end of the next panel
        if (la) HIPCHK(hipStreamWaitEvent(su, e_panel, 0));
        const int Kw = (K1 - K0) * 128;
        // (a) columns of the next panel: rows >= K1, cols [K1,K2)
        GemmArgs a{};
        a.A = L + (long)(K1 * 128) * ld + K0 * 128; a.lda = ld; a.B = a.A; a.ldb = ld;
        a.C = L + (long)(K1 * 128) * ld + K1 * 128; a.ldc = ld;
        a.M = n - K1 * 128; a.N = (K2 - K1) * 128; a.K = Kw; a.alpha = -1.0; a.beta = 1.0; a.lower_only = 0; a.kmode = KMODE_FULL;
        HIPCHK(gemm_f64(su, LAY_KC, LAY_KC, a));
        if (la) {
            hipEvent_t e = next_event();
            HIPCHK(hipEventRecord(e, su));
            HIPCHK(hipStreamWaitEvent(sp, e, 0));
        }
        HIPCHK(panel(sp, K1, K2));
        if (la) {
            e_panel = next_event();
            HIPCHK(hipEventRecord(e_panel, sp));
        }
        // (b) the rest of the trailing matrix: rows, cols >= K2 (lower tiles)
        const int rows = n - K2 * 128;
        if (rows > 0 && K2 < nb) {
            GemmArgs u{};
            u.A = L + (long)(K2 * 128) * ld + K0 * 128; u.lda = ld; u.B = u.A; u.ldb = ld;
            u.C = L + (long)(K2 * 128) * ld + K2 * 128; u.ldc = ld;
            u.M = rows; u.N = rows; u.K = Kw; u.alpha = -1.0; u.beta = 1.0; u.lower_only = 1; u.kmode = KMODE_FULL;
            if (rows / 128 >= 24) {
                const int T = rows / 128;
                auto it = tile_maps.find(T);
                if (it != tile_maps.end()) {
                    u.tile_map = it->second.first;
                    u.n_map = it->second.second;
                }
            }
            HIPCHK(timed_gemm(su, u, (double)rows * ((double)rows + 1.0) * (double)Kw));
        }
        K0 = K1;
        K1 = K2;
    }
    if (la) {   // the main stream continues only after the last panel and the last update
        hipEvent_t e1 = next_event(), e2 = next_event();
        HIPCHK(hipEventRecord(e1, sp));
        HIPCHK(hipStreamWaitEvent(stream, e1, 0));
        if (su != stream) {
            HIPCHK(hipEventRecord(e2, su));
            HIPCHK(hipStreamWaitEvent(stream, e2, 0));
        }
    }
    return hipGetLastError();
}

// L' X = Z for the right-hand sides that rode through the factorisation, and x = (L L')^-1 b for one that did not (b, tmp, X: distinct
// device vectors of length nfact): the substitution chains (chains.hip)
hipError_t DenseSolver::backsolve_aug(double *X, long xs, int nrhs) {
    if (!aug || nrhs < 1 || nrhs > DENSE_MAX_RHS) return hipErrorInvalidValue;
    return chains.backward(rhs_row(0), ld, X, xs, nrhs, flow.abort_word());
}

hipError_t DenseSolver::solve_rhs(const double *b, double *tmp, double *X) { return chains.solve(b, tmp, X, flow.abort_word()); }

// W = L^-1 (lower), level by level from the inverted diagonal blocks upwards.  At level h (blocks of h x 128 columns)
// every pair [lo, lo+h) | [lo+h, lo+2h) is merged independently:  W21 = -W22 (L21 W11).  All full pairs of a level
// have the same shape and a constant address stride, so a level is two batched launches (product T = L21 W11 into the
// W21-position of Q, which is free until lauum() fills it; then W21 = -W22 T); a ragged last pair gets its own two.
// Tile orders of the two products of a merge, longest k-range first (the tiles of these launches do triangular work: in
// T = L21 W11 the k-range of a tile shrinks with its COLUMN, in W21 = -W22 T it grows with its ROW).  In the kernel's
// row-major default the last tiles dispatched include the longest ones, and the launch ends with one long tile's time on a
// nearly empty chip (1-2 ms of the top level's 10 ms at config 4); longest-first leaves only short tiles for the tail.
const int2 *DenseSolver::trtri_tile_order(int tm, int tn, int kind) {
    const long key = ((long)kind << 40) | ((long)tm << 20) | tn;
    auto it = trtri_maps.find(key);
    if (it != trtri_maps.end()) return it->second.get();
    std::vector<int2> m;
    m.reserve((size_t)tm * tn);
    if (kind == 0) {            // KMODE_GE_COL: column 0 has the longest k-range
        for (int j = 0; j < tn; j++)
            for (int i = 0; i < tm; i++) m.push_back(make_int2(i, j));
    } else {                    // KMODE_LE_ROW: the last row has the longest k-range
        for (int i = tm - 1; i >= 0; i--)
            for (int j = 0; j < tn; j++) m.push_back(make_int2(i, j));
    }
    DevBuf<int2> d;
    if (d.reserve(m.size()) != hipSuccess) return nullptr;
    if (hipMemcpy(d.get(), m.data(), m.size() * sizeof(int2), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return trtri_maps.emplace(key, std::move(d)).first->second.get();
}

hipError_t DenseSolver::trtri() {
    const int nb = nfact / 128;
    if (!Q) return hipErrorInvalidValue;
    // tiles of the products longest k-range first (row-major order: 24.7 instead of 18.5 ms at config 4)
    HIPCHK(hipMemsetAsync(W, 0, (size_t)n * ld * sizeof(double), stream));
    hipLaunchKernelGGL(copy_diag_blocks_kernel, dim3(nb), dim3(256), 0, stream, invd, W, ld);
    for (int h = 1; h < nb; h *= 2) {
        const int full = nb / (2 * h);                         // pairs with both halves complete
        const long pair_stride = (long)(2 * h) * 128 * (ld + 1);
        auto merge = [&](int lo, int mid, int hi, int batch) -> hipError_t {
            const int M = (hi - mid) * 128, N = (mid - lo) * 128;
            GemmArgs t{};
            t.A = L + (long)(mid * 128) * ld + lo * 128; t.lda = ld;          // L21 (KC)
            t.B = W + (long)(lo * 128) * ld + lo * 128; t.ldb = ld;           // W11 (k,j) row-major = XC, lower-triangular
            t.C = Q + (long)(mid * 128) * ld + lo * 128; t.ldc = ld;
            t.M = M; t.N = N; t.K = N; t.alpha = 1.0; t.beta = 0.0; t.kmode = KMODE_GE_COL;
            t.strideA = t.strideB = t.strideC = pair_stride;
            if ((M / 128) * (N / 128) >= 64) { t.tile_map = trtri_tile_order(M / 128, N / 128, 0); t.n_map = t.tile_map ? (M / 128) * (N / 128) : 0; }
            HIPCHK(gemm_f64(stream, LAY_KC, LAY_XC, t, batch));
            GemmArgs w{};
            w.A = W + (long)(mid * 128) * ld + mid * 128; w.lda = ld;         // W22 (KC), lower-triangular
            w.B = t.C; w.ldb = ld;                                            // T (k,j) row-major = XC
            w.C = W + (long)(mid * 128) * ld + lo * 128; w.ldc = ld;
            w.M = M; w.N = N; w.K = M; w.alpha = -1.0; w.beta = 0.0; w.kmode = KMODE_LE_ROW;
            w.strideA = w.strideB = w.strideC = pair_stride;
            if ((M / 128) * (N / 128) >= 64) { w.tile_map = trtri_tile_order(M / 128, N / 128, 1); w.n_map = w.tile_map ? (M / 128) * (N / 128) : 0; }
            return gemm_f64(stream, LAY_KC, LAY_XC, w, batch);
        };
        if (full > 0) HIPCHK(merge(0, h, 2 * h, full));
        const int lo = full * 2 * h, mid = lo + h;
        if (mid < nb) HIPCHK(merge(lo, mid, nb, 1));          // ragged pair: second half shorter than h
    }
    return hipGetLastError();
}

hipError_t DenseSolver::lauum() {
    GemmArgs g{};
    g.A = W; g.lda = ld; g.B = W; g.ldb = ld; g.C = Q; g.ldc = ld;
    g.M = nfact; g.N = nfact; g.K = nfact; g.alpha = 1.0; g.beta = 0.0; g.lower_only = 1; g.kmode = KMODE_GE_ROW;
    return gemm_f64(stream, LAY_XC, LAY_XC, g);
}

hipError_t DenseSolver::symmetrize(double *M) {
    const int nt = nfact / 32;
    hipLaunchKernelGGL(symmetrize_kernel, dim3(nt * (nt + 1) / 2), dim3(256), 0, stream, M, ld, nt);
    return hipGetLastError();
}

void DenseSolver::prof_collect() {
    for (size_t i = 0; i + 1 < prof_used; i += 2) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, prof_ev[i].get(), prof_ev[i + 1].get()) == hipSuccess) {
            stat_launches += 1.0;
            stat_ms += ms;
            stat_flops += prof_flops[i / 2];
        }
    }
    prof_used = 0;
    prof_flops.clear();
    float ms = 0;
    if (flow.elapsed_ms(&ms)) {
        const double o = flops_order > 0 ? flops_order : (double)nfact;
        stat_launches += 1.0;
        stat_ms += ms;
        stat_flops += o * o * o / 3.0;
    }
}

int DenseSolver::fetch_info() {
    int h = -1;
    if (hipMemcpyAsync(&h, d_info, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess) return -1;
    int cw[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // cholflow.hip's control words
    if (flow.ready() && flow.read_ctrl(cw) != hipSuccess) return -1;
    if (hipStreamSynchronize(stream) != hipSuccess) return -1;
    if (flow.collect(cw)) {            // a wait of the dataflow factorisation ran into its time limit
        flow.report_stall();
        return -9;
    }
    return h;
}

// fp64 MFMA issue-rate ceiling: every wave runs `iters` x 16 independent v_mfma_f64_16x16x4 on register operands
__global__ __launch_bounds__(256) void mfma_peak_kernel(double *out, int iters) {
    d4_t acc[16];
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = (d4_t){0.0, 0.0, 0.0, 0.0};
    // iters < 0: random full-mantissa operands that change every iteration (DVFS: zero/constant data clocks higher)
    const bool rnd = iters < 0;
    if (rnd) iters = -iters;
    unsigned long long st = 0x9E3779B97F4A7C15ull * (threadIdx.x + 1 + 256ull * blockIdx.x);
    double a = 1.0 + 1e-9 * threadIdx.x, b = 1.0 - 1e-9 * threadIdx.x;
    for (int it = 0; it < iters; it++) {
        if (rnd) {
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            a = __longlong_as_double((long long)((st >> 12) | 0x3FF0000000000000ull)) - 1.5;
            b = __longlong_as_double((long long)(((st * 0x2545F4914F6CDD1Dull) >> 12) | 0x3FF0000000000000ull)) - 1.5;
        }
#pragma unroll
        for (int i = 0; i < 16; i++)
            asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(acc[i]) : "v"(a), "v"(b));
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 16; i++) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 123.456) out[0] = s;
}

// the MFMA peak kernel twice on `st`, the second launch timed
static hipError_t peak_on_stream(hipStream_t st, int blocks, int iters, float *ms_out, double *tflops) {
    DevBuf<double> out;
    DevEvent e0, e1;
    HIPCHK(out.reserve(1));
    HIPCHK(e0.create());
    HIPCHK(e1.create());
    hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(256), 0, st, out.get(), iters);
    hipEventRecord(e0.get(), st);
    hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(256), 0, st, out.get(), iters);
    hipEventRecord(e1.get(), st);
    hipEventSynchronize(e1.get());
    hipEventElapsedTime(ms_out, e0.get(), e1.get());
    *tflops = (double)blocks * 4.0 * (iters < 0 ? -iters : iters) * 16.0 * 2048.0 / (*ms_out * 1e-3) / 1e12;
    return hipGetLastError();
}

hipError_t mfma_peak_bench(int blocks, int iters, float *ms_out, double *tflops) { return peak_on_stream(nullptr, blocks, iters, ms_out, tflops); }

// does hipExtStreamCreateWithCUMask work here?  runs the MFMA peak kernel on a stream restricted by `mask` (8 words)
hipError_t cumask_bench(const uint32_t *mask, int blocks, int iters, float *ms_out, double *tflops) {
    DevStream st;
    HIPCHK(st.create_with_cu_mask(8, mask));
    return peak_on_stream(st.get(), blocks, iters, ms_out, tflops);
}

// timing hook for the diagonal-block kernel (diagnostics): `iters` back-to-back launches on an SPD 128x128 block
hipError_t diag_kernel_bench(int dbg, int iters, float *ms_out) {
    DevBuf<double> A_store, inv_store;
    DevBuf<int> info_store;
    DevEvent ev0, ev1;
    HIPCHK(A_store.reserve(16384));
    HIPCHK(inv_store.reserve(16384));
    HIPCHK(info_store.reserve(1));
    HIPCHK(ev0.create());
    HIPCHK(ev1.create());
    double *A = A_store.get(), *inv = inv_store.get();
    int *info = info_store.get();
    const hipEvent_t e0 = ev0.get(), e1 = ev1.get();
    std::vector<double> h(16384);
    for (int r = 0; r < 128; r++)
        for (int c = 0; c < 128; c++) h[r * 128 + c] = (r == c) ? 4.0 : 0.5 / (1.0 + (r > c ? r - c : c - r));
    hipMemset(inv, 0, 16384 * sizeof(double));
    hipMemset(info, 0, sizeof(int));
    hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters; i++) {
        hipMemcpyAsync(A, h.data(), 16384 * sizeof(double), hipMemcpyHostToDevice, nullptr);
        hipLaunchKernelGGL(potrf_diag_kernel, dim3(1), dim3(256), 0, nullptr, A, 128L, inv, info, 0, dbg);
    }
    hipEventRecord(e1, nullptr);
    hipEventSynchronize(e1);
    hipEventElapsedTime(ms_out, e0, e1);
    *ms_out /= iters;
    return hipGetLastError();
}

}  // namespace jaicov
