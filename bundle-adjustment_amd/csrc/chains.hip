// The substitution chains of the dense fp64 SPD solver: kernels + their host side (see chains.h).  gfx950 only.
#include "chains.h"

#include <stdio.h>

#include <algorithm>
#include <vector>

#include "gemm_f64.h"
#include "status.h"

namespace jaicov {

// ---------------------------------------------------------------------------------------------------------------
// substitution (nrhs <= 8 right-hand sides).
// Forward: none.  The right-hand sides ride through the factorisation as 128 extra rows below the matrix
// (DenseSolver::aug): chol([[M, Y'], [Y, *]]) = [[L, 0], [Z, *]] with Z = Y L^-T, i.e. row q of Z is (L^-1 y_q)'.
// Backward: L' X = Z in ONE launch.  Workgroup b owns block column k = nb-1-b: it streams the blocks L[j][k], j > k,
// (double-buffered in registers) and subtracts L[j][k]' x_j as soon as the owner of column j has published x_j, then
// applies the inverse of its diagonal block and publishes x_k.  The data are their own flags: X is preset to an
// all-ones bit pattern, results are written and polled with relaxed agent-scope atomics (coherent across the XCDs,
// no cache-wide fences), a value counts as published once it differs from the pattern.  A workgroup only ever waits
// for workgroups with a smaller index, which the dispatcher starts first: the chain cannot deadlock whatever the
// residency; a bounded spin turns a lost predecessor into NaNs instead of a hang.  Per chain link the latency is one
// store-to-load round trip + one 128x128 block instead of a kernel launch.
// ---------------------------------------------------------------------------------------------------------------
constexpr unsigned long long BS_UNSET = ~0ull;
constexpr int BS_SPIN_MAX = 1 << 22;

// NR = right-hand sides carried (1, 2, 4 or 8: the smallest that holds nrhs; an adjustment without datum defect has ONE,
// and the 8-wide form spent 2 of its 8 us per link of the chain on seven columns of zeros)
template <int NR>
__device__ __forceinline__ void bs_row(const double *p, double (&v)[NR]) {
    if constexpr (NR % 4 == 0) {
#pragma unroll
        for (int h = 0; h < NR / 4; h++) {
            const d4_t t = *reinterpret_cast<const d4_t *>(p + 4 * h);
            v[4 * h] = t[0]; v[4 * h + 1] = t[1]; v[4 * h + 2] = t[2]; v[4 * h + 3] = t[3];
        }
    } else {
#pragma unroll
        for (int q = 0; q < NR; q++) v[q] = p[q];
    }
}
template <int NR>
__global__ __launch_bounds__(256) void backsolve_chain_kernel(const double *__restrict__ L, long ld,
                                                              const double *__restrict__ invd, const double *__restrict__ Z,
                                                              long zs, double *X, long xs, int nb, int nrhs, const int *abort_word) {
    __shared__ __attribute__((aligned(32))) double xj[2][128][NR];     // x_j (then v_k), [row][rhs]
    // behind an abandoned dataflow factorisation (cholflow.hip: abort word set) the factor is garbage and the host will repeat
    // everything: leave at once (X keeps its "not published" pattern, which reads as NaN)
    if (abort_word && __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    __shared__ __attribute__((aligned(32))) double red[4][128][NR];    // partial sums
    const int tid = threadIdx.x;
    const int k = nb - 1 - (int)blockIdx.x;
    const int c2 = tid & 63, qd = tid >> 6;        // block phase: columns 2*c2, 2*c2+1; rows 32*qd .. 32*qd+31
    const int di = tid & 127, dh = tid >> 7;       // diagonal phase: output row di, half dh of the sum
    const int sr = tid & 127, sq = tid >> 7;       // staging: row sr, right-hand sides sq, sq+2, sq+4, sq+6
    // inverse of the diagonal block and the right-hand side of this block, fetched ahead
    double dinv[64], zk[4];
    {
        const double *w = invd + (long)k * 16384 + (long)(64 * dh) * 128 + di;
#pragma unroll
        for (int r = 0; r < 64; r++) dinv[r] = w[(long)r * 128];
#pragma unroll
        for (int i = 0; i < 4; i++) zk[i] = sq + 2 * i < nrhs ? Z[(long)(sq + 2 * i) * zs + k * 128 + sr] : 0.0;   // nrhs <= NR
    }
    double acc[2][NR];
#pragma unroll
    for (int q = 0; q < NR; q++) acc[0][q] = acc[1][q] = 0.0;
    d2_t blk[32], nblk[32];
    int j = nb - 1;
    if (j > k) {
        const double *lp = L + (long)(j * 128 + 32 * qd) * ld + k * 128 + 2 * c2;
#pragma unroll
        for (int r = 0; r < 32; r++) blk[r] = *reinterpret_cast<const d2_t *>(lp + (long)r * ld);
    }
    for (; j > k; --j) {
        if (j - 1 > k) {
            const double *lp = L + (long)((j - 1) * 128 + 32 * qd) * ld + k * 128 + 2 * c2;
#pragma unroll
            for (int r = 0; r < 32; r++) nblk[r] = *reinterpret_cast<const d2_t *>(lp + (long)r * ld);
        }
        {   // wait for x_j: every thread polls the (up to four) values it stages
            unsigned long long b[4];
            const unsigned long long *xp = reinterpret_cast<const unsigned long long *>(X) + j * 128 + sr;
            int spin = 0;
            bool ready;
            do {
                ready = true;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    b[i] = 0;
                    if (sq + 2 * i < nrhs) {
                        // every 1024th poll by a read-modify-write at agent scope: never served from a stale line of this
                        // XCD's L2 (cholflow.hip, "Visibility": plain polls were seen to miss a set flag about once in 300
                        // factorisations)
                        const unsigned long long *q = xp + (long)(sq + 2 * i) * xs;
                        b[i] = (spin & 1023) == 1023
                                   ? __hip_atomic_fetch_or(const_cast<unsigned long long *>(q), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                   : __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        ready = ready && b[i] != BS_UNSET;
                    }
                }
                if (!ready) __builtin_amdgcn_s_sleep(2);
            } while (!ready && ++spin < BS_SPIN_MAX);
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (sq + 2 * i < NR) xj[j & 1][sr][sq + 2 * i] = __longlong_as_double((long long)b[i]);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 32; r++) {
            double xv[NR];
            bs_row<NR>(&xj[j & 1][32 * qd + r][0], xv);
#pragma unroll
            for (int q = 0; q < NR; q++) {
                acc[0][q] += blk[r].x * xv[q];
                acc[1][q] += blk[r].y * xv[q];
            }
        }
#pragma unroll
        for (int r = 0; r < 32; r++) blk[r] = nblk[r];
    }
#pragma unroll
    for (int q = 0; q < NR; q++) {
        red[qd][2 * c2][q] = acc[0][q];
        red[qd][2 * c2 + 1][q] = acc[1][q];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int q = sq + 2 * i;
        if (q < NR) xj[0][sr][q] = zk[i] - (red[0][sr][q] + red[1][sr][q] + red[2][sr][q] + red[3][sr][q]);
    }
    __syncthreads();
    // x_k[di] = sum_r W[r][di] v[r]
    double out[NR];
#pragma unroll
    for (int q = 0; q < NR; q++) out[q] = 0.0;
#pragma unroll
    for (int r = 0; r < 64; r++) {
        double vv[NR];
        bs_row<NR>(&xj[0][64 * dh + r][0], vv);
#pragma unroll
        for (int q = 0; q < NR; q++) out[q] += dinv[r] * vv[q];
    }
    if (dh == 1) {
#pragma unroll
        for (int q = 0; q < NR; q++) red[0][di][q] = out[q];
    }
    __syncthreads();
    if (dh == 0) {
        unsigned long long *xp = reinterpret_cast<unsigned long long *>(X) + k * 128 + di;
#pragma unroll
        for (int q = 0; q < NR; q++) {
            if (q >= nrhs) break;
            unsigned long long bits = (unsigned long long)__double_as_longlong(out[q] + red[0][di][q]);
            if (bits == BS_UNSET) bits = 0x7FF8000000000000ull;
            __hip_atomic_store(xp + (long)q * xs, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Forward substitution L z = b for ONE right-hand side in one launch: the mirror image of the chain above, for right-hand
// sides that did not ride through the factorisation (iterative refinement, engine.hip: the residual exists only after the
// first solution).  Workgroup k owns block ROW k: it streams the blocks L[k][j], j < k (rows of 1 KB: one cache line per
// 16 lanes), subtracts L[k][j] z_j as soon as the owner of row j has published z_j, then applies the inverse of its
// diagonal block.  Same flag protocol (Z preset to the all-ones pattern, relaxed agent-scope atomics), same progress
// argument (a workgroup waits only for workgroups with a smaller index) and the same bounded spin.
__global__ __launch_bounds__(256) void forwardsolve_chain_kernel(const double *__restrict__ L, long ld,
                                                                 const double *__restrict__ invd, const double *__restrict__ B,
                                                                 double *Z, int nb) {
    __shared__ __attribute__((aligned(16))) double zj[2][128];      // z_j
    __shared__ double red[128][65];                                 // per-lane partial sums of the 128 rows
    __shared__ double part[2][128];
    __shared__ double bk[128];
    const int tid = threadIdx.x;
    const int k = blockIdx.x;
    const int c2 = tid & 63, qd = tid >> 6;        // block phase: columns 2*c2, 2*c2+1; rows 32*qd .. 32*qd+31
    const int di = tid & 127, dh = tid >> 7;       // diagonal phase: output row di, columns 64*dh .. 64*dh+63
    double dinv[64];
    {
        const double *w = invd + (long)k * 16384 + (long)di * 128 + 64 * dh;     // row di of inv(L_kk)
#pragma unroll
        for (int c = 0; c < 64; c += 2) {
            const d2_t t = *reinterpret_cast<const d2_t *>(w + c);
            dinv[c] = t.x; dinv[c + 1] = t.y;
        }
        if (tid < 128) bk[tid] = B[k * 128 + tid];
    }
    double acc[32];
#pragma unroll
    for (int r = 0; r < 32; r++) acc[r] = 0.0;
    d2_t blk[32], nblk[32];
    if (k > 0) {
        const double *lp = L + (long)(k * 128 + 32 * qd) * ld + 2 * c2;
#pragma unroll
        for (int r = 0; r < 32; r++) blk[r] = *reinterpret_cast<const d2_t *>(lp + (long)r * ld);
    }
    for (int j = 0; j < k; ++j) {
        if (j + 1 < k) {
            const double *lp = L + (long)(k * 128 + 32 * qd) * ld + (j + 1) * 128 + 2 * c2;
#pragma unroll
            for (int r = 0; r < 32; r++) nblk[r] = *reinterpret_cast<const d2_t *>(lp + (long)r * ld);
        }
        if (tid < 128) {   // wait for z_j
            const unsigned long long *zp = reinterpret_cast<const unsigned long long *>(Z) + j * 128 + tid;
            unsigned long long b;
            int spin = 0;
            do {
                b = (spin & 1023) == 1023
                        ? __hip_atomic_fetch_or(const_cast<unsigned long long *>(zp), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                        : __hip_atomic_load(zp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (b == BS_UNSET) __builtin_amdgcn_s_sleep(2);
            } while (b == BS_UNSET && ++spin < BS_SPIN_MAX);
            zj[j & 1][tid] = __longlong_as_double((long long)b);
        }
        __syncthreads();
        const d2_t z = *reinterpret_cast<const d2_t *>(&zj[j & 1][2 * c2]);
#pragma unroll
        for (int r = 0; r < 32; r++) acc[r] += blk[r].x * z.x + blk[r].y * z.y;
#pragma unroll
        for (int r = 0; r < 32; r++) blk[r] = nblk[r];
    }
#pragma unroll
    for (int r = 0; r < 32; r++) red[32 * qd + r][c2] = acc[r];
    __syncthreads();
    {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 32; c++) s += red[di][32 * dh + c];
        part[dh][di] = s;
    }
    __syncthreads();
    double out = 0.0;
#pragma unroll
    for (int c = 0; c < 64; c++) {
        const int cc = 64 * dh + c;
        out += dinv[c] * (bk[cc] - (part[0][cc] + part[1][cc]));
    }
    __syncthreads();                 // every read of part[] is done before it is reused for the two halves of `out`
    if (dh == 1) part[0][di] = out;
    __syncthreads();
    if (dh == 0) {
        unsigned long long bits = (unsigned long long)__double_as_longlong(out + part[0][di]);
        if (bits == BS_UNSET) bits = 0x7FF8000000000000ull;
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(Z) + k * 128 + di, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The backward chain for ONE right-hand side: a polling wave and seven streaming waves per workgroup (round 3).
//
// A link of the chain above takes 3.4 us although the hop itself -- agent-scope store in one workgroup, agent-scope load in
// another -- takes 0.42-0.53 us inside an XCD and 0.59-0.65 us across XCDs (scripts/micro/hop_latency.hip; the same test shows that a
// workgroup-scope load (sc0) is served by the CU's L1 and NEVER sees another workgroup's store, so there is no cheaper poll for
// neighbours on one XCD).  The rest is how a workgroup waits and what it still has to do once the last result it depends on is
// there (JAICOV_CHAIN_TRACE prints the link times and the phases of a workgroup):
//  * every workgroup consumes the results in order, one 128 KB block of L per result: it issues the next block's loads, polls
//    (the poll's s_waitcnt vmcnt(0) also waits for the loads just issued: loads return in order), meets at a barrier, does 64
//    FMAs per thread, copies the next block's registers into the current ones (which waits for them once more).  Polls issued
//    ahead of the loads do not help: every REPEATED poll still queues behind them;
//  * behind its last block it reduces the partial sums, multiplies with inv(L_kk), and only then publishes: four barriers,
//    each of which (__syncthreads) also waits for every global load in flight.
// Here the two kinds of waiting are separated and most of the work behind the last block is moved in front of it:
//  * wave 0 does nothing but poll: it has no other memory operation in flight, runs up to CH_RD results ahead of the stream and
//    hands them over through a ring in LDS (values + a sequence word per slot; a count of the waves that are done with a slot
//    lets it be reused);
//  * waves 1..7 stream the blocks (18 or 19 rows each), two buffers used in turn, every refill issued right behind the last use
//    of its buffer.  They wait for results by spinning on the sequence word in LDS -- lgkmcnt, not vmcnt: their block loads stay
//    in flight -- and for a block with the exact s_waitcnt vmcnt the compiler derives from straight-line code (all loads are
//    unconditional; past the end of the stream they re-read one 16-byte piece that sits in the L1).  No workgroup barrier in
//    the loop;
//  * the LAST blocks of every stream (CH_PM = 5, or 4 where that makes the rest an even number) are multiplied into the diagonal
//    inverse beforehand,
//        x_k = W_k'(z_k - S) - sum_m P_m[k]' x_{k+m},   P_m[k] = L[k+m][k] W_k,   S = the sum over the other blocks
//    (SolveChains::premultiply(): one batched launch of 128^3 MFMA GEMMs after the factorisation), so that u = W_k'(z_k - S) --
//    the reduction over the waves, three barriers, the product with inv(L_kk) from LDS: ~2.5 us -- is formed four or five links
//    before the workgroup's turn.  The pre-multiplied blocks are streamed like the others (same buffers, same ring); what is
//    left of a link is: the polling wave sees x_{k+1}, hands it over, 38 FMAs per streaming thread, ONE exchange through LDS +
//    barrier, store.  The barriers behind the stream order LDS traffic only (chain_lds_barrier()).
// Same flag protocol towards the other workgroups (results preset to the all-ones pattern, relaxed agent-scope atomics), same
// progress argument (a workgroup waits only for workgroups with a smaller index) and the same bounded spin as above.
// What it gives at config 4 (118 links): 0.41 -> 0.31 ms, links of 2.6 us on average (1.5 - 2.1 and 2.7 - 3.9 in turn; the first
// links of a chain, whose successors are waiting, take 1.2 - 1.5).  That average is what ONE CU can stream: every workgroup reads
// one 128 KB block per link, and 128 KB / 2.6 us = 50 GB/s is the rate a single CU reaches on this chip whatever is in flight
// (the longest column alone, 15 MB, takes 0.3 ms).  With CH_PM = 4, 5, 6 the two-link sum stays at 5.2 - 5.4 us, only its split
// between the two links moves.  Going below takes two CUs per block column: backsolve_chain8_kernel<2>.  Steps on the way, all measured: polling wave + ring + two
// pre-multiplied blocks resident behind the stream 0.345 ms (the u-phase still ended after the predecessor had published);
// every wave polling the last two results itself instead of the polling wave: no gain; touching the pre-multiplied blocks into the
// L2 ahead of their loads: 0.41 ms (the polls queue behind the touches).  The forward chain has this form too where two
// workgroups can share a block row (forwardsolve_chain8_kernel: 10 row sums per lane instead of 19, which spilled).
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double readlane_f64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ unsigned long long chain_poll(const unsigned long long *p, int spin) {
    // every 1024th poll by a read-modify-write at agent scope (see backsolve_chain_kernel)
    return (spin & 1023) == 1023 ? __hip_atomic_fetch_or(const_cast<unsigned long long *>(p), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                 : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void chain_publish(double *dst, double v) {
    unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    if (bits == BS_UNSET) bits = 0x7FF8000000000000ull;
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(dst), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
constexpr int CHAIN8_THREADS = 512;
constexpr int CH_RD = 8;              // slots of the ring between the polling wave and the streaming waves
constexpr int CH_SW = 7;              // streaming waves
constexpr int CH_ROWS = 19;           // rows of a block per streaming wave: waves 1..5 take 18, waves 6 and 7 take 19
#ifndef JAICOV_CH_PM
#define JAICOV_CH_PM 5
#endif
constexpr int CH_PM = JAICOV_CH_PM;              // blocks below a diagonal block that are multiplied into its inverse (SolveChains::premultiply)
struct ChainRing {
    double xs[CH_RD][128];            // published results, in the order of the stream
    int ready[CH_RD];                 // 1 + index of the stream entry the slot holds
    int consumed[CH_RD];              // streaming waves that are done with the slot, counted over all its uses
};
__device__ __forceinline__ void chain_ring_init(ChainRing &rg, int tid) {
    if (tid < CH_RD) { rg.ready[tid] = 0; rg.consumed[tid] = 0; }
}
// A workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every global load in flight (s_waitcnt
// vmcnt(0)): behind the stream those are the two pre-multiplied blocks and the first polls for the predecessors' results, which
// the u-phase does not need -- its three barriers cost 7 us that way (JAICOV_CHAIN_TRACE), on the chain's critical path.
__device__ __forceinline__ void chain_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// the polling wave: entry i of the stream = the 128 values at src
__device__ __forceinline__ void chain_ring_put(ChainRing &rg, int i, const double *src, int lane) {
    const int slot = i & (CH_RD - 1);
    if (i >= CH_RD) {       // every streaming wave is done with what the slot held
        const int need = CH_SW * (i / CH_RD);
        while (__hip_atomic_load(&rg.consumed[slot], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < need) __builtin_amdgcn_s_sleep(1);
    }
    const unsigned long long *p = reinterpret_cast<const unsigned long long *>(src) + lane;
    unsigned long long b0, b1;
    int spin = 0;
    do {
        b0 = chain_poll(p, spin);
        b1 = chain_poll(p + 64, spin);
        if (b0 == BS_UNSET || b1 == BS_UNSET) __builtin_amdgcn_s_sleep(1);
    } while ((b0 == BS_UNSET || b1 == BS_UNSET) && ++spin < BS_SPIN_MAX);
    rg.xs[slot][lane] = __longlong_as_double((long long)b0);
    rg.xs[slot][lane + 64] = __longlong_as_double((long long)b1);
    __hip_atomic_store(&rg.ready[slot], i + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);   // one wave: every lane writes the same word
}
// a streaming wave: waits for entry i, returns its slot.  No time limit of its own: the polling wave's waits are the bounded
// ones (chain_ring_put gives up on a lost predecessor after BS_SPIN_MAX polls and hands over the "not published" pattern, a NaN),
// and it sets `ready` for every entry whatever happened, so this loop ends whenever that one does -- and a predecessor that is
// merely LATE is waited for as long as the polling wave waits, instead of being replaced by stale ring contents after a shorter
// spin of this wave's own (a finite but wrong x_k; the tests rely on a lost link showing up as NaNs).
// (No poll limit of its own: the only producer is this workgroup's polling wave, whose own wait for the predecessor IS limited
// (BS_SPIN_MAX) and which then hands over the "not published" pattern -- every slot is filled after a bounded time, with a NaN at worst.)
__device__ __forceinline__ int chain_ring_get(ChainRing &rg, int i) {
    const int slot = i & (CH_RD - 1);
    while (__hip_atomic_load(&rg.ready[slot], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != i + 1) __builtin_amdgcn_s_sleep(0);
    return slot;
}
__device__ __forceinline__ void chain_ring_done(ChainRing &rg, int slot, int lane) {
    if (lane == 0) __hip_atomic_fetch_add(&rg.consumed[slot], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// SPLIT = 2: workgroups 2 p and 2 p + 1 share chain position p; each streams the 64 columns of every block that belong to its 64
// outputs (half the load instructions per link: the chain with one workgroup per column runs at what ONE CU can stream, a 128 KB
// block per 2.6 us; loading 10 of a wave's 19 rows -- wrong results, right timing -- gave 1.05 us per link), forms its half of
// v = z_k - S, passes it to the other through `xch` (preset to the "not published" pattern like X; once per column, several links
// before the workgroup's turn), and publishes its half of x_k.  Used when the whole grid is resident at once (2 nb <= CUs): a
// workgroup then also waits for its partner, which has the higher index in one of the two cases (progress: the partner is the
// next workgroup the dispatcher starts).  0.31 -> 0.265 ms at config 4, links of 2.2 us: what is left is the way of a result from
// the store through the successor's polling wave, ring, products and barrier to its store.
template <int SPLIT>
__global__ __launch_bounds__(CHAIN8_THREADS) void backsolve_chain8_kernel(const double *__restrict__ L, long ld, const double *__restrict__ invd,
                                                                          const double *__restrict__ PM, const double *__restrict__ Z,
                                                                          double *X, double *xch, int nb, const int *abort_word, long long *trace) {
    __shared__ double red[8][128];
    __shared__ double comb[4][128];
    __shared__ double vv[128];
    __shared__ double Wl[128 * 129 / 2];           // inv(L_kk), lower triangle packed by rows
    __shared__ ChainRing ring;
    if (abort_word && __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pos = SPLIT == 2 ? (int)(blockIdx.x >> 1) : (int)blockIdx.x;          // position in the chain
    const int half = SPLIT == 2 ? (int)(blockIdx.x & 1) : 0;                        // which 64 outputs are this workgroup's
    const int k = nb - 1 - pos;
    if (SPLIT == 2 && half == 1) trace = nullptr;
    // The c = pos predecessors x_{k+1} .. x_{nb-1} are ONE stream, in the order they are published (x_{nb-1} first):
    //   entries 0 .. n_plain-1   blocks L[nb-1-i][k] of the factor, summed into S;  u = W_k'(z_k - S) is formed behind them,
    //   entries n_plain .. c-1   the pre-multiplied blocks P_m, m = c - i = npre .. 1, whose products go straight into x_k.
    // npre = CH_PM or CH_PM - 1, whichever makes n_plain even (the first loop then has no half step), or all of them.
    const int c = pos;
    const int npre = c <= CH_PM ? c : (((c - CH_PM) & 1) ? CH_PM - 1 : CH_PM);
    const int n_plain = c - npre;
    const int di = tid & 127, h4 = tid >> 7;       // diagonal phase: output di, operand quarter h4
    // streaming waves 1..7: rows r0 .. r0 + nrows - 1, columns 2*lane, 2*lane+1
    const int nrows = wave <= 5 ? 18 : 19;
    const int last_row = nrows - 1;                // buffer entry 18 of a wave with 18 rows repeats row 17 (its product is dropped)
    const int r0 = wave == 0 ? 0 : (wave <= 5 ? 18 * (wave - 1) : 90 + 19 * (wave - 6));
#define CHAIN8_STAMP(q) if (trace && tid == 64) trace[nb + 8 * pos + (q)] = wall_clock64();
#define CHAIN8_STAMP_T(q, t) if (trace && tid == (t)) trace[nb + 8 * pos + (q)] = wall_clock64();
    CHAIN8_STAMP(0);
    chain_ring_init(ring, tid);
    {   // inv(L_kk) -> LDS
        const double *w = invd + (long)k * 16384 + (long)(32 * h4) * 128 + di;
        double tw[32];
#pragma unroll
        for (int r = 0; r < 32; r++) tw[r] = w[(long)r * 128];
#pragma unroll
        for (int r = 0; r < 32; r++) {
            const int rr = 32 * h4 + r;
            if (di <= rr) Wl[rr * (rr + 1) / 2 + di] = tw[r];
        }
    }
    double zk = 0.0;
    if (tid < 128) zk = Z[k * 128 + tid];
    __syncthreads();
    const char *lcol = reinterpret_cast<const char *>(L + (long)r0 * ld + k * 128);
    const long bstep = 128 * ld * 8;               // bytes from one block row to the next
    // SPLIT = 1: a lane holds columns 2 lane, 2 lane + 1 of the wave's 18 / 19 rows, one row per load instruction.
    // SPLIT = 2: a lane holds columns 64 half + 2 (lane & 31), + 1 of every second row (lanes 0..31 the even, 32..63 the odd rows of
    //            the wave's share): TWO rows per load instruction, ten instructions per block -- what a CU can stream is set by
    //            the number of its load instructions (lane requests), not by their bytes: 8-byte loads of 64 columns x 19 rows gave
    //            0.27 ms, no better than the bytes of the unsplit chain would suggest.
    constexpr int NBUF = SPLIT == 2 ? (CH_ROWS + 1) / 2 : CH_ROWS;
    const int hr = SPLIT == 2 ? lane >> 5 : 0;                  // row parity of this lane
    const unsigned colbytes = SPLIT == 2 ? 8u * (unsigned)(64 * half + 2 * (lane & 31)) : 16u * (unsigned)lane;
    const bool own = SPLIT == 1 || (tid >> 6) == half;          // (of a thread tid < 128: its output is this workgroup's)
    const char *dummy = reinterpret_cast<const char *>(invd);
    const double *pmk = PM + (long)k * 16384;      // P_m of this column: pmk + (m - 1) * nb * 16384
    const long pmstep = (long)nb * 16384;
    d2_t A[NBUF], B[NBUF];                         // two stream buffers
    double acc0 = 0.0, acc1 = 0.0;                 // S (streamed blocks of the factor), then the pre-multiplied part
    // Stream entry i into a buffer: a block of the factor, a pre-multiplied block, or (past the end) nothing.  Addresses =
    // wave-uniform row base (scalar registers) + a 32-bit lane offset.  Loads past the end are issued all the same (straight-line
    // code keeps the s_waitcnt counts exact) but read one 16-byte piece that is in the L1.  A __builtin_amdgcn_sched_barrier(0)
    // stands on either side: without it the scheduler moves the refill loads about, and the register copies the compiler places on
    // the loop's back edge (it renames one buffer: 38 v_mov_b64) came behind an s_waitcnt vmcnt(0) -- the refill just issued had to
    // land before the loop went on, and the second buffer bought nothing; with it the copies wait for the older refill only.
#define CHAIN8_ENTRY(buf, i)                                                                                               \
    {                                                                                                                      \
        const bool fac = (i) < n_plain, pre = !fac && (i) < c;                                                             \
        const char *bp = fac ? lcol + (long)(nb - 1 - (i)) * bstep                                                         \
                             : (pre ? reinterpret_cast<const char *>(pmk + (long)(c - (i) - 1) * pmstep + (long)r0 * 128) : dummy); \
        const long st = fac ? ld * 8 : (pre ? 1024 : 0);                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                                 \
        if (SPLIT == 2) {                                                                                                  \
            const unsigned vo = (fac || pre) ? colbytes : 0u;                                                              \
            _Pragma("unroll") for (int r = 0; r < NBUF; r++) {                                                             \
                /* row 2 r + hr of the wave's share; past its end the last row again (that product is dropped: x = 0) */   \
                const int row = 2 * r + hr < last_row ? 2 * r + hr : last_row;                                             \
                buf[r] = *reinterpret_cast<const d2_t *>(bp + (long)row * st + vo);                                        \
            }                                                                                                              \
        } else {                                                                                                           \
            const unsigned vo = (fac || pre) ? colbytes : 0u;                                                              \
            _Pragma("unroll") for (int r = 0; r < NBUF; r++)                                                               \
                buf[r] = *reinterpret_cast<const d2_t *>(bp + (long)(r < 18 ? r : last_row) * st + vo);                    \
        }                                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                                 \
    }
#define CHAIN8_USE(buf, slot)                                                        \
    {                                                                                \
        const double xl = ring.xs[slot][xlane];     /* one LDS read per lane, then scalar broadcasts */ \
        const double xv = xdrop ? 0.0 : xl;         /* entries past the wave's share */ \
        if (SPLIT == 2) {                                                            \
            _Pragma("unroll") for (int r = 0; r < NBUF; r++) {                       \
                const double x0 = readlane_f64(xv, 2 * r), x1 = readlane_f64(xv, 2 * r + 1); \
                const double xr = hr ? x1 : x0;                                      \
                acc0 += buf[r].x * xr;                                               \
                acc1 += buf[r].y * xr;                                               \
            }                                                                        \
        } else {                                                                     \
            _Pragma("unroll") for (int r = 0; r < NBUF; r++) {                       \
                const double xr = readlane_f64(xv, r);                               \
                acc0 += buf[r].x * xr;                                               \
                acc1 += buf[r].y * xr;                                               \
            }                                                                        \
        }                                                                            \
    }
    const int xlane = r0 + (lane < nrows ? lane : last_row);
    const bool xdrop = lane >= nrows;               // (v_readlane indices run to 2 NBUF - 1 = 19)
    // ---- the blocks of the factor -----------------------------------------------------------------------------------
    if (wave == 0) {
        for (int i = 0; i < n_plain; i++) chain_ring_put(ring, i, X + (long)(nb - 1 - i) * 128, lane);
        CHAIN8_STAMP_T(6, 0);
    } else {
        CHAIN8_ENTRY(A, 0);
        CHAIN8_ENTRY(B, 1);
        for (int i = 0; i < n_plain; i += 2) {      // n_plain is even
            const int sa = chain_ring_get(ring, i);
            CHAIN8_USE(A, sa);
            chain_ring_done(ring, sa, lane);
            CHAIN8_ENTRY(A, i + 2);
            const int sb = chain_ring_get(ring, i + 1);
            CHAIN8_USE(B, sb);
            chain_ring_done(ring, sb, lane);
            CHAIN8_ENTRY(B, i + 3);
        }
        CHAIN8_STAMP(1);
        CHAIN8_STAMP_T(7, 448);
        if (SPLIT == 2) {       // the two row parities of a column pair sit 32 lanes apart
            acc0 += __shfl_xor(acc0, 32, 64);
            acc1 += __shfl_xor(acc1, 32, 64);
            if (lane < 32) { red[wave][64 * half + 2 * lane] = acc0; red[wave][64 * half + 2 * lane + 1] = acc1; }
        } else { red[wave][2 * lane] = acc0; red[wave][2 * lane + 1] = acc1; }
        acc0 = acc1 = 0.0;                          // from here on: the pre-multiplied part
    }
    // ---- u = W_k'(z_k - S): t + 2 links before this workgroup's turn ----------------------------------------------------
    chain_lds_barrier();
    CHAIN8_STAMP(2);
    if (tid < 128) {
        if (own) {
            double s = 0.0;
#pragma unroll
            for (int q = 1; q <= CH_SW; q++) s += red[q][tid];
            vv[tid] = zk - s;
            if (SPLIT == 2) chain_publish(xch + (long)k * 128 + tid, zk - s);
        } else {        // the other workgroup's half of v
            const unsigned long long *xp = reinterpret_cast<const unsigned long long *>(xch) + (long)k * 128 + tid;
            unsigned long long b;
            int spin = 0;
            do {
                b = chain_poll(xp, spin);
                if (b == BS_UNSET) __builtin_amdgcn_s_sleep(2);
            } while (b == BS_UNSET && ++spin < BS_SPIN_MAX);
            vv[tid] = __longlong_as_double((long long)b);
        }
    }
    chain_lds_barrier();
    CHAIN8_STAMP(3);
    {   // branch-free: entries above the diagonal read the row's first entry and are dropped
        double o0 = 0.0, o1 = 0.0;
        int base = 16 * h4 * (32 * h4 + 1);                       // rr (rr + 1) / 2 at rr = 32 h4
#pragma unroll 4
        for (int r = 0; r < 32; r += 2) {
            const int rr = 32 * h4 + r;
            const double w0 = Wl[base + (di <= rr ? di : 0)];
            const double w1 = Wl[base + rr + 1 + (di <= rr + 1 ? di : 0)];
            o0 += (di <= rr ? w0 : 0.0) * vv[rr];
            o1 += (di <= rr + 1 ? w1 : 0.0) * vv[rr + 1];
            base += 2 * rr + 3;
        }
        comb[h4][di] = o0 + o1;
    }
    chain_lds_barrier();
    double u = 0.0;
    if (tid < 128) u = (comb[0][tid] + comb[1][tid]) + (comb[2][tid] + comb[3][tid]);
    CHAIN8_STAMP(4);
    // ---- the pre-multiplied blocks (at most CH_PM): from here on a link of the chain is poll -> LDS -> 38 FMAs -> LDS -> store ------
    if (wave == 0) {
        // (touching the pre-multiplied blocks into the L2 ahead of their loads was tried here: 0.31 -> 0.41 ms, the polls queue behind it)
        for (int i = n_plain; i < c; i++) chain_ring_put(ring, i, X + (long)(nb - 1 - i) * 128, lane);
    } else {
#define CHAIN8_PRE(buf, e)                                      \
    if ((e) < npre) {                                           \
        const int sl = chain_ring_get(ring, n_plain + (e));     \
        CHAIN8_USE(buf, sl);                                    \
        chain_ring_done(ring, sl, lane);                        \
        CHAIN8_ENTRY(buf, n_plain + (e) + 2);                   \
    }
        CHAIN8_PRE(A, 0);
        CHAIN8_PRE(B, 1);
        CHAIN8_PRE(A, 2);
        CHAIN8_PRE(B, 3);
        CHAIN8_PRE(A, 4);
        CHAIN8_PRE(B, 5);
        static_assert(CH_PM <= 6, "one CHAIN8_PRE per pre-multiplied block");
#undef CHAIN8_PRE
        CHAIN8_STAMP(5);
        if (SPLIT == 2) {       // the two row parities of a column pair sit 32 lanes apart
            acc0 += __shfl_xor(acc0, 32, 64);
            acc1 += __shfl_xor(acc1, 32, 64);
            if (lane < 32) { red[wave][64 * half + 2 * lane] = acc0; red[wave][64 * half + 2 * lane + 1] = acc1; }
        } else { red[wave][2 * lane] = acc0; red[wave][2 * lane + 1] = acc1; }
    }
    if (c > 0) {
        chain_lds_barrier();
        if (tid < 128 && own) {
            double s = 0.0;
#pragma unroll
            for (int q = 1; q <= CH_SW; q++) s += red[q][tid];
            u -= s;
        }
    }
    if (tid < 128 && own) chain_publish(X + (long)k * 128 + tid, u);
#undef CHAIN8_STAMP
#undef CHAIN8_STAMP_T
#undef CHAIN8_USE
#undef CHAIN8_ENTRY
    if (trace && tid == 0) trace[pos] = wall_clock64();          // JAICOV_CHAIN_TRACE: when each link was published (100 MHz)
}

// ---------------------------------------------------------------------------------------------------------------
// The forward chain L z = b for ONE right-hand side in the form of backsolve_chain8_kernel<2>: two workgroups per block row k, each
// owning 64 of its 128 outputs; polling wave + ring; the blocks next to the diagonal (CH_PM or CH_PM - 1 of them) pre-multiplied,
//     z_k = W_k (b_k - S) - sum_m Ft_m[k]' z_{k-m},   Ft_m[k] = (W_k L[k][k-m])'   (rows: index into z_{k-m}, columns: outputs),
// and u = W_k (b_k - S) formed ahead of them.  The blocks of the factor are used as rows here (L[k][i] z_i: a workgroup streams the
// 64 rows of its outputs, whole 1 KB rows per load instruction, 9 or 10 rows per streaming wave, one partial sum per row and lane,
// reduced over the lanes through LDS in the u-phase); the pre-multiplied blocks as in the backward chain (64 columns, two rows per
// load instruction).  Both kinds go through the same two buffers of ten entries.  Only launched when the whole grid is resident
// at once (2 nb <= CUs); forwardsolve_chain_kernel otherwise.
// ---------------------------------------------------------------------------------------------------------------
constexpr int CHF_ROWS = 10;          // rows of a block per streaming wave in the forward chain: waves 1..6 take 9, wave 7 takes 10
__global__ __launch_bounds__(CHAIN8_THREADS) void forwardsolve_chain8_kernel(const double *__restrict__ L, long ld, const double *__restrict__ invd,
                                                                             const double *__restrict__ FT, const double *__restrict__ Bv,
                                                                             double *Z, double *xch, int nb) {
    __shared__ double red[64][65];                 // per-lane partial sums of the 64 rows; the partial sums of the pre-multiplied part ([8][128]) afterwards
    __shared__ double part[8][64];
    __shared__ double comb[8][64];
    __shared__ double vv[128];
    __shared__ double Wl[128 * 129 / 2];           // inv(L_kk), lower triangle packed by columns: (row, c) at c * 128 - c (c - 1) / 2 + (row - c)
    __shared__ ChainRing ring;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x >> 1, half = blockIdx.x & 1;      // block row = position in the chain; which 64 outputs
    const int c = k;                               // predecessors z_0 .. z_{k-1}, published in this order: ONE stream
    const int npre = c <= CH_PM ? c : (((c - CH_PM) & 1) ? CH_PM - 1 : CH_PM);
    const int n_plain = c - npre;                  // entries i < n_plain: L[k][i] with z_i; then Ft_m[k], m = c - i, with z_i
    const int di = tid & 127, h4 = tid >> 7;
    // streaming waves 1..7, blocks of the factor: rows 64 half + r0f .. + nrf - 1 (all 128 columns: 2 lane, 2 lane + 1)
    const int nrf = wave <= 6 ? 9 : 10, r0f = wave == 0 ? 0 : 9 * (wave - 1);
    // pre-multiplied blocks: rows r0 .. r0 + nrows - 1 (every second one per lane half), columns 64 half + 2 (lane & 31), + 1
    const int nrows = wave <= 5 ? 18 : 19, last_row = nrows - 1;
    const int r0 = wave == 0 ? 0 : (wave <= 5 ? 18 * (wave - 1) : 90 + 19 * (wave - 6));
    const int hr = lane >> 5;
    chain_ring_init(ring, tid);
    {
        const double *w = invd + (long)k * 16384 + (long)di * 128 + 32 * h4;     // row di of inv(L_kk)
        d4_t t[8];
#pragma unroll
        for (int q = 0; q < 8; q++) t[q] = *reinterpret_cast<const d4_t *>(w + 4 * q);
#pragma unroll
        for (int q = 0; q < 32; q++) {
            const int cc = 32 * h4 + q;
            if (cc <= di) Wl[cc * 128 - cc * (cc - 1) / 2 + (di - cc)] = t[q >> 2][q & 3];
        }
    }
    double bk = 0.0;
    if (tid < 128) bk = Bv[k * 128 + tid];
    __syncthreads();
    const bool own = (tid >> 6) == half;           // (of a thread tid < 128: its output is this workgroup's)
    const char *lrow = reinterpret_cast<const char *>(L + (long)(k * 128 + 64 * half + r0f) * ld);
    const char *dummy = reinterpret_cast<const char *>(invd);
    const double *ftk = FT + (long)k * 16384;      // Ft_m of this block row: ftk + (m - 1) * nb * 16384
    const long pmstep = (long)nb * 16384;
    const unsigned cb_fac = 16u * (unsigned)lane, cb_pre = 8u * (unsigned)(64 * half + 2 * (lane & 31));
    d2_t A[CHF_ROWS], B[CHF_ROWS];
    static_assert(CHF_ROWS == (CH_ROWS + 1) / 2, "one pair of buffers serves both kinds of blocks");
    double acc[CHF_ROWS];
#pragma unroll
    for (int r = 0; r < CHF_ROWS; r++) acc[r] = 0.0;
    double p0 = 0.0, p1 = 0.0;
    // stream entry i into a buffer (see backsolve_chain8_kernel): a block of the factor (rows of this workgroup), a pre-multiplied
    // block (columns of this workgroup), or nothing
#define CHAINF_ENTRY(buf, i)                                                                                               \
    {                                                                                                                      \
        const bool fac = (i) < n_plain, pre = !fac && (i) < c;                                                             \
        const char *bp = fac ? lrow + (long)(i) * 1024                                                                     \
                             : (pre ? reinterpret_cast<const char *>(ftk + (long)(c - (i) - 1) * pmstep + (long)r0 * 128) : dummy); \
        const long st = fac ? ld * 8 : (pre ? 1024 : 0);                                                                   \
        const unsigned vo = fac ? cb_fac : (pre ? cb_pre : 0u);                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                                                 \
        _Pragma("unroll") for (int r = 0; r < CHF_ROWS; r++) {                                                             \
            const int rf = r < nrf ? r : nrf - 1, rp = 2 * r + hr < last_row ? 2 * r + hr : last_row;                      \
            buf[r] = *reinterpret_cast<const d2_t *>(bp + (long)(fac ? rf : rp) * st + vo);                                \
        }                                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                                 \
    }
    if (wave == 0) {
        for (int i = 0; i < n_plain; i++) chain_ring_put(ring, i, Z + (long)i * 128, lane);
    } else {
#define CHAINF_USE(buf, slot)                                                                                              \
    {                                                                                                                      \
        const d2_t z = *reinterpret_cast<const d2_t *>(&ring.xs[slot][2 * lane]);                                          \
        _Pragma("unroll") for (int r = 0; r < CHF_ROWS; r++) acc[r] = __builtin_fma(buf[r].y, z.y, __builtin_fma(buf[r].x, z.x, acc[r])); \
    }
        CHAINF_ENTRY(A, 0);
        CHAINF_ENTRY(B, 1);
        for (int i = 0; i < n_plain; i += 2) {      // n_plain is even
            const int sa = chain_ring_get(ring, i);
            CHAINF_USE(A, sa);
            chain_ring_done(ring, sa, lane);
            CHAINF_ENTRY(A, i + 2);
            const int sb = chain_ring_get(ring, i + 1);
            CHAINF_USE(B, sb);
            chain_ring_done(ring, sb, lane);
            CHAINF_ENTRY(B, i + 3);
        }
#undef CHAINF_USE
#pragma unroll
        for (int r = 0; r < CHF_ROWS; r++)
            if (r < nrf) red[r0f + r][lane] = acc[r];
    }
    // ---- u = W_k (b_k - S) for this workgroup's outputs: npre links before its turn ------------------------------------
    chain_lds_barrier();
    {   // row sums: thread (row, group of eight lanes)
        const int rl = tid & 63, g = tid >> 6;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 8; q++) s += red[rl][8 * g + q];
        part[g][rl] = s;
    }
    chain_lds_barrier();
    if (tid < 128) {
        if (own) {
            const int rl = tid & 63;
            const double s = ((part[0][rl] + part[1][rl]) + (part[2][rl] + part[3][rl])) + ((part[4][rl] + part[5][rl]) + (part[6][rl] + part[7][rl]));
            vv[tid] = bk - s;
            chain_publish(xch + (long)k * 128 + tid, bk - s);
        } else {        // the other workgroup's half of v
            const unsigned long long *xp = reinterpret_cast<const unsigned long long *>(xch) + (long)k * 128 + tid;
            unsigned long long b;
            int spin = 0;
            do {
                b = chain_poll(xp, spin);
                if (b == BS_UNSET) __builtin_amdgcn_s_sleep(2);
            } while (b == BS_UNSET && ++spin < BS_SPIN_MAX);
            vv[tid] = __longlong_as_double((long long)b);
        }
    }
    chain_lds_barrier();
    {   // thread (output 64 half + (tid & 63), columns 16 g .. 16 g + 15)
        const int o = 64 * half + (tid & 63), g = tid >> 6;
        double out = 0.0;
#pragma unroll 4
        for (int q = 0; q < 16; q++) {
            const int cc = 16 * g + q;
            const double w = Wl[cc * 128 - cc * (cc - 1) / 2 + (cc <= o ? o - cc : 0)];
            out += (cc <= o ? w : 0.0) * vv[cc];
        }
        comb[g][tid & 63] = out;
    }
    chain_lds_barrier();
    double u = 0.0;
    if (tid < 128 && own) {
        const int ol = tid & 63;
        u = ((comb[0][ol] + comb[1][ol]) + (comb[2][ol] + comb[3][ol])) + ((comb[4][ol] + comb[5][ol]) + (comb[6][ol] + comb[7][ol]));
    }
    // ---- the pre-multiplied blocks --------------------------------------------------------------------------------------------
    double *red2 = &red[0][0];                     // [8][128]; every read of red[][] is three barriers back
    if (wave == 0) {
        for (int i = n_plain; i < c; i++) chain_ring_put(ring, i, Z + (long)i * 128, lane);
    } else {
        const int xlane = r0 + (lane < nrows ? lane : last_row);
        const bool xdrop = lane >= nrows;
#define CHAINF_PRE(buf, e)                                                                   \
    if ((e) < npre) {                                                                        \
        const int sl = chain_ring_get(ring, n_plain + (e));                                  \
        const double xl = ring.xs[sl][xlane];                                                \
        const double xv = xdrop ? 0.0 : xl;                                                  \
        _Pragma("unroll") for (int r = 0; r < CHF_ROWS; r++) {                               \
            const double x0 = readlane_f64(xv, 2 * r), x1 = readlane_f64(xv, 2 * r + 1);     \
            const double xr = hr ? x1 : x0;                                                  \
            p0 += buf[r].x * xr;                                                             \
            p1 += buf[r].y * xr;                                                             \
        }                                                                                    \
        chain_ring_done(ring, sl, lane);                                                     \
        CHAINF_ENTRY(buf, n_plain + (e) + 2);                                                \
    }
        CHAINF_PRE(A, 0);
        CHAINF_PRE(B, 1);
        CHAINF_PRE(A, 2);
        CHAINF_PRE(B, 3);
        CHAINF_PRE(A, 4);
        CHAINF_PRE(B, 5);
#undef CHAINF_PRE
        p0 += __shfl_xor(p0, 32, 64);
        p1 += __shfl_xor(p1, 32, 64);
        if (lane < 32) { red2[wave * 128 + 64 * half + 2 * lane] = p0; red2[wave * 128 + 64 * half + 2 * lane + 1] = p1; }
    }
    if (c > 0) {
        chain_lds_barrier();
        if (tid < 128 && own) {
            double s = 0.0;
#pragma unroll
            for (int q = 1; q <= CH_SW; q++) s += red2[q * 128 + tid];
            u -= s;
        }
    }
    if (tid < 128 && own) chain_publish(Z + (long)k * 128 + tid, u);
#undef CHAINF_ENTRY
}

// ---------------------------------------------------------------------------------------------------------------
// The polling-wave chains pay two batched GEMM launches per factorisation (~0.1 ms) for ~1.2 us per link and chain: from this many
// block columns on (config 2, 6 block columns: 0.085 -> 0.14 ms per pass with them; config 3, 29: 0.28 -> 0.27)
int chain8_min_blocks(const FlowHooks &h) { return h.chain8_min_nb != HOOK_UNSET ? h.chain8_min_nb : 24; }

// Which sums a solution vector is made of.  backsolve_chain_kernel<1 / 2 / 4 / 8> form every right-hand side in the same order
// (one accumulator pair per vector, the same reduction), so a vector has the same bits under every NR and beside any other
// vectors -- held at nrhs = 1 .. 8 by test_dense_spd_solve_at_every_count_of_right_hand_sides.  ON PURPOSE not so for ONE
// right-hand side from chain8_min_blocks() block columns on (default 24): the polling-wave form multiplies by pre-multiplied
// blocks P_m = L W (premultiply) instead of L and then W, other products and another summation order.  Its vector agrees with the
// chain kernel's to rounding (the same test: 1e-13 of max|x|), not bit for bit.
ChainDecision chain_decide(int nb, int nrhs, int cus, bool have_buffers, const FlowHooks &h) {
    ChainDecision d{};
    d.polling_wave = nrhs <= 1 && have_buffers && nb >= chain8_min_blocks(h);
    // two workgroups per block column / row when the whole grid is resident at once: a workgroup then also waits for its partner
    d.workgroups = d.polling_wave && nb >= 8 && 2 * nb <= cus ? 2 : 1;
    d.nr = nrhs <= 1 ? 1 : (nrhs <= 2 ? 2 : (nrhs <= 4 ? 4 : 8));
    return d;
}

hipError_t SolveChains::init(const ChainView &view, const FlowHooks &hooks) {
    SolveChains c;
    const size_t nbq = (size_t)(view.nfact / 128) * 16384;
    HIPCHK(c.xch_.reserve((size_t)view.nfact));
    HIPCHK(c.pm_e0_.create(hipEventDisableTiming));
    HIPCHK(c.pm_done_.create(hipEventDisableTiming));
    HIPCHK(c.pm_.reserve(nbq * 2 * CH_PM));
    HIPCHK(hipMemset(c.pm_.get(), 0, nbq * 2 * CH_PM * sizeof(double)));      // blocks that do not exist stay zero
    c.v_ = view;
    c.trace_ = hooks.chain_trace;
    *this = std::move(c);
    return hipSuccess;
}

ChainDecision SolveChains::decide(int nrhs) const {      // (the hooks asked at every call: the tests lower chain8_min_nb)
    return chain_decide(v_.nfact / 128, nrhs, v_.cus, pm_.get() && xch_.get(), flow_hooks());
}

hipError_t SolveChains::preset(double *p, size_t count) { return hipMemsetAsync(p, 0xFF, count * sizeof(double), v_.stream); }

hipError_t SolveChains::wait_premultiplied() {
    if (pm_wait_) { HIPCHK(hipStreamWaitEvent(v_.stream, pm_done_.get(), 0)); pm_wait_ = false; }
    return hipSuccess;
}

hipError_t SolveChains::factor_changes() {
    pm_ready_ = false;
    return wait_premultiplied();
}

// The CH_PM blocks below every diagonal block multiplied into its inverse, once per factorisation, for backsolve_chain8_kernel:
// P_m[k] = L[k+m][k] W_k, m = 1 .. CH_PM.  pm = [P_1[0] .. P_1[nb-1]][P_2[0] ..] .., 128 x 128 row-major each (blocks that do not
// exist stay zero).  ONE launch: batches (k, m - 1), those with k + m >= nb left out.
hipError_t SolveChains::premultiply() {
    if (pm_ready_ || !pm_.get()) return hipSuccess;
    const int nb = v_.nfact / 128;
    const long ld = v_.ld;
    double *pm = pm_.get();
    if (nb > 1) {
        GemmArgs p{};
        p.A = v_.L + (long)128 * ld; p.lda = ld; p.strideA = 128 * (ld + 1); p.strideA2 = (long)128 * ld;     // L[k+m][k]   (KC)
        p.B = v_.invd; p.ldb = 128; p.strideB = 16384; p.strideB2 = 0;                                    // W_k (k, j) row-major (XC)
        p.C = pm; p.ldc = 128; p.strideC = 16384; p.strideC2 = (long)nb * 16384;
        p.M = p.N = p.K = 128; p.alpha = 1.0; p.beta = 0.0; p.kmode = KMODE_FULL;
        p.batch_sum_limit = nb - 1;                 // k + (m - 1) <= nb - 2
        HIPCHK(gemm_f64(v_.stream, LAY_KC, LAY_XC, p, nb - 1, 0, 0, std::min(CH_PM, nb - 1)));
        // Ft_m[k] = (W_k L[k][k-m])' = L[k][k-m]' W_k', k >= m: behind the P blocks, batches (k - m, m - 1)
        GemmArgs f{};
        f.A = v_.L + (long)128 * ld; f.lda = ld; f.strideA = 128 * (ld + 1); f.strideA2 = (long)128 * ld;     // L[k][k-m] read transposed (XC)
        f.B = v_.invd + 16384; f.ldb = 128; f.strideB = 16384; f.strideB2 = 16384;                        // W_k' (kk, j) = W_k[j][kk] (KC)
        f.C = pm + (size_t)CH_PM * nb * 16384 + 16384; f.ldc = 128; f.strideC = 16384; f.strideC2 = (long)nb * 16384 + 16384;
        f.M = f.N = f.K = 128; f.alpha = 1.0; f.beta = 0.0; f.kmode = KMODE_FULL;
        f.batch_sum_limit = nb - 1;
        // the Ft blocks are needed by the forward chain of the refinement only: on the side stream, beside the first backward chain
        // and the residual (solve() waits for pm_done_)
        if (v_.pstream && pm_e0_.get() && pm_done_.get()) {
            HIPCHK(hipEventRecord(pm_e0_.get(), v_.stream));
            HIPCHK(hipStreamWaitEvent(v_.pstream, pm_e0_.get(), 0));
            HIPCHK(gemm_f64(v_.pstream, LAY_XC, LAY_KC, f, nb - 1, 0, 0, std::min(CH_PM, nb - 1)));
            HIPCHK(hipEventRecord(pm_done_.get(), v_.pstream));
            pm_wait_ = true;
        } else {
            HIPCHK(gemm_f64(v_.stream, LAY_XC, LAY_KC, f, nb - 1, 0, 0, std::min(CH_PM, nb - 1)));
        }
    }
    pm_ready_ = true;
    return hipGetLastError();
}

// the backward chain for one right-hand side in its polling-wave form (X preset by the caller); two workgroups per block column pass
// their halves of v through xch_, which they poll like X
hipError_t SolveChains::launch_backward8(const ChainDecision &d, const double *Z, double *X, const int *abort_word, long long *trace) {
    const int nb = v_.nfact / 128;
    if (d.workgroups == 2) {
        HIPCHK(preset(xch_.get(), (size_t)v_.nfact));
        hipLaunchKernelGGL(backsolve_chain8_kernel<2>, dim3(2 * nb), dim3(CHAIN8_THREADS), 0, v_.stream, v_.L, v_.ld, v_.invd, pm_.get(), Z, X, xch_.get(), nb, abort_word, trace);
    } else {
        hipLaunchKernelGGL(backsolve_chain8_kernel<1>, dim3(nb), dim3(CHAIN8_THREADS), 0, v_.stream, v_.L, v_.ld, v_.invd, pm_.get(), Z, X, xch_.get(), nb, abort_word, trace);
    }
    return hipGetLastError();
}

// the backward chain that carries d.nr right-hand sides (X preset by the caller)
hipError_t SolveChains::launch_backward(const ChainDecision &d, const double *Z, long zs, double *X, long xs, int nrhs, const int *abort_word) {
    const int nb = v_.nfact / 128;
    if (d.nr == 1) hipLaunchKernelGGL(backsolve_chain_kernel<1>, dim3(nb), dim3(256), 0, v_.stream, v_.L, v_.ld, v_.invd, Z, zs, X, xs, nb, nrhs, abort_word);
    else if (d.nr == 2) hipLaunchKernelGGL(backsolve_chain_kernel<2>, dim3(nb), dim3(256), 0, v_.stream, v_.L, v_.ld, v_.invd, Z, zs, X, xs, nb, nrhs, abort_word);
    else if (d.nr == 4) hipLaunchKernelGGL(backsolve_chain_kernel<4>, dim3(nb), dim3(256), 0, v_.stream, v_.L, v_.ld, v_.invd, Z, zs, X, xs, nb, nrhs, abort_word);
    else hipLaunchKernelGGL(backsolve_chain_kernel<8>, dim3(nb), dim3(256), 0, v_.stream, v_.L, v_.ld, v_.invd, Z, zs, X, xs, nb, nrhs, abort_word);
    return hipGetLastError();
}

// the forward chain (Z preset by the caller); its split form reads the Ft blocks: behind wait_premultiplied()
hipError_t SolveChains::launch_forward(const ChainDecision &d, const double *b, double *Z) {
    const int nb = v_.nfact / 128;
    if (d.workgroups == 2) {
        HIPCHK(preset(xch_.get(), (size_t)v_.nfact));
        hipLaunchKernelGGL(forwardsolve_chain8_kernel, dim3(2 * nb), dim3(CHAIN8_THREADS), 0, v_.stream, v_.L, v_.ld, v_.invd, pm_.get() + (size_t)CH_PM * nb * 16384, b, Z, xch_.get(), nb);
    } else {
        hipLaunchKernelGGL(forwardsolve_chain_kernel, dim3(nb), dim3(256), 0, v_.stream, v_.L, v_.ld, v_.invd, b, Z, nb);
    }
    return hipGetLastError();
}

hipError_t SolveChains::backward(const double *Z, long zs, double *X, long xs, int nrhs, const int *abort_word) {
    const ChainDecision d = decide(nrhs);
    HIPCHK(preset(X, (size_t)nrhs * xs));
    if (!d.polling_wave) return launch_backward(d, Z, zs, X, xs, nrhs, abort_word);
    HIPCHK(premultiply());
    return launch_backward8(d, Z, X, abort_word, nullptr);
}

hipError_t SolveChains::solve(const double *b, double *tmp, double *X, const int *abort_word) {
    const int nb = v_.nfact / 128;
    const ChainDecision d = decide(1);
    HIPCHK(preset(tmp, (size_t)v_.nfact));
    HIPCHK(preset(X, (size_t)v_.nfact));
    if (!d.polling_wave) {
        HIPCHK(launch_forward(d, b, tmp));
        return launch_backward(d, tmp, (long)v_.nfact, X, (long)v_.nfact, 1, abort_word);
    }
    HIPCHK(premultiply());
    DevBuf<long long> trbuf;      // development: link times of the backward chain on stderr
    if (trace_) { HIPCHK(trbuf.reserve((size_t)9 * nb)); HIPCHK(hipMemsetAsync(trbuf.get(), 0, (size_t)9 * nb * sizeof(long long), v_.stream)); }
    HIPCHK(wait_premultiplied());
    HIPCHK(launch_forward(d, b, tmp));
    HIPCHK(launch_backward8(d, tmp, X, abort_word, trbuf.get()));   // behind an abandoned factorisation: leave at once (as backward())
    if (trace_) HIPCHK(dump_trace(trbuf.get()));
    return hipGetLastError();
}

// JAICOV_CHAIN_TRACE: what backsolve_chain8_kernel stamped, on stderr (synchronises the stream)
hipError_t SolveChains::dump_trace(const long long *trace) {
    const int nb = v_.nfact / 128;
    std::vector<long long> h((size_t)9 * nb);
    HIPCHK(hipMemcpyAsync(h.data(), trace, h.size() * sizeof(long long), hipMemcpyDeviceToHost, v_.stream));
    HIPCHK(hipStreamSynchronize(v_.stream));
    fprintf(stderr, "[jaicov chain trace] backward, nb %d, link times in 10 ns:", nb);
    for (int q = 1; q < nb; q++) fprintf(stderr, " %lld", h[q] - h[q - 1]);
    fprintf(stderr, "\n[jaicov chain trace] per position: start, stream done (wave 1), barrier 1, barrier 2, u ready, tails done, polling wave done, stream done (wave 7), relative to the predecessor's publication (10 ns)\n");
    for (int q = 1; q < nb; q += (q < 12 ? 1 : 9)) {
        fprintf(stderr, "   pos %3d:", q);
        for (int c = 0; c < 8; c++) fprintf(stderr, " %6lld", h[(size_t)nb + 8 * q + c] - h[q - 1]);
        fprintf(stderr, "   published %6lld\n", h[q] - h[q - 1]);
    }
    return hipSuccess;
}

}  // namespace jaicov

// tests: the form of the chains for nb block columns, nrhs right-hand sides and `cus` compute units under the hooks of the environment,
// the buffers present: {polling_wave, workgroups, nr}
extern "C" void jaicov_debug_chain_decision(int nb, int nrhs, int cus, int *out3) {
    const jaicov::ChainDecision d = jaicov::chain_decide(nb, nrhs, cus, true, jaicov::flow_hooks());
    out3[0] = d.polling_wave; out3[1] = d.workgroups; out3[2] = d.nr;
}
