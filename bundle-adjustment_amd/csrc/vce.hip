// Variance components of observation groups (include/jaicov_vce.h), formed from what the reliability run leaves on the device.
// gfx950 only, wave64.
//
//   vce_block_kernel   omega_b = v_b' P_b v_b and rho_b = sum r_i of every DENSE weight block (image blocks from blk_w, dense directly
//                      observed groups from dg_w): one workgroup per block, the lower triangle of P_b only
//   vce_small_kernel   the same pair of every other weight block, one lane per block: the 2 x 2 of an image point, the scalar of a
//                      scale bar, the diagonal of a directly observed group
//   vce_group_kernel   one wave per group: n_g, Omega_g, r_g over the group's blocks in ascending row order, the derived columns and
//                      the status; one more wave forms the totals over all blocks in the same way
//
// Slots.  Every weight block has a slot for (omega_b, rho_b): image point k of the caller's order has slot k, scale bar s has
// n_ip + s, directly observed group j has n_ip + n_sb + j.  A dense image block uses the slot of its first image point; the slots of
// its other points stay unused and appear in no list.  Ascending slots are ascending rows.
//
// Order of the sums.  vce_block_kernel: residuals are staged in LDS, `cap` at a time (all of them for blocks up to VB_CAP rows).
// Within a stage with the columns j0 .. j1 - 1, wave w takes the rows i = j0 + w, j0 + w + VB_WAVES, ... and lane l the entries
// j = j0 + l, j0 + l + 64, ... <= i of such a row: s = sum P_ij v_j (twice for j < i), then acc += v_i s.  A lane's acc runs over
// its rows of all stages; the 64 lanes are combined through the xor butterfly, the waves in the order 0, 1, 2, 3.  vce_group_kernel:
// lane l takes the group's blocks l, l + 64, ... of its list, then the butterfly.  No atomics: two runs give the same bits, and a
// group's sums depend on its own list alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/jaicov_vce.h"
#include "obsmodel.h"
#include "qview.h"
#include "reliability.h"
#include "status.h"
#include "vce.h"

namespace jaicov {

constexpr int VB_NT = 256;                 // threads per workgroup of vce_block_kernel
constexpr int VB_WAVES = VB_NT / 64;
constexpr int VB_CAP = 2048;               // residuals staged at a time (16 KB of LDS): config 4's 2m = 1000 in one stage
constexpr double VCE_UNCONTROLLED = 1e-10; // r_g <= this * n_g: the group is not controlled

// a dense weight block: kind 0 an image block (first = its first engine image point), 1 a directly observed group (first = its
// first direct row); w_off into blk_w / dg_w; m rows
struct VceBlock {
    int64_t w_off;
    int32_t kind, first, m, slot;
};

// row i of a dense block in the reliability result (the caller's row order)
__device__ __forceinline__ long vb_row(const VceBlock &b, const int32_t *__restrict__ new2old, long row_dg0, int i) {
    if (b.kind == 0) {
        const int ip = b.first + (i >> 1);
        return 2 * (long)(new2old ? new2old[ip] : ip) + (i & 1);
    }
    return row_dg0 + b.first + i;
}

// the same sum in every lane, in the butterfly's order
__device__ __forceinline__ double vce_wave_sum(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// A sum carried with its rounding error (Knuth's two-sum): a group of thousands of small blocks is added up as exactly as one block
// is, so that the error of Omega_g stays that of its blocks.  Sums only, no products: nothing here can be contracted.
struct VcePair {
    double hi, lo;
};
__device__ __forceinline__ void vce_pair_add(VcePair &a, double x) {
    const double s = a.hi + x, b = s - a.hi;
    a.lo += (a.hi - (s - b)) + (x - b);
    a.hi = s;
}
// the same value in every lane, in the butterfly's order
__device__ __forceinline__ double vce_pair_wave_sum(VcePair a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double h = __shfl_xor(a.hi, off, 64), l = __shfl_xor(a.lo, off, 64);
        // both partners must form the same bits: add the smaller index's pair to the larger's in one order
        const bool upper = (threadIdx.x & off) != 0;
        VcePair x{upper ? h : a.hi, upper ? l : a.lo};
        vce_pair_add(x, upper ? a.hi : h);
        x.lo += upper ? a.lo : l;
        a = x;
    }
    return a.hi + a.lo;
}

// rel: [4][n_rows] of the reliability run (v, qvv, r, t); row_dg0: first row of the directly observed groups
__global__ __launch_bounds__(VB_NT) void vce_block_kernel(const VceBlock *__restrict__ blocks, const double *__restrict__ blk_w,
                                                          const double *__restrict__ dg_w, const int32_t *__restrict__ new2old,
                                                          const double *__restrict__ rel, long n_rows, long row_dg0, double s0, int cap,
                                                          double *__restrict__ omega, double *__restrict__ rho) {
    __shared__ double sv[VB_CAP];
    __shared__ double sred[2 * VB_WAVES];
    const VceBlock b = blocks[blockIdx.x];
    const double *__restrict__ W = (b.kind == 0 ? blk_w : dg_w) + b.w_off;
    const double *__restrict__ v = rel, *__restrict__ r = rel + 2 * n_rows;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = b.m;
    double acc = 0.0, rs = 0.0;
    for (int i = tid; i < m; i += VB_NT) rs += r[vb_row(b, new2old, row_dg0, i)];
    for (int j0 = 0; j0 < m; j0 += cap) {
        const int j1 = min(m, j0 + cap);
        __syncthreads();                                   // the previous stage has been read
        for (int j = j0 + tid; j < j1; j += VB_NT) sv[j - j0] = v[vb_row(b, new2old, row_dg0, j)];
        __syncthreads();
        for (int i = j0 + wave; i < m; i += VB_WAVES) {
            const double vi = i < j1 ? sv[i - j0] : v[vb_row(b, new2old, row_dg0, i)];
            const double *__restrict__ Wi = W + (long)i * m;
            const int je = min(j1, i + 1);                 // the lower triangle: j <= i
            double s = 0.0;
#pragma unroll 4
            for (int j = j0 + lane; j < je; j += 64) {
                const double pv = Wi[j] * sv[j - j0];
                s += j < i ? 2.0 * pv : pv;
            }
            acc = fma(vi, s, acc);
        }
    }
    acc = vce_wave_sum(acc);
    rs = vce_wave_sum(rs);
    if (lane == 0) { sred[wave] = acc; sred[VB_WAVES + wave] = rs; }
    __syncthreads();
    if (tid == 0) {
        double a = sred[0], c = sred[VB_WAVES];
#pragma unroll
        for (int w = 1; w < VB_WAVES; w++) { a += sred[w]; c += sred[VB_WAVES + w]; }
        omega[b.slot] = s0 * a;
        rho[b.slot] = c;
    }
}

// thread t: engine image point t (t < n_ip, skipped where dense[t]), scale bar t - n_ip, directly observed group t - n_ip - n_sb
// (skipped where its weights are dense)
__global__ __launch_bounds__(256) void vce_small_kernel(DevProblem p, const uint8_t *__restrict__ dense, const int32_t *__restrict__ new2old,
                                                        const double *__restrict__ rel, long n_rows, double s0,
                                                        double *__restrict__ omega, double *__restrict__ rho) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const double *__restrict__ v = rel, *__restrict__ r = rel + 2 * n_rows;
    const long n_ip = p.n_ip;
    if (t < n_ip) {
        if (dense[t]) return;
        const long o = new2old ? new2old[t] : t;
        double p00, p01, p11;
        if (p.ip_w3) {
            const double *w = p.ip_w3 + 3 * t;
            p00 = s0 * w[0]; p01 = s0 * w[1]; p11 = s0 * w[2];
        } else {
            obs_weight(p, (int)t, s0, p00, p01, p11);
        }
        const double v0 = v[2 * o], v1 = v[2 * o + 1];
        omega[o] = fma(p00 * v0, v0, fma(2.0 * p01 * v0, v1, p11 * v1 * v1));
        rho[o] = r[2 * o] + r[2 * o + 1];
        return;
    }
    const long s = t - n_ip;
    if (s < p.n_sb) {
        const long row = 2 * n_ip + s;
        omega[n_ip + s] = s0 / p.sb_var[s] * v[row] * v[row];
        rho[n_ip + s] = r[row];
        return;
    }
    const long g = s - p.n_sb;
    if (g >= p.n_dg || p.dg_w_offset[g] >= 0) return;
    const int b = p.dg_row_begin[g], e = p.dg_row_begin[g + 1];
    const long row0 = 2 * n_ip + p.n_sb;
    double a = 0.0, c = 0.0;
    for (int i = b; i < e; i++) {
        const double vi = v[row0 + i];
        a = fma(s0 / p.dg_var[i] * vi, vi, a);
        c += r[row0 + i];
    }
    omega[n_ip + p.n_sb + g] = a;
    rho[n_ip + p.n_sb + g] = c;
}

// Wave g < n_groups: group g; wave n_groups: all blocks.  begin: CSR over list (slots, ascending within a group); rows[slot]: rows of
// the block.  table: [JAICOV_VCE_COLUMNS][n_groups + 1]
__global__ __launch_bounds__(64) void vce_group_kernel(const int32_t *__restrict__ begin, const int32_t *__restrict__ list,
                                                       const int32_t *__restrict__ rows, const double *__restrict__ omega,
                                                       const double *__restrict__ rho, double s0, int n_groups, double *__restrict__ table,
                                                       int32_t *__restrict__ status) {
    const int g = blockIdx.x, lane = threadIdx.x;
    double n = 0.0;
    VcePair o2{0.0, 0.0}, r2{0.0, 0.0};
    for (int k = begin[g] + lane; k < begin[g + 1]; k += 64) {
        const int s = list[k];
        n += (double)rows[s];
        vce_pair_add(o2, omega[s]);
        vce_pair_add(r2, rho[s]);
    }
    n = vce_wave_sum(n);
    const double om = vce_pair_wave_sum(o2), rs = vce_pair_wave_sum(r2);
    if (lane != 0) return;
    int st = 0;
    if (n == 0.0) st = JAICOV_VCE_EMPTY;
    else if (!isfinite(om) || !isfinite(rs)) st = JAICOV_VCE_NOT_FINITE;
    else if (rs <= VCE_UNCONTROLLED * n) st = JAICOV_VCE_UNCONTROLLED;
    const double nan = (double)NAN;
    const double s2 = st ? nan : om / rs;
    const double k = st ? nan : s2 / s0;
    const double sd = st ? nan : k * sqrt(2.0 / rs);
    const long ld = n_groups + 1;
    table[g] = n;
    table[ld + g] = om;
    table[2 * ld + g] = rs;
    table[3 * ld + g] = s2;
    table[4 * ld + g] = k;
    table[5 * ld + g] = sd;
    status[g] = st;
}

}  // namespace jaicov

using namespace jaicov;

static int group_ids_ok(const int32_t *ids, long n, int n_groups) {
    if (!ids) return 1;
    for (long i = 0; i < n; i++)
        if (ids[i] < -1 || ids[i] >= n_groups) return 0;
    return 1;
}

// the sums once the reliability result is in its slot
static int vce_run_impl(const QView &v, VceState *st, const int32_t *ip_group, const int32_t *sb_group, const int32_t *dg_group, int n_groups,
                        const std::vector<int32_t> &new2old, const std::vector<uint8_t> &dense, const std::vector<VceBlock> &img_blocks) {
    const DevProblem &p = *v.p;
    const long n_ip = p.n_ip, n_sb = p.n_sb, n_dg = p.n_dg, n_rows = 2 * n_ip + n_sb + p.n_dg_rows;
    const long n_slots = n_ip + n_sb + n_dg;
    const hipStream_t s = v.stream;
    const double *d_rel = v.slot->rel->out.get();
    DevBag w;
    // the directly observed groups: their rows and which of them are dense
    std::vector<int32_t> dg_begin(n_dg + 1, 0);
    std::vector<int64_t> dg_off(n_dg, -1);
    if (n_dg > 0)
        TRY(q_download(v, {{dg_begin.data(), p.dg_row_begin, (size_t)(n_dg + 1) * sizeof(int32_t)},
                           {dg_off.data(), p.dg_w_offset, (size_t)n_dg * sizeof(int64_t)}}));
    std::vector<VceBlock> blocks(img_blocks);
    std::vector<int32_t> rows(n_slots, 0);
    for (const VceBlock &b : blocks) rows[b.slot] = b.m;
    for (long q = 0; q < n_ip; q++)
        if (!dense[q]) rows[new2old.empty() ? q : new2old[q]] = 2;
    for (long k = 0; k < n_sb; k++) rows[n_ip + k] = 1;
    for (long g = 0; g < n_dg; g++) {
        const int m = dg_begin[g + 1] - dg_begin[g];
        rows[n_ip + n_sb + g] = m;
        if (dg_off[g] >= 0 && m > 0) blocks.push_back(VceBlock{dg_off[g], 1, dg_begin[g], m, (int32_t)(n_ip + n_sb + g)});
    }
    // group of every slot, then the CSR of the groups (ascending slots) with the list of all blocks behind them
    auto group_of = [&](long slot) {
        if (slot < n_ip) return ip_group ? ip_group[slot] : -1;
        if (slot < n_ip + n_sb) return sb_group ? sb_group[slot - n_ip] : -1;
        return dg_group ? dg_group[slot - n_ip - n_sb] : -1;
    };
    std::vector<int32_t> begin(n_groups + 2, 0);
    long grouped = 0, all = 0;
    for (long k = 0; k < n_slots; k++) {
        if (rows[k] == 0) continue;
        const int g = group_of(k);
        if (g >= 0) { begin[g + 1]++; grouped += rows[k]; }
        begin[n_groups + 1]++;
        all += rows[k];
    }
    for (int g = 0; g <= n_groups; g++) begin[g + 1] += begin[g];
    std::vector<int32_t> list(std::max<size_t>(begin[n_groups + 1], 1)), fill(begin.begin(), begin.end() - 1);
    for (long k = 0; k < n_slots; k++) {
        if (rows[k] == 0) continue;
        const int g = group_of(k);
        if (g >= 0) list[fill[g]++] = (int32_t)k;
        list[fill[n_groups]++] = (int32_t)k;
    }
    const size_t n_tab = (size_t)n_groups + 1;
    HIPE(*v.err, st->table.reserve(JAICOV_VCE_COLUMNS * n_tab));
    HIPE(*v.err, st->status.reserve(n_tab));
    double *d_omega = nullptr, *d_rho = nullptr;
    int32_t *d_rows = nullptr, *d_begin = nullptr, *d_list = nullptr, *d_new2old = nullptr;
    uint8_t *d_dense = nullptr;
    VceBlock *d_blocks = nullptr;
    HIPE(*v.err, w.alloc(&d_omega, (size_t)n_slots));
    HIPE(*v.err, w.alloc(&d_rho, (size_t)n_slots));
    HIPE(*v.err, w.alloc(&d_rows, (size_t)n_slots));
    HIPE(*v.err, w.alloc(&d_begin, begin.size()));
    HIPE(*v.err, w.alloc(&d_list, list.size()));
    HIPE(*v.err, w.alloc(&d_dense, (size_t)n_ip));
    HIPE(*v.err, w.alloc(&d_blocks, blocks.size()));
    auto up = [&](void *dst, const void *src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    };
    HIPE(*v.err, up(d_rows, rows.data(), (size_t)n_slots * sizeof(int32_t)));
    HIPE(*v.err, up(d_begin, begin.data(), begin.size() * sizeof(int32_t)));
    HIPE(*v.err, up(d_list, list.data(), list.size() * sizeof(int32_t)));
    HIPE(*v.err, up(d_dense, dense.data(), (size_t)n_ip));
    HIPE(*v.err, up(d_blocks, blocks.data(), blocks.size() * sizeof(VceBlock)));
    if (!new2old.empty()) {
        HIPE(*v.err, w.alloc(&d_new2old, new2old.size()));
        HIPE(*v.err, up(d_new2old, new2old.data(), new2old.size() * sizeof(int32_t)));
    }
    int cap = VB_CAP;
    if (const char *hook = getenv("JAICOV_VCE_STAGE")) cap = std::min(VB_CAP, std::max(1, atoi(hook)));   // test hook
    QTimer<4> timer(s);
    HIPE(*v.err, timer.arm(st->timing));
    HIPE(*v.err, timer.mark(0));
    if (!blocks.empty()) {
        hipLaunchKernelGGL(vce_block_kernel, dim3((unsigned)blocks.size()), dim3(VB_NT), 0, s, d_blocks, p.blk_w, p.dg_w, d_new2old, d_rel, n_rows,
                           2 * n_ip + n_sb, v.sigma2, cap, d_omega, d_rho);
        HIPE(*v.err, hipGetLastError());
    }
    HIPE(*v.err, timer.mark(1));
    if (n_slots > 0) {
        hipLaunchKernelGGL(vce_small_kernel, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, s, p, d_dense, d_new2old, d_rel, n_rows, v.sigma2,
                           d_omega, d_rho);
        HIPE(*v.err, hipGetLastError());
    }
    HIPE(*v.err, timer.mark(2));
    hipLaunchKernelGGL(vce_group_kernel, dim3((unsigned)n_tab), dim3(64), 0, s, d_begin, d_list, d_rows, d_omega, d_rho, v.sigma2, n_groups,
                       st->table.get(), st->status.get());
    HIPE(*v.err, hipGetLastError());
    HIPE(*v.err, timer.mark(3));
    double tot[2] = {0.0, 0.0};
    TRY(q_download(v, {{&tot[0], st->table.get() + n_tab + n_groups, sizeof(double)},
                       {&tot[1], st->table.get() + 2 * n_tab + n_groups, sizeof(double)}}));   // the host vectors above end their use here
    HIPE(*v.err, timer.read(st->ms));
    st->summary[0] = tot[0];
    st->summary[1] = tot[1];
    st->summary[2] = (double)grouped;
    st->summary[3] = (double)(all - grouped);
    st->summary[4] = v.lambda;
    st->n_groups = n_groups;
    return JAICOV_OK;
}

extern "C" int jaicov_vce_run(jaicov_engine *e, double sigma2_test, const double *dx, const int32_t *ip_group, const int32_t *sb_group,
                              const int32_t *dg_group, int32_t n_groups, int32_t *n_rows) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    TRY(q_guard(v, "variance components need an engine that holds every observation (not a shard)",
                "no full cofactor matrix: solve with JAICOV_INVERT_FULL or JAICOV_INVERT_FULL_EXPANDED first"));
    const DevProblem &p = *v.p;
    if (!(sigma2_test > 0) || !std::isfinite(sigma2_test)) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "sigma2_test must be positive and finite");
    if (n_groups <= 0) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "n_groups must be positive");
    if (!group_ids_ok(ip_group, p.n_ip, n_groups) || !group_ids_ok(sb_group, p.n_sb, n_groups) || !group_ids_ok(dg_group, p.n_dg, n_groups))
        FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "a group id must be -1 or 0 .. n_groups - 1");
    const long n_ip = p.n_ip, rows = 2 * n_ip + p.n_sb + p.n_dg_rows;
    if (rows > INT32_MAX) FAIL(*v.err, JAICOV_ERR_UNSUPPORTED, "more than 2^31 - 1 observation rows");
    // the dense image blocks, each in one group
    const QImageBlocks ib = q_image_blocks(v);
    std::vector<VceBlock> blocks;
    const std::vector<int32_t> &bb = *v.blk_ip_begin;
    for (const int32_t g : ib.blocks) {
        int32_t first = INT32_MAX;
        for (int q = bb[g]; q < bb[g + 1]; q++) first = std::min(first, ib.caller(q));
        if (ip_group)
            for (int q = bb[g]; q < bb[g + 1]; q++)
                if (ip_group[ib.caller(q)] != ip_group[first]) {
                    const long cb = v.caller_block->empty() ? (long)g : (long)(*v.caller_block)[g];
                    FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT,
                         "the image points of dense image block " + std::to_string(cb) + " name more than one group: a group is a union of weight blocks");
                }
        blocks.push_back(VceBlock{(*v.blk_w_off)[g], 0, bb[g], 2 * (bb[g + 1] - bb[g]), first});
    }
    // accepted: the reliability run, then the sums
    VceState *st = q_state(v.slot->vce);
    st->have = false;
    TRY(rel_run_plain(e, v, sigma2_test, dx, rows));
    const int rc = vce_run_impl(v, st, ip_group, sb_group, dg_group, n_groups, ib.new2old, ib.dense, blocks);
    if (rc != JAICOV_OK) {
        hipStreamSynchronize(v.stream);
        return rc;
    }
    st->have = true;
    if (n_rows) *n_rows = (int32_t)rows;
    return JAICOV_OK;
}

static const char VCE_NONE[] = "no variance components: call jaicov_vce_run first";

static VceState *vce_result(const QView &v) {
    VceState *st = v.slot->vce.get();
    if (!st || !st->have) {
        *v.err = VCE_NONE;
        return nullptr;
    }
    return st;
}

extern "C" int jaicov_vce_get(jaicov_engine *e, double *table, int32_t *status, int32_t n_groups) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    VceState *st = vce_result(v);
    if (!st) return JAICOV_ERR_BAD_STATE;
    if (n_groups != st->n_groups) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "n_groups must equal that of the last run");
    // the device's table has one more column, the totals: row by row
    const size_t ld = (size_t)n_groups + 1, bytes = (size_t)n_groups * sizeof(double);
    const double *src = st->table.get();
    if (table)
        TRY(q_download(v, {{table, src, bytes}, {table + n_groups, src + ld, bytes}, {table + 2 * (size_t)n_groups, src + 2 * ld, bytes},
                           {table + 3 * (size_t)n_groups, src + 3 * ld, bytes}, {table + 4 * (size_t)n_groups, src + 4 * ld, bytes},
                           {table + 5 * (size_t)n_groups, src + 5 * ld, bytes}}));
    return q_download(v, {{status, st->status.get(), (size_t)n_groups * sizeof(int32_t)}});
}

extern "C" int jaicov_vce_summary(jaicov_engine *e, double *out, int32_t n) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    VceState *st = vce_result(v);
    if (!st) return JAICOV_ERR_BAD_STATE;
    if (n != 5 || !out) FAIL(*v.err, JAICOV_ERR_BAD_ARGUMENT, "the summary has 5 entries");
    memcpy(out, st->summary, 5 * sizeof(double));
    return JAICOV_OK;
}

extern "C" int jaicov_vce_release(jaicov_engine *e) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    q_release(v, v.slot->vce);
    return JAICOV_OK;
}

// The hook of scripts/vce_bench.py: on != 0 makes the following runs time their kernels by events on the engine's stream;
// ms[0 .. 2]: what vce_block_kernel, vce_small_kernel and vce_group_kernel of the last run took.
extern "C" int jaicov_debug_vce_timing(jaicov_engine *e, int on, float *ms) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    const QView v = q_view(e);
    VceState *st = on ? q_state(v.slot->vce) : v.slot->vce.get();       // asking an engine that never ran the call allocates nothing
    if (st) st->timing = on != 0;
    if (ms)
        for (int k = 0; k < 3; k++) ms[k] = st ? st->ms[k] : 0.f;
    return JAICOV_OK;
}
