// jaicov_neq_create, second stage: what happens on the device, from the finished plan (create_plan.h) to an engine that can
// accumulate; with it the dense dispersions' way to weights (batchinv.hip).  gfx950 only.
#include <string.h>

#include <algorithm>

#include "batchinv.h"
#include "create_plan.h"
#include "engine_state.h"
#include "obsmodel.h"

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
    double w00, w01, w11;
    jaicov::obs_weight(vx[q], vy[q], rho[q], 1.0, w00, w01, w11);
    out[3 * (long)q] = w00; out[3 * (long)q + 1] = w01; out[3 * (long)q + 2] = w11;
}

// inv(D) of an ordinary image served as a block: 2 x 2 blocks [[vx, rho s], [rho s, vy]]^-1, s = sqrt(vx vy), on the diagonal
// (PDF:313-319 divided by sigma0^2; rho == 0: 1 / vx, 1 / vy as PDF:308-312), zeros elsewhere.  One workgroup per row.
__global__ void fill_diag_weight_kernel(const double *__restrict__ vx, const double *__restrict__ vy, const double *__restrict__ rho, int ipb, int m,
                                        double *__restrict__ out) {
    const int i = blockIdx.x, q = i >> 1, r = i & 1;
    double w00, w01, w11;
    jaicov::obs_weight(vx[ipb + q], vy[ipb + q], rho[ipb + q], 1.0, w00, w01, w11);
    const double w0 = r == 0 ? w00 : w01, w1 = r == 0 ? w01 : w11;   // entries (i, 2q), (i, 2q + 1)
    double *o = out + (long)i * m;
    for (int j = threadIdx.x; j < m; j += blockDim.x) o[j] = j == 2 * q ? w0 : (j == 2 * q + 1 ? w1 : 0.0);
}

// DOPG:82-86 for every jointly dispersed group of the problem: items of one padded order are inverted in chunks (one set of
// batched launches per chunk); the upload of chunk c + 1 runs on a copy stream beside the inversion of chunk c.
// Timings (ms) are left in e->create_ms: host time spent in the uploads, and everything (wall).
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
    e->create_ms[CREATE_DISP_UPLOAD] = up_ms;
    e->create_ms[CREATE_WEIGHTS] =std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_all).count();
    if (status != JAICOV_OK) FAIL(e->err, status, msg);
    return JAICOV_OK;
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

int jaicov::engine_create_impl(jaicov_engine *e, const jaicov_problem_desc *desc) {
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
    e->create_ms[CREATE_STRUCTURE] = ms_since(t);
    TRY(create_weights(e, pl));
    t = std::chrono::steady_clock::now();
    TRY(alloc_work_buffers(e, pl));
    e->create_ms[CREATE_WORK] = ms_since(t);
    t = std::chrono::steady_clock::now();
    if (pl.dense_mode) {
        HIPE(e->err, e->dm.init(pl.max_m, pl.max_k1, e->n_blk_list, e->opts.assembly_mode == 2));
        e->dense_mode = true;
    } else if (pl.schur_ok)
        TRY(init_elimination(e, pl));
    e->create_ms[CREATE_ELIMINATION] = ms_since(t);
    keep_host_tables(e, pl);
    HIPE(e->err, hipStreamSynchronize(e->stream));
    return JAICOV_OK;
}
