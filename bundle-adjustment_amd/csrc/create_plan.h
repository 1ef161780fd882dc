// Engine creation, first stage: everything jaicov_neq_create decides and tabulates on the host, before anything exists on
// the device.  The plan is a pure function of (description, options, assembly form): no device call, no launch, no
// knowledge of the engine.  engine_create.hip uploads what the plan holds (engine_create_impl); jaicov_debug_create_plan exposes the
// decisions and tests/test_create_plan.py holds the tables to their invariants on any machine.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/jaicov_neq.h"
#include "ba_kernels.h"

namespace jaicov {

constexpr int NOCOL = 1 << 30;   // lowest column of an image point whose object point has no free coordinate

struct CreatePlan {
    int status = JAICOV_OK;      // JAICOV_OK, or why the description was refused ...
    std::string err;             // ... and the text of jaicov_neq_last_error
    // The effective description: the caller's, with every image a block when ordinary images are served as blocks, and
    // with the observations of dense blocks in column order.  Its pointers refer to the caller's arrays or to vectors
    // of this plan (blk_ip_begin, syn_off, pv_*), never to anything else.
    jaicov_problem_desc D{};
    int U = 0, Upad = 0, d = 0, n_slots = 0;
    std::vector<int32_t> slot_col;       // column of every slot [3P | 3C | n_dist | 6I]
    std::vector<uint8_t> point_datum;
    int ib = 0, ie = 0, ip0 = 0, ip_count = 0;   // images [ib, ie) of this engine and their image points
    // ordinary images as image blocks
    bool synthesized = false;
    std::vector<int32_t> blk_ip_begin;   // D.blk_ip_begin (the caller's, copied, or one block per image)
    std::vector<int64_t> syn_off;        // D.blk_disp_offset when synthesized (-1: no dispersion of its own)
    std::vector<int32_t> caller_block;   // internal image block -> the caller's block index (-1: an ordinary image); empty: identity
    // blocks and segments
    std::vector<uint8_t> in_block, blk_mine;
    std::vector<int32_t> blk_list, blk_ip_list, seg_b, seg_e;
    std::vector<int> blk_images;         // image of every block of blk_list
    std::vector<int64_t> blk_w_off;      // offset of every block's weight in DevProblem::blk_w (-1: compact 2 x 2 weights)
    int64_t w_total = 0;
    bool compact_blocks = false;
    int max_m = 0;
    // column-sorted storage of dense blocks
    std::vector<int32_t> lo_col, hi_col;              // lowest / highest free column of an image point of blk_ip_list, engine order
    std::vector<int32_t> pv_image, pv_point, perm_local, ip_old2new;   // empty: nothing moved
    std::vector<double> pv_x, pv_y, pv_vx, pv_vy, pv_rho;
    // tables of the point x point gather (PPGather); gather == false: none
    bool gather = false, plain_ok = false;
    std::vector<int32_t> pt_ip_begin, ipcol, range;
    std::vector<PPRecord> recs;
    int cw = PP_CW, n_chunks = 0, cmin = 0, cmax = -1;
    // EO pre-elimination and dense mode
    bool schur_ok = false, dense_mode = false;
    int e0 = 0, max_k1 = 0;
    double dm_flops_per_pass = 0.0;
};

inline bool plan_fail(CreatePlan &pl, int status, const char *msg) {
    pl.status = status;
    pl.err = msg;
    return false;
}

inline bool validate_distortion_sets(CreatePlan &pl) {
    const jaicov_problem_desc *D = &pl.D;
    for (int c = 0; c < D->n_cameras; c++) {
        const int jb = D->cam_dist_begin[c], je = D->cam_dist_begin[c + 1];
        if (je - jb > JAICOV_MAX_DIST_PER_CAMERA) return plan_fail(pl, JAICOV_ERR_UNSUPPORTED, "too many distortion coefficients for one camera");
        for (int j = jb + 1; j < je; j++)
            if (D->dist_kind[j] < D->dist_kind[j - 1]) return plan_fail(pl, JAICOV_ERR_BAD_ARGUMENT, "distortion coefficients must be in DistortionModel.Type order");
        // AffinityShearDistortionModel always owns Cx and Cy, TangentialDistortionModel Bx and By (+ optional Bi): a lone
        // member would silently drop out of the model (ASF:37-81, TDF:39-134 read both)
        int cnt[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int j = jb; j < je; j++) {
            if (D->dist_kind[j] < 0 || D->dist_kind[j] > JAICOV_DIST_ZERNIKE_Z) return plan_fail(pl, JAICOV_ERR_BAD_ARGUMENT, "unknown distortion coefficient kind");
            if (D->dist_kind[j] >= JAICOV_DIST_ZERNIKE_X && (D->dist_order[j] < 1 || D->dist_order[j] > 119))
                return plan_fail(pl, JAICOV_ERR_BAD_ARGUMENT, "Zernike coefficient order must be 1..119 (ZernikeDistortionModel.java:67-68)");
            cnt[D->dist_kind[j]]++;
        }
        if (cnt[0] != cnt[1] || cnt[0] > 1 || cnt[2] != cnt[3] || cnt[2] > 1 || (cnt[4] > 0 && cnt[2] == 0))
            return plan_fail(pl, JAICOV_ERR_BAD_ARGUMENT, "affinity (Cx, Cy) and tangential (Bx, By [, Bi]) coefficients come as complete models");
    }
    return true;
}

// slot -> column of every parameter; the columns in use must be a permutation of d..U-1
inline bool validate_columns(CreatePlan &pl) {
    const jaicov_problem_desc *D = &pl.D;
    pl.slot_col.resize(pl.n_slots);
    int s = 0;
    for (int i = 0; i < 3 * D->n_points; i++) pl.slot_col[s++] = D->point_col[i];
    for (int i = 0; i < 3 * D->n_cameras; i++) pl.slot_col[s++] = D->io_col[i];
    for (int i = 0; i < D->n_dist; i++) pl.slot_col[s++] = D->dist_col[i];
    for (int i = 0; i < 6 * D->n_images; i++) pl.slot_col[s++] = D->eo_col[i];
    std::vector<char> seen(pl.U > 0 ? pl.U : 1, 0);
    for (int c : pl.slot_col) {
        if (c == JAICOV_COL_FIXED) continue;
        if (c < pl.d || c >= pl.U || seen[c]) return plan_fail(pl, JAICOV_ERR_BAD_ARGUMENT, "columns must be a permutation of d..U-1");
        seen[c] = 1;
    }
    pl.point_datum.assign(D->point_datum, D->point_datum + D->n_points);
    return true;
}

// Everything that refuses a description, before anything is derived from it.  Also leaves the sizes, the slot columns
// and the image range of this engine in the plan.
inline bool validate(CreatePlan &pl, const jaicov_engine_options &o) {
    const jaicov_problem_desc *D = &pl.D;
    const int U = D->n_unknowns, d = D->rank_defect;
    pl.U = U; pl.d = d;
    pl.Upad = ((U + 127) / 128) * 128;
    if (pl.Upad == 0) pl.Upad = 128;
    pl.n_slots = 3 * D->n_points + 3 * D->n_cameras + D->n_dist + 6 * D->n_images;
    if (__builtin_popcount((unsigned)D->datum_flags) != d || d < 0 || d > 7) return plan_fail(pl, JAICOV_ERR_BAD_ARGUMENT, "datum_flags / rank_defect mismatch");
    if (!validate_distortion_sets(pl)) return false;
    for (int i = 1; i < D->n_image_points; i++)
        if (D->ip_image[i] < D->ip_image[i - 1]) return plan_fail(pl, JAICOV_ERR_BAD_ARGUMENT, "image points must be image-major");
    for (int ip = 0; ip < D->n_image_points; ip++)
        if (D->ip_image[ip] < 0 || D->ip_image[ip] >= D->n_images) return plan_fail(pl, JAICOV_ERR_BAD_ARGUMENT, "image index out of range");
    if (!validate_columns(pl)) return false;
    // ---- image range of this engine
    pl.ib = 0; pl.ie = D->n_images;
    if (o.image_begin >= 0 && o.image_end >= 0) { pl.ib = o.image_begin; pl.ie = o.image_end; }
    if (pl.ib < 0 || pl.ie > D->n_images || pl.ib > pl.ie) return plan_fail(pl, JAICOV_ERR_BAD_ARGUMENT, "bad image range");
    const int32_t *b = std::lower_bound(D->ip_image, D->ip_image + D->n_image_points, pl.ib);
    const int32_t *en = std::lower_bound(D->ip_image, D->ip_image + D->n_image_points, pl.ie);
    pl.ip0 = (int)(b - D->ip_image);
    pl.ip_count = (int)(en - b);
    // ---- the caller's image blocks
    for (int g = 0; g < D->n_image_blocks; g++) {
        const int bb = D->blk_ip_begin[g], be = D->blk_ip_begin[g + 1];
        if (be < bb || bb < 0 || be > D->n_image_points) return plan_fail(pl, JAICOV_ERR_BAD_ARGUMENT, "image blocks must be ascending ranges");
        for (int ip = bb; ip < be; ip++)
            if (D->ip_image[ip] != D->ip_image[bb]) return plan_fail(pl, JAICOV_ERR_BAD_ARGUMENT, "an image block must not span images");
    }
    if (o.assembly_mode < 0 || o.assembly_mode > 2)
        return plan_fail(pl, JAICOV_ERR_BAD_ARGUMENT, "assembly_mode must be 0 (structure-aware), 1 (densified fp64 MFMA contraction) or 2 (the same with fp32 operands and accumulation)");
    return true;
}

// The EO columns are the trailing columns e0 + 6*image + k, and no directly observed parameter is an EO parameter:
// returns e0, or -1.  Ordinary images become blocks, and the EO pre-elimination is on, only where this holds.
inline int eo_columns_trailing(const jaicov_problem_desc &D) {
    const int e0 = D.n_images > 0 ? D.eo_col[0] : -1;
    bool ok = e0 >= D.rank_defect && e0 + 6 * D.n_images == D.n_unknowns;
    for (int i = 0; ok && i < 6 * D.n_images; i++) ok = D.eo_col[i] == e0 + i;
    const int s_eo = 3 * D.n_points + 3 * D.n_cameras + D.n_dist;
    for (int r = 0; ok && r < D.n_direct_rows; r++) ok = D.dg_slot[r] < s_eo;
    return ok ? e0 : -1;
}

// ---- ordinary image groups as jointly dispersed groups with a block-diagonal weight ----------------------------------
// reduceNormalEquationSystem (BA:1197-1342) eliminates the exterior orientation of EVERY image, whatever its stochastic
// model; the device path of that elimination (schur.hip) is written for image groups with a joint weight matrix.  An image
// whose points are ordinary ImageCoordinate groups (diagonal / 2 x 2 weights, PDF:296-319) is the special case of a
// block-diagonal joint weight: when the whole problem qualifies, every such image becomes an internal image block whose
// inv(D) is filled from (var_x, var_y, rho) in closed form -- no dispersion is uploaded or inverted -- and the
// elimination, the point x point gather and the reduced solve serve it like any other block.  All or nothing, decided on
// the WHOLE problem (every rank of a sharded run must assemble a system of the same order).
inline void synthesize_blocks(CreatePlan &pl, const jaicov_engine_options &o, int form) {
    const jaicov_problem_desc *D = &pl.D;
    pl.blk_ip_begin.assign(D->blk_ip_begin, D->blk_ip_begin + D->n_image_blocks + 1);
    pl.D.blk_ip_begin = pl.blk_ip_begin.data();
    bool ok = o.ordinary_group_elimination >= 0 && o.assembly_mode == 0 && D->n_images > 0 && eo_columns_trailing(*D) >= 0;
    if (!ok) return;
    std::vector<int32_t> img_b(D->n_images + 1, 0), img_blk(std::max(1, D->n_images), -1);
    for (int ip = 0; ip < D->n_image_points; ip++) img_b[D->ip_image[ip] + 1]++;
    for (int i = 0; i < D->n_images; i++) img_b[i + 1] += img_b[i];
    for (int g = 0; ok && g < D->n_image_blocks; g++) {       // a caller's block must be ALL observations of its image
        const int b = D->blk_ip_begin[g], en = D->blk_ip_begin[g + 1];
        if (en <= b || b < 0 || en > D->n_image_points) { ok = false; break; }
        const int img = D->ip_image[b];
        ok = img_b[img] == b && img_b[img + 1] == en && img_blk[img] < 0;
        if (ok) img_blk[img] = g;
    }
    int64_t syn_bytes = 0;
    bool any = false;
    for (int i = 0; ok && i < D->n_images; i++) {
        const int64_t cnt = img_b[i + 1] - img_b[i];
        if (img_blk[i] >= 0) continue;
        any = true;
        ok = cnt >= 3 && 2 * cnt <= 4096;
        syn_bytes += 4 * cnt * cnt * (int64_t)sizeof(double);
    }
    // (the dense form of the block-diagonal weights -- the alternative assembly forms only -- needs m^2 doubles per image)
    ok = ok && any && (form == ASSEMBLY_DEFAULT || form == ASSEMBLY_NO_FORK || syn_bytes <= ((int64_t)16 << 30));
    // Size rule (round 5; option 0 = default): serving ordinary images as blocks costs six block-kernel launches where the ordinary assembly
    // is one (+0.10 ms per pass at BASELINE config 2), and pays through the factorisation's block columns: eliminate when the 6 I exterior-
    // orientation columns are at least two 128-blocks of it (config 2: order 726 -> 606, six block columns -> five: not worth it, 0.79 vs
    // 0.86 ms per pass; config 3: 29 -> 24, the bundled example 10 -> 4: yes).  A property of the WHOLE problem, so every rank of a
    // sharded run decides alike.  > 0 forces the elimination at any size (tests), < 0 switches it off.
    // (A problem that ALSO has jointly dispersed images runs the block kernels anyway, and only with every image served as a block
    // can any exterior orientation be eliminated: no size rule there.)
    if (ok && o.ordinary_group_elimination == 0 && D->n_image_blocks == 0)
        ok = (pl.U + 127) / 128 - (pl.U - 6 * D->n_images + 127) / 128 >= 2;
    if (!ok) return;
    for (int i = 0; i < D->n_images; i++) {
        pl.syn_off.push_back(img_blk[i] >= 0 ? D->blk_disp_offset[img_blk[i]] : (int64_t)-1);
        pl.caller_block.push_back(img_blk[i]);
    }
    pl.blk_ip_begin = img_b;
    pl.D.n_image_blocks = D->n_images;
    pl.D.blk_ip_begin = pl.blk_ip_begin.data();
    pl.D.blk_disp_offset = pl.syn_off.data();
    pl.synthesized = true;
}

// which blocks are this engine's, where their weights go, and the segments of the image points outside blocks
inline void blocks_and_segments(CreatePlan &pl, int form) {
    const jaicov_problem_desc *D = &pl.D;
    pl.in_block.assign(D->n_image_points + 1, 0);
    pl.blk_w_off.assign(D->n_image_blocks + 1, 0);
    pl.blk_mine.assign(D->n_image_blocks, 0);
    for (int g = 0; g < D->n_image_blocks; g++) {
        const int b = D->blk_ip_begin[g], en = D->blk_ip_begin[g + 1];
        for (int ip = b; ip < en; ip++) pl.in_block[ip] = 1;
        // an ordinary image served as a block (no dispersion of its own): block-diagonal weights in compact form (DevProblem::ip_w3),
        // dense only under the alternative assembly forms, whose kernels read m x m weights
        const bool compact = pl.synthesized && D->blk_disp_offset[g] < 0 && (form == ASSEMBLY_DEFAULT || form == ASSEMBLY_NO_FORK);
        pl.blk_w_off[g] = compact ? -1 : pl.w_total;
        const bool mine = en > b && D->ip_image[b] >= pl.ib && D->ip_image[b] < pl.ie;
        if (mine) {
            const int64_t m = 2 * (int64_t)(en - b);
            if (!compact) pl.w_total += m * m;
            else pl.compact_blocks = true;
            pl.blk_mine[g] = 1;
            pl.blk_list.push_back(g);
            pl.blk_images.push_back(D->ip_image[b]);
            for (int ip = b; ip < en; ip++) pl.blk_ip_list.push_back(ip);
            pl.max_m = std::max(pl.max_m, (int)m);
        }
    }
    for (int ip = pl.ip0; ip < pl.ip0 + pl.ip_count;) {
        if (pl.in_block[ip]) { ip++; continue; }
        int en = ip;
        while (en < pl.ip0 + pl.ip_count && !pl.in_block[en] && D->ip_image[en] == D->ip_image[ip] && en - ip < SEG) en++;
        pl.seg_b.push_back(ip); pl.seg_e.push_back(en);
        ip = en;
    }
}

// ---- column-sorted storage inside dense image blocks -------------------------------------------------------
// The point x point gather (assemble.hip) streams, for one object point and one range of columns, the weights of
// the partner points of an image; with the image's observations stored in the order of their points' columns
// those partners are contiguous.  The engine therefore keeps the observations of every dense block (and the
// block's dispersion) in column order; ip_old2new maps the caller's observation index for get_rows().
inline void sort_blocks_by_column(CreatePlan &pl) {
    const jaicov_problem_desc *D = &pl.D;
    const size_t n = (size_t)D->n_image_points;
    std::vector<int32_t> lo(n, NOCOL), hi(n, -1);      // in the caller's order; the sort key is lo
    for (int ip : pl.blk_ip_list)
        for (int a = 0; a < 3; a++) {
            const int c = D->point_col[3 * D->ip_point[ip] + a];
            if (c >= 0) { lo[ip] = std::min(lo[ip], c); hi[ip] = std::max(hi[ip], c); }
        }
    std::vector<int32_t> new2old(n);
    for (size_t ip = 0; ip < n; ip++) new2old[ip] = (int32_t)ip;
    bool permuted = false;
    for (int g : pl.blk_list) {
        const int b = D->blk_ip_begin[g], en = D->blk_ip_begin[g + 1];
        std::stable_sort(new2old.begin() + b, new2old.begin() + en, [&](int x, int y) { return lo[x] < lo[y]; });
        for (int ip = b; ip < en && !permuted; ip++) permuted = new2old[ip] != ip;
    }
    if (!permuted) { pl.lo_col.swap(lo); pl.hi_col.swap(hi); return; }
    pl.pv_image.resize(n); pl.pv_point.resize(n); pl.pv_x.resize(n); pl.pv_y.resize(n); pl.pv_vx.resize(n); pl.pv_vy.resize(n); pl.pv_rho.resize(n);
    pl.perm_local.resize(n); pl.ip_old2new.resize(n); pl.lo_col.resize(n); pl.hi_col.resize(n);
    for (size_t i = 0; i < n; i++) {
        const int o = new2old[i];
        pl.pv_image[i] = D->ip_image[o]; pl.pv_point[i] = D->ip_point[o]; pl.pv_x[i] = D->ip_x[o]; pl.pv_y[i] = D->ip_y[o];
        pl.pv_vx[i] = D->ip_var_x[o]; pl.pv_vy[i] = D->ip_var_y[o]; pl.pv_rho[i] = D->ip_rho[o];
        pl.lo_col[i] = lo[o]; pl.hi_col[i] = hi[o];
        pl.ip_old2new[o] = (int32_t)i;
    }
    for (int g : pl.blk_list)
        for (int ip = D->blk_ip_begin[g]; ip < D->blk_ip_begin[g + 1]; ip++) pl.perm_local[ip] = new2old[ip] - D->blk_ip_begin[g];
    pl.D.ip_image = pl.pv_image.data(); pl.D.ip_point = pl.pv_point.data(); pl.D.ip_x = pl.pv_x.data(); pl.D.ip_y = pl.pv_y.data();
    pl.D.ip_var_x = pl.pv_vx.data(); pl.D.ip_var_y = pl.pv_vy.data(); pl.D.ip_rho = pl.pv_rho.data();
}

// The strip width follows the scene: a wave takes the partners of ONE image inside the strip's columns, 64 at a time.  With
// random visibility the default width holds 55 +- 7 of an image's 500 points; on a block flown in strips the
// points of an image are neighbours in column order and sit in two or three strips, hundreds in each -- eight segments of one
// image inside one turn of the deterministic form.  Then the strip is narrowed until an image's partners in a strip are about
// one wave again (never below 256 columns: the range table has one entry per image point and strip).
inline int gather_strip_width(const CreatePlan &pl) {
    const jaicov_problem_desc *D = &pl.D;
    int cw_rt = std::max(64, std::min(PP_CW, 6400)) / 4 * 4;  // 3 * cw doubles of LDS (<= 150 KB), quarters for the DET form
    double span = 0.0, cnt = 0.0;                             // default-width strips touched by the blocks, and their points
    for (size_t t = 0; t < pl.blk_list.size(); t++) {
        const int g = pl.blk_list[t], ipb = D->blk_ip_begin[g], mp = D->blk_ip_begin[g + 1] - ipb;
        // distinct default-width strips touched by this block's points
        int touched = 0, last = -1;
        for (int j = 0; j < mp; j++) {
            if (pl.lo_col[ipb + j] == NOCOL) continue;
            const int c = (pl.lo_col[ipb + j] - pl.cmin) / cw_rt;
            if (c != last) { ++touched; last = c; }
        }
        if (touched > 0) { span += touched; cnt += mp; }
    }
    const double per_strip = span > 0 ? cnt / span : 0.0;   // mean partners of an image per touched strip
    if (per_strip > 96.0) {
        int cw2 = (int)(cw_rt * 56.0 / per_strip) / 64 * 64;
        cw_rt = std::max(256, std::min(cw_rt, cw2));
    }
    return cw_rt;
}

// per record (entry of `list`: image points of blk_ip_list, by object point) and column chunk: the range of partner
// positions (the block is stored in column order)
inline bool gather_ranges(CreatePlan &pl, const std::vector<int32_t> &list, const std::vector<int32_t> &blk_of_ip) {
    const jaicov_problem_desc *D = &pl.D;
    const int n_chunks = pl.n_chunks, cw_rt = pl.cw;
    std::vector<int32_t> chunk_lo((size_t)pl.blk_list.size() * n_chunks), chunk_hi((size_t)pl.blk_list.size() * n_chunks);
    std::vector<int32_t> blk_pos(D->n_image_blocks, -1);
    for (size_t t = 0; t < pl.blk_list.size(); t++) {
        const int g = pl.blk_list[t], ipb = D->blk_ip_begin[g], mp = D->blk_ip_begin[g + 1] - ipb;
        blk_pos[g] = (int)t;
        for (int j = 1; j < mp; j++)
            if (pl.lo_col[ipb + j] < pl.lo_col[ipb + j - 1]) return plan_fail(pl, JAICOV_ERR_DEVICE, "internal: dense block not in column order");
        for (int c = 0; c < n_chunks; c++) {
            const int c0 = pl.cmin + c * cw_rt, c1 = c0 + cw_rt;
            int lo = mp, hi = 0;
            for (int j = 0; j < mp; j++)
                if (pl.hi_col[ipb + j] >= c0 && pl.lo_col[ipb + j] < c1) { lo = std::min(lo, j); hi = j + 1; }
            chunk_lo[t * n_chunks + c] = lo; chunk_hi[t * n_chunks + c] = std::max(hi, lo);
        }
    }
    pl.range.resize((size_t)2 * list.size() * n_chunks);
    for (size_t o = 0; o < list.size(); o++) {
        const int ip = list[o], g = blk_of_ip[ip], ipb = D->blk_ip_begin[g], mp = D->blk_ip_begin[g + 1] - ipb;
        const int t = blk_pos[g];
        // partners whose first column is <= the largest row column of this point: a prefix of the block
        const int qend = (int)(std::upper_bound(pl.lo_col.begin() + ipb, pl.lo_col.begin() + ipb + mp, pl.hi_col[ip]) - (pl.lo_col.begin() + ipb));
        for (int c = 0; c < n_chunks; c++) {
            const int lo = chunk_lo[(size_t)t * n_chunks + c], hi = std::min(chunk_hi[(size_t)t * n_chunks + c], qend);
            pl.range[2 * (o * n_chunks + c)] = lo;
            pl.range[2 * (o * n_chunks + c) + 1] = std::max(hi, lo);
        }
    }
    return true;
}

// point -> block image points (CSR, image order) for the atomics-free point x point gather, and what it reads beside them
inline bool gather_tables(CreatePlan &pl) {
    const jaicov_problem_desc *D = &pl.D;
    if (pl.blk_ip_list.empty()) return true;
    std::vector<int32_t> cnt(D->n_points + 1, 0), blk_of_ip(D->n_image_points, -1);
    for (size_t t = 0; t < pl.blk_list.size(); t++)
        for (int ip = D->blk_ip_begin[pl.blk_list[t]]; ip < D->blk_ip_begin[pl.blk_list[t] + 1]; ip++) blk_of_ip[ip] = pl.blk_list[t];
    for (int ip : pl.blk_ip_list) cnt[D->ip_point[ip] + 1]++;
    for (int i = 0; i < D->n_points; i++) cnt[i + 1] += cnt[i];
    std::vector<int32_t> fill(cnt.begin(), cnt.end() - 1), list(pl.blk_ip_list.size());
    int cmin = NOCOL, cmax = -1;
    for (int ip : pl.blk_ip_list) {
        list[fill[D->ip_point[ip]]++] = ip;
        if (pl.lo_col[ip] != NOCOL) { cmin = std::min(cmin, pl.lo_col[ip]); cmax = std::max(cmax, pl.hi_col[ip]); }
    }
    if (cmax < cmin) return true;
    pl.recs.resize(list.size());
    for (size_t t = 0; t < list.size(); t++) {
        const int ip = list[t], g = blk_of_ip[ip];
        PPRecord r{};
        r.ipb = D->blk_ip_begin[g]; r.mp = D->blk_ip_begin[g + 1] - r.ipb; r.lp = ip - r.ipb; r.poff = pl.blk_w_off[g];
        pl.recs[t] = r;
    }
    // the gather reads the columns as three arrays over the image points (coalesced like A_q and U_q)
    const size_t S = (size_t)D->n_image_points;
    pl.ipcol.assign(3 * S, -1);
    for (int ip : pl.blk_ip_list)
        for (int a = 0; a < 3; a++) pl.ipcol[(size_t)a * S + ip] = D->point_col[3 * D->ip_point[ip] + a];
    pl.cmin = cmin; pl.cmax = cmax;
    pl.cw = gather_strip_width(pl);
    pl.n_chunks = (cmax - cmin + pl.cw) / pl.cw;
    if (!gather_ranges(pl, list, blk_of_ip)) return false;
    pl.pt_ip_begin.swap(cnt);
    // rows cmin..cmax all point rows?  (points are numbered first and contiguously, BA:667-782)
    std::vector<char> is_pt(cmax - cmin + 1, 0);
    for (int i = 0; i < 3 * D->n_points; i++) {
        const int c = D->point_col[i];
        if (c >= cmin && c <= cmax) is_pt[c - cmin] = 1;
    }
    bool all = true;
    for (char f : is_pt) all = all && f;
    pl.plain_ok = all;
    pl.gather = true;
    return true;
}

// EO pre-elimination is possible when every image point sits in an image block, the EO columns are trailing
// (eo_columns_trailing) and every block has at least three points; assembly_mode 1 / 2 (densemode.hip) replaces it.
// Eligibility is a property of the WHOLE problem, not of this engine's image range: every rank of a sharded run must
// reach the same decision, or their reduce buffers differ in length (and only some ranks enter the EO exchange).
inline void decide_elimination(CreatePlan &pl, const jaicov_engine_options &o) {
    const jaicov_problem_desc *D = &pl.D;
    size_t n_in_block = 0;
    for (int ip = 0; ip < D->n_image_points; ip++) n_in_block += pl.in_block[ip] ? 1 : 0;
    bool ok = D->n_images > 0 && D->n_image_blocks > 0 && n_in_block == (size_t)D->n_image_points;
    if ((o.assembly_mode == 1 || o.assembly_mode == 2) && !pl.blk_list.empty()) {   // densified MFMA contraction of the image groups (densemode.hip)
        for (int g : pl.blk_list) {
            const int mp = D->blk_ip_begin[g + 1] - D->blk_ip_begin[g], cam = D->image_camera[D->ip_image[D->blk_ip_begin[g]]];
            const int k1 = 3 * mp + 9 + D->cam_dist_begin[cam + 1] - D->cam_dist_begin[cam] + 1;
            pl.max_k1 = std::max(pl.max_k1, k1);
            pl.dm_flops_per_pass += 2.0 * (2.0 * mp) * (2.0 * mp) * k1 + (2.0 * mp) * k1 * (k1 + 1.0);
        }
        pl.dense_mode = true;
        ok = false;
    }
    const int e0 = ok ? eo_columns_trailing(*D) : -1;
    ok = ok && e0 >= 0;
    for (int g = 0; ok && g < D->n_image_blocks; g++) ok = D->blk_ip_begin[g + 1] - D->blk_ip_begin[g] >= 3;
    pl.schur_ok = ok;
    if (ok) pl.e0 = e0;
}

// the whole plan, in the order its steps depend on each other; false: pl.status / pl.err say why
inline bool build_create_plan(CreatePlan &pl, const jaicov_problem_desc &desc, const jaicov_engine_options &o, int form) {
    pl.D = desc;
    if (!validate(pl, o)) return false;
    synthesize_blocks(pl, o, form);
    blocks_and_segments(pl, form);
    sort_blocks_by_column(pl);
    if (!gather_tables(pl)) return false;
    decide_elimination(pl, o);
    return true;
}

// the options of a caller that passes none
inline jaicov_engine_options default_options() {
    jaicov_engine_options o{};
    o.image_begin = o.image_end = -1;
    o.apply_shared = 1;
    return o;
}

}  // namespace jaicov
