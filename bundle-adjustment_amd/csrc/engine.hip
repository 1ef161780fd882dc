// C ABI of the normal-equation engine (include/jaicov_neq.h): lifecycle, parameters, accumulate / finalize / build, the reduce buffers,
// the getters and the timings, with the glue kernels they launch.  Creation's device stage is engine_create.hip, solve and estimate
// engine_solve.hip; the three share engine_state.h.  gfx950 only.  There is NO CPU fallback here: every entry point fails with
// JAICOV_ERR_NO_DEVICE / JAICOV_ERR_DEVICE when HIP is unusable.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "create_plan.h"
#include "engine_state.h"
#include "gemm_f64.h"      // d4_t
#include "launchers.h"
// jaicov_neq_create and _destroy make and delete the engine with its QSlots: the states of every reader are complete types here
#include "calibration.h"
#include "datum.h"
#include "forms.h"
#include "newpoints.h"
#include "parameters.h"
#include "precision.h"
#include "predict.h"
#include "reliability.h"
#include "transform.h"
#include "vce.h"

// ---------------------------------------------------------------------------------------------------------------
// glue kernels
// ---------------------------------------------------------------------------------------------------------------
// BA:814-828: damping on unknown columns, then V = 1/sqrt(diag) where diag > EPS (V = 1 on the border, whose
// diagonal is zero); padded rows get V = 1
__global__ void damp_and_precond_kernel(double *N, long ld, int U, int Upad, int d, double lambda, double *V,
                                        const double *diagcorr) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Upad) return;
    double v = 1.0;
    if (c >= d && c < U) {
        double diag = N[(long)c * ld + c];
        if (lambda > 0.0) {
            // the reference damps the diagonal of the UNREDUCED normal matrix; diagcorr = what the EO elimination took
            diag += lambda * (diag + (diagcorr ? diagcorr[c] : 0.0));
            N[(long)c * ld + c] = diag;
        }
        v = diag > 1.1102230246251565e-16 ? 1.0 / sqrt(diag) : 1.0;
    }
    V[c] = v;
}

// zero the lower triangle (row r: columns 0 .. r, rounded up to 4) of the leading `rows` rows; grid (ceil(rows/1024), rows)
// rows skip_lo..skip_hi (the point rows the gather stores itself, PPGather::plain): only the columns before skip_lo
__global__ __launch_bounds__(256) void zero_lower_kernel(double *__restrict__ N, long ld, int rows, int skip_lo, int skip_hi, int row0) {
    const int r = row0 + blockIdx.y, c = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (c > r || r >= rows) return;
    if (r >= skip_lo && r <= skip_hi) {
        if (c >= skip_lo) return;
        if (c + 4 > skip_lo) {           // the quad straddles the first stored column
            for (int k = c; k < skip_lo; k++) N[(long)r * ld + k] = 0.0;
            return;
        }
    }
    *reinterpret_cast<d4_t *>(N + (long)r * ld + c) = (d4_t){0.0, 0.0, 0.0, 0.0};
}

// row-major lower square <-> packed ('U' column-major == row-major lower packed)
__global__ __launch_bounds__(256) void pack_kernel(const double *__restrict__ M, long ld, int U, double *__restrict__ ap) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j > i || i >= U) return;
    ap[(size_t)i * (i + 1) / 2 + j] = M[(long)i * ld + j];
}
__global__ __launch_bounds__(256) void unpack_kernel(const double *__restrict__ ap, long ld, int U, double *__restrict__ M) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j > i || i >= U) return;
    M[(long)i * ld + j] = ap[(size_t)i * (i + 1) / 2 + j];
}
__global__ void gather_sub_kernel(const double *__restrict__ Q, long ld, const int32_t *idx, int k, double *out, double scale) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k * k) return;
    const int a = t / k, b = t - a * k;
    const int i = idx[a], j = idx[b];
    out[t] = scale * (i >= j ? Q[(long)i * ld + j] : Q[(long)j * ld + i]);
}
void jaicov::launch_pack(hipStream_t s, const double *M, long ld, int U, double *ap) {
    hipLaunchKernelGGL(pack_kernel, dim3((U + 255) / 256, std::max(U, 1)), dim3(256), 0, s, M, ld, U, ap);
}
void jaicov::launch_unpack(hipStream_t s, const double *ap, long ld, int U, double *M) {
    hipLaunchKernelGGL(unpack_kernel, dim3((U + 255) / 256, std::max(U, 1)), dim3(256), 0, s, ap, ld, U, M);
}

extern "C" int jaicov_neq_abi_version(void) { return JAICOV_NEQ_ABI_VERSION; }

extern "C" const char *jaicov_neq_last_error(const jaicov_engine *e) { return e ? e->err.c_str() : "null engine"; }

extern "C" void jaicov_neq_destroy(jaicov_engine *e) {
    if (!e) return;
    hipSetDevice(e->device);
    if (e->stream) hipStreamSynchronize(e->stream);
    delete e;      // every member frees what it holds; the stream's lease goes last (see the member)
}

extern "C" int jaicov_neq_create(const jaicov_problem_desc *desc, const jaicov_engine_options *opts, jaicov_engine **out) {
    if (!out) return JAICOV_ERR_BAD_ARGUMENT;
    *out = nullptr;
    if (!desc || desc->struct_size != sizeof(jaicov_problem_desc)) return JAICOV_ERR_BAD_ARGUMENT;
    std::string err;
    int rc = check_device(err);
    if (rc != JAICOV_OK) return rc;
    if (opts && opts->struct_size != sizeof(jaicov_engine_options)) return JAICOV_ERR_BAD_ARGUMENT;
    jaicov_engine *e = new jaicov_engine();
    e->opts = opts ? *opts : default_options();
    e->device = e->opts.device;
    *out = e;     // returned even on failure so that the caller can read jaicov_neq_last_error(); destroy() frees it
    const auto t0 = std::chrono::steady_clock::now();
    rc = engine_create_impl(e, desc);
    e->create_ms[CREATE_TOTAL] = ms_since(t0);
    return rc;
}

extern "C" size_t jaicov_neq_num_slots(const jaicov_engine *e) { return e ? (size_t)e->n_slots : 0; }
extern "C" size_t jaicov_neq_packed_length(const jaicov_engine *e) { return e ? (size_t)e->U * (e->U + 1) / 2 : 0; }

extern "C" int jaicov_neq_set_parameters(jaicov_engine *e, const double *slots, size_t n) {
    if (!e || !slots || n != (size_t)e->n_slots) return JAICOV_ERR_BAD_ARGUMENT;
    HIPE(e->err, hipSetDevice(e->device));
    memcpy(e->h_vals.data(), slots, n * sizeof(double));
    HIPE(e->err, hipMemcpyAsync(e->d_vals, e->h_vals.data(), n * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    e->rows_valid = false;
    if (e->state == jaicov_engine::ST_NEW) e->state = jaicov_engine::ST_PARAMS;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_get_parameters(jaicov_engine *e, double *slots, size_t n) {
    if (!e || !slots || n != (size_t)e->n_slots) return JAICOV_ERR_BAD_ARGUMENT;
    memcpy(slots, e->h_vals.data(), n * sizeof(double));
    return JAICOV_OK;
}

int jaicov::engine_ensure_rows(jaicov_engine *e) {
    if (e->rows_valid) return JAICOV_OK;
    HIPE(e->err, launch_rows(e->stream, e->p, e->d_vals, e->ip0, e->ip_count, e->d_rowsA, e->d_rowsW));
    e->rows_valid = true;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_accumulate(jaicov_engine *e, double sigma2) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state == jaicov_engine::ST_NEW) FAIL(e->err, JAICOV_ERR_BAD_STATE, "set_parameters first");
    if (!(sigma2 > 0)) FAIL(e->err, JAICOV_ERR_BAD_ARGUMENT, "variance of unit weight must be positive (DOPG:68-69)");
    HIPE(e->err, hipSetDevice(e->device));
    e->reduced = false;          // a packed buffer of an earlier accumulate must not be unpacked over this one
    e->sigma2_acc = sigma2;
    const size_t sq = (size_t)e->Upad * e->Upad;
    HIPE(e->err, hipEventRecord(e->ev[EV_ACC_BEGIN].get(), e->stream));
    TRY(engine_ensure_rows(e));
    HIPE(e->err, hipEventRecord(e->ev[EV_ROWS].get(), e->stream));
    e->schur_active = e->schur_ok && e->inverse_mode_next != JAICOV_INVERT_FULL;
    // The point x point gather owns every entry of rows cmin..cmax from column cmin on: when it runs before everything
    // else that adds into that region it stores its strips, and the region needs neither zeroing nor reading back.
    const bool plain = e->pp_plain_ok && !e->dense_mode && e->pp.pt_ip_begin != nullptr && e->n_blk_list > 0;
    {   // only the lower triangle of N is ever written or read (nadd, pack, scale_copy); the reduced system has e0 rows
        const int rows = e->schur_active ? std::min(e->Upad, ((e->e0 + 127) / 128) * 128) : e->Upad;
        // three launches, each over the rows and columns that need zeroing only (one launch over the whole square spent 60 us at
        // config 4 dispatching 226 000 workgroups of which 99.9 % returned at once): rows above the stored strips, the stored rows'
        // columns before the first stored column (nothing when the points come first and there is no datum border), rows below
        const int slo = plain ? e->pp.cmin : rows, shi = plain ? e->pp.cmax : -1;
        auto zero_rows = [&](int r0, int r1, int cols) {
            if (r1 > r0 && cols > 0)
                hipLaunchKernelGGL(zero_lower_kernel, dim3((cols + 1023) / 1024, r1 - r0), dim3(256), 0, e->stream, e->d_N, (long)e->Upad, rows, slo, shi, r0);
        };
        zero_rows(0, std::min(slo, rows), std::min(slo, rows));
        if (plain) {
            zero_rows(slo, std::min(shi + 1, rows), slo);
            zero_rows(std::min(shi + 1, rows), rows, rows);
        }
        HIPE(e->err, hipMemsetAsync(e->d_N + sq, 0, (size_t)e->Upad * sizeof(double), e->stream));
    }
    if (!plain)
        HIPE(e->err, launch_assemble_small(e->stream, e->p, e->d_seg_begin, e->d_seg_end, e->n_seg, e->d_rowsA, e->d_rowsW, sigma2, e->d_N, e->d_n));
    SchurBufs sb = e->sb;
    sb.active = e->schur_active;
    sb.lambda = e->lambda_acc;
    if (e->schur_active) {
        HIPE(e->err, hipMemsetAsync(e->sb.info, 0, sizeof(int), e->stream));
        HIPE(e->err, hipMemsetAsync(e->sb.diagcorr, 0, (size_t)e->Upad * sizeof(double), e->stream));
    }
    if (e->dense_mode) {
        float ms = 0.f;
        HIPE(e->err, e->dm.assemble(e->stream, e->p, e->d_blk_list, e->n_blk_list, e->d_rowsA, e->d_rowsW, sigma2, e->d_N, e->d_n,
                               e->solver.profile ? &ms : nullptr));
        if (e->solver.profile) { e->dm_stat_passes += 1.0; e->dm_stat_ms += ms; e->dm_stat_flops += e->dm_flops_per_pass; }
    } else {
        PPGather ppg = e->pp;
        ppg.plain = plain ? 1 : 0;
        ppg.ug = sb.active ? sb.Ug : nullptr;
        HIPE(e->err, launch_assemble_blocks(e->stream, e->p, e->d_blk_list, e->n_blk_list, e->max_m, e->d_blk_ip_list, e->n_blk_ip,
                                       e->d_rowsA, e->d_rowsW, e->d_T, sigma2, e->d_N, e->d_n, ppg, sb, e->d_cc_partial,
                                       e->solver.pstream, e->ev_fork.get(), e->ev_join.get()));   // side stream: the solver's (idle during the assembly)
    }
    if (plain)   // the images outside the dense blocks come after the stores
        HIPE(e->err, launch_assemble_small(e->stream, e->p, e->d_seg_begin, e->d_seg_end, e->n_seg, e->d_rowsA, e->d_rowsW, sigma2, e->d_N, e->d_n));
    if (e->opts.apply_shared) HIPE(e->err, launch_shared_groups(e->stream, e->p, e->d_vals, sigma2, e->d_N, e->d_n, nullptr, nullptr));
    HIPE(e->err, hipEventRecord(e->ev[EV_ASSEMBLED].get(), e->stream));
    e->exp_ready = false;            // the expansion buffer of an earlier pass is stale now
    e->state = jaicov_engine::ST_ACCUMULATED;
    e->q.valid = false;
    return JAICOV_OK;
}

// datum rows (BA:493-635) of the point mask at the slot values `vals`: B [d][stride] (columns >= stride are not stored)
static int datum_rows(jaicov_engine *e, const uint8_t *mask, const double *vals, std::vector<double> &hB, int stride) {
    const int d = e->d;
    std::fill(hB.begin(), hB.end(), 0.0);
    if (d == 0) return JAICOV_OK;
    double x0 = 0, y0 = 0, z0 = 0;
    int count = 0;
    for (int pt = 0; pt < e->n_points; pt++) {
        const int32_t *c = &e->h_slot_col[3 * pt];
        if (!mask[pt] || c[0] < 0 || c[1] < 0 || c[2] < 0) continue;
        x0 += vals[3 * pt]; y0 += vals[3 * pt + 1]; z0 += vals[3 * pt + 2];
        count++;
    }
    if (count < 3) FAIL(e->err, JAICOV_ERR_BAD_ARGUMENT, "not enough object points to realise the frame datum (BA:515-516)");
    x0 /= (double)count; y0 /= (double)count; z0 /= (double)count;
    int row = 0;
    const int f = e->datum_flags;
    const int tx = (f & JAICOV_DATUM_TX) ? row++ : -1, ty = (f & JAICOV_DATUM_TY) ? row++ : -1, tz = (f & JAICOV_DATUM_TZ) ? row++ : -1;
    const int rx = (f & JAICOV_DATUM_RX) ? row++ : -1, ry = (f & JAICOV_DATUM_RY) ? row++ : -1, rz = (f & JAICOV_DATUM_RZ) ? row++ : -1;
    const int ms = (f & JAICOV_DATUM_SCALE) ? row++ : -1;
    double norm[7] = {0, 0, 0, 0, 0, 0, 0};
    double sink = 0.0;
    auto B = [&](int r, int c) -> double & { return c < stride ? hB[(size_t)r * stride + c] : sink; };
    for (int pt = 0; pt < e->n_points; pt++) {
        const int32_t *c = &e->h_slot_col[3 * pt];
        if (!mask[pt] || c[0] < 0 || c[1] < 0 || c[2] < 0) continue;
        const double x = vals[3 * pt] - x0, y = vals[3 * pt + 1] - y0, z = vals[3 * pt + 2] - z0;
        if (tx >= 0) { B(tx, c[0]) = 1.0; norm[tx] += 1.0; }
        if (ty >= 0) { B(ty, c[1]) = 1.0; norm[ty] += 1.0; }
        if (tz >= 0) { B(tz, c[2]) = 1.0; norm[tz] += 1.0; }
        if (rx >= 0) { B(rx, c[1]) = z; B(rx, c[2]) = -y; norm[rx] += z * z + y * y; }
        if (ry >= 0) { B(ry, c[0]) = -z; B(ry, c[2]) = x; norm[ry] += z * z + x * x; }
        if (rz >= 0) { B(rz, c[0]) = y; B(rz, c[1]) = -x; norm[rz] += x * x + y * y; }
        if (ms >= 0) { B(ms, c[0]) = x; B(ms, c[1]) = y; B(ms, c[2]) = z; norm[ms] += x * x + y * y + z * z; }
    }
    const int cend = std::min(e->U, stride);
    for (int r = 0; r < d; r++) {
        const double s = sqrt(norm[r]);
        for (int c = 0; c < cend; c++)
            if (hB[(size_t)r * stride + c] != 0.0) hB[(size_t)r * stride + c] = hB[(size_t)r * stride + c] / s;
    }
    return JAICOV_OK;
}

// datum rows of the build from the host copy of the parameter values
static int datum_rows_host(jaicov_engine *e) {
    return datum_rows(e, e->h_point_datum.data(), e->h_vals.data(), e->hB, e->Upad);
}

extern "C" int jaicov_neq_finalize(jaicov_engine *e, double sigma2, double lambda, int simulation) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    (void)sigma2;
    if (e->state != jaicov_engine::ST_ACCUMULATED) FAIL(e->err, JAICOV_ERR_BAD_STATE, "accumulate first");
    HIPE(e->err, hipSetDevice(e->device));
    TRY(datum_rows_host(e));
    if (e->reduced) {   // the host has summed the packed buffer over ranks: bring it back into the square
        const int Ua = e->schur_active ? e->e0 : e->U;
        const size_t len = (size_t)Ua * (Ua + 1) / 2;
        launch_unpack(e->stream, e->d_packed, (long)e->Upad, Ua, e->d_N);
        HIPE(e->err, hipMemcpyAsync(e->d_n, e->d_packed + len, (size_t)Ua * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        if (e->schur_active)   // what the EO elimination took from the diagonal, summed over the ranks like N itself (LM damping)
            HIPE(e->err, hipMemcpyAsync(e->sb.diagcorr, e->d_packed + len + Ua, (size_t)Ua * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        e->reduced = false;
    }
    if (e->schur_active && lambda != e->lambda_acc && (lambda > 0 || e->lambda_acc > 0))
        FAIL(e->err, JAICOV_ERR_BAD_ARGUMENT, "EO pre-elimination: pass the damping value to accumulate2()/build() as well");
    hipLaunchKernelGGL(damp_and_precond_kernel, dim3((e->Upad + 255) / 256), dim3(256), 0, e->stream, e->d_N, (long)e->Upad,
                       e->schur_active ? e->e0 : e->U, e->Upad, e->d, lambda > 0 ? lambda : 0.0, e->d_V,
                       e->schur_active ? e->sb.diagcorr : nullptr);
    if (simulation) HIPE(e->err, hipMemsetAsync(e->d_n, 0, e->Upad * sizeof(double), e->stream));   // BA:830-831
    e->sim_built = simulation != 0;
    HIPE(e->err, hipEventRecord(e->ev[EV_BUILT].get(), e->stream));
    e->lambda_used = lambda;
    e->state = jaicov_engine::ST_BUILT;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_prepare_inverse(jaicov_engine *e, int inverse_follows) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    if (inverse_follows < 0 || inverse_follows > JAICOV_INVERT_FULL_EXPANDED) return JAICOV_ERR_BAD_ARGUMENT;
    inverse_follows = effective_invert(e, inverse_follows);
    e->inverse_mode_next = inverse_follows;
    // the inverse's buffers are allocated HERE, when the final pass is announced (BA:250: known before the build), not inside
    // the solve: hipMalloc of 2 x 1.8 .. 2.6 GB cost the first inverting solve 45 ms at config 4
    if (inverse_follows == JAICOV_INVERT_NONE) return JAICOV_OK;
    HIPE(e->err, hipSetDevice(e->device));
    const bool reduced = e->schur_ok && (inverse_follows == JAICOV_INVERT_REDUCED || inverse_follows == JAICOV_INVERT_FULL_EXPANDED) && e->solverS_ready;
    return ensure_inverse_buffers(e, reduced, inverse_follows);
}

extern "C" int jaicov_neq_cofactor_order(const jaicov_engine *e) {
    if (!e || !e->q.valid) return -1;
    return e->q.order;
}

extern "C" int jaicov_neq_reduced_order(const jaicov_engine *e) {
    if (!e) return -1;
    return e->schur_active ? e->e0 : e->U;
}

extern "C" int jaicov_neq_accumulate2(jaicov_engine *e, double sigma2, double lambda) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    e->lambda_acc = lambda > 0 ? lambda : 0.0;
    return jaicov_neq_accumulate(e, sigma2);
}

extern "C" int jaicov_neq_build(jaicov_engine *e, double sigma2, double lambda, int simulation) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    e->lambda_acc = lambda > 0 ? lambda : 0.0;
    TRY(jaicov_neq_accumulate(e, sigma2));
    return jaicov_neq_finalize(e, sigma2, lambda, simulation);
}

static int reduce_buffer_impl(jaicov_engine *e, void **device_ptr, size_t *count, bool sync) {
    if (!e || !device_ptr || !count) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state != jaicov_engine::ST_ACCUMULATED) FAIL(e->err, JAICOV_ERR_BAD_STATE, "accumulate first");
    HIPE(e->err, hipSetDevice(e->device));
    // packed lower triangle (== UPLO='U' packed) followed by n: one contiguous array the collective sums as it is.
    // With the EO pre-elimination only the reduced system (order e0) exists.
    const int Ua = e->schur_active ? e->e0 : e->U;
    const size_t len = (size_t)Ua * (Ua + 1) / 2;
    if (!e->d_packed) TRY(dalloc(e, (size_t)e->U * (e->U + 1) / 2 + 2 * (size_t)e->U, &e->d_packed));
    launch_pack(e->stream, e->d_N, (long)e->Upad, Ua, e->d_packed);
    HIPE(e->err, hipMemcpyAsync(e->d_packed + len, e->d_n, (size_t)Ua * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    // with the EO pre-elimination the LM damping needs diag(N) - diag(N_reduced), also a sum over the ranks' images
    if (e->schur_active)
        HIPE(e->err, hipMemcpyAsync(e->d_packed + len + Ua, e->sb.diagcorr, (size_t)Ua * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    if (sync) HIPE(e->err, hipStreamSynchronize(e->stream));   // the caller's collective runs on its own stream
    e->reduced = true;
    *device_ptr = e->d_packed;
    *count = len + Ua + (e->schur_active ? (size_t)Ua : 0);
    return JAICOV_OK;
}

extern "C" int jaicov_neq_reduce_buffer(jaicov_engine *e, void **device_ptr, size_t *count) {
    return reduce_buffer_impl(e, device_ptr, count, true);
}

extern "C" int jaicov_neq_reduce_buffer_async(jaicov_engine *e, void **device_ptr, size_t *count, void **stream) {
    if (!stream) return JAICOV_ERR_BAD_ARGUMENT;
    const int rc = reduce_buffer_impl(e, device_ptr, count, false);
    if (rc == JAICOV_OK) *stream = (void *)e->stream;
    return rc;
}

extern "C" int jaicov_neq_expansion_buffer(jaicov_engine *e, void **device_ptr, size_t *count) {
    if (!e || !device_ptr || !count) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state != jaicov_engine::ST_ACCUMULATED || !e->schur_active || !e->solverS_ready)
        FAIL(e->err, JAICOV_ERR_BAD_STATE, "expansion buffer: accumulate a pre-eliminated system first (prepare_inverse(JAICOV_INVERT_FULL_EXPANDED))");
    HIPE(e->err, hipSetDevice(e->device));
    size_t I6p, Up;
    expansion_fits(e, &I6p, &Up);
    const size_t len = I6p * Up + (size_t)36 * e->p.n_images;
    HIPE(e->err, e->expF.reserve(len));
    e->expF_len = len;
    double *d_expF = e->expF.get();
    TRY(engine_ensure_rows(e));
    HIPE(e->err, hipMemsetAsync(d_expF, 0, I6p * Up * sizeof(double), e->stream));       // foreign images' bands: zero
    HIPE(e->err, launch_schur_expand_f(e->stream, e->p, e->d_blk_list, e->n_blk_list, e->d_rowsA, e->sb.U, e->sb.Linv, e->sb.G, d_expF, (long)Up));
    // L_E^-1: written for this engine's images only (blk_elim_kernel), zero elsewhere since create
    HIPE(e->err, hipMemcpyAsync(d_expF + I6p * Up, e->sb.Linv, (size_t)36 * e->p.n_images * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    e->exp_ready = true;
    *device_ptr = d_expF;
    *count = len;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_eo_step_buffer(jaicov_engine *e, void **device_ptr, size_t *count) {
    if (!e || !device_ptr || !count) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state != jaicov_engine::ST_SOLVED || !e->schur_active || !e->d_xE) FAIL(e->err, JAICOV_ERR_BAD_STATE, "no pre-eliminated exterior orientations: solve a reduced system first");
    *device_ptr = e->d_xE;
    *count = (size_t)6 * e->p.n_images;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_omega(jaicov_engine *e, double sigma2, const double *dx, double *omega) {
    if (!e || !dx || !omega) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state == jaicov_engine::ST_NEW) FAIL(e->err, JAICOV_ERR_BAD_STATE, "set_parameters first");
    HIPE(e->err, hipSetDevice(e->device));
    TRY(engine_ensure_rows(e));
    hipEvent_t t0 = e->ev[EV_OMEGA_BEGIN].get(), t1 = e->ev[EV_OMEGA_END].get();
    HIPE(e->err, hipEventRecord(t0, e->stream));
    HIPE(e->err, hipMemcpyAsync(e->d_dx, dx, (size_t)e->U * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPE(e->err, hipMemsetAsync(e->d_omega, 0, sizeof(double), e->stream));
    HIPE(e->err, launch_omega(e->stream, e->p, e->d_in_block, e->ip0, e->ip_count, e->d_blk_list, e->n_blk_list, e->max_m,
                         e->d_rowsA, e->d_rowsW, e->d_dx, sigma2, e->d_vbuf, e->d_omega));
    if (e->opts.apply_shared) HIPE(e->err, launch_shared_groups(e->stream, e->p, e->d_vals, sigma2, nullptr, nullptr, e->d_dx, e->d_omega));
    HIPE(e->err, hipEventRecord(t1, e->stream));
    HIPE(e->err, hipMemcpyAsync(omega, e->d_omega, sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    float ms;
    hipEventElapsedTime(&ms, t0, t1);
    e->timings[T_OMEGA] = ms;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_update(jaicov_engine *e, const double *dx, double *max_abs_dx) {
    if (!e || !dx) return JAICOV_ERR_BAD_ARGUMENT;
    HIPE(e->err, hipSetDevice(e->device));
    double mx = 0.0;
    for (int s = 0; s < e->n_slots; s++) {
        const int c = e->h_slot_col[s];
        if (c >= 0) {
            const double dv = dx[c];
            mx = std::max(mx, fabs(dv));
            e->h_vals[s] = e->h_vals[s] + dv;
        }
    }
    if (max_abs_dx) *max_abs_dx = mx;
    HIPE(e->err, hipMemcpyAsync(e->d_vals, e->h_vals.data(), (size_t)e->n_slots * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    e->rows_valid = false;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_get_normal(jaicov_engine *e, double *N_packed, size_t len, double *n, size_t Ulen) {
    if (!e || !N_packed || !n) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state != jaicov_engine::ST_BUILT && e->state != jaicov_engine::ST_SOLVED && e->state != jaicov_engine::ST_ACCUMULATED)
        FAIL(e->err, JAICOV_ERR_BAD_STATE, "build first");
    const int U = e->U;
    if (len != (size_t)U * (U + 1) / 2 || Ulen != (size_t)U) return JAICOV_ERR_BAD_ARGUMENT;
    HIPE(e->err, hipSetDevice(e->device));
    // with the exterior orientations pre-eliminated only the reduced system (order e0) was assembled: the rows from e0 on
    // of the square are neither zeroed nor written in such a pass.  The header's contract: reduced system in the leading
    // e0 rows / columns, zeros elsewhere.
    const int Ua = e->schur_active ? e->e0 : U;
    const size_t lenA = (size_t)Ua * (Ua + 1) / 2;
    DevBuf<double> ap;
    HIPE(e->err, ap.reserve(std::max<size_t>(lenA, 1)));
    launch_pack(e->stream, e->d_N, (long)e->Upad, Ua, ap.get());
    HIPE(e->err, hipMemcpyAsync(N_packed, ap.get(), lenA * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPE(e->err, hipMemcpyAsync(n, e->d_n, Ua * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    if (lenA < len) memset(N_packed + lenA, 0, (len - lenA) * sizeof(double));
    for (int c = Ua; c < U; c++) n[c] = 0.0;
    // the datum border lives on the host (rows 0..d-1): K[r][c] = B[r][c]  (BA:548-593), packed index r + c(c+1)/2
    if (e->state != jaicov_engine::ST_ACCUMULATED)
        for (int r = 0; r < e->d; r++)
            for (int c = e->d; c < Ua; c++) N_packed[(size_t)r + (size_t)c * (c + 1) / 2] = e->hB[(size_t)r * e->Upad + c];
    return JAICOV_OK;
}

extern "C" int jaicov_neq_get_cofactor(jaicov_engine *e, double *Q_packed, size_t len) {
    if (!e || !Q_packed) return JAICOV_ERR_BAD_ARGUMENT;
    if (!e->q.valid) FAIL(e->err, JAICOV_ERR_BAD_STATE, "no cofactor matrix: solve with invert != 0 first (MatrixInversion.NONE, BA:1177)");
    const int U = e->q.order;
    if (len != (size_t)U * (U + 1) / 2) FAIL(e->err, JAICOV_ERR_BAD_ARGUMENT, "cofactor buffer length must be order(order+1)/2 with order = jaicov_neq_cofactor_order()");
    HIPE(e->err, hipSetDevice(e->device));
    const DenseSolver &qs = e->q_solver();
    DevBuf<double> ap;
    HIPE(e->err, ap.reserve(std::max<size_t>(len, 1)));
    launch_pack(e->stream, qs.Q, qs.ld, U, ap.get());
    HIPE(e->err, hipMemcpyAsync(Q_packed, ap.get(), len * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    return JAICOV_OK;
}

// every consumer of the cofactor matrix sees the engine through this view (qview.h)
void jaicov::engine_q_view(jaicov_engine *e, QView *v) {
    DenseSolver &qs = e->q_solver();
    v->device = e->device;
    v->stream = e->stream;
    v->Q = qs.Q;
    v->ld = qs.ld;
    v->order = e->q.order;
    v->U = e->U;
    v->d = e->d;
    v->n_points = e->n_points;
    v->have_q = e->q.valid;
    v->reduced = e->q.reduced;
    v->full_q = e->q.valid && !e->q.reduced && e->q.order == e->U;
    v->sharded = !e->all_images || !e->opts.apply_shared || e->ip0 != 0 || e->ip_count != e->p.n_ip;
    v->sigma2 = e->q.sigma2;
    v->lambda = e->q.lambda;
    v->p = &e->p;
    v->d_vals = e->d_vals;
    v->rowsA = e->d_rowsA;
    v->rowsW = e->d_rowsW;
    v->ll_diag = e->d_ll_diag;
    v->slot_col = &e->h_slot_col;
    v->ip_old2new = &e->ip_old2new;
    v->blk_ip_begin = &e->h_blk_ip_begin;
    v->blk_w_off = &e->h_blk_w_off;
    v->caller_block = &e->h_caller_block;
    v->slot = &e->slot;
    v->err = &e->err;
}

int jaicov::engine_datum_rows(jaicov_engine *e, const uint8_t *mask, std::vector<double> &B, int stride) {
    if (e->q.vals.size() != (size_t)e->n_slots) FAIL(e->err, JAICOV_ERR_BAD_STATE, "no inverting solve has recorded its parameter values");
    B.assign((size_t)e->d * stride, 0.0);
    return datum_rows(e, mask, e->q.vals.data(), B, stride);
}

static int cofactor_sub_impl(jaicov_engine *e, const int32_t *idx, int32_t k, double scale, double *out) {
    if (!e || !idx || !out || k <= 0) return JAICOV_ERR_BAD_ARGUMENT;
    if (!e->q.valid) FAIL(e->err, JAICOV_ERR_BAD_STATE, "no cofactor matrix: solve with invert != 0 first");
    for (int i = 0; i < k; i++)
        if (idx[i] < 0 || idx[i] >= e->q.order) return JAICOV_ERR_BAD_ARGUMENT;
    const DenseSolver &qs = e->q_solver();
    HIPE(e->err, hipSetDevice(e->device));
    DevBuf<int32_t> d_idx;
    DevBuf<double> d_out;
    HIPE(e->err, d_idx.reserve((size_t)k));
    HIPE(e->err, d_out.reserve((size_t)k * k));
    HIPE(e->err, hipMemcpyAsync(d_idx.get(), idx, (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(gather_sub_kernel, dim3(((size_t)k * k + 255) / 256), dim3(256), 0, e->stream, qs.Q, qs.ld, d_idx.get(), k, d_out.get(), scale);
    HIPE(e->err, hipMemcpyAsync(out, d_out.get(), (size_t)k * k * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    return JAICOV_OK;
}

extern "C" int jaicov_neq_get_cofactor_sub(jaicov_engine *e, const int32_t *idx, int32_t k, double *out) {
    return cofactor_sub_impl(e, idx, k, 1.0, out);
}

extern "C" int jaicov_neq_get_dispersion_sub(jaicov_engine *e, double sigma2_aposteriori, const int32_t *idx, int32_t k, double *out) {
    return cofactor_sub_impl(e, idx, k, sigma2_aposteriori, out);
}

extern "C" int jaicov_neq_get_rows(jaicov_engine *e, int32_t ip_begin, int32_t ip_count, double *w, double *A) {
    if (!e || !w || !A || ip_begin < e->ip0 || ip_count < 0 || ip_begin + ip_count > e->ip0 + e->ip_count) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state == jaicov_engine::ST_NEW) FAIL(e->err, JAICOV_ERR_BAD_STATE, "set_parameters first");
    HIPE(e->err, hipSetDevice(e->device));
    TRY(engine_ensure_rows(e));
    const size_t S = (size_t)e->p.n_ip;
    std::vector<double> hA((size_t)2 * KROW * S), hW(2 * S);
    HIPE(e->err, hipMemcpyAsync(hA.data(), e->d_rowsA, hA.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPE(e->err, hipMemcpyAsync(hW.data(), e->d_rowsW, hW.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPE(e->err, hipStreamSynchronize(e->stream));
    for (int i = 0; i < ip_count; i++) {
        const size_t ip = e->ip_old2new.empty() ? (size_t)ip_begin + i : (size_t)e->ip_old2new[(size_t)ip_begin + i];
        w[2 * i] = hW[ip]; w[2 * i + 1] = hW[S + ip];
        for (int r = 0; r < 2; r++)
            for (int l = 0; l < KROW; l++) A[((size_t)2 * i + r) * KROW + l] = hA[(size_t)(2 * l + r) * S + ip];
    }
    return JAICOV_OK;
}

extern "C" int jaicov_neq_set_profiling(jaicov_engine *e, int enable) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    e->solver.profile = enable != 0;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_kernel_stats(jaicov_engine *e, double *stats, int32_t n, int reset) {
    if (!e || !stats || n < 3) return JAICOV_ERR_BAD_ARGUMENT;
    stats[0] = e->solver.stat_launches; stats[1] = e->solver.stat_ms; stats[2] = e->solver.stat_flops;
    if (n >= 6) { stats[3] = e->dm_stat_passes; stats[4] = e->dm_stat_ms; stats[5] = e->dm_stat_flops; }
    if (n >= 10) {   // health of the dataflow factorisation since create (never reset): see jaicov_neq.h
        stats[6] = (double)e->flow_retries;
        const FlowCounters &c = e->solver.flow.counters(), &cS = e->solverS.flow.counters();
        stats[7] = (double)(c.stale_events + cS.stale_events);
        stats[8] = (double)(c.stale_confirmed + cS.stale_confirmed);
        stats[9] = (double)(c.rescued + cS.rescued);
    }
    if (n >= 11) stats[10] = e->last_refine_correction;
    if (n >= 12) stats[11] = (double)e->refine_steps;      // refinement steps per solve the engine actually runs (option `refinement`, clamped)
    if (n >= 13) stats[12] = (double)e->pp.cw;             // columns of one LDS strip of the point x point gather (chosen at create from the scene)
    if (reset) e->solver.stat_launches = e->solver.stat_ms = e->solver.stat_flops = e->dm_stat_passes = e->dm_stat_ms = e->dm_stat_flops = 0.0;
    return JAICOV_OK;
}

extern "C" int jaicov_neq_create_timings(jaicov_engine *e, double *ms, int32_t n) {
    if (!e || !ms) return JAICOV_ERR_BAD_ARGUMENT;
    for (int i = 0; i < n && i < CREATE_COUNT; i++) ms[i] = e->create_ms[i];
    return JAICOV_OK;
}

// diagnostic / parity hook: the cached inverse dispersion inv(D) of image block `block` (DOPG:82-86 caches sigma0^2 inv(D / sigma0^2),
// which is sigma0^2 times this), m x m row-major in the CALLER's order of the block's observations
extern "C" int jaicov_neq_get_block_weight(jaicov_engine *e, int32_t block, double *out, size_t len) {
    if (!e || !out) return JAICOV_ERR_BAD_ARGUMENT;
    if (!e->h_caller_block.empty()) {      // the engine's internal blocks are the images; find the caller's
        int internal = -1;
        for (size_t g = 0; g < e->h_caller_block.size(); g++)
            if (e->h_caller_block[g] == block) internal = (int)g;
        block = internal;
    }
    if (block < 0 || block >= (int)e->h_blk_mine.size() || !e->h_blk_mine[block]) FAIL(e->err, JAICOV_ERR_BAD_ARGUMENT, "no such image block on this engine");
    const int b = e->h_blk_ip_begin[block], mpts = e->h_blk_ip_begin[block + 1] - b, m = 2 * mpts;
    if (len != (size_t)m * m) FAIL(e->err, JAICOV_ERR_BAD_ARGUMENT, "len must be (2 * points of the block)^2");
    HIPE(e->err, hipSetDevice(e->device));
    if (e->h_blk_w_off[block] < 0) FAIL(e->err, JAICOV_ERR_BAD_ARGUMENT, "this block has no dispersion of its own");
    std::vector<double> w((size_t)m * m);
    HIPE(e->err, hipMemcpy(w.data(), e->p.blk_w + e->h_blk_w_off[block], w.size() * sizeof(double), hipMemcpyDeviceToHost));
    const int32_t *perm = e->h_perm_local.empty() ? nullptr : e->h_perm_local.data() + b;
    for (int i = 0; i < m; i++) {
        const int si = perm ? 2 * perm[i >> 1] + (i & 1) : i;
        for (int j = 0; j < m; j++) {
            const int sj = perm ? 2 * perm[j >> 1] + (j & 1) : j;
            out[(size_t)si * m + sj] = w[(size_t)i * m + j];
        }
    }
    return JAICOV_OK;
}

extern "C" int jaicov_neq_last_timings(jaicov_engine *e, double *ms, int32_t n) {
    if (!e || !ms) return JAICOV_ERR_BAD_ARGUMENT;
    for (int i = 0; i < n && i < T_COUNT; i++) ms[i] = e->timings[i];
    return JAICOV_OK;
}

// BundleAdjustment.interrupt() (BA:1455-1457): may be called from another thread while estimate() runs
extern "C" int jaicov_neq_cancel(jaicov_engine *e) {
    if (!e) return JAICOV_ERR_BAD_ARGUMENT;
    e->cancel.store(1);
    return JAICOV_OK;
}
