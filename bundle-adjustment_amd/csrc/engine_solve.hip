// jaicov_neq_solve (one call = one Solve, its stages in the order they run) and jaicov_neq_estimate, the LM loop over build, solve,
// omega and update; with the glue kernels that only the solve launches.  gfx950 only.
#include <math.h>
#include <stdio.h>

#include <algorithm>

#include "batchinv.h"
#include "datum.h"
#include "engine_state.h"
#include "gemm_f64.h"
#include "launchers.h"
#include "small_inverse.h"

static const double EPS53 = 1.1102230246251565e-16;   // Constant.EPS = 2^-53 (Constant.java:68-75)

// M = V N V + Bh' Bh on the unknown block (lower part), identity on border and padding.  Bh: [d][bstride]
__global__ __launch_bounds__(256) void scale_copy_kernel(const double *__restrict__ N, long ldN, double *__restrict__ M,
                                                         long ld, int U, int Upad, int d, const double *__restrict__ V,
                                                         const double *__restrict__ Bh, int bstride, int c_begin, int c_end) {
    const int j = c_begin + blockIdx.x * 256 + threadIdx.x;   // columns [c_begin, c_end)
    const int i = blockIdx.y;
    if (j > i || j >= c_end) return;
    double v;
    if (i < d || i >= U || j < d) v = (i == j) ? 1.0 : 0.0;
    else {
        v = V[i] * N[(long)i * ldN + j] * V[j];
        for (int a = 0; a < d; a++) v += Bh[(long)a * bstride + i] * Bh[(long)a * bstride + j];
    }
    M[(long)i * ld + j] = v;
}

__global__ void scale_vec_kernel(const double *n, const double *V, double *out, int U, int Upad, int d) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Upad) return;
    out[c] = (c >= d && c < U) ? V[c] * n[c] : 0.0;
}

// final cofactor: Qxx[i][j] = V_i V_j (Q[i][j] - sum_a G[a][i] H[a][j]) on the unknown block, border from F, E.
// G: [d][gs]; H, F: [d][Upad]; E: [d][d].  Lower part (j <= i) of the leading `order` rows only.
__global__ __launch_bounds__(256) void qfix_kernel(double *__restrict__ Q, long ld, int U, int Upad, int d,
                                                   const double *__restrict__ V, const double *__restrict__ G, long gs,
                                                   const double *__restrict__ H, const double *__restrict__ F,
                                                   const double *__restrict__ E, int order) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j > i || j >= order) return;
    double v;
    if (i >= U) v = 0.0;
    else if (i < d) v = E[i * d + j];
    else if (j < d) v = F[(long)j * Upad + i];
    else {
        v = Q[(long)i * ld + j];
        for (int a = 0; a < d; a++) v -= G[(long)a * gs + i] * H[(long)a * Upad + j];
        v *= V[i] * V[j];
    }
    Q[(long)i * ld + j] = v;
}

// Full cofactor matrix from the inverse of the EO-reduced system (JAICOV_INVERT_FULL_EXPANDED):
//   rows / columns < e0        Qr (the reduced inverse, final: unscaled, border included)
//   EO row e0 + r, column < e0   T1[r][c] = -(F Q_RR)[r][c]
//   EO row, EO column            T2 = -(T1 F') (lower) + N_EE^-1 on the 6 x 6 diagonal blocks, N_EE^-1 = L_E^-T L_E^-1
// lower part (j <= i) of the leading U rows of Qf.
__global__ __launch_bounds__(256) void expand_cofactor_kernel(double *__restrict__ Qf, long ldf, int U, int e0,
                                                              const double *__restrict__ Qr, long ldr,
                                                              const double *__restrict__ T1, long ld1,
                                                              const double *__restrict__ T2, long ld2,
                                                              const double *__restrict__ Linv) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j > i || i >= U) return;
    double v;
    if (i < e0) v = Qr[(long)i * ldr + j];
    else if (j < e0) v = T1[(long)(i - e0) * ld1 + j];
    else {
        const int ri = i - e0, rj = j - e0;
        v = T2[(long)ri * ld2 + rj];
        if (ri / 6 == rj / 6) {
            const double *Li = Linv + (long)(ri / 6) * 36;
            const int a = ri % 6, b = rj % 6;
            for (int m = a > b ? a : b; m < 6; m++) v += Li[6 * m + a] * Li[6 * m + b];
        }
    }
    Qf[(long)i * ldf + j] = v;
}

// buffers of the inverse (W = L^-1 and Q, two squares of the solver's order) of the solver that factorises; for the effective mode
// FULL_EXPANDED also the Q of the full-order solver, where the expanded matrix lives
int jaicov::ensure_inverse_buffers(jaicov_engine *e, bool reduced_system, int mode) {
    HIPE(e->err, (reduced_system ? e->solverS : e->solver).reserve_inverse(true));
    if (mode == JAICOV_INVERT_FULL_EXPANDED) HIPE(e->err, e->solver.reserve_inverse(false));
    return JAICOV_OK;
}

// the expansion's workspace is the reduced solver's W square: F and T1 ([6 images, padded] x order) and T2 must fit (they do
// unless the exterior orientations outnumber the other unknowns several times over: then the literal route is taken)
// *I6p: EO unknowns of all images, padded; *Up: padded order of the reduced system
bool jaicov::expansion_fits(const jaicov_engine *e, size_t *I6p, size_t *Up) {
    *I6p = ((size_t)6 * e->p.n_images + 127) / 128 * 128;
    *Up = (size_t)e->solverS.nfact;
    return *I6p * (2 * *Up + *I6p) <= (size_t)e->solverS.n * e->solverS.ld;
}

// FULL_EXPANDED is FULL wherever the expansion cannot be done: no EO pre-elimination, or an engine that sees a shard of the images
// and whose caller has not promised to sum the expansion's inputs over the ranks (engine option expansion_exchange)
int jaicov::effective_invert(const jaicov_engine *e, int invert) {
    if (invert != JAICOV_INVERT_FULL_EXPANDED) return invert;
    if (!(e->schur_ok && (e->all_images || e->opts.expansion_exchange != 0) && e->solverS_ready)) return JAICOV_INVERT_FULL;
    size_t I6p, Up;
    return expansion_fits(e, &I6p, &Up) ? invert : JAICOV_INVERT_FULL;
}

// ---- one call of jaicov_neq_solve: what its stages share, then the stages in the order they run ------------------------------
struct Solve {
    jaicov_engine *const e;
    const bool schur;                   // the EO-reduced system is at hand
    const int U, d, Upad;               // order of the system that is factorised (reduced: points, IO, distortion; or full); rank of the datum border; ld of N, V, B, rhs
    DenseSolver &slv;
    const int Up, vs;                   // padded order of the factorised system == stride between the solution vectors (the solver's order)
    const long ld;
    int invert = 0;                     // the effective mode
    bool expand = false;                // ... is FULL_EXPANDED: all of Qxx from the reduced inverse
    std::vector<double> Bh, X, delta0;  // datum rows R B V [8][Upad]; y~ and G^ [d + 1][vs]; the correction of the device's own refinement step
    double R[7] = {1, 1, 1, 1, 1, 1, 1}, Sinv[49];
    bool fast_refined = false;          // d = 0: the first refinement step went out behind the substitution, without the host
    float refine_ms = 0.f;
    explicit Solve(jaicov_engine *eng)
        : e(eng), schur(e->schur_active), U(schur ? e->e0 : e->U), d(e->d), Upad(e->Upad), slv(schur ? e->solverS : e->solver),
          Up(slv.nfact), vs(Up), ld(slv.ld) {}

    double border_dot(int a, const double *v) const {      // Bh[a] . v over the unknowns
        double s = 0.0;
        for (int c = d; c < U; c++) s += Bh[(size_t)a * Upad + c] * v[c];
        return s;
    }
    void border_multipliers(const double *v, const double *rk, double *k) const {      // k = S^-1 (Bh v - rk)
        double t[7];
        for (int a = 0; a < d; a++) t[a] = border_dot(a, v) - rk[a];
        for (int a = 0; a < d; a++) {
            double s = 0.0;
            for (int b = 0; b < d; b++) s += Sinv[a * d + b] * t[b];
            k[a] = s;
        }
    }

    int solve_mode(int requested) {
        invert = effective_invert(e, requested);
        if (invert == JAICOV_INVERT_FULL_EXPANDED && !schur) invert = JAICOV_INVERT_FULL;     // the system at hand was assembled unreduced
        expand = invert == JAICOV_INVERT_FULL_EXPANDED;
        if (schur && invert == JAICOV_INVERT_FULL)
            FAIL(e->err, JAICOV_ERR_BAD_STATE, "the normal equations were assembled with the EO blocks pre-eliminated: call "
                                          "jaicov_neq_prepare_inverse(e, JAICOV_INVERT_FULL) before the build whose solve shall invert");
        slv.profile = e->solver.profile;
        slv.flops_order = (double)U;
        // normally done by prepare_inverse(); a host that did not announce the final pass pays the allocation here
        return invert ? ensure_inverse_buffers(e, schur, invert) : JAICOV_OK;
    }
    // V to the host, scaled + row-normalised datum rows Bh = R B V (NES:82-91 scaling of the border)
    // This round trip stays even where nothing of it is needed before the factorisation (d = 0): with the host running ahead of
    // the assembly -- enqueuing the factorisation and spinning in its residency handshake while the assembly kernels still run --
    // every pass was 0.6 ms SLOWER (assembly +0.19, factorisation +0.4; measured A/B in round 3).
    // What d = 0 does save is the round trip between the substitution and the first refinement step (factor_and_substitute).
    int border_rows() {
        int hinfo = 0;   // status of the per-image EO eliminations, fetched in the same round trip
        HIPE(e->err, hipMemcpyAsync(e->h_V.data(), e->d_V, Upad * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        if (schur) HIPE(e->err, hipMemcpyAsync(&hinfo, e->sb.info, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        HIPE(e->err, hipStreamSynchronize(e->stream));
        if (hinfo != 0) FAIL(e->err, JAICOV_ERR_SINGULAR, "exterior orientation block of image " + std::to_string(hinfo - 1000000) + " is not positive definite");
        Bh.assign((size_t)8 * Upad, 0.0);
        for (int a = 0; a < d; a++) {
            double s = 0.0;
            for (int c = d; c < U; c++) {
                const double v = e->hB[(size_t)a * Upad + c] * e->h_V[c];
                Bh[(size_t)a * Upad + c] = v;
                s += v * v;
            }
            if (!(s > 0.0)) FAIL(e->err, JAICOV_ERR_SINGULAR, "empty datum condition row");
            R[a] = 1.0 / sqrt(s);
            for (int c = d; c < U; c++) Bh[(size_t)a * Upad + c] *= R[a];
        }
        if (d > 0) HIPE(e->err, hipMemcpyAsync(e->d_B, Bh.data(), (size_t)d * Upad * sizeof(double), hipMemcpyHostToDevice, e->stream));
        HIPE(e->err, hipEventRecord(e->ev[EV_BORDER].get(), e->stream));
        return JAICOV_OK;
    }
    // ---- iterative refinement (refine.hip): residual of the unscaled bordered system in two-fold precision, one forward and
    // one backward substitution with the factor at hand per step.  The correction of the border follows the same rank-d
    // algebra as the step itself with r_y = V rho_x, r_k = R rho_kappa:  delta0 = M^-1 (r_y + Bh' r_k),
    // dk = S^-1 (Bh delta0 - r_k),  dy = delta0 - G^ dk.
    // The device's part of a step: refine_begin, then whatever gives d_dx its value, then refine_step.
    int refine_begin() {
        const int nbk = Up / 128;
        HIPE(e->err, e->refP.reserve((size_t)nbk * nbk * 256));      // ahead of the event: an allocation is no part of the step's time
        HIPE(e->err, hipEventRecord(e->ev_r0.get(), e->stream));
        return JAICOV_OK;
    }
    // residual of d_dx, delta = M^-1 residual, and delta on its way to the host (complete once the stream has been synchronised)
    int refine_step(const RefineBorder &bd, std::vector<double> &delta) {
        double *d_rhs = e->d_ref, *d_tmp = e->d_ref + Upad, *d_delta = e->d_ref + 2 * (size_t)Upad;
        HIPE(e->err, launch_residual_dd(e->stream, e->d_N, (long)Upad, U, d, Up, e->d_dx, e->d_n, e->d_V, e->d_Braw, e->d_B, (long)Upad,
                                   bd, e->refP.get(), d_rhs));
        HIPE(e->err, slv.solve_rhs(d_rhs, d_tmp, d_delta));
        HIPE(e->err, hipEventRecord(e->ev_r1.get(), e->stream));
        delta.assign((size_t)Up, 0.0);
        HIPE(e->err, hipMemcpyAsync(delta.data(), d_delta, delta.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
        return JAICOV_OK;
    }
    // a completed step: its time, dx += the correction that belongs to delta (d = 0: V delta), max |correction| / max |dx|
    int apply_correction(const RefineBorder &bd, const std::vector<double> &dl, double *dx_out) {
        float ms1 = 0.f;
        hipEventElapsedTime(&ms1, e->ev_r0.get(), e->ev_r1.get());
        refine_ms += ms1;
        double dk[7] = {0, 0, 0, 0, 0, 0, 0};
        border_multipliers(dl.data(), bd.rk, dk);
        double cmax = 0.0, xmax = 0.0;
        for (int c = d; c < U; c++) {
            double dy = dl[c];
            for (int a = 0; a < d; a++) dy -= X[(size_t)(1 + a) * vs + c] * dk[a];
            const double corr = e->h_V[c] * dy;
            if (!std::isfinite(corr)) FAIL(e->err, JAICOV_ERR_NOT_FINITE, "non-finite refinement step");
            dx_out[c] += corr;
            cmax = std::max(cmax, fabs(corr)); xmax = std::max(xmax, fabs(dx_out[c]));
        }
        for (int a = 0; a < d; a++) dx_out[a] += R[a] * dk[a];
        e->last_refine_correction = xmax > 0.0 ? cmax / xmax : 0.0;
        return JAICOV_OK;
    }
    // right-hand sides: row 0 = V n, rows 1..d = Bh.  They are the extra rows below the matrix, so the factorisation
    // itself carries out the forward substitution (dense.hip).
    // dataflow factorisation: the tile kernel reads N itself and scales on the fly (no copy of the matrix at all);
    // stream-scheduled one: the columns of the first panel go first, together with the right-hand sides; the panel then
    // factors on its stream while the rest of the matrix is still being scaled and copied (0.4 ms at config 4).
    // (in a loop: a dataflow factorisation that was abandoned -- cholflow.hip, "Visibility": a wait ran into its time limit, seen
    // about once in 1 000 factorisations at config 4 -- is repeated; N, V and the datum rows are untouched by it)
    int factor_and_substitute() {
        const int nrhs = d + 1;
        const bool fused = slv.flow.ready();
        const int c1 = std::min(slv.first_panel_cols(), Up);
        int info = 0;
        for (int attempt = 0;; attempt++) {
            HIPE(e->err, slv.begin_refactor());      // the side stream's premultiply of the last pass may still read the old factor: nothing writes L before this
            if (!fused)
                hipLaunchKernelGGL(scale_copy_kernel, dim3((c1 + 255) / 256, Up), dim3(256), 0, e->stream, e->d_N, (long)Upad, slv.L, ld, U,
                                   Up, d, e->d_V, e->d_B, Upad, 0, c1);
            HIPE(e->err, hipMemsetAsync(slv.rhs_row(0), 0, (size_t)128 * ld * sizeof(double), e->stream));
            hipLaunchKernelGGL(scale_vec_kernel, dim3((Up + 255) / 256), dim3(256), 0, e->stream, e->d_n, e->d_V, slv.rhs_row(0), U, Up, d);
            if (d > 0)
                HIPE(e->err, hipMemcpy2DAsync(slv.rhs_row(1), (size_t)ld * sizeof(double), e->d_B, (size_t)Upad * sizeof(double),
                                         (size_t)Up * sizeof(double), (size_t)d, hipMemcpyDeviceToDevice, e->stream));
            HIPE(e->err, hipEventRecord(e->ev_first.get(), e->stream));
            if (!fused && c1 < Up)
                hipLaunchKernelGGL(scale_copy_kernel, dim3((Up - c1 + 255) / 256, Up), dim3(256), 0, e->stream, e->d_N, (long)Upad, slv.L,
                                   ld, U, Up, d, e->d_V, e->d_B, Upad, c1, Up);
            HIPE(e->err, hipEventRecord(e->ev_all.get(), e->stream));
            if (fused) slv.flow.set_source(e->d_N, (long)Upad, e->d_V, e->d_B, Upad, d, U);
            HIPE(e->err, slv.potrf(e->ev_first.get(), e->ev_all.get()));
            HIPE(e->err, hipEventRecord(e->ev[EV_FACTORED].get(), e->stream));
            HIPE(e->err, slv.backsolve_aug(e->d_G, vs, nrhs));           // G <- L^-T (L^-1 Y)   (row 0: y~, rows 1..d: G^)
            HIPE(e->err, hipEventRecord(e->ev[EV_SUBSTITUTED].get(), e->stream));
            X.assign((size_t)nrhs * vs, 0.0);
            HIPE(e->err, hipMemcpyAsync(X.data(), e->d_G, X.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
            fast_refined = false;
            if (d == 0 && e->refine_steps >= 1 && !e->sim_built) {
                // first refinement step without the host: dx = V y on the device, residual of the unscaled system in two-fold precision,
                // forward + backward substitution (refine.hip, dense.hip); the correction comes back together with y
                TRY(refine_begin());
                hipLaunchKernelGGL(scale_vec_kernel, dim3((Up + 255) / 256), dim3(256), 0, e->stream, e->d_G, e->d_V, e->d_dx, U, Up, 0);   // dx = V y
                TRY(refine_step(RefineBorder{}, delta0));
                fast_refined = true;
            }
            info = slv.fetch_info();
            if (info == -9 && attempt < 2) {
                ++e->flow_retries;
                fprintf(stderr, "jaicov: factorisation abandoned on the device (a wait ran into its time limit); repeating it (%d)\n", attempt + 1);
                continue;
            }
            break;
        }
        if (info < 0) FAIL(e->err, JAICOV_ERR_DEVICE, "factorisation did not complete on the device (code " + std::to_string(info) + ")");
        if (info != 0) FAIL(e->err, JAICOV_ERR_SINGULAR, "normal-equation matrix is singular / not positive definite at pivot " + std::to_string(info));
        return JAICOV_OK;
    }
    // ---- rank-d border algebra on the host ---------------------------------------------------------------------
    int border_step(double *dx_out) {
        double Sm[49], kh[7];
        std::vector<double> y(X.begin(), X.begin() + vs);
        if (d > 0) {
            for (int a = 0; a < d; a++)
                for (int b = 0; b < d; b++) Sm[a * d + b] = border_dot(a, &X[(size_t)(1 + b) * vs]);
            if (!small_inverse(d, Sm, Sinv)) FAIL(e->err, JAICOV_ERR_SINGULAR, "datum conditions are linearly dependent");
            const double no_rk[7] = {0, 0, 0, 0, 0, 0, 0};
            border_multipliers(X.data(), no_rk, kh);
            for (int c = d; c < U; c++) {
                double s = 0.0;
                for (int a = 0; a < d; a++) s += X[(size_t)(1 + a) * vs + c] * kh[a];
                y[c] -= s;
            }
        }
        for (int c = 0; c < U; c++) dx_out[c] = c < d ? R[c] * kh[c] : e->h_V[c] * y[c];
        for (int c = 0; c < U; c++)
            if (!std::isfinite(dx_out[c])) FAIL(e->err, JAICOV_ERR_NOT_FINITE, "non-finite step");
        return JAICOV_OK;
    }
    // the step the device took on its own (d = 0: no border algebra), then the others with the host in between
    int refine(double *dx_out) {
        e->last_refine_correction = 0.0;
        if (fast_refined) TRY(apply_correction(RefineBorder{}, delta0, dx_out));
        for (int step = fast_refined ? 1 : 0; step < e->refine_steps && !e->sim_built; step++) {
            RefineBorder bd{};
            for (int a = 0; a < d; a++) {
                long double sacc = 0.0L;
                for (int c = d; c < U; c++) sacc += (long double)e->hB[(size_t)a * Upad + c] * (long double)dx_out[c];
                bd.kappa[a] = dx_out[a];
                bd.rk[a] = (double)(-(long double)R[a] * sacc);
            }
            TRY(refine_begin());
            if (d > 0 && step == 0)
                HIPE(e->err, hipMemcpyAsync(e->d_Braw, e->hB.data(), (size_t)d * Upad * sizeof(double), hipMemcpyHostToDevice, e->stream));
            HIPE(e->err, hipMemcpyAsync(e->d_dx, dx_out, (size_t)U * sizeof(double), hipMemcpyHostToDevice, e->stream));
            std::vector<double> dl;
            TRY(refine_step(bd, dl));
            HIPE(e->err, hipStreamSynchronize(e->stream));
            TRY(apply_correction(bd, dl, dx_out));
        }
        return JAICOV_OK;
    }
    // EO step of every image of this engine: dx_E = L_E^-T U' (w - A_r dx_R), from d_dx into d_xE   (schur.hip)
    int eo_backsub() {
        HIPE(e->err, launch_omega(e->stream, e->p, e->d_in_block, e->ip0, e->ip_count, e->d_blk_list, 0, e->max_m, e->d_rowsA,
                             e->d_rowsW, e->d_dx, 1.0, e->d_vbuf, e->d_omega));
        HIPE(e->err, launch_schur_backsub(e->stream, e->p, e->d_blk_list, e->n_blk_list, e->sb.U, e->sb.Linv, e->d_vbuf, e->d_xE));
        return JAICOV_OK;
    }
    // Round 5: once in ~10 runs of the GPU test-suite a solve returned an EO step of EXACT zeros for every image (N, n and the reduced
    // step correct; 1 200 solves of the same scene alone: never).  The back-substitution kernel cannot produce that from finite
    // operands, so the copy is checked: all zeros -> read again with a blocking copy after a device-wide wait, and say so.
    int eo_zero_step_guard(std::vector<double> &xE) {
        bool all_zero = !e->h_blk_images.empty();
        for (int img : e->h_blk_images)
            for (int k = 0; k < 6 && all_zero; k++) all_zero = xE[(size_t)6 * img + k] == 0.0;
        if (!all_zero) return JAICOV_OK;
        HIPE(e->err, hipDeviceSynchronize());
        HIPE(e->err, hipMemcpy(xE.data(), e->d_xE, xE.size() * sizeof(double), hipMemcpyDeviceToHost));
        bool still = true;
        for (int img : e->h_blk_images)
            for (int k = 0; k < 6 && still; k++) still = xE[(size_t)6 * img + k] == 0.0;
        if (still) {      // the kernel itself left zeros: run the two kernels once more
            TRY(eo_backsub());
            HIPE(e->err, hipStreamSynchronize(e->stream));
            HIPE(e->err, hipMemcpy(xE.data(), e->d_xE, xE.size() * sizeof(double), hipMemcpyDeviceToHost));
        }
        fprintf(stderr, "jaicov: the exterior-orientation step came back as exact zeros; %s\n",
                still ? "the back-substitution was run again" : "a second, blocking copy had the values (the first copy returned before the data)");
        return JAICOV_OK;
    }
    // the EO entries of the step, which the reduced system does not hold
    int eo_entries(double *dx_out) {
        const bool quirk = e->opts.reduced_reference_quirk && invert == JAICOV_INVERT_REDUCED;
        if (schur)
            for (int c = U; c < e->U; c++) dx_out[c] = 0.0;
        // SIMULATION zeroes the right-hand side of the WHOLE system (BA:830-831 `n.zero()`): the eliminated exterior
        // orientations get no step either (their back substitution would use the real misclosures)
        if (schur && e->sim_built) return JAICOV_OK;
        if (schur && quirk) {
            // what the reference's last pass leaves in the EO entries of dx under MatrixInversion.REDUCED (quirk Q1): V_c^2 n_c
            std::vector<double> xq((size_t)6 * e->p.n_images);
            HIPE(e->err, hipMemcpyAsync(xq.data(), e->sb.xq, xq.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
            HIPE(e->err, hipStreamSynchronize(e->stream));
            for (int img : e->h_blk_images)
                for (int k = 0; k < 6; k++) dx_out[e->e0 + 6 * img + k] = xq[(size_t)6 * img + k];
        } else if (schur) {
            HIPE(e->err, hipMemcpyAsync(e->d_dx, dx_out, (size_t)e->U * sizeof(double), hipMemcpyHostToDevice, e->stream));
            TRY(eo_backsub());
            std::vector<double> xE((size_t)6 * e->p.n_images);
            HIPE(e->err, hipMemcpyAsync(xE.data(), e->d_xE, xE.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
            HIPE(e->err, hipStreamSynchronize(e->stream));
            TRY(eo_zero_step_guard(xE));
            for (int img : e->h_blk_images)
                for (int k = 0; k < 6; k++) {
                    dx_out[e->e0 + 6 * img + k] = xE[(size_t)6 * img + k];
                    if (!std::isfinite(xE[(size_t)6 * img + k])) FAIL(e->err, JAICOV_ERR_NOT_FINITE, "non-finite step");
                }
        } else if (quirk) {
            // full-order path (no EO pre-elimination possible): the same quirk from the assembled right-hand side, V_c^2 n_c
            std::vector<double> hn((size_t)e->U);
            HIPE(e->err, hipMemcpyAsync(hn.data(), e->d_n, hn.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
            HIPE(e->err, hipStreamSynchronize(e->stream));
            const int ns = e->n_slots, s_eo = ns - 6 * e->p.n_images;
            for (int sl = s_eo; sl < ns; sl++) {
                const int c = e->h_slot_col[sl];
                if (c >= 0) dx_out[c] = e->h_V[c] * e->h_V[c] * hn[c];
            }
        }
        return JAICOV_OK;
    }
    // FULL: Qxx of all unknowns.  REDUCED on a pre-eliminated system: the inverse of the reduced normal equations,
    // which IS the block of Qxx that belongs to the datum border, points, interior orientation and distortion
    // (MatrixInversion.REDUCED / PRE_ELIMINATION, BA:261-267: solve(N, n, numRows, true) on the reduced system).
    int invert_and_expand() {
        HIPE(e->err, slv.trtri());
        HIPE(e->err, slv.lauum());
        if (e->opts.inverse_refinement >= 0 && Up <= 8192) {
            // One Newton-Schulz step on Q = inv(M) with the residual I - M Q formed exactly (batchinv.hip): M is materialised once more
            // (scaled, with the datum border's term; the factor in slv.L is not needed again before the next factorisation), W is free
            // after lauum(), three more squares are kept with the engine.
            const size_t sq = (size_t)Up * ld;
            HIPE(e->err, e->ns_work.reserve(3 * sq));
            double *ns = e->ns_work.get();
            HIPE(e->err, slv.begin_refactor());
            HIPE(e->err, slv.symmetrize(slv.Q));
            hipLaunchKernelGGL(scale_copy_kernel, dim3((Up + 255) / 256, Up), dim3(256), 0, e->stream, e->d_N, (long)Upad, slv.L, ld, U,
                               Up, d, e->d_V, e->d_B, Upad, 0, Up);
            HIPE(e->err, slv.symmetrize(slv.L));
            HIPE(e->err, newton_schulz_exact(e->stream, Up, ld, slv.L, slv.Q, slv.W, ns, ns + sq, ns + 2 * sq));
        }
        // H = Sinv G^ ; F = R (Sinv G^) V ; E = R (I - Sinv) R
        std::vector<double> H((size_t)8 * Upad, 0.0), F((size_t)8 * Upad, 0.0);
        double E[49];
        for (int a = 0; a < d; a++) {
            for (int c = d; c < U; c++) {
                double s = 0.0;
                for (int b = 0; b < d; b++) s += Sinv[a * d + b] * X[(size_t)(1 + b) * vs + c];
                H[(size_t)a * Upad + c] = s;
                F[(size_t)a * Upad + c] = R[a] * s * e->h_V[c];
            }
            for (int b = 0; b < d; b++) E[a * d + b] = R[a] * ((a == b ? 1.0 : 0.0) - Sinv[a * d + b]) * R[b];
        }
        if (d > 0) {
            HIPE(e->err, hipMemcpyAsync(e->d_H, H.data(), (size_t)d * Upad * sizeof(double), hipMemcpyHostToDevice, e->stream));
            HIPE(e->err, hipMemcpyAsync(e->d_F, F.data(), (size_t)d * Upad * sizeof(double), hipMemcpyHostToDevice, e->stream));
            HIPE(e->err, hipMemcpyAsync(e->d_E, E, (size_t)d * d * sizeof(double), hipMemcpyHostToDevice, e->stream));
        }
        hipLaunchKernelGGL(qfix_kernel, dim3((Up + 255) / 256, Up), dim3(256), 0, e->stream, slv.Q, ld, U, Upad, d,
                           e->d_V, e->d_G + vs, (long)vs, e->d_H, e->d_F, e->d_E, Up);
        return expand ? expand_cofactor() : JAICOV_OK;
    }
    // ---- the full cofactor matrix from the reduced one (schur.hip, blk_expand_f_kernel): workspace = W of the reduced
    //      solver, free again after lauum():  F [6I pad][Up] | T1 = -F Q_RR [6I pad][Up] | T2 = -T1 F' [6I pad][6I pad]
    int expand_cofactor() {
        size_t I6, UpS;
        if (!expansion_fits(e, &I6, &UpS))
            FAIL(e->err, JAICOV_ERR_UNSUPPORTED, "FULL_EXPANDED: more exterior orientations than the workspace holds; use JAICOV_INVERT_FULL");
        const int I6p = (int)I6;
        double *Fm = slv.W, *T1 = Fm + (size_t)I6p * Up, *T2 = T1 + (size_t)I6p * Up;
        const double *LinvAll = e->sb.Linv;
        if (e->all_images) {
            HIPE(e->err, hipMemsetAsync(Fm, 0, (size_t)I6p * Up * sizeof(double), e->stream));
            HIPE(e->err, launch_schur_expand_f(e->stream, e->p, e->d_blk_list, e->n_blk_list, e->d_rowsA, e->sb.U, e->sb.Linv, e->sb.G, Fm, (long)Up));
        } else {      // a shard: F and L_E^-1 of EVERY image, summed over the ranks by the caller (jaicov_neq_expansion_buffer)
            if (!e->exp_ready || e->expF_len != (size_t)I6p * Up + (size_t)36 * e->p.n_images)
                FAIL(e->err, JAICOV_ERR_BAD_STATE, "FULL_EXPANDED on a sharded engine: all-reduce jaicov_neq_expansion_buffer() between accumulate and solve");
            HIPE(e->err, hipMemcpyAsync(Fm, e->expF.get(), (size_t)I6p * Up * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
            // the summed L_E^-1 records are READ from the buffer, never copied over sb.Linv: that array must keep zeros for the
            // foreign images, or the next pass's expansion buffer would carry their stale records into the sum (ADVICE r4, high:
            // a second sharded FULL_EXPANDED pass gave R times the EO cofactors)
            LinvAll = e->expF.get() + (size_t)I6p * Up;
        }
        HIPE(e->err, slv.symmetrize(slv.Q));
        GemmArgs g1{};
        g1.A = Fm; g1.lda = Up; g1.B = slv.Q; g1.ldb = ld; g1.C = T1; g1.ldc = Up;
        g1.M = I6p; g1.N = Up; g1.K = Up; g1.alpha = -1.0; g1.beta = 0.0; g1.kmode = KMODE_FULL;
        HIPE(e->err, gemm_f64(e->stream, LAY_KC, LAY_KC, g1));             // Q_RR symmetric: F Q_RR = F Q_RR'
        GemmArgs g2{};
        g2.A = T1; g2.lda = Up; g2.B = Fm; g2.ldb = Up; g2.C = T2; g2.ldc = I6p;
        g2.M = I6p; g2.N = I6p; g2.K = Up; g2.alpha = -1.0; g2.beta = 0.0; g2.kmode = KMODE_FULL; g2.lower_only = 1;
        HIPE(e->err, gemm_f64(e->stream, LAY_KC, LAY_KC, g2));
        hipLaunchKernelGGL(expand_cofactor_kernel, dim3((e->U + 255) / 256, e->U), dim3(256), 0, e->stream, e->solver.Q, e->solver.ld,
                           e->U, e->e0, slv.Q, ld, T1, (long)Up, T2, (long)I6p, LinvAll);
        return JAICOV_OK;
    }
    // end of the device's work, what the cofactor matrix at hand is, the timings
    int finish() {
        HIPE(e->err, hipEventRecord(e->ev[EV_SOLVED].get(), e->stream));
        HIPE(e->err, hipStreamSynchronize(e->stream));
        if (invert) {
            e->q.valid = true;
            e->q.sigma2 = e->sigma2_acc;
            e->q.lambda = e->lambda_used;
            e->q.vals = e->h_vals;
            jaicov::datum_state_invalidate(e->slot.datum.get());
            e->q.reduced = schur && !expand;
            e->q.order = expand ? e->U : U;
        }
        slv.prof_collect();
        if (schur) {
            e->solver.stat_launches += slv.stat_launches; e->solver.stat_ms += slv.stat_ms; e->solver.stat_flops += slv.stat_flops;
            slv.stat_launches = slv.stat_ms = slv.stat_flops = 0.0;
        }
        float ms;
        hipEventElapsedTime(&ms, e->ev[EV_ACC_BEGIN].get(), e->ev[EV_ROWS].get()); e->timings[T_ROWS] = ms;
        hipEventElapsedTime(&ms, e->ev[EV_ROWS].get(), e->ev[EV_ASSEMBLED].get()); e->timings[T_ASSEMBLY] = ms;
        hipEventElapsedTime(&ms, e->ev[EV_ASSEMBLED].get(), e->ev[EV_BUILT].get()); e->timings[T_FINALIZE] = ms;
        hipEventElapsedTime(&ms, e->ev[EV_BORDER].get(), e->ev[EV_FACTORED].get()); e->timings[T_FACTOR] = ms;
        hipEventElapsedTime(&ms, e->ev[EV_FACTORED].get(), e->ev[EV_SUBSTITUTED].get()); e->timings[T_SOLVE] = ms + refine_ms;   // substitution + refinement steps
        hipEventElapsedTime(&ms, e->ev[EV_SUBSTITUTED].get(), e->ev[EV_SOLVED].get()); e->timings[T_INVERSE] = std::max(0.f, ms - refine_ms);   // the refinement sits between these events: counted under T_SOLVE
        hipEventElapsedTime(&ms, e->ev[EV_ACC_BEGIN].get(), e->ev[EV_SOLVED].get()); e->timings[T_TOTAL] = ms;
        e->state = jaicov_engine::ST_SOLVED;
        return JAICOV_OK;
    }
};

extern "C" int jaicov_neq_solve(jaicov_engine *e, int invert, double *dx_out) {
    if (!e || !dx_out) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state != jaicov_engine::ST_BUILT) FAIL(e->err, JAICOV_ERR_BAD_STATE, "build first");
    HIPE(e->err, hipSetDevice(e->device));
    if (invert < 0 || invert > JAICOV_INVERT_FULL_EXPANDED) return JAICOV_ERR_BAD_ARGUMENT;
    Solve s(e);
    TRY(s.solve_mode(invert));
    TRY(s.border_rows());
    TRY(s.factor_and_substitute());
    TRY(s.border_step(dx_out));
    TRY(s.refine(dx_out));
    TRY(s.eo_entries(dx_out));
    if (s.invert) TRY(s.invert_and_expand());
    return s.finish();
}

// BA.estimateModel (BA:203-387) + updateModel (BA:389-442); inversion modes NONE / FULL / REDUCED (PRE_ELIMINATION = REDUCED:
// the engine pre-eliminates the exterior orientations in every pass whenever the problem allows it)
extern "C" int jaicov_neq_estimate(jaicov_engine *e, const jaicov_estimate_options *o, jaicov_estimate_result *res) {
    if (!e || !o || !res || o->struct_size != sizeof(jaicov_estimate_options)) return JAICOV_ERR_BAD_ARGUMENT;
    if (e->state == jaicov_engine::ST_NEW) FAIL(e->err, JAICOV_ERR_BAD_STATE, "set_parameters first");
    const double SQRT_EPS = sqrt(EPS53);
    if (o->invert < 0 || o->invert > JAICOV_INVERT_FULL_EXPANDED) return JAICOV_ERR_BAD_ARGUMENT;
    // MatrixInversion.FULL: all of Qxx, computed from the EO-reduced system where the engine can (jaicov_neq.h, FULL_EXPANDED)
    const int inv_mode = o->invert == JAICOV_INVERT_FULL ? JAICOV_INVERT_FULL_EXPANDED : o->invert;
    const int max_iter = o->max_iterations;
    auto t0 = std::chrono::steady_clock::now();
    bool deriveFirst = o->lambda0 > 0;
    double adapted = 0.0;
    const double damping = fabs(o->lambda0);
    double maxAbsDx = 0.0, lastValid = 0.0, omega = 0.0;
    int runs = max_iter - 1;
    bool isEstimated = false, complete = false, isConverge = true;
    if (max_iter == 0) { complete = isEstimated = true; adapted = 0; }
    const double sigma2 = o->sigma2apriori > 0 ? o->sigma2apriori : 1.0;
    std::vector<double> dx(e->U > 0 ? e->U : 1);
    int state = 0, iter = 0, rc = JAICOV_OK;
    do {
        auto tp = std::chrono::steady_clock::now();
        maxAbsDx = 0.0;
        iter = max_iter - runs;
        if (deriveFirst) { adapted = damping; deriveFirst = false; }
        jaicov_neq_prepare_inverse(e, isEstimated ? inv_mode : JAICOV_INVERT_NONE);
        rc = jaicov_neq_build(e, sigma2, adapted, o->simulation);
        if (rc == JAICOV_ERR_OUT_OF_MEMORY) { state = -7; break; }
        if (rc) { state = rc == JAICOV_ERR_BAD_ARGUMENT || rc > 0 ? -2 : -1; break; }
        if (e->cancel.exchange(0)) { state = -1; rc = JAICOV_OK; break; }       // BA:240-245: INTERRUPT, flag cleared
        complete = isEstimated;
        rc = jaicov_neq_solve(e, complete ? inv_mode : JAICOV_INVERT_NONE, dx.data());
        if (rc == JAICOV_ERR_OUT_OF_MEMORY) { state = -7; break; }
        if (rc) { state = (rc > 0 || rc == JAICOV_ERR_BAD_ARGUMENT) ? -2 : -1; break; }
        bool rejected = false;
        if (adapted > 0) {
            double alpha = 0.25 * pow(adapted, -0.05);
            alpha = std::min(alpha, 0.75);
            for (auto &v : dx) v *= alpha;
            double prevOmega = omega, curOmega = 0.0;
            if ((rc = jaicov_neq_omega(e, sigma2, dx.data(), &curOmega))) { state = -1; break; }
            prevOmega = prevOmega <= 0 ? 1.7976931348623157e308 : prevOmega;
            const bool lmaConverge = prevOmega >= curOmega;
            omega = curOmega;
            if (lmaConverge) adapted *= 0.2;
            else {
                adapted *= 5.0;
                if (adapted > 1.0 / SQRT_EPS) { adapted = 1.0 / SQRT_EPS; omega = 0.0; }
            }
            if (!lmaConverge) { maxAbsDx = lastValid; rejected = true; }
        }
        if (!rejected) {
            if (complete) {
                if (o->simulation) omega = 0.0;
                else if ((rc = jaicov_neq_omega(e, sigma2, dx.data(), &omega))) { state = -1; break; }
            }
            if ((rc = jaicov_neq_update(e, dx.data(), &maxAbsDx))) { state = -1; break; }
            lastValid = maxAbsDx;
        }
        res->seconds_last_pass = std::chrono::duration<double>(std::chrono::steady_clock::now() - tp).count();
        if (e->cancel.exchange(0)) { state = -1; rc = JAICOV_OK; break; }       // BA:320-325
        if (std::isinf(maxAbsDx) || std::isnan(maxAbsDx)) { state = -2; break; }
        else if (maxAbsDx <= SQRT_EPS && runs > 0 && adapted == 0) isEstimated = true;
        else if (runs-- <= 1) {
            if (complete) isConverge = false;
            isEstimated = true;
        }
        if (isEstimated || adapted <= SQRT_EPS || runs < max_iter * 0.5 + 1) adapted = 0.0;
    } while (!complete);
    if (state == 0) state = isConverge ? 1 : -4;
    res->state = state;
    res->iterations = iter;
    res->omega = omega;
    res->max_abs_dx = maxAbsDx;
    res->final_lambda = adapted;
    res->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return (state == 1 || state == -4 || state == -2 || state == -1) ? (state == -1 && rc ? rc : JAICOV_OK) : rc;
}
