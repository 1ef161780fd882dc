// include/jaicov_dense.h: the stand-alone dense calls, which need no engine.  gfx950 only.
#include <stdio.h>

#include <string>

#include "../../include/jaicov_dense.h"
#include "dense.h"
#include "gemm_f64.h"
#include "launchers.h"
#include "status.h"

using namespace jaicov;

// identity on the leading mp x mp square (leading dimension ld); grid (ceil(mp/256), mp)
__global__ void fill_identity_kernel(double *__restrict__ L, long ld, int mp) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= mp) return;
    L[(long)i * ld + j] = (i == j) ? 1.0 : 0.0;
}

// stand-alone dense SPD solve / inverse (MX.solve / MX.inv on UpperSPDPackMatrix, MX:239-264,304-324)
extern "C" int jaicov_dense_spd_solve_packed(int32_t n, double *ap, double *b, int32_t nrhs, int32_t invert, double *ms_out) {
    if (n <= 0 || !ap || nrhs < 0 || nrhs > DENSE_MAX_RHS || (nrhs > 0 && !b)) return JAICOV_ERR_BAD_ARGUMENT;
    std::string err;
    int rc = check_device(err);
    if (rc) return rc;
    DevStream stream;                  // first, so that the solver and the buffers go before the stream does
    if (stream.create() != hipSuccess) return JAICOV_ERR_DEVICE;
    const hipStream_t s = stream.get();
    const int np = ((n + 127) / 128) * 128;
    DenseSolver ds;
    DevBuf<double> ap_store, Y_store;
    DevEvent ev0, ev1;
    const size_t len = (size_t)n * (n + 1) / 2;
    if (ev0.create() != hipSuccess || ev1.create() != hipSuccess) return JAICOV_ERR_DEVICE;
    const hipEvent_t e0 = ev0.get(), e1 = ev1.get();
    if (ds.init(s, np, invert != 0, true) != hipSuccess || ap_store.reserve(len) != hipSuccess ||
        Y_store.reserve((size_t)DENSE_MAX_RHS * np) != hipSuccess)
        return JAICOV_ERR_OUT_OF_MEMORY;
    double *d_ap = ap_store.get(), *d_Y = Y_store.get();
    hipMemcpyAsync(d_ap, ap, len * sizeof(double), hipMemcpyHostToDevice, s);
    int info = 0;
    for (int attempt = 0;; attempt++) {      // an abandoned dataflow factorisation (-9) is repeated: the packed input is still there
        // identity padding, then unpack the lower triangle
        hipLaunchKernelGGL(fill_identity_kernel, dim3((np + 255) / 256, np), dim3(256), 0, s, ds.L, ds.ld, np);
        launch_unpack(s, d_ap, ds.ld, n, ds.L);
        hipMemsetAsync(ds.rhs_row(0), 0, (size_t)128 * ds.ld * sizeof(double), s);
        for (int q = 0; q < nrhs; q++) hipMemcpyAsync(ds.rhs_row(q), b + (size_t)q * n, n * sizeof(double), hipMemcpyHostToDevice, s);
        hipEventRecord(e0, s);
        if (ds.potrf() != hipSuccess) { info = -1; break; }
        if (nrhs > 0) ds.backsolve_aug(d_Y, np, nrhs);
        if (invert) {
            ds.trtri();
            ds.lauum();
        }
        hipEventRecord(e1, s);
        info = ds.fetch_info();
        if (info == -9 && attempt < 2) {
            fprintf(stderr, "jaicov: factorisation abandoned on the device (a wait ran into its time limit); repeating it (%d)\n", attempt + 1);
            continue;
        }
        break;
    }
    if (info < 0) return JAICOV_ERR_DEVICE;
    if (info != 0) return JAICOV_ERR_SINGULAR;
    for (int q = 0; q < nrhs; q++) hipMemcpyAsync(b + (size_t)q * n, d_Y + (size_t)q * np, n * sizeof(double), hipMemcpyDeviceToHost, s);
    if (invert) {
        launch_pack(s, ds.Q, ds.ld, n, d_ap);
        hipMemcpyAsync(ap, d_ap, len * sizeof(double), hipMemcpyDeviceToHost, s);
    }
    const bool ok = hipStreamSynchronize(s) == hipSuccess;
    if (ms_out) { float ms = 0; hipEventElapsedTime(&ms, e0, e1); *ms_out = ms; }
    return ok ? JAICOV_OK : JAICOV_ERR_DEVICE;
}

// C (M x N row-major) = alpha * op(A) op(B) + beta * C on the device, host buffers in/out (kernel parity + timing)
extern "C" int jaicov_dense_gemm(int32_t alay, int32_t blay, int32_t M, int32_t N, int32_t K, double alpha, const double *A,
                                 int64_t lda, const double *B, int64_t ldb, double beta, double *C, int64_t ldc,
                                 int32_t lower_only, int32_t kmode, int32_t repeats, double *ms_out) {

    if (M % 128 || N % 128 || K % 16 || M <= 0 || N <= 0 || K <= 0 || !A || !B || !C) return JAICOV_ERR_BAD_ARGUMENT;
    if (alpha == 0.0) return JAICOV_ERR_BAD_ARGUMENT;      // gemm_f64_plan refuses it: the kernel forms (beta/alpha) C
    std::string err;
    int rc = check_device(err);
    if (rc) return rc;
    const size_t sa = (size_t)(alay == LAY_KC ? M : K) * lda, sb = (size_t)(blay == LAY_KC ? N : K) * ldb, sc = (size_t)M * ldc;
    DevBuf<double> A_store, B_store, C_store;
    DevEvent ev0, ev1;
    if (A_store.reserve(sa) != hipSuccess || B_store.reserve(sb) != hipSuccess || C_store.reserve(sc) != hipSuccess) return JAICOV_ERR_OUT_OF_MEMORY;
    if (ev0.create() != hipSuccess || ev1.create() != hipSuccess) return JAICOV_ERR_DEVICE;
    double *dA = A_store.get(), *dB = B_store.get(), *dC = C_store.get();
    const hipEvent_t e0 = ev0.get(), e1 = ev1.get();
    hipMemcpy(dA, A, sa * 8, hipMemcpyHostToDevice);
    hipMemcpy(dB, B, sb * 8, hipMemcpyHostToDevice);
    hipMemcpy(dC, C, sc * 8, hipMemcpyHostToDevice);
    GemmArgs g{};
    g.A = dA; g.B = dB; g.C = dC; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.alpha = alpha; g.beta = beta; g.lower_only = lower_only; g.kmode = kmode;
    hipError_t he = gemm_f64(nullptr, alay, blay, g);
    hipMemcpy(C, dC, sc * 8, hipMemcpyDeviceToHost);
    if (repeats > 0) {
        hipEventRecord(e0, nullptr);
        for (int r = 0; r < repeats; r++) gemm_f64(nullptr, alay, blay, g);
        hipEventRecord(e1, nullptr);
        hipEventSynchronize(e1);
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        if (ms_out) *ms_out = ms / repeats;
    }
    he = he == hipSuccess ? hipDeviceSynchronize() : he;
    return he == hipSuccess ? JAICOV_OK : JAICOV_ERR_DEVICE;
}
