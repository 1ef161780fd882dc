// launchers.h -- the one declaration of every free function that one .hip file defines and another calls, and of the structs such a
// call passes by value.  The defining file and every caller include it: a changed signature is a compile error, not garbage in a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ba_kernels.h"

namespace jaicov {

// rows.hip
hipError_t launch_rows(hipStream_t s, const DevProblem &p, const double *vals, int ip0, int count, double *rowsA, double *rowsW);
// assemble.hip
hipError_t launch_assemble_small(hipStream_t s, const DevProblem &p, const int32_t *seg_begin, const int32_t *seg_end, int n_seg,
                                 const double *rowsA, const double *rowsW, double sigma2, double *N, double *n);
hipError_t launch_assemble_blocks(hipStream_t s, const DevProblem &p, const int32_t *blk_list, int n_list, int max_m, const int32_t *ip_list,
                                  int n_ip_list, const double *rowsA, const double *rowsW, double *T, double sigma2, double *N, double *n,
                                  const PPGather &pp, const SchurBufs &sb, double *cc_partial, hipStream_t side, hipEvent_t ev_fork,
                                  hipEvent_t ev_join);
hipError_t launch_shared_groups(hipStream_t s, const DevProblem &p, const double *vals, double sigma2, double *N, double *n, const double *dx,
                                double *omega);
hipError_t launch_omega(hipStream_t s, const DevProblem &p, const uint8_t *in_block, int ip0, int count, const int32_t *blk_list, int n_list,
                        int max_m, const double *rowsA, const double *rowsW, const double *dx, double sigma2, double *vbuf, double *omega);
// schur.hip
hipError_t launch_schur_eliminate(hipStream_t s, const DevProblem &p, const int32_t *blk_list, int n_list, int max_m, const int32_t *ip_list,
                                  int n_ip_list, const double *rowsA, const double *rowsW, double *T, double sigma2, double lambda,
                                  double *Ubuf, double *Linv, double *G, double *Pp, int *info, double *diagcorr, double *xq,
                                  const PPGather *det_pp, double *Ug);
hipError_t launch_schur_tfix(hipStream_t s, const DevProblem &p, const int32_t *ip_list, int n_ip_list, const double *Ubuf, const double *G,
                             double sigma2, double *T);
hipError_t launch_schur_backsub(hipStream_t s, const DevProblem &p, const int32_t *blk_list, int n_list, const double *Ubuf, const double *Linv,
                                const double *vbuf, double *xE);
hipError_t launch_schur_expand_f(hipStream_t s, const DevProblem &p, const int32_t *blk_list, int n_list, const double *rowsA,
                                 const double *Ubuf, const double *Linv, const double *G, double *F, long ldf);
// refine.hip
struct RefineBorder {       // datum border of the system, d <= 7 (by value: 7 * 2 doubles)
    double kappa[7];        // unscaled multipliers (dx[0..d))
    double rk[7];           // scaled border residual  r_k = -R (B dx)
};
hipError_t launch_residual_dd(hipStream_t s, const double *N, long ld, int U, int d, int order_pad, const double *x, const double *n,
                              const double *V, const double *Braw, const double *Bh, long bstride, const RefineBorder &bd, double *P,
                              double *rhs);
// dense.hip: the bench hooks behind jaicov_debug_diag_bench, _mfma_peak and _cumask (debug.hip)
hipError_t diag_kernel_bench(int dbg, int iters, float *ms_out);
hipError_t mfma_peak_bench(int blocks, int iters, float *ms_out, double *tflops);
hipError_t cumask_bench(const uint32_t *mask, int blocks, int iters, float *ms_out, double *tflops);
// engine.hip: row-major lower square (leading dimension ld, order U) <-> packed ('U' column-major == row-major lower packed)
void launch_pack(hipStream_t s, const double *M, long ld, int U, double *ap);
void launch_unpack(hipStream_t s, const double *ap, long ld, int U, double *M);

}  // namespace jaicov
