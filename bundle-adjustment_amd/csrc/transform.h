// Internal interface between engine.hip (owner of jaicov_engine) and transform.hip (include/jaicov_transform.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/jaicov_neq.h"
#include "ba_kernels.h"
#include "devbuf.h"

namespace jaicov {

// result of jaicov_xform_run, kept by the engine until the next run / release
struct XformState {
    int nT = 0;                           // transformed points
    long R = 0;                           // rows = 3 nT
    std::vector<int32_t> ids;             // (point, src, ref) per transformed point
    DevBuf<double> xyz, Jv, ap;
    DevBuf<int32_t> tp, Jc;
    DevBuf<int2> chunks;
    int n_chunks = 0;
};

// What the transformation reads of an engine: the cofactor matrix (lower, row-major square, as gather_sub_kernel reads it), the
// device slot vector and the structure.  Pointers stay owned by the engine.
struct XformView {
    int device = 0;
    hipStream_t stream = nullptr;
    bool full_q = false;               // an inverting solve left all of Qxx (order U)
    const double *Q = nullptr;         // solver.Q, lower part valid, leading dimension ld
    long ld = 0;
    int U = 0;
    const double *d_vals = nullptr;    // current slot vector on the device
    const DevProblem *p = nullptr;     // counts + device tables (ip_image / ip_point: every image point of the problem)
    const std::vector<int32_t> *slot_col = nullptr;   // column of every slot (JAICOV_COL_FIXED for fixed parameters)
    std::unique_ptr<XformState> *state = nullptr;   // the engine's slot for the result
    std::string *err = nullptr;        // jaicov_neq_last_error text
};

void engine_xform_view(jaicov_engine *e, XformView *v);

}  // namespace jaicov
