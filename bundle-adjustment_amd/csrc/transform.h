// Internal interface between engine.hip (owner of jaicov_engine) and transform.hip (include/jaicov_transform.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/jaicov_neq.h"
#include "ba_kernels.h"

namespace jaicov {

struct XformState;

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
    XformState **state = nullptr;      // the engine's slot for the result (freed by jaicov_neq_destroy)
    std::string *err = nullptr;        // jaicov_neq_last_error text
};

void engine_xform_view(jaicov_engine *e, XformView *v);
void xform_state_free(XformState *s);

}  // namespace jaicov
