// Internal interface between engine.hip (owner of jaicov_engine) and precision.hip (include/jaicov_precision.h).
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

// work buffers of the precision calls, kept by the engine (they only grow)
struct PrecisionState {
    DevBuf<int32_t> tab;      // column table of the items | status
    DevBuf<double> out;       // the items' figures
    DevBuf<double> work;      // components: Xt [8][np] | Xr [np][8] | Y [np][8] | W [np][8] | small | partial sums | table [nbk][nbk][128][8]
};

// What the precision calls read of an engine.  Pointers stay owned by the engine.
struct PrecView {
    int device = 0;
    hipStream_t stream = nullptr;
    bool have_q = false;               // an inverting solve left a cofactor matrix
    bool reduced = false;              // ... of the EO-reduced system: no columns of the exterior orientations
    bool sharded = false;              // the engine accumulates a range of images or leaves the shared groups to another rank
    const double *Q = nullptr;         // the cofactor matrix: lower part valid, leading dimension ld, order `order`, border rows 0 .. d-1
    long ld = 0;
    int order = 0;
    int d = 0;
    const double *d_vals = nullptr;    // current slot vector on the device
    const DevProblem *p = nullptr;     // counts (n_points, n_cameras, n_dist, n_images: the slot layout)
    const std::vector<int32_t> *slot_col = nullptr;   // column of every slot (JAICOV_COL_FIXED for fixed parameters)
    std::unique_ptr<PrecisionState> *state = nullptr; // the engine's slot for the work buffers
    std::string *err = nullptr;        // jaicov_neq_last_error text
};

void engine_prec_view(jaicov_engine *e, PrecView *v);

}  // namespace jaicov
