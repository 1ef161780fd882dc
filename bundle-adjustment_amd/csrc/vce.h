// What vce.hip (include/jaicov_vce.h) keeps in its slot of the engine; the engine itself it sees through qview.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "devbuf.h"

namespace jaicov {

// result of jaicov_vce_run, kept by the engine until the next run / release
struct VceState {
    bool have = false;                    // a run has left a result (the buffers stay for the next one)
    int n_groups = 0;
    DevBuf<double> table;                 // [JAICOV_VCE_COLUMNS][n_groups + 1]: the groups, then the totals over all rows
    DevBuf<int32_t> status;               // [n_groups + 1]
    double summary[5] = {0, 0, 0, 0, 0};  // jaicov_vce_summary
    bool timing = false;                  // jaicov_debug_vce_timing: the next runs record events around their kernels
    float ms[3] = {0.f, 0.f, 0.f};        // ... and leave here what vce_block_kernel, vce_small_kernel and vce_group_kernel took
};

}  // namespace jaicov
