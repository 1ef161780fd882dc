// What predict.hip (include/jaicov_predict.h) keeps in its slot of the engine; the engine itself it sees through qview.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "devbuf.h"

namespace jaicov {

// work buffers of the jaicov_pred_* calls, kept by the engine (they only grow): O(n) for n pairs, nothing of order n^2
struct PredictState {
    DevBuf<int32_t> tab;       // image [n] | point [n] | first pair [W] | pairs [W] of the W workgroups | status [n] | group_begin [G + 1] |
                               // member -> sorted position [n] | group status [G]
    DevBuf<double> rows;       // the PairRows block (pairrows.h) of the pairs sorted by image
    DevBuf<double> out;        // out [10 n] or [8 n] | gout [4 G]
    std::vector<uint64_t> observed;   // (image << 32 | point) of every image point of the problem, ascending: read from the device once
    bool have_observed = false;
    bool timing = false;       // jaicov_debug_pred_timing: the next calls record events around their kernels
    float ms[3] = {0.f, 0.f, 0.f};    // ... and leave here what the rows, pred_cov_kernel and pred_group_kernel took
};

}  // namespace jaicov
