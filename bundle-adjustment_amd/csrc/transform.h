// What transform.hip (include/jaicov_transform.h) keeps in its slot of the engine; the engine itself it sees through qview.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

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

}  // namespace jaicov
