// What precision.hip (include/jaicov_precision.h) keeps in its slot of the engine; the engine itself it sees through qview.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "devbuf.h"

namespace jaicov {

// work buffers of the precision calls, kept by the engine (they only grow)
struct PrecisionState {
    DevBuf<int32_t> tab;      // column table of the items | status
    DevBuf<double> out;       // the items' figures
    DevBuf<double> work;      // components: Xt [8][np] | Xr [np][8] | Y [np][8] | W [np][8] | small | partial sums | table [nbk][nbk][128][8]
};

}  // namespace jaicov
