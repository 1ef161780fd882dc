// What parameters.hip (include/jaicov_parameters.h) keeps in its slot of the engine; the engine itself it sees through qview.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "devbuf.h"

namespace jaicov {

// one candidate of the maxima pass: what a tile found for one of its rows or columns (16 bytes)
struct alignas(16) ParCand {
    double key;          // |rho| of the best admissible partner, -1 without one
    int32_t idx2;        // 2 partner + (rho < 0), INT32_MAX without one
    int32_t status;      // JAICOV_PAR_NOT_FINITE when the tile met an entry of this row or column that is not finite
};

// work buffers of the jaicov_par_* calls, kept by the engine (they only grow)
struct ParamState {
    DevBuf<double> scale;      // s [np]
    DevBuf<int32_t> tab;       // class [np] | item [np] | status of the diagonal [np]
    DevBuf<ParCand> cand;      // maxima: the candidate table [nbk][nbk][128]
    DevBuf<int64_t> count;     // pairs: count of every tile [nt] | offset of every tile [nt] | total
    DevBuf<double> out_d;      // the call's figures (and x0 of the group members behind them)
    DevBuf<int32_t> out_i;     // the call's int tables and results
};

}  // namespace jaicov
