// What calibration.hip (include/jaicov_calibration.h) keeps in its slot of the engine; the engine itself it sees through qview.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "devbuf.h"

namespace jaicov {

// work buffers of the jaicov_calib_* calls, kept by the engine (they only grow): O(n) for n nodes, nothing of order n^2
struct CalibState {
    DevBuf<int32_t> tab;       // the tables of a call: see calib_run
    DevBuf<double> rows;       // the PairRows block (pairrows.h) of side A, then that of side B
    DevBuf<double> vals;       // the private slot vector of side A, then that of side B
    DevBuf<double> out;        // node coordinates and depths | out | jac | reference covariance | summary
    std::vector<int32_t> cam_dist_begin, dist_kind;   // the camera tables of the problem: read from the device once
    bool have_tables = false;
    bool timing = false;       // jaicov_debug_calib_timing: the next calls record events around their kernels
    float ms[3] = {0.f, 0.f, 0.f};    // ... and leave here what the rows, calib_cov_kernel and calib_summary_kernel took
};

}  // namespace jaicov
