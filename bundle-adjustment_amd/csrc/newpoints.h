// What newpoints.hip (include/jaicov_newpoints.h) keeps in its slot of the engine; the engine itself it sees through qview.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "devbuf.h"

namespace jaicov {

// work buffers of jaicov_newpt_intersect, kept by the engine (they only grow): O(rays + columns + pairs), nothing of order n^2
struct NewPointState {
    DevBuf<int32_t> tab;       // ray image [R] | ray point [R] | ray_begin [n + 1] | col_begin [n + 1] | flag [n] | cols [C] |
                               // ray local -> position [KC_MAX R] | pairs [2 G] | state [n] | iterations [n] | status [n] | pair status [G] | moving [1]
    DevBuf<double> rows;       // the PairRows block (pairrows.h) of the R rays
    DevBuf<double> vals;       // the private slot vector: X, Y, Z of the new points [3 n] | the engine's slots behind its object points
    DevBuf<double> out;        // out [20 n] | F [3 C] (per point [3][M]) | pout [7 G] | ray_w [2 R]
    std::vector<int32_t> image_camera, cam_dist_begin;     // read from the device tables once per engine
    bool have_tables = false;
    bool timing = false;       // jaicov_debug_newpt_timing: the next calls record events around their kernels
    float ms[3] = {0.f, 0.f, 0.f};    // ... and leave here what the Gauss-Newton loop, newpt_gain_kernel and newpt_pair_kernel took
    int steps = 0;             // Gauss-Newton steps the last call enqueued
};

}  // namespace jaicov
