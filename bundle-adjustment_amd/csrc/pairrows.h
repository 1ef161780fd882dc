// pairrows.h -- the rows of a call that brings image measurements of its own (predict.hip: pairs of an image and a point,
// newpoints.hip: rays).  J and w of its n pairs come from launch_rows (rows.hip) on a copy of the engine's DevProblem whose image-point
// tables are the call's pairs, so a measurement from outside meets the arithmetic of the adjustment's own rows.  One block of doubles,
// which stays the caller's own DevBuf:
//   J [2 KROW][n] | w [2][n] | x [n] | y [n] | disp [3 n]
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "ba_kernels.h"
#include "launchers.h"

namespace jaicov {

struct PairRows {
    const size_t n, o_w, o_x, o_disp, size;      // pairs, offsets of w, x and disp, doubles in all
    double *J = nullptr, *w = nullptr, *x = nullptr, *y = nullptr, *disp = nullptr;
    std::vector<double> meas;                    // x | y | disp on their way to the device: lives as long as the call
    explicit PairRows(size_t n_) : n(n_), o_w(2 * KROW * n_), o_x(o_w + 2 * n_), o_disp(o_x + 2 * n_), size(o_disp + 3 * n_) {}
    // the block lies at `base` (`size` doubles)
    void bind(double *base) { J = base; w = base + o_w; x = base + o_x; y = x + n; disp = base + o_disp; }
    // x | y | disp of the caller's pairs to the device: xy [2 n] (null: zeros) and disp [3 n], the caller's pair order[s] at position s
    // (order null: as they come).  Without dispersions, or without pairs, nothing is copied.
    hipError_t stage(hipStream_t s, const double *xy, const double *dsp, const int32_t *order) {
        if (!dsp || n == 0) return hipSuccess;
        meas.assign(5 * n, 0.0);
        for (size_t k = 0; k < n; k++) {
            const size_t i = order ? (size_t)order[k] : k;
            if (xy) { meas[k] = xy[2 * i]; meas[n + k] = xy[2 * i + 1]; }
            for (int c = 0; c < 3; c++) meas[2 * n + 3 * k + c] = dsp[3 * i + c];
        }
        return hipMemcpyAsync(x, meas.data(), 5 * n * sizeof(double), hipMemcpyHostToDevice, s);
    }
    // the engine's problem with the call's pairs as its image points
    DevProblem problem(const DevProblem &p, const int32_t *image, const int32_t *point) const {
        DevProblem q = p;
        q.n_ip = (int)n; q.ip_image = image; q.ip_point = point; q.ip_x = x; q.ip_y = y;
        return q;
    }
    // J and w at the slot vector `vals`
    hipError_t rows(hipStream_t s, const DevProblem &q, const double *vals) const { return launch_rows(s, q, vals, 0, (int)n, J, w); }
};

}  // namespace jaicov
