// argcheck.h -- checks of caller's arrays that the one-shot batched calls (batchcall.h) and the readers of the cofactor matrix
// (qview.h) share.  They touch no device.
#pragma once
#include <math.h>
#include <stdint.h>

namespace jaicov {

// begin[0 .. n] are the bounds of n ranges: they start at 0 and do not decrease
inline bool ranges_ok(int32_t n, const int32_t *begin) {
    if (begin[0] != 0) return false;
    for (int32_t g = 0; g < n; g++)
        if (begin[g + 1] < begin[g]) return false;
    return true;
}

// var (may be NULL: unit weights) holds vx > 0, vy > 0, |rho| < 1 for each of n_obs observations
inline bool dispersions_ok(const double *var, long n_obs) {
    if (!var) return true;
    for (long k = 0; k < n_obs; k++)
        if (!(var[3 * k] > 0.0) || !(var[3 * k + 1] > 0.0) || !(fabs(var[3 * k + 2]) < 1.0)) return false;
    return true;
}

}  // namespace jaicov
