// batchcall.h -- what the one-shot batched calls (dlt.hip, intersect.hip, resect.hip, relorient.hip, simil.hip) check on the host before they
// touch a device.  Every argument check comes first, then the device check, so that a bad call is refused as such on any machine.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string.h>

namespace jaicov {

// the current device is an MI355X-class one (gfx950): these calls ship code for nothing else
inline bool device_is_gfx950() {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return false;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

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
