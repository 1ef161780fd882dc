// obsweight.h -- the 2 x 2 weight of an image point (PDF:308-319), the one place of the library's device code that writes it out.
// Like rotation.h it sets no floating-point contraction of its own and includes nothing of the engine: wavealg.h includes it below
// its `fp contract(off)`, so the stand-alone start-value kernels round every product on its own; obsmodel.h includes it as it stands,
// so the engine's kernels keep the compiler's fused 1 - rho^2.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>

namespace jaicov {

// the weights of one observation from its dispersions vx, vy, rho.  It takes the three values, not the array and an index: the
// loads stay with the caller's other loads of the same index, and resect.hip's kernel keeps its register allocation.
__device__ inline void obs_weight(double vx, double vy, double rho, double s0, double &p11, double &p12, double &p22) {
    if (rho == 0.0) {
        p11 = s0 / vx; p22 = s0 / vy; p12 = 0.0;
    } else {
        const double inv = s0 / ((1.0 - rho * rho) * vx * vy);
        p11 = inv * vy; p22 = inv * vx; p12 = -inv * rho * sqrt(vx * vy);
    }
}

}  // namespace jaicov
