// Internal constants of the spatial resection (resect.hip, include/jaicov_resect.h).
#pragma once

namespace jaicov {

constexpr int RESECT_LANES = 64;          // one wave works one image: the workgroup is exactly one wave (resect.hip relies on it)
constexpr int RESECT_CHUNK = 128;         // observations staged in LDS at a time; an image with at most this many keeps them resident
constexpr int RESECT_POLAR_STEPS = 10;    // Newton steps X <- (X + X^-T) / 2 of the polar factor
constexpr int RESECT_JACOBI_SWEEPS = 6;   // cyclic Jacobi sweeps over the 3 x 3 scatter matrix

// the sums of one pass, per lane.  Space start: of the 66 + 11 entries of its normal equations 51 are distinct sums (resect.hip);
// plane start: 36 + 8; step and evaluation: 21 + 6 + Omega
constexpr int RESECT_NACC = 51;
constexpr int RESECT_NACC_STEP = 21 + 6 + 1;
constexpr int RESECT_NACC_PLANE = 36 + 8;

}  // namespace jaicov
