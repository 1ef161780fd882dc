// Internal constants of the absolute orientation (simil.hip, include/jaicov_simil.h).
#pragma once

namespace jaicov {

constexpr int SIMIL_LANES = 64;           // one wave works one model: the workgroup is exactly one wave (simil.hip relies on it)
constexpr int SIMIL_CHUNK = 128;          // points staged in LDS at a time; a model with at most this many keeps them resident
constexpr int SIMIL_SWEEPS3 = 6;          // cyclic Jacobi sweeps over M'M

// the sums of one pass, per lane.  Means: 3 + 3; closed start: M (9) and sum |s - sbar|^2; step and evaluation: 28 + 7 + Omega
constexpr int SIMIL_NACC = 28 + 7 + 1;
constexpr int SIMIL_NACC_MEAN = 6;
constexpr int SIMIL_NACC_START = 10;

}  // namespace jaicov
