// Internal constants of the relative orientation (relorient.hip, include/jaicov_relorient.h).
#pragma once

namespace jaicov {

constexpr int RELOR_LANES = 64;           // one wave works one pair: the workgroup is exactly one wave (relorient.hip relies on it)
constexpr int RELOR_CHUNK = 128;          // observations staged in LDS at a time; a pair with at most this many keeps them resident
constexpr int RELOR_SWEEPS9 = 10;         // cyclic Jacobi sweeps over the 9 x 9 moment matrix of the space start
constexpr int RELOR_SWEEPS3 = 6;          // cyclic Jacobi sweeps over E'E and H'H
constexpr int RELOR_SLOTS = 12;           // candidate slots (M, b): 4 of the space start, 8 of the plane start
constexpr int RELOR_SLOT_LEN = 15;        // M (9), b (3), M b (3)
constexpr int RELOR_STARTS = 3;           // starts that run Gauss-Newton: one of the space start, two of the plane start

// the sums of one pass, per lane.  Space start: the upper triangle of the 9 x 9 matrix; plane start: 36 + 8; cheirality: one count per
// slot; step and evaluation: 15 + 5 + Omega
constexpr int RELOR_NACC = 45;
constexpr int RELOR_NACC_STEP = 15 + 5 + 1;
constexpr int RELOR_NACC_PLANE = 36 + 8;

}  // namespace jaicov
