// Internal constants of the batched DLT (dlt.hip, include/jaicov_dlt.h).
#pragma once

namespace jaicov {

constexpr int DLT_NB = 11;            // b11..b14, b21..b24, b31..b33 (DT:280-303)
constexpr int DLT_MAX_RESTR = 5;      // six types, IDENTICAL dropped when both FIXED_PRINCIPLE_DISTANCE_* are present (DT:269-278)
constexpr int DLT_MAX_ORDER = DLT_NB + DLT_MAX_RESTR;
constexpr int DLT_CHUNK = 128;        // observations staged in LDS at a time
constexpr int DLT_TYPES = 6;          // jaicov_dlt_restriction ids 0..5

struct DltRestrictions {              // the validated list, passed by value
    int n;
    int id[DLT_MAX_RESTR];
};

}  // namespace jaicov
