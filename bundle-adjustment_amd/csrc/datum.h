// What datum.hip (include/jaicov_datum.h) keeps in its slot of the engine, and what the two call of each other beside qview.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/jaicov_neq.h"
#include "devbuf.h"

namespace jaicov {

// S of the last jaicov_datum_transform and its work buffer, kept by the engine
struct DatumState {
    bool valid = false;              // S of the last transform belongs to the cofactor matrix at hand
    int order = 0, d = 0;
    std::vector<double> Z, B;        // [order][d], [d][order]: S = I - Z B'
    DevBuf<double> work;             // B' [d][np] | Y [np][d] | (Z, Y~) [np][2d] | table [nbk][nbk][128][d]
};

// Rows of the engine's datum rule (BA:493-635) for the mask at the slot values of the inverting solve: B [d][stride], columns
// 0 .. stride-1 (a jaicov_status: BAD_ARGUMENT with fewer than 3 datum points)
int engine_datum_rows(jaicov_engine *e, const uint8_t *mask, std::vector<double> &B, int stride);
// An inverting solve replaces the cofactor matrix: S of an earlier transform no longer applies
void datum_state_invalidate(DatumState *s);

}  // namespace jaicov
