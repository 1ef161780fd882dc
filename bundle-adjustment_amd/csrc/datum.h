// Internal interface between engine.hip (owner of jaicov_engine) and datum.hip (include/jaicov_datum.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <string>
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

// What the datum transformation reads and writes of an engine.  Pointers stay owned by the engine.
struct DatumView {
    int device = 0;
    hipStream_t stream = nullptr;
    bool have_q = false;               // an inverting solve left a cofactor matrix
    bool sharded = false;              // the engine accumulates a range of images or leaves the shared groups to another rank
    double *Q = nullptr;               // the cofactor matrix: lower part valid, leading dimension ld, order `order`, border rows 0 .. d-1
    long ld = 0;
    int order = 0;
    int d = 0;
    int n_points = 0;
    std::unique_ptr<DatumState> *state = nullptr;   // the engine's slot for S of the last transform and the work buffer
    std::string *err = nullptr;        // jaicov_neq_last_error text
};

void engine_datum_view(jaicov_engine *e, DatumView *v);
// Rows of the engine's datum rule (BA:493-635) for the mask at the slot values of the inverting solve: B [d][stride], columns
// 0 .. stride-1 (a jaicov_status: BAD_ARGUMENT with fewer than 3 datum points)
int engine_datum_rows(jaicov_engine *e, const uint8_t *mask, std::vector<double> &B, int stride);
// An inverting solve replaces the cofactor matrix: S of an earlier transform no longer applies
void datum_state_invalidate(DatumState *s);

}  // namespace jaicov
