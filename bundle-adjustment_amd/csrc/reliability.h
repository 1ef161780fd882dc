// What reliability.hip (include/jaicov_reliability.h) keeps in its slot of the engine; the engine itself it sees through qview.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jaicov_neq.h"
#include "devbuf.h"

namespace jaicov {

// result of jaicov_rel_run / jaicov_rel_run_points, kept by the engine until the next run / release
struct RelState {
    long n_rows = 0;
    DevBuf<double> out;                   // [4][n_rows]: v, qvv, r, t in the caller's row order
    double summary[6] = {0, 0, 0, 0, 0, 0};  // rel_summary_kernel's five, then the damping of the build Qxx inverts
    long n_points = -1;                   // image points of the table below; -1: a plain jaicov_rel_run, no table
    DevBuf<double> points;                // [JAICOV_REL_POINT_COLUMNS][n_points] in the caller's order (jaicov_rel_run_points)
};

struct QView;            // qview.h

// The run of jaicov_rel_run behind its refusals: brings the rows up to date, drops the previous result and leaves v, qvv, r, t of
// the `rows` observation rows in the engine's slot.  vce.hip begins with it, after refusals of its own.
int rel_run_plain(jaicov_engine *e, const QView &v, double sigma2_test, const double *dx, long rows);

}  // namespace jaicov
