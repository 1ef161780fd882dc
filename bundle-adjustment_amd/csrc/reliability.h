// Internal interface between engine.hip (owner of jaicov_engine) and reliability.hip (include/jaicov_reliability.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/jaicov_neq.h"
#include "ba_kernels.h"
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

// What the reliability analysis reads of an engine.  Pointers stay owned by the engine.
struct RelView {
    int device = 0;
    hipStream_t stream = nullptr;
    bool full_q = false;               // an inverting solve left all of Qxx (order U)
    bool sharded = false;              // the engine accumulates a range of images or leaves the shared groups to another rank
    const double *Q = nullptr;         // solver.Q, lower part valid, leading dimension ld
    long ld = 0;
    int U = 0;
    double sigma2 = 0.0;               // a-priori variance factor of the build whose system was inverted
    double lambda = 0.0;               // and its damping value (jaicov_rel_summary [5]: sum r = f needs 0)
    const DevProblem *p = nullptr;     // counts + device tables, image points in engine order
    const double *rowsA = nullptr;     // compact rows of the current parameter values (rows.hip layout [2 KROW][n_ip])
    const double *rowsW = nullptr;     // misclosures [2][n_ip]
    const double *d_vals = nullptr;    // current slot vector on the device
    const double *ll_diag = nullptr;   // diag(D): [2 n_ip] of the image coordinates in engine order (variances, or the dense block's
                                       // diagonal), then [n_dg_rows] of the directly observed rows (dg_var, or the dense group's diagonal)
    const std::vector<int32_t> *ip_old2new = nullptr;   // empty, or the engine position of the caller's image point
    const std::vector<int32_t> *blk_ip_begin = nullptr; // engine image blocks (ordinary images served as blocks included)
    const std::vector<int64_t> *blk_w_off = nullptr;    // their weight offsets in p->blk_w (< 0: 2 x 2 weights)
    std::unique_ptr<RelState> *state = nullptr;   // the engine's slot for the result
    std::string *err = nullptr;        // jaicov_neq_last_error text
};

// Fills the view; with rows != 0 it also brings the compact rows up to the current parameter values first (returns a jaicov_status).
int engine_rel_view(jaicov_engine *e, RelView *v, int rows);

}  // namespace jaicov
