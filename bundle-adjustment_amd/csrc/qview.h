// The one interface between the engine (engine.hip; jaicov_engine itself is engine_state.h, not for readers) and whatever reads the cofactor matrix an inverting solve leaves on
// the device: transform.hip, reliability.hip, datum.hip (the one writer), precision.hip, parameters.hip, forms.hip, predict.hip,
// newpoints.hip, vce.hip and calibration.hip.  Here are the view of the engine (QView), the shell of a call and the device's reads of the matrix.  A consumer adds
// a state struct of its own and a slot for it in QSlots; a call of it is, in the order of refusals that the headers under include/
// promise (engine, shard, state, arguments):
//   q_view, q_guard with the call's own texts, the argument checks (argcheck.h; q_column for a slot's column), q_state for the work
//   buffers, the launches on v.stream (QTimer around them where a bench hook times them), q_download.
// Its kernels read the matrix through q_sym or q_at.  Calls that bring image measurements of their own build their rows with
// pairrows.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "../../include/jaicov_neq.h"
#include "argcheck.h"
#include "ba_kernels.h"
#include "devbuf.h"
#include "status.h"

namespace jaicov {

struct XformState;       // transform.h
struct RelState;         // reliability.h
struct DatumState;       // datum.h
struct PrecisionState;   // precision.h
struct ParamState;       // parameters.h
struct FormState;        // forms.h
struct PredictState;     // predict.h
struct NewPointState;    // newpoints.h
struct VceState;         // vce.h
struct CalibState;       // calibration.h

// The engine's slots for what its consumers keep.  A result (xform, rel) stays until the next run of its family or its release, a
// later inverting solve included; an inverting solve withdraws the S of the datum state alone (datum_state_invalidate).
struct QSlots {
    std::unique_ptr<XformState> xform;       // result of jaicov_xform_run
    std::unique_ptr<RelState> rel;           // result of jaicov_rel_run / jaicov_rel_run_points
    std::unique_ptr<DatumState> datum;       // S of the last jaicov_datum_transform and its work buffer
    std::unique_ptr<PrecisionState> prec;    // work buffers of the precision calls
    std::unique_ptr<ParamState> par;         // work buffers of the jaicov_par_* calls
    std::unique_ptr<FormState> form;         // work buffers of jaicov_form_fit
    std::unique_ptr<PredictState> pred;      // work buffers of the jaicov_pred_* calls
    std::unique_ptr<NewPointState> newpt;    // work buffers of jaicov_newpt_intersect
    std::unique_ptr<VceState> vce;           // result of jaicov_vce_run
    std::unique_ptr<CalibState> calib;       // work buffers of the jaicov_calib_* calls
};

// What a consumer sees of an engine.  Pointers stay owned by the engine.
struct QView {
    int device = 0;
    hipStream_t stream = nullptr;
    double *Q = nullptr;               // the cofactor matrix: lower part valid (row-major square, as gather_sub_kernel reads it), leading
    long ld = 0;                       // dimension ld, order `order`, border rows 0 .. d-1
    int order = 0;                     // order of the matrix: U, or the first EO column for the one of the EO-reduced system
    int U = 0;                         // the engine's full order
    int d = 0;
    int n_points = 0;
    bool have_q = false;               // an inverting solve left a cofactor matrix
    bool reduced = false;              // ... of the EO-reduced system: no columns of the exterior orientations
    bool full_q = false;               // ... all of Qxx: have_q, not reduced, order U
    bool sharded = false;              // the engine accumulates a range of images or leaves the shared groups to another rank
    double sigma2 = 0.0;               // a-priori variance factor of the build whose system was inverted
    double lambda = 0.0;               // and its damping value (jaicov_rel_summary [5]: sum r = f needs 0)
    const DevProblem *p = nullptr;     // counts + device tables (ip_image / ip_point: every image point of the problem, in engine order)
    const double *d_vals = nullptr;    // current slot vector on the device
    const double *rowsA = nullptr;     // compact rows of the current parameter values (rows.hip layout [2 KROW][n_ip]) and the
    const double *rowsW = nullptr;     // misclosures [2][n_ip]: up to date after engine_ensure_rows
    const double *ll_diag = nullptr;   // diag(D): [2 n_ip] of the image coordinates in engine order (variances, or the dense block's
                                       // diagonal), then [n_dg_rows] of the directly observed rows (dg_var, or the dense group's diagonal)
    const std::vector<int32_t> *slot_col = nullptr;     // column of every slot (JAICOV_COL_FIXED for fixed parameters)
    const std::vector<int32_t> *ip_old2new = nullptr;   // empty, or the engine position of the caller's image point
    const std::vector<int32_t> *blk_ip_begin = nullptr; // engine image blocks (ordinary images served as blocks included)
    const std::vector<int64_t> *blk_w_off = nullptr;    // their weight offsets in p->blk_w (< 0: 2 x 2 weights)
    const std::vector<int32_t> *caller_block = nullptr; // empty, or the caller's index of an engine image block (-1: an ordinary image)
    QSlots *slot = nullptr;            // the engine's slots
    std::string *err = nullptr;        // jaicov_neq_last_error text
};

void engine_q_view(jaicov_engine *e, QView *v);
// Brings the compact rows up to the current parameter values (a jaicov_status)
int engine_ensure_rows(jaicov_engine *e);

inline QView q_view(jaicov_engine *e) {
    QView v;
    engine_q_view(e, &v);
    return v;
}

// The refusals a reader begins with: a sharded engine (UNSUPPORTED), then the matrix (BAD_STATE).  full_text null: any cofactor
// matrix will do; otherwise all of Qxx is needed, and this is what its absence is called.
inline int q_guard(const QView &v, const char *sharded_text, const char *full_text = nullptr) {
    if (v.sharded) FAIL(*v.err, JAICOV_ERR_UNSUPPORTED, sharded_text);
    if (full_text ? !v.full_q : !v.have_q) FAIL(*v.err, JAICOV_ERR_BAD_STATE, full_text ? full_text : "no cofactor matrix: solve with invert != 0 first");
    return JAICOV_OK;
}

// the state of a slot, created on first use
template <typename S>
inline S *q_state(std::unique_ptr<S> &slot) {
    if (!slot) slot.reset(new S());
    return slot.get();
}

// *c = the matrix column of a slot, -1 for a fixed parameter; a column outside the reduced matrix is refused with `what`
inline int q_column(const QView &v, size_t slot_index, const char *what, int *c) {
    const int col = (*v.slot_col)[slot_index];
    if (col >= v.order) FAIL(*v.err, JAICOV_ERR_BAD_STATE, what);
    *c = col < 0 ? -1 : col;
    return JAICOV_OK;
}

// N marks on the engine's stream behind a bench hook's switch; not armed, it creates no event and does nothing
template <int N>
class QTimer {
    DevEvent ev_[N];
    hipStream_t stream_;
    bool on_ = false;
  public:
    explicit QTimer(hipStream_t stream) : stream_(stream) {}
    hipError_t arm(bool on) {
        on_ = on;
        for (int k = 0; on_ && k < N; k++) HIPCHK(ev_[k].create());
        return hipSuccess;
    }
    hipError_t mark(int k) { return on_ ? hipEventRecord(ev_[k].get(), stream_) : hipSuccess; }
    // ms[k]: from mark k to mark k + 1, once the stream has been synchronised
    hipError_t read(float *ms) {
        for (int k = 0; on_ && k + 1 < N; k++) HIPCHK(hipEventElapsedTime(&ms[k], ev_[k].get(), ev_[k + 1].get()));
        return hipSuccess;
    }
};

// the state a slot holds, or null with `none` as the error text
template <typename S>
inline S *q_result(const QView &v, const std::unique_ptr<S> &slot, const char *none) {
    if (!slot) *v.err = none;
    return slot.get();
}

// the device's work on the state ends before the state goes
template <typename S>
inline void q_release(const QView &v, std::unique_ptr<S> &slot) {
    if (!slot) return;
    hipSetDevice(v.device);
    hipStreamSynchronize(v.stream);
    slot.reset();
}

// device -> host on the engine's stream, complete on return; an entry without a destination or without bytes is skipped
struct QCopy { void *dst; const void *src; size_t bytes; };
inline int q_download(const QView &v, std::initializer_list<QCopy> copies) {
    HIPE(*v.err, hipSetDevice(v.device));
    for (const QCopy &c : copies)
        if (c.dst && c.bytes) HIPE(*v.err, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, v.stream));
    HIPE(*v.err, hipStreamSynchronize(v.stream));
    return JAICOV_OK;
}

// What reliability.hip and vce.hip need to know of the engine's image blocks before they launch
struct QImageBlocks {
    std::vector<int32_t> new2old;   // engine position -> the caller's image point; empty: the two orders are one
    std::vector<uint8_t> dense;     // [n_ip] 1: in a block with a dense weight matrix; 0: 2 x 2 weights (compact-weight blocks included)
    std::vector<int32_t> blocks;    // the engine image blocks with a dense weight matrix and at least one point, ascending
    int max_m = 0;                  // rows of the largest of them
    int caller(long q) const { return new2old.empty() ? (int)q : new2old[q]; }
};
inline QImageBlocks q_image_blocks(const QView &v) {
    QImageBlocks ib;
    const long n_ip = v.p->n_ip;
    if (!v.ip_old2new->empty()) {
        ib.new2old.resize(n_ip);
        for (long o = 0; o < n_ip; o++) ib.new2old[(*v.ip_old2new)[o]] = (int32_t)o;
    }
    ib.dense.assign(n_ip, 0);
    const std::vector<int32_t> &bb = *v.blk_ip_begin;
    const std::vector<int64_t> &bw = *v.blk_w_off;
    for (size_t g = 0; g + 1 < bb.size(); g++) {
        if (bw[g] < 0 || bb[g + 1] <= bb[g]) continue;
        ib.blocks.push_back((int32_t)g);
        ib.max_m = std::max(ib.max_m, 2 * (bb[g + 1] - bb[g]));
        for (int q = bb[g]; q < bb[g + 1]; q++) ib.dense[q] = 1;
    }
    return ib;
}

// ---- the device's reads of the matrix

// entry (i, j) of the symmetric matrix from its lower part
__device__ __forceinline__ double q_sym(const double *__restrict__ Q, long ld, int i, int j) {
    return i >= j ? Q[(long)i * ld + j] : Q[(long)j * ld + i];
}

// the same by columns of parameters: a fixed parameter (column < 0) is a zero row and column
__device__ __forceinline__ double q_at(const double *__restrict__ Q, long ld, int ci, int cj) {
    if (ci < 0 || cj < 0) return 0.0;
    return q_sym(Q, ld, ci, cj);
}

}  // namespace jaicov
