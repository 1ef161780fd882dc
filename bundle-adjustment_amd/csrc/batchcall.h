// batchcall.h -- the host side of the one-shot batched calls (dlt.hip, intersect.hip, resect.hip, relorient.hip, simil.hip, lens.hip): what
// they check before they touch a device, and the shell that carries host arrays to one launch and back.  Every argument check comes
// first, then the device check, so that a bad call is refused as such on any machine.
//   BatchCall owns what such a call owns: its stream, its device buffers and the two events around the launch.  A call site is a
//   straight list of steps (in, alloc, filled, run, out, outcomes) and one finish().  The first hipError_t that goes wrong sticks:
//   every later step does nothing and hands out null, no kernel is launched, and finish() returns it as the public status.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/jaicov_neq.h"
#include "argcheck.h"      // ranges_ok, dispersions_ok
#include "devbuf.h"

namespace jaicov {

// the current device is an MI355X-class one (gfx950): these calls ship code for nothing else
inline bool device_is_gfx950() {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return false;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

class BatchCall {
    DevStream stream_;                 // first, so that the other owners go before the stream does
    DevBag bag_;
    DevEvent ev0_, ev1_;
    const bool timed_;
    hipError_t err_ = hipSuccess;
    bool out_of_memory_ = false;
    // the outcome records on their way back (outcomes): unpacked by finish(), after the synchronise
    std::vector<int32_t> records_;
    int width_ = 0;
    int32_t *status_ = nullptr, *iterations_ = nullptr, *start_kind_ = nullptr;

    bool step(hipError_t err) {
        if (err_ == hipSuccess) err_ = err;
        return err_ == hipSuccess;
    }
  public:
    // timed: the call reports the device time of its launch (finish(ms_out)) and holds the two events for it
    explicit BatchCall(bool timed = true) : timed_(timed) {
        if (step(stream_.create()) && timed_ && step(ev0_.create())) step(ev1_.create());
    }
    // room for `count` elements, at least one: never null unless the call has failed
    template <typename T>
    T *alloc(size_t count) {
        T *dev = nullptr;
        if (err_ == hipSuccess && !step(bag_.alloc(&dev, count))) out_of_memory_ = err_ == hipErrorOutOfMemory;
        return dev;
    }
    // the same with every byte set (hipMemsetAsync's `value`)
    template <typename T>
    T *filled(size_t count, int value) {
        T *dev = alloc<T>(count);
        if (dev) step(hipMemsetAsync(dev, value, (count > 0 ? count : 1) * sizeof(T), stream_.get()));
        return dev;
    }
    // an input on the device.  A null `host` (an optional input left out) gives null, which the kernels test; a `count` of 0 gives a
    // valid allocation of one element and no copy.
    template <typename T>
    T *in(const T *host, size_t count) {
        T *dev = host ? alloc<T>(count) : nullptr;
        if (dev && count > 0) step(hipMemcpyAsync(dev, host, count * sizeof(T), hipMemcpyHostToDevice, stream_.get()));
        return dev;
    }
    // a table that the call built itself: always an allocation, an empty table included
    template <typename T>
    T *in(const std::vector<T> &host) {
        T *dev = alloc<T>(host.size());
        if (dev && !host.empty()) step(hipMemcpyAsync(dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, stream_.get()));
        return dev;
    }
    // the launch or launches, launch(stream), between the two events; nothing is launched once a step has failed
    template <typename Launch>
    void run(Launch &&launch) {
        if (timed_) step(hipEventRecord(ev0_.get(), stream_.get()));
        if (err_ != hipSuccess) return;
        launch(stream_.get());
        if (step(hipGetLastError()) && timed_) step(hipEventRecord(ev1_.get(), stream_.get()));
    }
    // an output back to the host; a null `host` (an optional output left out) or a `count` of 0: nothing
    template <typename T>
    void out(T *host, const T *dev, size_t count) {
        if (err_ == hipSuccess && host && count > 0) step(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, stream_.get()));
    }
    // n outcome records of `width` words (status, iterations, and start kind where width is 3) back to the caller's arrays, of which
    // iterations and start_kind may be null.  They are staged in the call object, which outlives the synchronise of finish().
    void outcomes(const int32_t *dev, size_t n, int width, int32_t *status, int32_t *iterations, int32_t *start_kind) {
        records_.resize(n * width);
        width_ = width; status_ = status; iterations_ = iterations; start_kind_ = start_kind;
        out(records_.data(), dev, records_.size());
    }
    // the one synchronise of the call, then the outcome records and the device time of run() in milliseconds (ms_out may be null)
    int finish(double *ms_out = nullptr) {
        if (err_ == hipSuccess) step(hipStreamSynchronize(stream_.get()));
        if (err_ == hipSuccess && timed_ && ms_out) {
            float ms = 0;
            if (step(hipEventElapsedTime(&ms, ev0_.get(), ev1_.get()))) *ms_out = ms;
        }
        if (err_ != hipSuccess) {
            // copies queued before the failure may still read or write host arrays that go when the caller returns: wait for them as
            // far as the runtime still can; the status is the first error's whatever this wait gives
            if (stream_.get()) (void)hipStreamSynchronize(stream_.get());
            return out_of_memory_ ? JAICOV_ERR_OUT_OF_MEMORY : JAICOV_ERR_DEVICE;
        }
        for (size_t g = 0; width_ > 0 && g < records_.size() / width_; g++) {
            status_[g] = records_[width_ * g];
            if (iterations_) iterations_[g] = records_[width_ * g + 1];
            if (start_kind_) start_kind_[g] = records_[width_ * g + 2];
        }
        return JAICOV_OK;
    }
};

}  // namespace jaicov
