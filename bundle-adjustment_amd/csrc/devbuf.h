// Move-only owners of what the HIP runtime hands out: a device allocation, an event, a stream, a host-mapped allocation.  Each frees
// its resource exactly once, in its destructor, so a function may leave through an error return with any of them half acquired.
// This header is the only place of the library that allocates or frees device memory and creates or destroys events, so the
// count it keeps (device_live) is complete; beside the stream pool of dense.hip it is also the only one that creates or destroys streams.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <utility>
#include <vector>

namespace jaicov {

// device memory that DevBufs of this process hold right now: [0] bytes, [1] allocations (jaicov_debug_device_census, dense.hip)
inline std::atomic<long long> device_live[2];

// One owner for a device allocation that only grows: pointer and element count never get out of step, and the memory is
// freed exactly once, by the destructor.  hipFree waits for the device by itself, so an owner may go out of scope on an
// error path with work still in flight; on a success path the caller synchronises its stream first.
template <typename T>
class DevBuf {
    T *ptr_ = nullptr;
    size_t count_ = 0;
    hipError_t adopt(hipError_t err, size_t count) {      // the outcome of an allocation into ptr_
        if (err != hipSuccess) { ptr_ = nullptr; return err; }
        count_ = count;
        device_live[0] += (long long)(count * sizeof(T));
        device_live[1] += 1;
        return err;
    }
  public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : ptr_(o.ptr_), count_(o.count_) { o.ptr_ = nullptr; o.count_ = 0; }   // move-only: no copies
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(ptr_, o.ptr_); std::swap(count_, o.count_); return *this; }
    ~DevBuf() { reset(); }
    // room for `count` elements: the allocation at hand if it is large enough, otherwise a new one (the contents are lost)
    hipError_t reserve(size_t count) {
        if (count <= count_) return hipSuccess;
        reset();
        return adopt(hipMalloc(&ptr_, count * sizeof(T)), count);
    }
    // the same in FINE-GRAINED device memory (hipExtMallocWithFlags: freed by hipFree like any other); no fallback here
    hipError_t reserve_finegrained(size_t count) {
        reset();
        return adopt(hipExtMallocWithFlags((void **)&ptr_, count * sizeof(T), hipDeviceMallocFinegrained), count);
    }
    void reset() {
        if (ptr_) {
            hipFree(ptr_);
            device_live[0] -= (long long)(count_ * sizeof(T));
            device_live[1] -= 1;
        }
        ptr_ = nullptr; count_ = 0;
    }
    T *get() const { return ptr_; }
    size_t count() const { return count_; }
};

// Many device buffers with one lifetime: every alloc() is a DevBuf of its own, all of them go with the bag.  A buffer that has to
// outlive the bag is not taken out of it: it is reserved straight into a DevBuf member of its longer-lived owner.
class DevBag {
    std::vector<DevBuf<unsigned char>> bufs_;
  public:
    template <typename T>
    hipError_t alloc(T **dst, size_t count) {      // at least one element, so that *dst is never null on success
        *dst = nullptr;
        DevBuf<unsigned char> b;
        const hipError_t err = b.reserve(std::max<size_t>(count, 1) * sizeof(T));
        if (err != hipSuccess) return err;
        *dst = reinterpret_cast<T *>(b.get());
        bufs_.push_back(std::move(b));
        return hipSuccess;
    }
};

class DevEvent {
    hipEvent_t ev_ = nullptr;
  public:
    DevEvent() = default;
    DevEvent(DevEvent &&o) noexcept : ev_(o.ev_) { o.ev_ = nullptr; }
    DevEvent &operator=(DevEvent &&o) noexcept { std::swap(ev_, o.ev_); return *this; }
    ~DevEvent() { reset(); }
    hipError_t create(unsigned flags = hipEventDefault) {
        reset();
        const hipError_t err = hipEventCreateWithFlags(&ev_, flags);
        if (err != hipSuccess) ev_ = nullptr;
        return err;
    }
    void reset() { if (ev_) hipEventDestroy(ev_); ev_ = nullptr; }
    hipEvent_t get() const { return ev_; }
};

// A stream with the lifetime of one call.  Declared before the other owners of a function, it is destroyed after them: the buffers
// and events that its work uses go first.  (The pooled streams of dense.hip, which live as long as the process, are another thing.)
class DevStream {
    hipStream_t s_ = nullptr;
  public:
    DevStream() = default;
    DevStream(DevStream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    DevStream &operator=(DevStream &&o) noexcept { std::swap(s_, o.s_); return *this; }
    ~DevStream() { reset(); }
    hipError_t create(unsigned flags = hipStreamDefault) {
        reset();
        const hipError_t err = hipStreamCreateWithFlags(&s_, flags);
        if (err != hipSuccess) s_ = nullptr;
        return err;
    }
    // a stream restricted to the compute units of `mask` (`words` 32-bit words)
    hipError_t create_with_cu_mask(unsigned words, const uint32_t *mask) {
        reset();
        const hipError_t err = hipExtStreamCreateWithCUMask(&s_, words, mask);
        if (err != hipSuccess) s_ = nullptr;
        return err;
    }
    void reset() { if (s_) hipStreamDestroy(s_); s_ = nullptr; }
    hipStream_t get() const { return s_; }
};

// host memory that the device can address (hipHostMallocMapped): words a kernel and the host pass to each other while the kernel runs
template <typename T>
class HostMapped {
    T *ptr_ = nullptr;
  public:
    HostMapped() = default;
    HostMapped(HostMapped &&o) noexcept : ptr_(o.ptr_) { o.ptr_ = nullptr; }
    HostMapped &operator=(HostMapped &&o) noexcept { std::swap(ptr_, o.ptr_); return *this; }
    ~HostMapped() { reset(); }
    hipError_t alloc(size_t count) {
        reset();
        const hipError_t err = hipHostMalloc((void **)&ptr_, count * sizeof(T), hipHostMallocMapped);
        if (err != hipSuccess) ptr_ = nullptr;
        return err;
    }
    void reset() { if (ptr_) hipHostFree(ptr_); ptr_ = nullptr; }
    T *get() const { return ptr_; }
};

}  // namespace jaicov
