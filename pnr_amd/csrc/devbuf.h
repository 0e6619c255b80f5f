// devbuf.h -- the one place libpnr_hip.so allocates and frees HIP memory.  DevBuf<T> owns one hipMalloc allocation, PinBuf<T> one
// hipHostMalloc allocation; both are move-only and free in their destructor, so a stage declares its buffers and returns on any
// path.  Every byte is counted in live_device_bytes / live_pinned_bytes (test tap pnr_live_bytes).
// hipFree synchronises the whole device: where a buffer is released decides timing, so reserve() never shrinks.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstdint>

namespace pnr {

inline std::atomic<int64_t> live_device_bytes{0}, live_pinned_bytes{0};

template <typename T, bool Pinned>
class Buf {
    T *p_ = nullptr;
    size_t n_ = 0; // elements allocated (at least 1 while p_ is set)
    static std::atomic<int64_t> &live() { return Pinned ? live_pinned_bytes : live_device_bytes; }

public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept { adopt(o.p_, o.n_), o.release(); }
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) adopt(o.p_, o.n_), o.release();
        return *this;
    }
    ~Buf() { reset(); }

    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    size_t count() const { return n_; }

    // releases what it holds, then allocates exactly max(count, 1) elements; empty after a failure
    hipError_t alloc(size_t count)
    {
        reset();
        const size_t n = std::max<size_t>(count, 1);
        void *q = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, n * sizeof(T));
        if (e == hipSuccess) adopt((T *)q, n);
        return e;
    }
    // grow-only: nothing happens while the capacity suffices
    hipError_t reserve(size_t count) { return p_ && n_ >= count ? hipSuccess : alloc(count); }
    void reset()
    {
        if (T *p = release()) (void)(Pinned ? hipHostFree(p) : hipFree(p));
    }
    // the hand-over of one allocation of `count` elements between owners
    void adopt(T *p, size_t count)
    {
        reset();
        p_ = p, n_ = p ? count : 0;
        live() += (int64_t)(n_ * sizeof(T));
    }
    T *release()
    {
        T *p = p_;
        live() -= (int64_t)(n_ * sizeof(T));
        p_ = nullptr, n_ = 0;
        return p;
    }
};

template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinBuf = Buf<T, true>;

} // namespace pnr
