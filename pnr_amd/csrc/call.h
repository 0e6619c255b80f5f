// call.h -- the staging of one bounded call on the context's stream: its device buffers as typed parts of ONE allocation, and the chain
// of HIP calls with one sticky error; timed() is a launch under a timer group of its own.  Users: the volume and tree tools (volume, radius, filter, distance, join, render, components, edt,
// geodesic, geojoin, morph, watershed and the rounds they share in tilework, threshold, prune), the side stages (recon, soma), the test taps (frangi.hip: eigen, hessian, gaussian, the direction volumes; smc.hip:
// expf) and the uploads and read-backs of the api*.cpp files.
#pragma once
#include "ctx.h"

namespace pnr {

// the one out-of-memory exit: "<who>: device allocation of <bytes> B [<what>] failed".  Grow-only (an empty buffer is allocated).
template <typename T>
int dev_alloc(DevBuf<T> &buf, size_t count, const char *who, const char *what = nullptr)
{
    if (buf.reserve(count) == hipSuccess) return PNR_OK;
    (void)hipGetLastError();
    set_error("%s: device allocation of %zu B%s%s failed", who, count * sizeof(T), what ? " " : "", what ? what : "");
    return PNR_E_NOMEM;
}

// the way out of a call that has work queued on st when a HIP call fails
inline int hip_fail(hipStream_t st, const char *who, hipError_t e)
{
    (void)hipStreamSynchronize(st);
    set_error("%s: %s", who, hipGetErrorString(e));
    return PNR_E_HIP;
}

class CallBuf;
// `count` elements of T inside a CallBuf; a T * once the CallBuf is allocated
template <typename T>
struct Part {
    const CallBuf *buf = nullptr;
    size_t off = 0, count = 0;
    T *get() const;
    operator T *() const { return get(); }
};

// All device buffers of one call as ONE DevBuf (pnr_live_bytes sees one allocation, which ends with its owner): add<T>() the parts --
// each starts on a 16-byte boundary --, alloc() once.
class CallBuf {
    DevBuf<char> buf_;
    size_t bytes_ = 0;

public:
    CallBuf() = default;
    CallBuf(const CallBuf &) = delete; // (the parts point at it)
    template <typename T>
    Part<T> add(size_t count)
    {
        const Part<T> p{this, bytes_, count};
        bytes_ += (count * sizeof(T) + 15) & ~(size_t)15;
        return p;
    }
    int alloc(const char *who) { return dev_alloc(buf_, bytes_, who); }
    char *base() const { return buf_.get(); }
};
template <typename T>
T *Part<T>::get() const { return (T *)(buf->base() + off); }

// The HIP calls of one tool call on c's stream.  After the first failure every further call is a no-op; finish() reports it.
class Call {
    pnr_ctx *c_;
    const char *who_;
    hipStream_t st_;
    hipError_t e_ = hipSuccess;

public:
    Call(pnr_ctx *c, const char *who) : c_(c), who_(who), st_(c->stream) {}
    hipStream_t stream() const { return st_; }
    bool ok() const { return e_ == hipSuccess; }
    void note(hipError_t e) // the result of a HIP call made elsewhere (pairmin.h pair_sweep)
    {
        if (ok()) e_ = e;
    }
    // the byte sizes come from the device side: a part's count, or `count` elements of T
    template <typename T>
    void up(T *dst, const void *src, size_t count) { if (ok()) e_ = hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, st_); }
    template <typename T>
    void up(const Part<T> &dst, const void *src) { up(dst.get(), src, dst.count); }
    template <typename T>
    void down(void *dst, const T *src, size_t count) { if (ok()) e_ = hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, st_); }
    template <typename T>
    void down(void *dst, const Part<T> &src) { down(dst, (const T *)src.get(), src.count); }
    template <typename T>
    void fill(T *dst, int byte, size_t count) { if (ok()) e_ = hipMemsetAsync(dst, byte, count * sizeof(T), st_); }
    template <typename T>
    void fill(const Part<T> &dst, int byte) { fill(dst.get(), byte, dst.count); }
    struct Lds { size_t bytes; }; // dynamic LDS of a launch, in front of the kernel's arguments
    template <typename... P, typename... A>
    void launch(void (*kernel)(P...), dim3 grid, dim3 block, Lds lds, const A &...args)
    {
        if (!ok()) return;
        hipLaunchKernelGGL(kernel, grid, block, lds.bytes, st_, args...);
        e_ = hipGetLastError();
    }
    template <typename... P, typename... A>
    void launch(void (*kernel)(P...), dim3 grid, dim3 block, const A &...args) { launch(kernel, grid, block, Lds{0}, args...); }
    // one launch as one entry of the timer group: tic, launch, toc(group, 1) on the call's context
    template <typename... P, typename... A>
    void timed(const char *group, void (*kernel)(P...), dim3 grid, dim3 block, Lds lds, const A &...args)
    {
        c_->tic();
        launch(kernel, grid, block, lds, args...);
        c_->toc(group, 1);
    }
    template <typename... P, typename... A>
    void timed(const char *group, void (*kernel)(P...), dim3 grid, dim3 block, const A &...args) { timed(group, kernel, grid, block, Lds{0}, args...); }
    // synchronises the stream: PNR_OK, or the first failure through hip_fail
    int finish()
    {
        if (ok()) e_ = hipStreamSynchronize(st_);
        return ok() ? PNR_OK : hip_fail(st_, who_, e_);
    }
};

} // namespace pnr
