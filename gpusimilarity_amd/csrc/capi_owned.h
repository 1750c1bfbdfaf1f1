// capi_owned.h -- the owning types of the C-ABI implementation: device and pinned-host buffers, events, streams.  Every
// hipMalloc / hipHostMalloc / hipFree / hipHostFree / hipEventDestroy / hipStreamDestroy of capi_*.cpp is in here.  All types
// are move-only and release in their destructor; none knows about streams: whoever frees or grows a buffer a kernel may
// still use drains the stream first.  Depends on the HIP runtime API alone (tests/cpp/owned_check.cpp includes it by itself).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace gsim_host
{

// Device memory (kPinned = false) or pinned host memory (hipHostMalloc with the flags given at construction).  Converts to
// T* where a pointer is wanted -- a kernel argument, `buf + 15`, `*buf`, `if (buf)` -- and has no operator bool, which would
// make those ambiguous.
template <class T, bool kPinned> class OwnedBuf
{
    T* p_ = nullptr;
    size_t bytes_ = 0;
    unsigned flags_ = 0;

    hipError_t allocate(size_t bytes, void** out) const
    {
        *out = nullptr;
        const size_t n = bytes ? bytes : 16; // (never a zero-byte allocation)
        hipError_t e;
        if constexpr (kPinned) e = hipHostMalloc(out, n, flags_);
        else e = hipMalloc(out, n);
        if (e != hipSuccess) {
            (void) hipGetLastError(); // (the caller gets the code; nothing stays behind for a later hipGetLastError)
            *out = nullptr;
        }
        return e;
    }
    void adopt(void* p, size_t bytes)
    {
        reset();
        p_ = static_cast<T*>(p);
        bytes_ = bytes;
    }

public:
    OwnedBuf() = default;
    explicit OwnedBuf(unsigned host_flags) : flags_(host_flags) {}
    OwnedBuf(OwnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)), flags_(o.flags_) {}
    OwnedBuf& operator=(OwnedBuf&& o) noexcept
    {
        if (this != &o) {
            adopt(std::exchange(o.p_, nullptr), std::exchange(o.bytes_, 0));
            flags_ = o.flags_;
        }
        return *this;
    }
    ~OwnedBuf() { reset(); }

    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    template <class U> U* as() const { return static_cast<U*>(static_cast<void*>(p_)); }
    size_t bytes() const { return bytes_; } // what the last grow asked for; 0 when empty

    void reset()
    {
        if (p_) {
            if constexpr (kPinned) (void) hipHostFree(p_);
            else (void) hipFree(p_);
        }
        p_ = nullptr;
        bytes_ = 0;
    }
    // The two ways to make the buffer hold at least `bytes`; neither touches a buffer that already does.  `allocated`: did
    // this call allocate (the caller's zero-fill of fresh memory hangs on it).
    // Free first -- the old and the new block may not fit side by side.  On failure the buffer is empty, bytes() == 0.
    hipError_t grow(size_t bytes, bool* allocated = nullptr)
    {
        if (allocated) *allocated = false;
        if (p_ && bytes <= bytes_) return hipSuccess;
        reset();
        return grow_keep(bytes, allocated);
    }
    // Allocate, then swap -- on failure the buffer is as it was.
    hipError_t grow_keep(size_t bytes, bool* allocated = nullptr)
    {
        if (allocated) *allocated = false;
        if (p_ && bytes <= bytes_) return hipSuccess;
        void* p = nullptr;
        const hipError_t e = allocate(bytes, &p);
        if (e != hipSuccess) return e;
        adopt(p, bytes);
        if (allocated) *allocated = true;
        return hipSuccess;
    }
};

template <class T = void> struct DevBuf : OwnedBuf<T, false> {
};
template <class T = void> struct HostBuf : OwnedBuf<T, true> {
    using OwnedBuf<T, true>::OwnedBuf;
};

// An event or a stream of our own making
template <class H, hipError_t (*kDestroy)(H)> struct OwnedHandle {
    H h = nullptr;
    OwnedHandle() = default;
    OwnedHandle(OwnedHandle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    OwnedHandle& operator=(OwnedHandle&& o) noexcept
    {
        if (this != &o) {
            reset();
            h = std::exchange(o.h, nullptr);
        }
        return *this;
    }
    ~OwnedHandle() { reset(); }
    void reset()
    {
        if (h) (void) kDestroy(h);
        h = nullptr;
    }
    operator H() const { return h; }
};

struct Event : OwnedHandle<hipEvent_t, hipEventDestroy> {
    // made on first use: nothing happens when it exists already
    hipError_t create(unsigned flags = hipEventDefault) { return h ? hipSuccess : hipEventCreateWithFlags(&h, flags); }
};

struct Stream : OwnedHandle<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags) { return h ? hipSuccess : hipStreamCreateWithFlags(&h, flags); }
};

struct EventPair {
    Event a, b;
    hipError_t create()
    {
        const hipError_t e = a.create();
        return e == hipSuccess ? b.create() : e;
    }
    double ms() const
    {
        float t = 0.0f;
        return hipEventElapsedTime(&t, a, b) == hipSuccess ? static_cast<double>(t) : 0.0;
    }
};

} // namespace gsim_host
