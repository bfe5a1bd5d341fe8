// Owning HIP handles (host only): what a member of one of these types holds is released when the member goes, so a
// destroy function lists nothing.  One move-only core, Owned<H, Release>; device memory, page-locked host memory,
// streams and events on top of it; a growable buffer and a typed array on top of those.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

namespace iqd {

// Holds one handle, releases it in the destructor and on reset(), empty (H{}) after a move.
template <class H, void (*Release)(H)>
class Owned {
    H h_{};

public:
    Owned() = default;
    Owned(Owned &&o) noexcept : h_(o.h_) { o.h_ = H{}; }
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) {
            reset();
            h_ = o.h_;
            o.h_ = H{};
        }
        return *this;
    }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { reset(); }
    void reset()
    {
        if (h_) Release(h_);
        h_ = H{};
    }
    H *put()   // for the create / allocate calls, which write a handle: releases what it held
    {
        reset();
        return &h_;
    }
    H get() const { return h_; }
    operator H() const { return h_; }
};

struct DeviceAlloc {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void release(void *p) { (void)hipFree(p); }
};
struct PinnedAlloc {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void release(void *p) { (void)hipHostFree(p); }
};
inline void release_stream(hipStream_t s) { (void)hipStreamDestroy(s); }
inline void release_event(hipEvent_t e) { (void)hipEventDestroy(e); }

using Stream = Owned<hipStream_t, release_stream>;
using Event = Owned<hipEvent_t, release_event>;

// A buffer that grows on demand and never shrinks.  Want(bytes) is what a growth allocates: the capacity shows in memory
// use and decides when p moves, so each buffer's policy is part of its type.
inline size_t grow_headroom(size_t bytes) { return bytes + bytes / 8 + 256; }
inline size_t grow_exact(size_t bytes) { return bytes; }

template <class A, size_t (*Want)(size_t)>
struct GrowBuf {
    Owned<void *, A::release> p;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        cap = 0;
        const size_t want = Want(bytes);
        hipError_t e = A::alloc(p.put(), want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    template <class T> T *as() const { return (T *)p.get(); }
};
using DevBuf = GrowBuf<DeviceAlloc, grow_headroom>;     // the engine's and its resamplers'
using DevBufExact = GrowBuf<DeviceAlloc, grow_exact>;   // the channelizer's

// n elements of T, allocated by alloc(); reads as a T * where one is wanted.
template <class T, class A>
struct Array {
    Owned<void *, A::release> mem;
    size_t n = 0;
    hipError_t alloc(size_t count)
    {
        n = 0;
        hipError_t e = A::alloc(mem.put(), count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    operator T *() const { return (T *)mem.get(); }
};
template <class T> using DevArray = Array<T, DeviceAlloc>;
template <class T> using PinnedArray = Array<T, PinnedAlloc>;

}  // namespace iqd
