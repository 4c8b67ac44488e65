// gnnvc_device_mem.h — the owning handles of everything libgnnvc_hip.so gets from the HIP runtime: device buffers, page-locked
// host buffers, events and streams.  Each frees what it holds in its destructor and is move-only, so an object made of them
// (gnnvc_engine, a part of a multi-device handle, a local of a host entry point) needs no list of things to release.  Internal.
//
// A destructor never waits for work in flight: whoever destroys an object that kernels may still use synchronises its
// streams first (gnnvc_destroy, multi_destroy).
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <utility>

namespace gnnvc {

// Allocations and handles alive in this process: every successful allocation / creation by a handle below adds one, every
// free / destroy takes one off (gnnvc_debug_probe(nullptr, kProbeLiveObjects) reads it: "destroy frees everything" as an
// exact assertion, which free-memory readings on a shared device cannot give).
inline std::atomic<long> g_live_objects{0};
constexpr int kProbeLiveObjects = 1000;   // `kind` of gnnvc_debug_probe

namespace mem_detail {

struct DeviceAlloc {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void *p) { (void)hipFree(p); }
    static size_t room(size_t count) { return count; }
    static size_t floor(size_t count) { return std::max<size_t>(count, 1); }
};
struct PinnedAlloc {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free(void *p) { (void)hipHostFree(p); }
    static size_t room(size_t count) { return std::max<size_t>(count + count / 8, 64); }   // head-room: the driver's graphs shrink
    static size_t floor(size_t count) { return count; }
};

// `cap` elements at `p`; reserve() grows (never shrinks, contents are not kept), release() frees early
template <class T, class A>
struct Buffer {
    T *p = nullptr;
    size_t cap = 0;  // elements
    Buffer() = default;
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    Buffer(Buffer &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Buffer &operator=(Buffer &&o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~Buffer() { release(); }
    hipError_t reserve(size_t count) {   // (a device buffer's caller has made its device current)
        if (count <= cap) return hipSuccess;
        release();
        const size_t want = A::room(count);
        hipError_t rc = A::alloc(reinterpret_cast<void **>(&p), A::floor(want) * sizeof(T));
        if (rc == hipSuccess) {
            cap = want;
            g_live_objects.fetch_add(1, std::memory_order_relaxed);
        } else {
            p = nullptr;
        }
        return rc;
    }
    void release() {
        if (p) {
            A::free(p);
            g_live_objects.fetch_sub(1, std::memory_order_relaxed);
        }
        p = nullptr;
        cap = 0;
    }
};

}  // namespace mem_detail

template <class T>
using DevBuf = mem_detail::Buffer<T, mem_detail::DeviceAlloc>;
// Page-locked host staging (graph hand-off: the copy engine reads it directly, no bounce buffer).
template <class T>
using PinBuf = mem_detail::Buffer<T, mem_detail::PinnedAlloc>;

// A HIP event / stream this object made: null until create(), destroyed with it, usable wherever the raw handle is.
template <class H, hipError_t (*Destroy)(H)>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) {
            reset();
            h = std::exchange(o.h, nullptr);
        }
        return *this;
    }
    ~Owned() { reset(); }
    void reset() {
        if (h) {
            (void)Destroy(h);
            g_live_objects.fetch_sub(1, std::memory_order_relaxed);
        }
        h = nullptr;
    }
    operator H() const { return h; }

protected:
    hipError_t made(hipError_t rc) {   // the outcome of a create call that wrote h
        if (rc == hipSuccess) g_live_objects.fetch_add(1, std::memory_order_relaxed);
        else h = nullptr;
        return rc;
    }
};

struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) {
        reset();
        return made(hipEventCreateWithFlags(&h, flags));
    }
};

struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags) {
        reset();
        return made(hipStreamCreateWithFlags(&h, flags));
    }
};

}  // namespace gnnvc
