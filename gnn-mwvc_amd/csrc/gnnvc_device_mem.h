// gnnvc_device_mem.h — the owning handles of everything libgnnvc_hip.so gets from the HIP runtime: device buffers, page-locked
// host buffers, events and streams.  Each frees what it holds in its destructor and is move-only, so an object made of them
// (gnnvc_engine, a part of a multi-device handle, a local of a host entry point) needs no list of things to release.  Internal.
//
// A destructor never waits for work in flight: whoever destroys an object that kernels may still use synchronises its
// streams first (gnnvc_destroy, multi_destroy).
//
// Guard bands (a process-wide debug switch, off by default, reached through gnnvc_debug_probe only): while it is on, every
// buffer a handle below allocates gets kGuardBytes of a byte pattern in front of and behind it and is entered in a registry;
// a check, and every free, reads the bands back and counts those a stray store has changed.  That sees a kernel WRITING up
// to kGuardBytes past either end of one of the library's own buffers, which page-rounded allocations, a neighbouring buffer
// or a buffer left large by an earlier graph otherwise hide.  Out of scope: over-READS (DESIGN.md section 4 keeps the
// speculative reads inside the buffers' own pads), strays further than kGuardBytes, and buffers the caller owns.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <utility>

namespace gnnvc {

// Allocations and handles alive in this process: every successful allocation / creation by a handle below adds one, every
// free / destroy takes one off (gnnvc_debug_probe(nullptr, kProbeLiveObjects) reads it: "destroy frees everything" as an
// exact assertion, which free-memory readings on a shared device cannot give).
inline std::atomic<long> g_live_objects{0};
constexpr int kProbeLiveObjects = 1000;   // `kind` of gnnvc_debug_probe

// further `kind`s of gnnvc_debug_probe: the guard bands (GuardRegistry below)
constexpr int kProbeGuardsOn = 1001;          // buffers allocated from now on get bands
constexpr int kProbeGuardsOff = 1002;         // new buffers are plain again; guarded ones stay registered until freed
constexpr int kProbeGuardsCheck = 1003;       // damaged bands now + those found at frees since the last check (-1: HIP error)
constexpr int kProbeGuardsAlive = 1004;       // registered buffers alive
constexpr int kProbeGuardsHitAfter = 1005;    // test hooks: damage one byte of the newest live guarded device buffer's bands,
constexpr int kProbeGuardsHitBefore = 1006;   //   the first byte after its end / the last before its start /
constexpr int kProbeGuardsHitBandEnd = 1007;  //   the last byte of the trailing band

// 4096: a multiple of 256, so the pointer handed out keeps hipMalloc's alignment (16-byte vector accesses, 64-byte rows), and
// one 64-vertex tile of 16-wide fp32 rows, which is as far as a tile that ignores n can write.
constexpr size_t kGuardBytes = 4096;
constexpr unsigned char kGuardFill = 0xA5;   // neither 0x00 nor 0xFF: stray stores mostly write zeros and all-ones
constexpr unsigned char kGuardHit = 0x5A;    // what the test hooks write

// The registry of guarded buffers, apart from the runtime it guards memory of.  Rt supplies, as static members:
//   int device(); bool set_device(int); bool sync()                       the current device
//   bool fill(void *p, int byte, size_t n, bool pinned)                   complete when it returns
//   const unsigned char *view(const void *p, size_t n, bool pinned, unsigned char *scratch)   n <= kGuardBytes host-readable
//                                                                         bytes of p (in scratch or in place), null on error
// so tests/support/guard_host.cpp drives it over malloc memory.  Everything but on() / any() takes the mutex: a
// multi-device handle allocates from one host thread per device.  take() and check() hold it while they wait for a device and
// copy the bands back, so a guarded free on one part's thread holds up the other parts' allocations and frees meanwhile: the
// price of a debug switch, paid by nobody while it is off.  A buffer's bands are read, refilled and hit with the buffer's own
// device current, not through another device's view of them; the caller's device is current again on return.
template <class Rt>
class GuardRegistry {
    struct Entry {
        unsigned char *base;   // what the allocator gave: leading band, `bytes` of the buffer, trailing band
        size_t bytes, elem;
        int device;
        unsigned long ordinal;
        bool pinned;
        unsigned char *band(int side) const { return side ? base + kGuardBytes + bytes : base; }
    };
    std::mutex mu_;
    std::map<const void *, Entry> live_;   // by the pointer handed out: a Buffer that moves takes its entry along
    std::atomic<bool> on_{false};
    std::atomic<long> alive_{0};
    unsigned long next_ordinal_ = 0;
    long at_frees_ = 0;      // damaged bands found by take() since the last check()
    bool failed_ = false;    // a band could not be read at a free

    // the damaged bands of one buffer (one stderr line each, refilled on request); -1 if one cannot be read
    int damaged(const Entry &e, bool refill, const char *when) {
        unsigned char scratch[kGuardBytes];
        int found = 0;
        for (int side = 0; side < 2; ++side) {
            const unsigned char *b = Rt::view(e.band(side), kGuardBytes, e.pinned, scratch);
            if (!b) return -1;
            size_t at = 0;
            while (at < kGuardBytes && b[at] == kGuardFill) ++at;
            if (at == kGuardBytes) continue;
            ++found;
            std::fprintf(stderr, "gnnvc guard (%s): buffer #%lu, %zu bytes, element size %zu, device %d%s: %s band damaged, "
                         "first at offset %zu, value 0x%02x\n", when, e.ordinal, e.bytes, e.elem, e.device,
                         e.pinned ? ", page-locked" : "", side ? "trailing" : "leading", at, (unsigned)b[at]);
            if (refill && !Rt::fill(e.band(side), kGuardFill, kGuardBytes, e.pinned)) return -1;
        }
        return found;
    }

public:
    bool on() const { return on_.load(std::memory_order_relaxed); }
    bool any() const { return alive_.load(std::memory_order_relaxed) != 0; }
    void set(bool v) { on_.store(v, std::memory_order_relaxed); }
    long alive() const { return alive_.load(std::memory_order_relaxed); }

    // `base` holds bytes + 2 * kGuardBytes, fresh from the allocator: fills the bands and registers it.  The pointer to hand
    // out, or null if the bands could not be filled (the caller then frees base).
    void *adopt(void *base, size_t bytes, size_t elem, bool pinned) {
        Entry e{static_cast<unsigned char *>(base), bytes, elem, Rt::device(), 0, pinned};
        if (!Rt::fill(e.band(0), kGuardFill, kGuardBytes, pinned) || !Rt::fill(e.band(1), kGuardFill, kGuardBytes, pinned))
            return nullptr;
        std::lock_guard<std::mutex> lock(mu_);
        e.ordinal = next_ordinal_++;
        void *user = e.base + kGuardBytes;
        live_[user] = e;
        alive_.store((long)live_.size(), std::memory_order_relaxed);
        return user;
    }

    // a buffer about to be freed: if it is registered, checks its bands (the damage shows in the next check()), forgets it
    // and returns what to give back to the allocator; null for a plain buffer
    void *take(void *user) {
        std::lock_guard<std::mutex> lock(mu_);
        auto it = live_.find(user);
        if (it == live_.end()) return nullptr;
        const Entry e = it->second;
        live_.erase(it);
        alive_.store((long)live_.size(), std::memory_order_relaxed);
        const int cur = Rt::device();   // (the free that follows waits for the buffer's device anyway)
        const bool there = cur == e.device || Rt::set_device(e.device);
        const int found = there && Rt::sync() ? damaged(e, false, "free") : -1;
        if (cur != e.device) (void)Rt::set_device(cur);
        if (found < 0) failed_ = true;
        else at_frees_ += found;
        return e.base;
    }

    // waits for every device that holds a registered buffer, reads all bands, refills the damaged ones: their number plus
    // those found at frees since the last call (that count is cleared), or -1 on a runtime error
    long check() {
        std::lock_guard<std::mutex> lock(mu_);
        bool ok = !std::exchange(failed_, false);
        const int cur = Rt::device();
        std::set<int> devices;
        for (const auto &kv : live_) devices.insert(kv.second.device);
        for (int d : devices) ok = Rt::set_device(d) && Rt::sync() && ok;   // all of them first: a part may write into a peer's buffer
        long total = std::exchange(at_frees_, 0);
        for (int d : devices) {
            if (!Rt::set_device(d)) {
                ok = false;
                continue;
            }
            for (const auto &kv : live_) {
                if (kv.second.device != d) continue;
                const int found = damaged(kv.second, true, "check");
                if (found < 0) ok = false;
                else total += found;
            }
        }
        if (!devices.empty()) ok = Rt::set_device(cur) && ok;
        return ok ? total : -1;
    }

    // the test hooks: one byte of the newest live guarded device buffer's bands; false if there is no such buffer
    bool hit(int kind) {
        std::lock_guard<std::mutex> lock(mu_);
        const Entry *newest = nullptr;
        for (const auto &kv : live_)
            if (!kv.second.pinned && (!newest || kv.second.ordinal > newest->ordinal)) newest = &kv.second;
        if (!newest) return false;
        unsigned char *at = kind == kProbeGuardsHitAfter    ? newest->band(1)
                            : kind == kProbeGuardsHitBefore ? newest->band(0) + kGuardBytes - 1
                                                            : newest->band(1) + kGuardBytes - 1;
        const int cur = Rt::device();
        const bool done = (cur == newest->device || Rt::set_device(newest->device)) && Rt::fill(at, kGuardHit, 1, false);
        if (cur != newest->device) (void)Rt::set_device(cur);
        return done;
    }

    // gnnvc_debug_probe's kinds kProbeGuardsOn .. kProbeGuardsHitBandEnd
    int probe(int kind) {
        switch (kind) {
        case kProbeGuardsOn: set(true); return 0;
        case kProbeGuardsOff: set(false); return 0;
        case kProbeGuardsCheck: return (int)check();
        case kProbeGuardsAlive: return (int)alive();
        default: return hit(kind) ? 0 : -1;
        }
    }
};
template <class Rt>
inline GuardRegistry<Rt> g_guards;

namespace mem_detail {

struct HipRuntime {
    static int device() {
        int d = 0;
        (void)hipGetDevice(&d);
        return d;
    }
    static bool set_device(int d) { return hipSetDevice(d) == hipSuccess; }
    static bool sync() { return hipDeviceSynchronize() == hipSuccess; }
    static bool fill(void *p, int byte, size_t n, bool pinned) {
        if (pinned) {
            std::memset(p, byte, n);
            return true;
        }
        return hipMemset(p, byte, n) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess;
    }
    static const unsigned char *view(const void *p, size_t n, bool pinned, unsigned char *scratch) {
        if (pinned) return static_cast<const unsigned char *>(p);
        return hipMemcpy(scratch, p, n, hipMemcpyDeviceToHost) == hipSuccess ? scratch : nullptr;
    }
};

struct DeviceAlloc {
    using runtime = HipRuntime;
    static constexpr bool pinned = false;
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void *p) { (void)hipFree(p); }
    static size_t room(size_t count) { return count; }
    static size_t floor(size_t count) { return std::max<size_t>(count, 1); }
};
struct PinnedAlloc {
    using runtime = HipRuntime;
    static constexpr bool pinned = true;
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
        const size_t bytes = A::floor(want) * sizeof(T);
        auto &guards = g_guards<typename A::runtime>;
        hipError_t rc;
        if (!guards.on()) {
            rc = A::alloc(reinterpret_cast<void **>(&p), bytes);
        } else {   // (the trailing band starts at the first byte after `bytes`, aligned or not)
            void *base = nullptr;
            rc = A::alloc(&base, bytes + 2 * kGuardBytes);
            if (rc == hipSuccess && !(p = static_cast<T *>(guards.adopt(base, bytes, sizeof(T), A::pinned)))) {
                A::free(base);
                rc = hipErrorUnknown;
            }
        }
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
            auto &guards = g_guards<typename A::runtime>;
            void *base = guards.any() ? guards.take(p) : nullptr;
            A::free(base ? base : p);
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
