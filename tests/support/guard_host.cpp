// The guard-band registry of csrc/gnnvc_device_mem.h driven on the host: Buffer<T, A> and GuardRegistry<Rt> over a
// malloc-backed allocator and runtime, so the bookkeeping (what is registered, what a check counts, what a free counts,
// what a move does) runs under -fsanitize=address,undefined with no device.  One line per scenario on stdout, "<name>: ok"
// or "<name>: FAIL <what>"; exit status 1 if any failed (tests/test_guard_bands_host.py asserts every line).
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../gnn-mwvc_amd/csrc/gnnvc_device_mem.h"

namespace {

std::atomic<long> g_allocs{0}, g_frees{0};

struct alignas(16) float4_like {   // the 16-byte elements ((n + 1) * 16 bytes of rows, uint4 steps)
    float v[4];
};

struct HostRuntime {
    static inline thread_local int current = 0;
    static inline std::atomic<long> syncs{0};
    static inline std::vector<int> *viewed_on = nullptr;   // where asked for: the device current at each view()
    static int device() { return current; }
    static bool set_device(int d) {
        current = d;
        return true;
    }
    static bool sync() {
        syncs.fetch_add(1);
        return true;
    }
    static bool fill(void *p, int byte, size_t n, bool) {
        std::memset(p, byte, n);
        return true;
    }
    static const unsigned char *view(const void *p, size_t n, bool pinned, unsigned char *scratch) {
        if (viewed_on) viewed_on->push_back(current);   // (under the registry's mutex)
        if (pinned) return static_cast<const unsigned char *>(p);
        std::memcpy(scratch, p, n);   // (as a device buffer's bands come back)
        return scratch;
    }
};

template <bool Pinned>
struct HostAlloc {
    using runtime = HostRuntime;
    static constexpr bool pinned = Pinned;
    static hipError_t alloc(void **p, size_t bytes) {
        *p = std::malloc(bytes);
        if (*p) g_allocs.fetch_add(1);
        return *p ? hipSuccess : hipErrorOutOfMemory;
    }
    static void free(void *p) {
        g_frees.fetch_add(1);
        std::free(p);
    }
    static size_t room(size_t count) { return Pinned ? std::max<size_t>(count + count / 8, 64) : count; }
    static size_t floor(size_t count) { return Pinned ? count : std::max<size_t>(count, 1); }
};

template <class T>
using Buf = gnnvc::mem_detail::Buffer<T, HostAlloc<false>>;
template <class T>
using Pin = gnnvc::mem_detail::Buffer<T, HostAlloc<true>>;

auto &G = gnnvc::g_guards<HostRuntime>;
constexpr size_t kBand = gnnvc::kGuardBytes;

int g_failed = 0;
std::string g_why;

#define EXPECT(cond)                                                                         \
    do {                                                                                     \
        if (!(cond) && g_why.empty()) g_why = std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"; \
    } while (0)

void scenario(const char *name, void (*body)()) {
    g_why.clear();
    body();
    if (g_why.empty()) std::printf("%s: ok\n", name);
    else std::printf("%s: FAIL %s\n", name, g_why.c_str()), ++g_failed;
    std::fflush(stdout);
}

template <class B>
unsigned char *bytes_of(B &b) { return reinterpret_cast<unsigned char *>(b.p); }

void switch_on_off_on() {
    Buf<float> a, b, c, d;
    EXPECT(!G.on() && G.alive() == 0);
    EXPECT(a.reserve(10) == hipSuccess && G.alive() == 0);
    EXPECT(G.probe(gnnvc::kProbeGuardsOn) == 0 && G.on());
    EXPECT(b.reserve(10) == hipSuccess && G.alive() == 1);
    EXPECT(G.probe(gnnvc::kProbeGuardsOff) == 0 && !G.on());
    EXPECT(c.reserve(10) == hipSuccess && G.alive() == 1);
    G.set(true);
    EXPECT(d.reserve(10) == hipSuccess && G.alive() == 2);
    EXPECT(G.probe(gnnvc::kProbeGuardsAlive) == 2);
    EXPECT(G.check() == 0);
    EXPECT(gnnvc::g_live_objects.load() == 4);   // (counted alike, guarded or not)
    a.release(), b.release(), c.release(), d.release();
    EXPECT(G.alive() == 0 && G.check() == 0 && gnnvc::g_live_objects.load() == 0);
    G.set(false);
}

// one buffer of `count` elements of T: every byte of it written, the bands clean; each of the four edge bytes of the bands
// found exactly once, and refilled
template <class T, class B>
void edges_of(size_t count) {
    B b;
    EXPECT(b.reserve(count) == hipSuccess && b.p && b.cap >= count);
    const size_t bytes = std::max<size_t>(b.cap, 1) * sizeof(T);
    EXPECT(reinterpret_cast<uintptr_t>(b.p) % 16 == 0);
    std::memset(b.p, 0x00, bytes);
    EXPECT(G.check() == 0);
    std::memset(b.p, 0xFF, bytes);
    EXPECT(G.check() == 0);
    unsigned char *const lead = bytes_of(b) - kBand, *const trail = bytes_of(b) + bytes;
    for (unsigned char *at : {lead, lead + kBand - 1, trail, trail + kBand - 1}) {
        EXPECT(*at == gnnvc::kGuardFill);
        *at = 0;
        EXPECT(G.check() == 1);
        EXPECT(*at == gnnvc::kGuardFill);
        EXPECT(G.check() == 0);
    }
    lead[7] = 0xFF, lead[9] = 0, trail[1] = 0xFF;   // a band counts once, however many of its bytes changed
    EXPECT(G.check() == 2);
    EXPECT(G.check() == 0);
}

void sizes_and_edges() {
    G.set(true);
    for (size_t count : {size_t(1), size_t(3), size_t(4097)}) {
        edges_of<unsigned char, Buf<unsigned char>>(count);
        edges_of<uint16_t, Buf<uint16_t>>(count);
        edges_of<float, Buf<float>>(count);
        edges_of<float4_like, Buf<float4_like>>(count);
        edges_of<float, Pin<float>>(count);
    }
    {
        Buf<float> empty;   // (a device buffer of no elements still holds one)
        EXPECT(empty.reserve(0) == hipSuccess && empty.p == nullptr);
    }
    EXPECT(G.alive() == 0 && G.check() == 0);
    G.set(false);
}

void hooks() {
    G.set(true);
    EXPECT(G.probe(gnnvc::kProbeGuardsHitAfter) == -1);
    Pin<float> pin;
    EXPECT(pin.reserve(3) == hipSuccess);
    EXPECT(G.probe(gnnvc::kProbeGuardsHitAfter) == -1);   // (page-locked buffers are not the hooks' target)
    Buf<float> first, newest;
    EXPECT(first.reserve(5) == hipSuccess && newest.reserve(3) == hipSuccess);
    unsigned char *const p = bytes_of(newest);
    EXPECT(G.probe(gnnvc::kProbeGuardsHitAfter) == 0 && p[12] == gnnvc::kGuardHit);
    EXPECT(G.check() == 1 && G.check() == 0 && p[12] == gnnvc::kGuardFill);
    EXPECT(G.probe(gnnvc::kProbeGuardsHitBefore) == 0 && p[-1] == gnnvc::kGuardHit);
    EXPECT(G.check() == 1 && G.check() == 0);
    EXPECT(G.probe(gnnvc::kProbeGuardsHitBandEnd) == 0 && p[12 + kBand - 1] == gnnvc::kGuardHit);
    EXPECT(G.check() == 1 && G.check() == 0);
    newest.release();   // the newest LIVE one is now `first`
    EXPECT(G.probe(gnnvc::kProbeGuardsHitBefore) == 0 && bytes_of(first)[-1] == gnnvc::kGuardHit);
    EXPECT(G.check() == 1 && G.check() == 0);
    G.set(false);
}

void damage_found_at_free() {
    G.set(true);
    {
        Buf<uint16_t> b;
        EXPECT(b.reserve(3) == hipSuccess);
        bytes_of(b)[6] = 0;   // the first byte past the end
        bytes_of(b)[-1] = 0;
    }
    EXPECT(G.alive() == 0);
    EXPECT(G.check() == 2);
    EXPECT(G.check() == 0);
    G.set(false);
}

void growth() {
    G.set(true);
    const long allocs = g_allocs.load(), frees = g_frees.load();
    Buf<float> b;
    EXPECT(b.reserve(10) == hipSuccess && G.alive() == 1);
    float *const p = b.p;
    EXPECT(b.reserve(5) == hipSuccess && b.p == p && b.cap == 10 && g_allocs.load() == allocs + 1);
    bytes_of(b)[40] = 0;   // an overrun the regrowth's free must still see
    EXPECT(b.reserve(100) == hipSuccess && b.cap == 100 && G.alive() == 1);
    EXPECT(g_allocs.load() == allocs + 2 && g_frees.load() == frees + 1);
    std::memset(b.p, 0, 400);
    EXPECT(G.check() == 1 && G.check() == 0);
    EXPECT(gnnvc::g_live_objects.load() == 1);
    b.release();
    EXPECT(G.alive() == 0 && g_frees.load() == frees + 2 && gnnvc::g_live_objects.load() == 0);
    G.set(false);
}

void moves() {
    G.set(true);
    const long frees = g_frees.load();
    Buf<float> a;
    EXPECT(a.reserve(3) == hipSuccess);
    float *const p = a.p;
    bytes_of(a)[12] = 0;
    Buf<float> b(std::move(a));   // the registry goes by the pointer: nothing to update, nothing counted twice
    EXPECT(a.p == nullptr && a.cap == 0 && b.p == p && b.cap == 3 && G.alive() == 1 && g_frees.load() == frees);
    EXPECT(G.check() == 1 && G.check() == 0);
    Buf<float> c;
    EXPECT(c.reserve(7) == hipSuccess && G.alive() == 2);
    bytes_of(c)[-1] = 0;
    c = std::move(b);             // frees c's own buffer (its damage is counted there), takes b's
    EXPECT(b.p == nullptr && c.p == p && c.cap == 3 && G.alive() == 1 && g_frees.load() == frees + 1);
    EXPECT(G.check() == 1 && G.check() == 0);
    Buf<float> &same = c;
    c = std::move(same);
    EXPECT(c.p == p && G.alive() == 1);
    a.release(), b.release();
    EXPECT(G.alive() == 1);
    c.release();
    EXPECT(G.alive() == 0 && g_frees.load() == frees + 2 && G.check() == 0 && gnnvc::g_live_objects.load() == 0);
    G.set(false);
}

void threads() {
    G.set(true);
    std::atomic<int> running{2};
    std::atomic<long> bad{0}, checks{0}, steps{0};
    auto worker = [&](int seed) {
        HostRuntime::current = seed;   // (each thread its own device, as the parts of a multi-device handle)
        std::vector<Buf<uint16_t>> held(8);
        for (int i = 0; i < 1000; ++i) {
            Buf<uint16_t> &b = held[(size_t)(i * 7 + seed) % held.size()];
            b.release();
            if (b.reserve((size_t)(1 + (i * 13 + seed) % 300)) != hipSuccess) bad.fetch_add(1);
            else std::memset(b.p, 0xFF, b.cap * sizeof(uint16_t));
            steps.fetch_add(1);
        }
        held.clear();
        running.fetch_sub(1);
    };
    // the checker: one check per 50 buffers the workers have turned over, and it gives the processor away in between, so that
    // on a single core it does not take the registry's mutex again and again ahead of the workers
    std::thread t1(worker, 1), t2(worker, 2), t3([&] {
        long next = 0;
        do {
            if (steps.load() >= next) {
                if (G.check() != 0) bad.fetch_add(1);
                checks.fetch_add(1);
                next += 50;
            }
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        } while (running.load() > 0);
    });
    t1.join(), t2.join(), t3.join();
    EXPECT(bad.load() == 0 && checks.load() > 0 && checks.load() <= 41 && steps.load() == 2000);
    EXPECT(G.alive() == 0 && G.check() == 0 && gnnvc::g_live_objects.load() == 0);
    G.set(false);
}

void devices() {
    G.set(true);
    Buf<float> on0, on1;
    HostRuntime::current = 0;
    EXPECT(on0.reserve(9) == hipSuccess);
    HostRuntime::current = 1;
    EXPECT(on1.reserve(9) == hipSuccess);
    HostRuntime::current = 2;
    const long syncs = HostRuntime::syncs.load();
    std::vector<int> where;
    HostRuntime::viewed_on = &where;
    EXPECT(G.check() == 0);
    EXPECT(HostRuntime::syncs.load() == syncs + 2 && HostRuntime::current == 2);   // both waited for, the current one restored
    EXPECT((where == std::vector<int>{0, 0, 1, 1}));   // each buffer's two bands read with its own device current
    where.clear();
    bytes_of(on0)[36] = 0;
    EXPECT(G.check() == 1 && G.check() == 0 && HostRuntime::current == 2);   // ... and refilled there
    where.clear();
    EXPECT(G.probe(gnnvc::kProbeGuardsHitAfter) == 0 && HostRuntime::current == 2);   // the newest: on1
    EXPECT(G.check() == 1 && G.check() == 0);
    where.clear();
    on0.release();   // from another device's thread: waits for the buffer's device, comes back
    EXPECT(HostRuntime::syncs.load() == syncs + 11 && HostRuntime::current == 2);
    EXPECT((where == std::vector<int>{0, 0}));
    HostRuntime::viewed_on = nullptr;
    on1.release();
    HostRuntime::current = 0;
    EXPECT(G.alive() == 0);
    G.set(false);
}

void allocated_on_freed_off() {
    G.set(true);
    const long frees = g_frees.load();
    Buf<float> b, hurt;
    EXPECT(b.reserve(3) == hipSuccess && hurt.reserve(3) == hipSuccess);
    G.set(false);
    EXPECT(G.alive() == 2);
    Buf<float> plain;
    EXPECT(plain.reserve(3) == hipSuccess && G.alive() == 2);
    plain.release();   // (looked up, as the registry is not empty: not found, freed as it is)
    b.release();
    EXPECT(G.alive() == 1 && G.check() == 0);
    bytes_of(hurt)[12 + kBand - 1] = 0xFF;
    hurt.release();
    EXPECT(G.alive() == 0 && g_frees.load() == frees + 3);
    EXPECT(G.check() == 1 && G.check() == 0);
}

void nothing_left() {
    EXPECT(!G.on());
    EXPECT(G.probe(gnnvc::kProbeGuardsAlive) == 0 && G.probe(gnnvc::kProbeGuardsCheck) == 0);
    EXPECT(gnnvc::g_live_objects.load() == 0);
    EXPECT(g_allocs.load() == g_frees.load() && g_allocs.load() > 2000);
}

}  // namespace

int main() {
    scenario("switch_on_off_on", switch_on_off_on);
    scenario("sizes_and_edges", sizes_and_edges);
    scenario("hooks", hooks);
    scenario("damage_found_at_free", damage_found_at_free);
    scenario("growth", growth);
    scenario("moves", moves);
    scenario("threads", threads);
    scenario("devices", devices);
    scenario("allocated_on_freed_off", allocated_on_freed_off);
    scenario("nothing_left", nothing_left);
    return g_failed ? 1 : 0;
}
