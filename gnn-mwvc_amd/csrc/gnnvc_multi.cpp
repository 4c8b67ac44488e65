// gnnvc_multi.cpp — several devices behind ONE handle of the C ABI (gnnvc_create_multi, include/gnnvc.h).
//
// SURVEY.md §8b's minimum surface has `gnnvc_create(..., int n_devices)` and §5 "one process driving 8 devices": the
// reference's only call site, m.predict(x, out, g) (src/GNN_VC.cpp:192, include/gnn_inference.hpp:50), is one thread in
// one process, so a drop-in that wants more than one GPU has to partition behind that call.  This file does: the graph
// handed to the front handle is cut into P contiguous row ranges of equal entry count, device r gets
// the CSR slice of its rows (global column ids) and full-size replicated feature buffers, and every device is driven by
// a HOST THREAD OF ITS OWN through the public ABI (round 4: one thread issuing for eight devices was host-bound — a stage
// of a part is a few dozen launches).  A stage of a part is computed in pieces; each piece's rows are PACKED to their
// live columns (gnnvc_pack_rows: 16 bytes a row on the metric graph instead of 64, + a short exception list — lossless,
// verified per forward) and pushed into every peer's receive buffer by ONE kernel whose stores cross the xGMI mesh
// (gnnvc_push_piece: one link per peer, no ring, no host hop, no copy call per peer), on a stream of its own so that it
// runs under the next piece's kernels; a receiver expands the pieces of all its peers with one launch per piece index
// (gnnvc_unpack_pieces).  Parts synchronise through HIP events only; the host threads only tell each other when an
// event has been recorded.  A row is still summed on one device in stored order: the bits are those of the
// single-device engine.  No reference counterpart.
//
// All of that is the TRAINED model's route (forward_part).  A model that is a generic stage list (gnnvc_create_multi_generic)
// takes a route of its own, forward_part_generic: S stages of any widths, full rows to every peer (gnnvc_push_rows), no packing.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "../../include/gnnvc.h"
#include "gnnvc_device_mem.h"
#include "gnnvc_multi.h"
#include "gnnvc_options.h"

namespace gnnvc {

namespace {

constexpr int kMaxPieces = 8;
constexpr uint32_t kExcWordsPerEntry = 4;   // {row - row_lo, column, value bits, 0}

// how the rows of one exchanged stage travel: the `kp` densest columns (mask) + an exception list of room `cap` per piece
struct Packing {
    bool known = false;   // decided for the current graph (by its first forward)
    bool on = false;      // packed; false = full 64-byte rows straight into the peers' feature buffers
    uint32_t mask = 0, kp = 0, cap = 0;
};

struct Part {
    int index = 0, device = 0;
    gnnvc_engine *eng = nullptr;
    hipStream_t stream = nullptr;   // the ENGINE'S OWN stream (its side queue was probed against it, gnnvc_create)
    Stream copy;                    // pushes: under the next piece's kernels
    uint32_t lo = 0, hi = 0;
    uint64_t nnz = 0;
    int pieces = 1;
    uint32_t cut[kMaxPieces + 1] = {0};   // piece k = rows [cut[k], cut[k + 1])
    DevBuf<uint32_t> rowptr, col, w, nw;
    DevBuf<float> x, h[2], scores, logits;
    DevBuf<float> send[2], recv[2];       // packed pieces of stage s: mine / my peers'
    DevBuf<uint32_t> flag;                // [2]: gnnvc_pack_rows' flags of stage 0 / 1
    PinBuf<uint32_t> flag_pin;            // (page-locked) their copy for the host
    Event packed[2][kMaxPieces];          // piece k of stage s is computed (and packed): on `stream`
    Event pushed[2][kMaxPieces];          // ... and has reached every peer: on `copy`
    Event t0, t1;                         // this part's span of the last forward (timing enabled)
    std::vector<Event> gdone, gpushed;    // the generic route's, [s * kMaxPieces + k] for its S - 1 exchanged stages: computed / at every peer
    uint64_t counts[2][16] = {{0}};                   // first forward on a graph: non-zeros per column of my rows of stage s
    int rc = GNNVC_OK;                                // of the job at hand
    std::string err;
    float span_ms = 0.0f;
    std::thread th;
};

enum Job { kIdle = 0, kUpload = 1, kForward = 2, kQuit = 3 };

}  // namespace

struct MultiState {
    std::vector<Part> parts;
    uint32_t n = 0;
    uint64_t nnz = 0;
    bool have_graph = false;
    int stages = 0;
    double last_ms = 0.0;
    // the generic route (gnnvc_create_multi_generic, a model that is a generic stage list): forward_part_generic instead of
    // forward_part, full rows of any width instead of the 16-wide codec
    bool generic = false;
    std::vector<int> gw_out;     // stage s writes rows of gw_out[s] floats
    std::vector<char> gdense;    // stage s has no graph layer (admitted at s = 0 only, multi_create)
    int in_width = 1, out_width = 1, wmax = 1;   // wmax: the widest intermediate stage output (the ping-pong buffers' row)
    bool ends_in_sigmoid = true;
    bool fw_audit = false;       // this forward is audited: k_audit_any right behind every piece's stage call
    bool peer_stores = true;     // every pair of distinct devices can store into each other's memory
    // options (gnnvc_set_option on the front handle: keys "multi_*", and what the front hands on — kMultiRows)
    struct Opts {
        int pieces = 0;          // pieces per part and stage: 0 = by the number of parts
        int pack = 1;            // 0 = full rows always
        int push = 1;            // 0 = hipMemcpyPeerAsync per peer instead of the push kernel
        int only_part = -1;      // >= 0: a forward runs THIS part's share only (timing rehearsal on one device; results are not complete)
        int poison = 0;          // "poison_features": a forward starts by filling every part's feature buffers with NaN bit patterns (tests, fuzz)
        int audit_repair = 0;    // "audit_repair" (also set on every part): a part's mismatch repaired is no failure of the forward
        int announce = -1;       // a part announces a 16-wide stage's complete input (compact table over its rows): -1 = up to 4 parts, 0 / 1
    } opt;
    bool parts_audit = false;    // the parts' "audit_period" is 1 (this forward is audited) — the handle counts the calls
    int audit_last_part = -1;    // the first failing part of the last forward whose audit failed
    Packing pk[2];
    std::vector<uint64_t> region_words[2];   // [r * kMaxPieces + k]: words of part r's piece k of stage s (dense + list)
    std::vector<uint64_t> region_pre[2];     // prefix over (r, k) in that order
    std::vector<uint64_t> part_words[2];     // all pieces of part r
    // the workers
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    uint64_t gen = 0;
    int job = kIdle, pending = 0;
    // the job's arguments
    const uint64_t *up_rp64 = nullptr;
    const uint32_t *up_rp32 = nullptr, *up_col = nullptr, *up_w = nullptr, *up_nw = nullptr;
    const float *fw_x = nullptr;
    float *fw_scores = nullptr, *fw_logits = nullptr;
    uint64_t epoch = 0;
    std::atomic<int> failed{0};
    // rec[(r * 2 + s) * kMaxPieces + k] = epoch in which part r recorded pushed[s][k] (host-side order of record and wait)
    std::vector<std::atomic<uint64_t>> rec;
    // a barrier of the workers inside a job (first forward on a graph: the packing is chosen from every part's counts)
    std::mutex bar_mu;
    std::condition_variable bar_cv;
    int bar_count = 0;
    uint64_t bar_gen = 0;
};

namespace {

int hip_fail(std::string &err, hipError_t rc, const char *what) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(rc));
    err = buf;
    return rc == hipErrorOutOfMemory ? GNNVC_ERR_NOMEM : GNNVC_ERR_DEVICE;
}

#define MTRY(call)                                                  \
    do {                                                            \
        hipError_t rc_ = (call);                                    \
        if (rc_ != hipSuccess) return hip_fail(err, rc_, #call);    \
    } while (0)

int part_fail(std::string &err, const Part &p, int rc, const char *what) {
    char buf[512];
    snprintf(buf, sizeof buf, "device %d: %s: %s", p.device, what, p.eng ? gnnvc_last_error(p.eng) : "");
    err = buf;
    return rc;
}

#define PTRY(p, call, what)                                           \
    do {                                                              \
        int rc_ = (call);                                             \
        if (rc_ != GNNVC_OK) return part_fail(err, (p), rc_, what);   \
    } while (0)

// every worker of the job meets here; false = the job has failed somewhere (nobody waits for a part that gave up)
bool barrier(MultiState *m, int parties) {
    std::unique_lock<std::mutex> lk(m->bar_mu);
    const uint64_t g = m->bar_gen;
    if (++m->bar_count == parties) {
        m->bar_count = 0;
        ++m->bar_gen;
        m->bar_cv.notify_all();
    } else {
        while (m->bar_gen == g && !m->failed.load(std::memory_order_acquire)) m->bar_cv.wait_for(lk, std::chrono::milliseconds(2));
    }
    return !m->failed.load(std::memory_order_acquire);
}

void fail_job(MultiState *m) {
    m->failed.store(1, std::memory_order_release);
    std::lock_guard<std::mutex> lk(m->bar_mu);
    m->bar_cv.notify_all();
}

// the generic route's description of the model, from part 0's stage list (every part read the same text under the same config), and
// what is sized by it: the events and the `rec` cells of its S - 1 exchanges
int describe_generic(MultiState *m, std::string &err) {
    gnnvc_engine *e0 = m->parts[0].eng;
    const int S = m->stages;
    m->gw_out.assign((size_t)S, 0);
    m->gdense.assign((size_t)S, 0);
    m->in_width = gnnvc_in_width(e0);
    m->out_width = gnnvc_out_width(e0);
    m->wmax = 1;
    for (int s = 0; s < S; ++s) {
        int fin = 0, fout = 0;
        long dense = 0, end = 0;
        const std::string at = std::to_string(s);
        if (gnnvc_stage_widths(e0, s, &fin, &fout) != GNNVC_OK || gnnvc_get_info(e0, ("generic_stage_dense_" + at).c_str(), &dense) != GNNVC_OK ||
            gnnvc_get_info(e0, ("generic_stage_end_" + at).c_str(), &end) != GNNVC_OK) {
            err = "reading the generic stage list failed";
            return GNNVC_ERR_STATE;
        }
        // the ordering invariant (forward_part_generic) holds for the admitted pattern [P] S*: the one stage that does not wait for
        // its peers, a dense one, stands at position 0 only
        if (dense && s > 0) {
            err = "a dense stage behind the first one: the exchange's ordering does not cover it";
            return GNNVC_ERR_UNSUPPORTED;
        }
        m->gw_out[(size_t)s] = fout;
        m->gdense[(size_t)s] = dense ? 1 : 0;
        if (s + 1 < S) m->wmax = std::max(m->wmax, fout);
        if (s + 1 == S) m->ends_in_sigmoid = end == 1;
    }
    const size_t cells = (size_t)std::max(S - 1, 1) * kMaxPieces;
    m->rec = std::vector<std::atomic<uint64_t>>(m->parts.size() * cells);
    for (auto &c : m->rec) c.store(0);
    for (Part &p : m->parts) {
        hipError_t h = hipSetDevice(p.device);
        p.gdone.resize((size_t)(S - 1) * kMaxPieces);
        p.gpushed.resize((size_t)(S - 1) * kMaxPieces);
        for (size_t i = 0; i < p.gdone.size() && h == hipSuccess; ++i) {
            h = p.gdone[i].create(hipEventDisableTiming);
            if (h == hipSuccess) h = p.gpushed[i].create(hipEventDisableTiming);
        }
        if (h != hipSuccess) return hip_fail(err, h, "event creation");
    }
    m->generic = true;
    return GNNVC_OK;
}

int pieces_for(const MultiState *m) {
    const int P = (int)m->parts.size();
    if (P <= 1) return 1;
    if (m->opt.pieces > 0) return std::min(m->opt.pieces, kMaxPieces);
    // up to 4 parts a part's rows are many enough for the per-rank plans (LDS table over the slice, announced compact table:
    // whole-range calls — measured per-rank compute, metric graph: P = 4 2.02 ms on the plans against 2.88 in plain pieces);
    // beyond, four plain pieces whose pushes run under the next piece's kernels (P = 8: 1.48 plain against 1.67 on the plans)
    return P <= 4 ? 1 : 4;
}

// piece k of a part = rows [cut[k], cut[k + 1]): K nearly equal ranges of its rows, cut at multiples of 64 rows
void cut_pieces(Part &p, int K) {
    p.pieces = K;
    for (int k = 0; k <= K; ++k) {
        const uint64_t at = p.lo + (uint64_t)(p.hi - p.lo) * k / K;
        p.cut[k] = k == K ? p.hi : (uint32_t)std::min<uint64_t>(p.hi, std::max<uint64_t>(p.lo, at / 64u * 64u));
    }
    for (int k = 1; k < K; ++k) p.cut[k] = std::max(p.cut[k], p.cut[k - 1]);
}

// ---- the packing of one exchanged stage, from the non-zeros per column of ALL rows (every part computes the same choice)
Packing choose_packing(const uint64_t (&counts)[16], uint32_t n, int total_pieces, bool allow) {
    Packing pk;
    pk.known = true;
    if (!allow || n == 0) return pk;
    int order[16];
    for (int c = 0; c < 16; ++c) order[c] = c;
    std::stable_sort(order, order + 16, [&](int a, int b) { return counts[a] > counts[b]; });
    double best_cost = 1e30;
    uint32_t best_kp = 0;
    uint64_t best_rest = 0;
    for (uint32_t kp = 4; kp <= 12; kp += 4) {
        uint64_t rest = 0;
        for (uint32_t i = kp; i < 16; ++i) rest += counts[order[i]];
        const double cost = 4.0 * kp + 16.0 * (double)rest / (double)n;   // bytes per row: dense part + its share of the list
        if (cost < best_cost) {
            best_cost = cost;
            best_kp = kp;
            best_rest = rest;
        }
    }
    if (best_cost > 48.0) return pk;   // (nothing beats three quarters of a full row: ship full rows)
    pk.on = true;
    pk.kp = best_kp;
    for (uint32_t i = 0; i < best_kp; ++i)
        if (counts[order[i]] > 0) pk.mask |= 1u << order[i];
    pk.cap = (uint32_t)std::min<uint64_t>(2 * best_rest / (uint64_t)std::max(total_pieces, 1) + 1024, 1u << 28);   // twice a piece's expected share, plus slack
    return pk;
}

uint64_t piece_words(const Packing &pk, uint32_t rows) { return (uint64_t)rows * pk.kp + 4 + (uint64_t)kExcWordsPerEntry * pk.cap; }

// region of part r's piece k inside the receive buffer of part q (q != r): the pieces of all parts but q in (part, piece) order
uint64_t recv_offset(const MultiState *m, int s, int q, int r, int k) {
    const uint64_t at = m->region_pre[s][(size_t)r * kMaxPieces + k];
    return r > q ? at - m->part_words[s][(size_t)q] : at;
}

void layout_stage(MultiState *m, int s) {
    const size_t P = m->parts.size();
    m->region_words[s].assign(P * kMaxPieces, 0);
    m->region_pre[s].assign(P * kMaxPieces + 1, 0);
    m->part_words[s].assign(P, 0);
    uint64_t at = 0;
    for (size_t r = 0; r < P; ++r)
        for (int k = 0; k < kMaxPieces; ++k) {
            const Part &p = m->parts[r];
            const uint64_t wds = (m->pk[s].on && k < p.pieces) ? piece_words(m->pk[s], p.cut[k + 1] - p.cut[k]) : 0;
            m->region_words[s][r * kMaxPieces + k] = wds;
            m->region_pre[s][r * kMaxPieces + k] = at;
            at += wds;
            m->part_words[s][r] += wds;
        }
    m->region_pre[s][P * kMaxPieces] = at;
}

// ------------------------------------------------------------------ one part's share of a hand-off
int upload_part(MultiState *m, Part &p, std::string &err) {
    const uint32_t n = m->n;
    auto rp = [&](uint32_t u) -> uint64_t { return m->up_rp64 ? m->up_rp64[u] : (uint64_t)m->up_rp32[u]; };
    const uint32_t rows = p.hi - p.lo;
    const uint64_t first = n ? rp(p.lo) : 0;
    // (the slices' device-side checks see relative row pointers: every part checks its own range of the global array)
    for (uint32_t u = p.lo; u < p.hi; ++u)
        if (rp(u) > rp(u + 1)) {
            err = "row pointers are not monotone from 0 to nnz";
            return GNNVC_ERR_INVALID;
        }
    MTRY(hipSetDevice(p.device));
    MTRY(p.rowptr.reserve((size_t)rows + 1));
    MTRY(p.col.reserve((size_t)p.nnz + GNNVC_COL_PAD));
    MTRY(p.w.reserve(std::max<uint32_t>(rows, 1u)));
    MTRY(p.nw.reserve(std::max<uint32_t>(rows, 1u)));
    const size_t frows = (size_t)n + 1;
    if (m->generic) {
        // every buffer a forward writes — this part's kernels or a peer's stores — is reserved HERE, never inside a forward: the
        // route needs no barrier of the workers.  Generic stages read no pad row: n rows each.
        MTRY(p.x.reserve((size_t)n * (size_t)m->in_width));
        if (m->stages > 1)
            for (auto &h : p.h) MTRY(h.reserve((size_t)n * (size_t)m->wmax));
        MTRY(p.scores.reserve((size_t)n * (size_t)m->out_width));
        MTRY(p.logits.reserve((size_t)n * (size_t)m->out_width));
    } else {
        MTRY(p.x.reserve(frows));
        MTRY(p.h[0].reserve(frows * 16));
        MTRY(p.h[1].reserve(frows * 16));
        MTRY(p.scores.reserve(frows));
        MTRY(p.logits.reserve(frows));
        MTRY(p.flag.reserve(2));
        MTRY(p.flag_pin.reserve(4));
    }
    std::vector<uint32_t> local((size_t)rows + 1);
    for (uint32_t i = 0; i <= rows; ++i) local[i] = (uint32_t)(rp(p.lo + i) - first);
    MTRY(hipMemcpyAsync(p.rowptr.p, local.data(), ((size_t)rows + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, p.stream));
    if (p.nnz) MTRY(hipMemcpyAsync(p.col.p, m->up_col + first, (size_t)p.nnz * sizeof(uint32_t), hipMemcpyHostToDevice, p.stream));
    MTRY(hipMemsetAsync(p.col.p + p.nnz, 0, GNNVC_COL_PAD * sizeof(uint32_t), p.stream));
    if (rows) {
        MTRY(hipMemcpyAsync(p.w.p, m->up_w + p.lo, (size_t)rows * sizeof(uint32_t), hipMemcpyHostToDevice, p.stream));
        MTRY(hipMemcpyAsync(p.nw.p, m->up_nw + p.lo, (size_t)rows * sizeof(uint32_t), hipMemcpyHostToDevice, p.stream));
    }
    // the pad rows of the 16-wide feature buffers read as zero: no kernel ever writes them, once per graph will do
    if (!m->generic)
        for (auto &h : p.h) MTRY(hipMemsetAsync(h.p + (size_t)n * 16, 0, 16 * sizeof(float), p.stream));
    MTRY(hipStreamSynchronize(p.stream));   // (`local` leaves scope; the attach below reads the arrays on the same stream anyway)
    if (n == 0) return GNNVC_OK;
    PTRY(p, gnnvc_attach_graph_slice(p.eng, n, p.lo, p.hi, p.nnz, p.rowptr.p, p.col.p, p.w.p, p.nw.p), "gnnvc_attach_graph_slice");
    return GNNVC_OK;
}

// ------------------------------------------------------------------ one part's share of a forward
// wait (host side) until part r has RECORDED pushed[s][k] in this forward, then make `stream` wait for it
int wait_piece(MultiState *m, Part &me, int r, int s, int k, std::string &err) {
    std::atomic<uint64_t> &cell = m->rec[((size_t)r * 2 + s) * kMaxPieces + k];
    int spins = 0;
    while (cell.load(std::memory_order_acquire) != m->epoch) {
        if (m->failed.load(std::memory_order_acquire)) {
            err = "another part of the forward failed";
            return GNNVC_ERR_STATE;
        }
        if (++spins > 64) std::this_thread::yield();
    }
    MTRY(hipStreamWaitEvent(me.stream, m->parts[(size_t)r].pushed[s][k], 0));
    return GNNVC_OK;
}

// the rows of piece k of stage s that `me` just computed into `out`: on their way to every peer
int ship_piece(MultiState *m, Part &me, int s, int k, float *out, std::string &err) {
    const size_t P = m->parts.size();
    const Packing &pk = m->pk[s];
    const uint32_t r0 = me.cut[k], r1 = me.cut[k + 1], rows = r1 - r0;
    const bool solo = m->opt.only_part >= 0;
    if (pk.on) {
        float *region = me.send[s].p + (m->region_pre[s][(size_t)me.index * kMaxPieces + k] - m->region_pre[s][(size_t)me.index * kMaxPieces]);
        uint32_t *exc = reinterpret_cast<uint32_t *>(region + (size_t)rows * pk.kp);
        PTRY(me, gnnvc_pack_rows(me.eng, out, 16, r0, r1, pk.mask, pk.kp, region, exc, pk.cap, me.flag.p + s), "gnnvc_pack_rows");
        MTRY(hipEventRecord(me.packed[s][k], me.stream));
        MTRY(hipStreamWaitEvent(me.copy, me.packed[s][k], 0));
        if (m->opt.push && m->peer_stores) {
            float *dst[64];
            uint32_t nd = 0;
            for (size_t q = 0; q < P; ++q)
                if ((int)q != me.index) dst[nd++] = m->parts[q].recv[s].p + recv_offset(m, s, (int)q, me.index, k);
            PTRY(me, gnnvc_push_piece(me.eng, region, rows, pk.kp, pk.cap, nd, dst, me.copy), "gnnvc_push_piece");
        } else {
            for (size_t q = 0; q < P; ++q)
                if ((int)q != me.index)
                    MTRY(hipMemcpyPeerAsync(m->parts[q].recv[s].p + recv_offset(m, s, (int)q, me.index, k), m->parts[q].device, region,
                                            me.device, (size_t)m->region_words[s][(size_t)me.index * kMaxPieces + k] * sizeof(float), me.copy));
        }
    } else {
        MTRY(hipEventRecord(me.packed[s][k], me.stream));
        MTRY(hipStreamWaitEvent(me.copy, me.packed[s][k], 0));
        if (!solo)   // full rows, straight into every peer's feature buffer
            for (size_t q = 0; q < P; ++q)
                if ((int)q != me.index)
                    MTRY(hipMemcpyPeerAsync(m->parts[q].h[s & 1].p + (size_t)r0 * 16, m->parts[q].device, out + (size_t)r0 * 16, me.device,
                                            (size_t)rows * 16 * sizeof(float), me.copy));
    }
    MTRY(hipEventRecord(me.pushed[s][k], me.copy));
    m->rec[((size_t)me.index * 2 + s) * kMaxPieces + k].store(m->epoch, std::memory_order_release);
    return GNNVC_OK;
}

int forward_part(MultiState *m, Part &me, std::string &err) {
    const uint32_t n = m->n;
    const size_t P = m->parts.size();
    const int dev0 = m->parts[0].device;
    const bool solo = m->opt.only_part >= 0;
    if (solo && m->opt.only_part != me.index) return GNNVC_OK;
    MTRY(hipSetDevice(me.device));
    MTRY(hipEventRecord(me.t0, me.stream));
    MTRY(hipMemsetAsync(me.flag.p, 0, 2 * sizeof(uint32_t), me.stream));
    MTRY(hipMemcpyPeerAsync(me.x.p, me.device, m->fw_x, dev0, (size_t)n * sizeof(float), me.stream));   // the input, replicated
    for (int s = 0; s < 3; ++s) {
        const float *in = s == 0 ? me.x.p : me.h[(s - 1) & 1].p;
        float *out = s == 2 ? me.scores.p : me.h[s & 1].p;
        if (s > 0 && P > 1) {
            // this stage's input is complete on this device once every peer's pieces of the last stage have landed (and been expanded)
            const Packing &pk = m->pk[s - 1];
            for (int k = 0; k < kMaxPieces; ++k) {
                gnnvc_piece list[64];
                uint32_t nl = 0;
                for (size_t r = 0; r < P; ++r) {
                    const Part &pr = m->parts[r];
                    if ((int)r == me.index || k >= pr.pieces) continue;
                    if (!solo) {
                        int rc = wait_piece(m, me, (int)r, s - 1, k, err);
                        if (rc) return rc;
                    }
                    if (pk.on && pr.cut[k + 1] > pr.cut[k])
                        list[nl++] = gnnvc_piece{me.recv[s - 1].p + recv_offset(m, s - 1, me.index, (int)r, k), pr.cut[k], pr.cut[k + 1]};
                }
                if (nl) PTRY(me, gnnvc_unpack_pieces(me.eng, list, nl, pk.cap, 16, pk.mask, pk.kp, me.h[(s - 1) & 1].p), "gnnvc_unpack_pieces");
            }
        }
        if (me.hi > me.lo && s >= 1 && me.pieces == 1 && (m->opt.announce < 0 ? P <= 4 : m->opt.announce != 0))
            PTRY(me, gnnvc_stage_input_ready(me.eng, s, in, me.lo, me.hi), "gnnvc_stage_input_ready");
        const bool choose = s < 2 && P > 1 && !m->pk[s].known;
        for (int k = 0; k < me.pieces; ++k) {
            const uint32_t r0 = me.cut[k], r1 = me.cut[k + 1];
            if (r1 > r0)
                PTRY(me, gnnvc_stage_forward_device(me.eng, s, r0, r1, in, out, s == 2 ? me.logits.p : nullptr), "gnnvc_stage_forward_device");
            if (s < 2 && P > 1 && !choose) {
                int rc = ship_piece(m, me, s, k, out, err);
                if (rc) return rc;
            }
        }
        if (choose) {
            // A graph's first forward: how this stage's rows travel is chosen from the non-zeros per column of ALL rows — every
            // part counts its own (a pass over the rows it just wrote), the counts meet on the host, every worker makes the same
            // choice — and only then do the pieces leave (packed, but one after the other: the later forwards pipeline)
            uint64_t cnt[16] = {0};
            if (me.hi > me.lo) PTRY(me, gnnvc_column_counts(me.eng, out + (size_t)me.lo * 16, me.hi - me.lo, 16, cnt), "gnnvc_column_counts");
            for (int c = 0; c < 16; ++c) me.counts[s][c] = cnt[c];
            if (!barrier(m, (int)P)) {
                err = "another part of the forward failed";
                return GNNVC_ERR_STATE;
            }
            if (me.index == 0) {
                uint64_t tot[16] = {0};
                int total_pieces = 0;
                for (const Part &p : m->parts) {
                    for (int c = 0; c < 16; ++c) tot[c] += p.counts[s][c];
                    total_pieces += p.pieces;
                }
                m->pk[s] = choose_packing(tot, n, total_pieces, m->opt.pack != 0);
                layout_stage(m, s);
            }
            if (!barrier(m, (int)P)) {
                err = "another part of the forward failed";
                return GNNVC_ERR_STATE;
            }
            if (m->pk[s].on) {
                MTRY(me.send[s].reserve((size_t)m->part_words[s][(size_t)me.index]));
                MTRY(me.recv[s].reserve((size_t)(m->region_pre[s][P * kMaxPieces] - m->part_words[s][(size_t)me.index])));
            }
            if (!barrier(m, (int)P)) {   // (every receive buffer exists before anybody pushes into it)
                err = "another part of the forward failed";
                return GNNVC_ERR_STATE;
            }
            for (int k = 0; k < me.pieces; ++k) {
                int rc = ship_piece(m, me, s, k, out, err);
                if (rc) return rc;
            }
        }
        if (s == 2 && me.hi > me.lo && !solo) {   // the scores (and logits) of these rows, to the caller's arrays on the first device
            const size_t rows = me.hi - me.lo;
            MTRY(hipMemcpyPeerAsync(m->fw_scores + me.lo, dev0, me.scores.p + me.lo, me.device, rows * sizeof(float), me.stream));
            if (m->fw_logits)
                MTRY(hipMemcpyPeerAsync(m->fw_logits + me.lo, dev0, me.logits.p + me.lo, me.device, rows * sizeof(float), me.stream));
        }
    }
    MTRY(hipMemcpyAsync(me.flag_pin.p, me.flag.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, me.stream));
    for (int s = 0; s < 2; ++s)   // (the span ends when the last push has landed; an event never recorded waits for nothing)
        MTRY(hipStreamWaitEvent(me.stream, me.pushed[s][std::max(me.pieces - 1, 0)], 0));
    MTRY(hipEventRecord(me.t1, me.stream));
    return GNNVC_OK;
}

// ------------------------------------------------------------------ the generic route (gnnvc_create_multi_generic)
// A model that is a generic stage list: S stages of any widths, every row computed by k_stage_any on one device in stored order
// (gnnvc_stage_forward_device on the part's slice, heavy and giant rows included), so the bits are the single engine's.  After
// every stage but the last a part ships the rows it computed, as FULL rows of gw_out[s] floats, straight into every peer's
// ping-pong buffer of that stage: one k_push_rows launch for all peers (gnnvc_push_rows) or one hipMemcpyPeerAsync per peer.
// Nothing is packed, nothing is chosen by a first forward, nothing is reserved here: no barrier of the workers.
//
// THE ORDERING INVARIANT.  Stage s reads buffer (s - 1) & 1 and writes buffer s & 1, so a peer's stage-s rows land in my buffer
// s & 1 — which is also the INPUT of my stage s - 1.  That is safe only because
//   - a peer cannot start graph stage s before it holds all my pieces of stage s - 1 (it waits for every pushed event), and
//   - I ship my last piece of stage s - 1 after my last stage-(s - 1) kernel (the event behind it, in my stream's order),
// so by the time a peer's stage-s row arrives my stage s - 1 has read its input to the end.  The same two facts keep my own
// stage-(s + 2) kernels, which write my rows of buffer s & 1 again, behind the copies that still read my stage-s rows from it.
// The one stage that waits for nobody is a dense stage (it reads its own rows only): multi_create admits it at s = 0 only.
std::atomic<uint64_t> &gen_cell(MultiState *m, int r, int s, int k) {
    return m->rec[((size_t)r * (size_t)std::max(m->stages - 1, 1) + (size_t)s) * kMaxPieces + (size_t)k];
}

// wait_piece for the generic route's cells and events
int wait_rows(MultiState *m, Part &me, int r, int s, int k, std::string &err) {
    std::atomic<uint64_t> &cell = gen_cell(m, r, s, k);
    int spins = 0;
    while (cell.load(std::memory_order_acquire) != m->epoch) {
        if (m->failed.load(std::memory_order_acquire)) {
            err = "another part of the forward failed";
            return GNNVC_ERR_STATE;
        }
        if (++spins > 64) std::this_thread::yield();
    }
    MTRY(hipStreamWaitEvent(me.stream, m->parts[(size_t)r].gpushed[(size_t)s * kMaxPieces + k], 0));
    return GNNVC_OK;
}

// ship_piece for full rows of any width: rows [cut[k], cut[k + 1]) of stage s, which `me` just computed into `out`
int ship_rows(MultiState *m, Part &me, int s, int k, float *out, std::string &err) {
    const size_t P = m->parts.size(), f = (size_t)m->gw_out[(size_t)s], at = (size_t)s * kMaxPieces + (size_t)k;
    const uint32_t r0 = me.cut[k], r1 = me.cut[k + 1];
    const float *src = out + (size_t)r0 * f;
    const uint64_t words = (uint64_t)(r1 - r0) * f;
    MTRY(hipEventRecord(me.gdone[at], me.stream));
    MTRY(hipStreamWaitEvent(me.copy, me.gdone[at], 0));
    if (m->opt.push && m->peer_stores) {   // (source and destinations share the row index and width in 256-byte-aligned buffers: one 16-byte phase)
        float *dst[64];
        uint32_t nd = 0;
        for (size_t q = 0; q < P; ++q)
            if ((int)q != me.index) dst[nd++] = m->parts[q].h[s & 1].p + (size_t)r0 * f;
        PTRY(me, gnnvc_push_rows(me.eng, src, words, nd, dst, me.copy), "gnnvc_push_rows");
    } else {
        for (size_t q = 0; q < P; ++q)
            if ((int)q != me.index)
                MTRY(hipMemcpyPeerAsync(m->parts[q].h[s & 1].p + (size_t)r0 * f, m->parts[q].device, src, me.device, (size_t)words * sizeof(float),
                                        me.copy));
    }
    MTRY(hipEventRecord(me.gpushed[at], me.copy));
    gen_cell(m, me.index, s, k).store(m->epoch, std::memory_order_release);
    return GNNVC_OK;
}

int forward_part_generic(MultiState *m, Part &me, std::string &err) {
    const uint32_t n = m->n;
    const size_t P = m->parts.size();
    const int dev0 = m->parts[0].device, S = m->stages;
    const bool solo = m->opt.only_part >= 0;
    if (solo && m->opt.only_part != me.index) return GNNVC_OK;
    MTRY(hipSetDevice(me.device));
    MTRY(hipEventRecord(me.t0, me.stream));
    MTRY(hipMemcpyPeerAsync(me.x.p, me.device, m->fw_x, dev0, (size_t)n * (size_t)m->in_width * sizeof(float), me.stream));   // the input, replicated
    hipEvent_t last_push = nullptr;
    for (int s = 0; s < S; ++s) {
        const bool last = s + 1 == S;
        const float *in = s == 0 ? me.x.p : me.h[(s - 1) & 1].p;
        float *out = last ? me.scores.p : me.h[s & 1].p;
        // a graph stage's input is complete on this device once every peer's pieces of the last stage have landed (a dense stage
        // reads its own rows only and waits for nothing; empty pieces were never shipped)
        if (s >= 1 && P > 1 && !solo && !m->gdense[(size_t)s])
            for (size_t r = 0; r < P; ++r) {
                const Part &pr = m->parts[r];
                if ((int)r == me.index) continue;
                for (int k = 0; k < pr.pieces; ++k)
                    if (pr.cut[k + 1] > pr.cut[k]) {
                        const int rc = wait_rows(m, me, (int)r, s - 1, k, err);
                        if (rc) return rc;
                    }
            }
        for (int k = 0; k < me.pieces; ++k) {
            const uint32_t r0 = me.cut[k], r1 = me.cut[k + 1];
            if (r1 <= r0) continue;   // (an empty piece, an empty part: no launch, nothing shipped, nobody waits for it)
            PTRY(me, gnnvc_stage_forward_device(me.eng, s, r0, r1, in, out, last ? me.logits.p : nullptr), "gnnvc_stage_forward_device");
            // an audited forward: k_audit_any over the piece right behind its stage call (it synchronises this part's stream; the
            // part's engine is quiet, so a mismatch is counted — or repaired, before the rows leave — and the worker goes on)
            if (m->fw_audit)
                PTRY(me, gnnvc_audit_stage_device(me.eng, s, r0, r1, in, out, last ? me.logits.p : nullptr), "gnnvc_audit_stage_device");
            if (!last && P > 1) {
                const int rc = ship_rows(m, me, s, k, out, err);
                if (rc) return rc;
                last_push = me.gpushed[(size_t)s * kMaxPieces + (size_t)k];
            }
        }
        if (last && me.hi > me.lo && !solo) {   // the scores (and logits) of these rows, to the caller's arrays on the first device
            const size_t ow = (size_t)m->out_width, words = (size_t)(me.hi - me.lo) * ow;
            MTRY(hipMemcpyPeerAsync(m->fw_scores + (size_t)me.lo * ow, dev0, me.scores.p + (size_t)me.lo * ow, me.device, words * sizeof(float), me.stream));
            if (m->fw_logits && m->ends_in_sigmoid)
                MTRY(hipMemcpyPeerAsync(m->fw_logits + (size_t)me.lo * ow, dev0, me.logits.p + (size_t)me.lo * ow, me.device, words * sizeof(float),
                                        me.stream));
        }
    }
    if (last_push) MTRY(hipStreamWaitEvent(me.stream, last_push, 0));   // (the span ends when the last push has landed: the copy stream runs in order)
    MTRY(hipEventRecord(me.t1, me.stream));
    return GNNVC_OK;
}

// whatever happened: nothing of this part's work is left in flight when the job returns (a failed forward must not
// leave kernels and peer copies writing into the caller's arrays behind an error return)
void drain_part(Part &p) {
    if (hipSetDevice(p.device) != hipSuccess) return;
    if (p.copy) (void)hipStreamSynchronize(p.copy);
    if (p.stream) (void)hipStreamSynchronize(p.stream);
    (void)hipGetLastError();
}

void worker(MultiState *m, Part *p) {
    uint64_t seen = 0;
    for (;;) {
        int job;
        {
            std::unique_lock<std::mutex> lk(m->mu);
            m->cv_go.wait(lk, [&] { return m->gen != seen; });
            seen = m->gen;
            job = m->job;
        }
        if (job == kQuit) return;
        p->err.clear();
        p->rc = GNNVC_OK;
        if (job == kUpload) p->rc = upload_part(m, *p, p->err);
        else if (job == kForward) p->rc = m->generic ? forward_part_generic(m, *p, p->err) : forward_part(m, *p, p->err);
        if (p->rc != GNNVC_OK) fail_job(m);
        if (job == kForward) {
            drain_part(*p);
            if (p->rc == GNNVC_OK && p->t0 && p->t1 && (m->opt.only_part < 0 || m->opt.only_part == p->index))
                if (hipEventElapsedTime(&p->span_ms, p->t0, p->t1) != hipSuccess) p->span_ms = 0.0f;
        }
        {
            std::lock_guard<std::mutex> lk(m->mu);
            if (--m->pending == 0) m->cv_done.notify_all();
        }
    }
}

// run one job on every worker; the first failure's code and message
int run_job(MultiState *m, int job, std::string &err) {
    m->failed.store(0, std::memory_order_release);
    {
        std::lock_guard<std::mutex> lk(m->mu);
        m->job = job;
        m->pending = (int)m->parts.size();
        ++m->gen;
    }
    m->cv_go.notify_all();
    {
        std::unique_lock<std::mutex> lk(m->mu);
        m->cv_done.wait(lk, [&] { return m->pending == 0; });
        m->job = kIdle;
    }
    int rc = GNNVC_OK;
    for (const Part &p : m->parts)   // (a part that only gave up because another one failed comes last)
        if (p.rc != GNNVC_OK && p.rc != GNNVC_ERR_STATE) {
            rc = p.rc;
            err = p.err;
            break;
        }
    if (rc == GNNVC_OK)
        for (const Part &p : m->parts)
            if (p.rc != GNNVC_OK) {
                rc = p.rc;
                err = p.err;
                break;
            }
    return rc;
}

}  // namespace

// the generic opt-ins of gnnvc_create_multi_generic on one part's engine (an ordinary engine: the public setters)
static int apply_generic_config(gnnvc_engine *e, const gnnvc_generic_config &c) {
    int rc = GNNVC_OK;
    if (c.heavy_rows != GNNVC_GENERIC_DEFAULT) rc = gnnvc_set_generic_heavy_rows(e, c.heavy_rows);
    if (rc == GNNVC_OK && (c.giant_rows != GNNVC_GENERIC_DEFAULT || c.giant_segments != -1)) {
        long from = 0;
        (void)gnnvc_get_info(e, "generic_giant_from", &from);
        rc = gnnvc_set_generic_giant_rows(e, c.giant_rows != GNNVC_GENERIC_DEFAULT ? c.giant_rows : (uint32_t)from, c.giant_segments);
    }
    if (rc == GNNVC_OK && c.big_stages_lds) rc = gnnvc_set_generic_big_stages(e, c.big_stages_lds);
    if (rc == GNNVC_OK && c.feature_width) rc = gnnvc_set_generic_feature_width(e, c.feature_width);
    if (rc == GNNVC_OK && c.patterns) rc = gnnvc_set_generic_patterns(e, c.patterns);
    return rc;
}

int multi_create(MultiState **out, const char *model_text, size_t len, const int *devices, int n_devices, bool generic,
                 const gnnvc_generic_config *cfg, std::string &err) {
    *out = nullptr;
    if (!devices || n_devices < 1 || n_devices > 64) {
        err = "gnnvc_create_multi: 1 .. 64 devices";
        return GNNVC_ERR_INVALID;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        err = "no HIP device — this engine has no CPU path";
        return GNNVC_ERR_DEVICE;
    }
    for (int r = 0; r < n_devices; ++r)
        if (devices[r] < 0 || devices[r] >= count) {
            char buf[128];
            snprintf(buf, sizeof buf, "no HIP device %d (found %d)", devices[r], count);
            err = buf;
            return GNNVC_ERR_DEVICE;
        }
    MultiState *m = new (std::nothrow) MultiState();
    if (!m) return GNNVC_ERR_NOMEM;
    m->parts.resize((size_t)n_devices);
    m->rec = std::vector<std::atomic<uint64_t>>((size_t)n_devices * 2 * kMaxPieces);
    for (auto &c : m->rec) c.store(0);
    int rc = GNNVC_OK;
    for (int r = 0; r < n_devices && rc == GNNVC_OK; ++r) {
        Part &p = m->parts[(size_t)r];
        p.index = r;
        p.device = devices[r];
        rc = gnnvc_create(&p.eng, model_text, len, p.device);
        if (rc != GNNVC_OK) {
            err = "creating a per-device engine failed";
            break;
        }
        // a part records its audits without failing its stage calls: the job's barriers do not recover from a part that gives
        // up, so mismatches are reported by multi_forward_device once the job has drained
        rc = gnnvc_set_option(p.eng, "audit_quiet", 1);
        // (gnnvc_create_multi_generic: the config before the stage list is read; a model of the trained shape keeps its own plans and
        // the config has no effect on it)
        long part_generic = 0;
        if (rc == GNNVC_OK && generic && cfg && gnnvc_get_info(p.eng, "generic_stages_model", &part_generic) == GNNVC_OK &&
            !(gnnvc_is_fused(p.eng) && part_generic == 0))
            rc = apply_generic_config(p.eng, *cfg);
        if (rc != GNNVC_OK) {
            err = std::string("setting up a per-device engine failed: ") + gnnvc_last_error(p.eng);
            break;
        }
        hipError_t h = hipSetDevice(p.device);
        // the part runs on its engine's OWN stream: the engine's side queue was probed against that one (ADVICE r3 — a stream
        // made here could share the side queue's hardware queue and serialise the long rows with the tile kernel)
        void *own = nullptr;
        if (h == hipSuccess && gnnvc_get_stream(p.eng, &own) != GNNVC_OK) h = hipErrorInvalidValue;
        p.stream = reinterpret_cast<hipStream_t>(own);
        if (h == hipSuccess) h = p.copy.create(hipStreamNonBlocking);
        for (int s = 0; s < 2 && h == hipSuccess; ++s)
            for (int k = 0; k < kMaxPieces && h == hipSuccess; ++k) {
                h = p.packed[s][k].create(hipEventDisableTiming);
                if (h == hipSuccess) h = p.pushed[s][k].create(hipEventDisableTiming);
            }
        if (h == hipSuccess) h = p.t0.create();
        if (h == hipSuccess) h = p.t1.create();
        if (h != hipSuccess) {
            rc = hip_fail(err, h, "stream / event creation");
            break;
        }
        // rows travel device to device: let each device write its peers' memory directly where the fabric allows it (without
        // peer access the pieces go by hipMemcpyPeerAsync, staged by the runtime)
        for (int q = 0; q < r; ++q) {
            const int a = p.device, b = m->parts[(size_t)q].device;
            if (a == b) continue;
            int ok_ab = 0, ok_ba = 0;
            if (hipDeviceCanAccessPeer(&ok_ab, a, b) == hipSuccess && ok_ab && hipDeviceCanAccessPeer(&ok_ba, b, a) == hipSuccess && ok_ba) {
                (void)hipSetDevice(a);
                (void)hipDeviceEnablePeerAccess(b, 0);
                (void)hipSetDevice(b);
                (void)hipDeviceEnablePeerAccess(a, 0);
                (void)hipGetLastError();   // ("already enabled" is not an error worth keeping)
            } else {
                m->peer_stores = false;
            }
        }
    }
    if (rc == GNNVC_OK) {
        m->stages = gnnvc_num_stages(m->parts[0].eng);
        // (a three-stage model of other widths reports fused too — option "generic_stages" — but the packers, the exchange and the
        // plans here are made for the trained shape's 16-wide rows)
        long is_generic = 0;
        (void)gnnvc_get_info(m->parts[0].eng, "generic_stages_model", &is_generic);
        if (generic && is_generic != 0 && m->stages >= 1 && gnnvc_is_fused(m->parts[0].eng)) {
            rc = describe_generic(m, err);   // gnnvc_create_multi_generic and a generic stage list: the generic route
        } else if (m->stages != 3 || !gnnvc_is_fused(m->parts[0].eng) || is_generic != 0) {
            err = generic ? "the model stays layer by layer under this config: a multi-device handle runs fused stages only"
                          : "a multi-device handle runs the fused three-stage model of the trained widths only";
            rc = GNNVC_ERR_UNSUPPORTED;
        }
    }
    if (rc != GNNVC_OK) {
        multi_destroy(m);
        return rc;
    }
    for (Part &p : m->parts) p.th = std::thread(worker, m, &p);
    *out = m;
    return GNNVC_OK;
}

void multi_destroy(MultiState *m) {
    if (!m) return;
    {
        std::lock_guard<std::mutex> lk(m->mu);
        m->job = kQuit;
        ++m->gen;
    }
    m->cv_go.notify_all();
    for (Part &p : m->parts)
        if (p.th.joinable()) p.th.join();
    for (Part &p : m->parts) {
        (void)hipSetDevice(p.device);
        if (p.copy) (void)hipStreamSynchronize(p.copy);
        if (p.stream) (void)hipStreamSynchronize(p.stream);
        if (p.eng) gnnvc_destroy(p.eng);   // (owns p.stream)
    }
    delete m;   // (the parts' buffers, events and copy streams: gnnvc_device_mem.h)
}

int multi_devices(const MultiState *m) { return m ? (int)m->parts.size() : 0; }
uint32_t multi_vertices(const MultiState *m) { return (m && m->have_graph) ? m->n : 0u; }
bool multi_has_graph(const MultiState *m) { return m && m->have_graph; }
double multi_last_forward_ms(const MultiState *m) { return m ? m->last_ms : 0.0; }

int multi_part_info(const MultiState *m, int part, uint32_t *row_lo, uint32_t *row_hi, uint64_t *entries) {
    if (!m || part < 0 || part >= (int)m->parts.size()) return GNNVC_ERR_INVALID;
    const Part &p = m->parts[(size_t)part];
    if (row_lo) *row_lo = p.lo;
    if (row_hi) *row_hi = p.hi;
    if (entries) *entries = p.nnz;
    return GNNVC_OK;
}

// what part r shipped to ONE peer in the last exchange of stage s: the dense part of every piece + the used part of its list
static uint64_t shipped_bytes(MultiState *m, const Part &p, int s) {
    if (m->parts.size() < 2) return 0;
    if (!m->pk[s].on) return (uint64_t)(p.hi - p.lo) * 16 * sizeof(float);
    uint64_t bytes = 0;
    if (hipSetDevice(p.device) != hipSuccess) return 0;
    for (int k = 0; k < p.pieces; ++k) {
        const uint32_t rows = p.cut[k + 1] - p.cut[k];
        const float *region = p.send[s].p + (m->region_pre[s][(size_t)p.index * kMaxPieces + k] - m->region_pre[s][(size_t)p.index * kMaxPieces]);
        uint32_t used = 0;
        if (hipMemcpy(&used, region + (size_t)rows * m->pk[s].kp, sizeof used, hipMemcpyDeviceToHost) != hipSuccess) return 0;
        bytes += ((uint64_t)rows * m->pk[s].kp + 4 + (uint64_t)kExcWordsPerEntry * std::min(used, m->pk[s].cap)) * sizeof(float);
    }
    return bytes;
}

bool multi_is_generic(const MultiState *m) { return m && m->generic; }

bool multi_sum_info(MultiState *m, const char *key, long *value) {
    long total = 0;
    if (m->have_graph && m->n == 0) {   // (a graph of no vertices is attached to no part: they still hold the one before it)
        *value = 0;
        return true;
    }
    for (const Part &p : m->parts) {
        long v = 0;
        if (gnnvc_get_info(p.eng, key, &v) != GNNVC_OK) return false;
        total += v;
    }
    *value = total;
    return true;
}

bool multi_get_info(MultiState *m, const char *key, long *value) {
    const std::string k(key);
    static const char kBytes[] = "multi_exchange_bytes_per_peer_stage";
    if (k == "multi_generic") *value = m->generic ? 1 : 0;
    else if (k == "multi_exchanges") *value = m->parts.size() > 1 ? std::max(m->stages - 1, 0) : 0;   // stages whose rows travel
    else if (m->generic && k.rfind(kBytes, 0) == 0) {   // full rows: the busiest part's rows x width x 4
        const char *num = k.c_str() + sizeof kBytes - 1;
        char *end = nullptr;
        const long s = strtol(num, &end, 10);
        if (*num < '0' || *num > '9' || *end != 0 || s + 1 >= (long)m->stages) return false;
        uint64_t most = 0;
        if (m->have_graph && m->parts.size() > 1)
            for (const Part &p : m->parts) most = std::max<uint64_t>(most, (uint64_t)(p.hi - p.lo) * (uint64_t)m->gw_out[(size_t)s] * sizeof(float));
        *value = (long)most;
    }
    else if (k == "multi_pieces") *value = m->parts.empty() ? 0 : m->parts[0].pieces;
    else if (k == "multi_packed_stage0" || k == "multi_packed_stage1") *value = m->pk[k.back() - '0'].known && m->pk[k.back() - '0'].on ? 1 : 0;
    else if (k == "multi_packed_columns_stage0" || k == "multi_packed_columns_stage1") *value = m->pk[k.back() - '0'].on ? (long)m->pk[k.back() - '0'].kp : 16;
    else if (k == "multi_exchange_bytes_per_peer_stage0" || k == "multi_exchange_bytes_per_peer_stage1") {
        // (diagnostic: reads the pieces' list counts back; the busiest part's figure)
        uint64_t most = 0;
        if (m->have_graph && m->pk[k.back() - '0'].known)
            for (const Part &p : m->parts) most = std::max(most, shipped_bytes(m, p, k.back() - '0'));
        (void)hipSetDevice(m->parts[0].device);
        *value = (long)most;
    }
    else if (k == "multi_peer_stores") *value = m->peer_stores && m->opt.push ? 1 : 0;
    else if (k.rfind("multi_part_span_us_", 0) == 0) {
        const int r = atoi(k.c_str() + 19);
        if (r < 0 || r >= (int)m->parts.size()) return false;
        *value = (long)(m->parts[(size_t)r].span_ms * 1000.0f);
    } else return false;
    return true;
}

int multi_set_weight_scale(MultiState *m, float ws) {
    for (Part &p : m->parts) {
        int rc = gnnvc_set_weight_scale(p.eng, ws);
        if (rc) return rc;
    }
    return GNNVC_OK;
}

// What a multi-device handle does with the keys it is handed (gnnvc_options.h has the engine's own table): write a member of
// its own, and then
enum MultiEffect : uint32_t {
    kMxRepack = 1u << 0,   // the pieces and the receive buffers are shaped again: decided on the next graph / forward
    kMxParts = 1u << 1,    // every part's engine gets the key too
};
using MultiRow = OptionRow<MultiState::Opts>;
static const MultiRow kMultiRows[] = {
    // the exchange's own options
    {"multi_pieces", &MultiState::Opts::pieces, range(0, kMaxPieces), kMxRepack},
    {"multi_pack", &MultiState::Opts::pack, kBool, kMxRepack},
    {"multi_push", &MultiState::Opts::push, kBool, 0},
    {"multi_only_part", &MultiState::Opts::only_part, range(-1, 64), 0},   // (and below the number of parts, multi_set_option)
    {"multi_announce", &MultiState::Opts::announce, kTri, 0},
    // handed on by the front engine
    {"poison_features", &MultiState::Opts::poison, kBool, 0},   // (the parts run stage by stage on THIS driver's buffers)
    // (audit_period: the front handle counts the calls, multi_forward_device switches the parts; audit_quiet: the parts stay quiet;
    // audit_log: the front handle prints for every part)
    {"audit_period", 0},
    {"audit_quiet", 0},
    {"audit_log", 0},
    {"audit_repair", &MultiState::Opts::audit_repair, kBool, kMxParts},
};

int multi_set_option(MultiState *m, const char *key, long value) {
    const MultiRow *r = find_option(kMultiRows, key);
    if (!r && strncmp(key, "multi_", 6) == 0) return GNNVC_ERR_INVALID;
    uint32_t fx = kMxParts;   // (any other key is an engine's)
    if (r) {
        r->store(m->opt, value);
        if (m->opt.only_part >= (int)m->parts.size()) m->opt.only_part = -1;   // (no such part: off)
        fx = r->fx;
    }
    if (fx & kMxRepack) {
        m->pk[0] = m->pk[1] = Packing();
        if (m->have_graph)
            for (Part &p : m->parts) cut_pieces(p, pieces_for(m));
    }
    if (fx & kMxParts)
        for (Part &p : m->parts) {
            int rc = gnnvc_set_option(p.eng, key, value);
            if (rc) return rc;
        }
    return GNNVC_OK;
}

int multi_upload(MultiState *m, uint32_t n, const uint64_t *rowptr64, const uint32_t *rowptr32, const uint32_t *col, const uint32_t *w,
                 const uint32_t *nw, std::string &err) {
    m->have_graph = false;
    m->pk[0] = m->pk[1] = Packing();
    const size_t P = m->parts.size();
    auto rp = [&](uint32_t u) -> uint64_t { return rowptr64 ? rowptr64[u] : (uint64_t)rowptr32[u]; };
    const uint64_t nnz = n ? rp(n) : 0;
    if (nnz >= 0xFFFFFFFFull - GNNVC_COL_PAD) {
        err = "nnz does not fit 32-bit row pointers";
        return GNNVC_ERR_UNSUPPORTED;
    }
    if (n && rp(0) != 0) {
        err = "row pointers are not monotone from 0 to nnz";
        return GNNVC_ERR_INVALID;
    }
    // contiguous row ranges of (nearly) equal entry count, cut at multiples of 64 rows (the tile kernels' unit).  (The cuts are
    // searched in an array not yet known to be monotone — every part checks its own range, upload_part — a broken one yields
    // uneven parts and then the error.)
    std::vector<uint32_t> cut(P + 1, 0);
    cut[P] = n;
    for (size_t r = 1; r < P; ++r) {
        uint32_t at;
        if (nnz == 0) {
            at = (uint32_t)((uint64_t)n * r / P);
        } else {
            const uint64_t target = nnz / P * r + std::min<uint64_t>(r, nnz % P);
            uint32_t a = 0, b = n;   // first row whose offset reaches the target
            while (a < b) {
                const uint32_t mid = a + (b - a) / 2;
                if (rp(mid) >= target) b = mid;
                else a = mid + 1;
            }
            at = a;
        }
        at = at / 64u * 64u;
        cut[r] = std::min(n, std::max(at, cut[r - 1]));
    }
    m->n = n;
    m->nnz = nnz;
    const int K = pieces_for(m);
    for (size_t r = 0; r < P; ++r) {
        Part &p = m->parts[r];
        p.lo = cut[r];
        p.hi = cut[r + 1];
        const uint64_t a = n ? rp(p.lo) : 0, b = n ? rp(p.hi) : 0;
        if (b < a || b - a > nnz) {
            err = "row pointers are not monotone from 0 to nnz";
            return GNNVC_ERR_INVALID;
        }
        p.nnz = b - a;
        cut_pieces(p, K);
    }
    m->up_rp64 = rowptr64;
    m->up_rp32 = rowptr32;
    m->up_col = col;
    m->up_w = w;
    m->up_nw = nw;
    const int rc = run_job(m, kUpload, err);   // every part copies, checks and attaches its own slice, side by side
    m->up_rp64 = nullptr;
    m->up_rp32 = m->up_col = m->up_w = m->up_nw = nullptr;
    if (rc != GNNVC_OK) return rc;
    m->have_graph = true;
    return GNNVC_OK;
}

bool multi_audit_info(MultiState *m, const char *key, long *value) {
    const std::string k(key);
    const bool sum = k == "audit_runs" || k == "audit_failures" || k == "audit_repairs" || k == "audit_nan_pairs";
    if (sum) {
        long total = 0;
        for (const Part &p : m->parts) {
            long v = 0;
            if (gnnvc_get_info(p.eng, key, &v) != GNNVC_OK) return false;
            total += v;
        }
        *value = total;
        return true;
    }
    // audit_last_*: the first failing part's (part 0's, -1 / 0, while none has failed)
    const Part &p = m->parts[(size_t)std::max(m->audit_last_part, 0)];
    return gnnvc_get_info(p.eng, key, value) == GNNVC_OK;
}

// multi_forward_device of the generic route: no packing to choose, no attempt to repeat; audit = gnnvc_forward_audited* (the parts'
// "audit_period" stays 0: a generic engine audits on demand only, each worker calls gnnvc_audit_stage_device itself)
static int forward_generic_handle(MultiState *m, const float *d_x, float *d_scores, float *d_logits, bool audit, std::string &err) {
    std::vector<long> failures(m->parts.size(), 0);
    if (audit)
        for (size_t r = 0; r < m->parts.size(); ++r)
            if (gnnvc_get_info(m->parts[r].eng, "audit_failures", &failures[r]) != GNNVC_OK) {
                err = "reading a part's audit counters failed";
                return GNNVC_ERR_STATE;
            }
    const auto t0 = std::chrono::steady_clock::now();
    if (m->opt.poison && m->opt.only_part < 0 && m->stages > 1) {   // (tests, fuzz; before any part starts: peers write into these buffers on their own streams)
        for (Part &p : m->parts) {
            if (hipSetDevice(p.device) != hipSuccess) continue;
            for (auto &h : p.h)
                if (h.p) (void)hipMemsetAsync(h.p, 0xFF, (size_t)m->n * (size_t)m->wmax * sizeof(float), p.stream);
            (void)hipStreamSynchronize(p.stream);
        }
    }
    m->fw_x = d_x;
    m->fw_scores = d_scores;
    m->fw_logits = d_logits;
    m->fw_audit = audit;
    ++m->epoch;
    int rc = run_job(m, kForward, err);
    m->fw_audit = false;
    if (rc == GNNVC_OK && audit) {   // every part has drained: did any part's audit find a mismatch?
        for (size_t r = 0; r < m->parts.size(); ++r) {
            long now = 0;
            if (gnnvc_get_info(m->parts[r].eng, "audit_failures", &now) != GNNVC_OK || now == failures[r]) continue;
            m->audit_last_part = (int)r;
            if (!m->opt.audit_repair) {
                err = "part " + std::to_string(r) + ": " + gnnvc_last_error(m->parts[r].eng);
                rc = GNNVC_ERR_AUDIT;
            }
            break;
        }
    }
    (void)hipSetDevice(m->parts[0].device);
    m->last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int multi_forward_device(MultiState *m, const float *d_x, float *d_scores, float *d_logits, bool audit, std::string &err) {
    if (!m->have_graph) {
        err = "no graph attached";
        return GNNVC_ERR_STATE;
    }
    if (m->n == 0) return GNNVC_OK;
    if (m->generic) return forward_generic_handle(m, d_x, d_scores, d_logits, audit, err);
    if (m->opt.only_part >= 0 && m->parts.size() > 1 && !(m->pk[0].known && m->pk[1].known)) {
        err = "multi_only_part needs a complete forward on this graph first";
        return GNNVC_ERR_STATE;
    }
    std::vector<long> failures(m->parts.size(), 0);
    if (audit || m->parts_audit) {   // (an unaudited forward after an unaudited one touches nothing)
        for (size_t r = 0; r < m->parts.size(); ++r) {
            Part &p = m->parts[r];
            if (gnnvc_set_option(p.eng, "audit_period", audit ? 1 : 0) != GNNVC_OK ||
                gnnvc_get_info(p.eng, "audit_failures", &failures[r]) != GNNVC_OK) {
                err = "switching a part's audit failed";
                return GNNVC_ERR_STATE;
            }
        }
        m->parts_audit = audit;
    }
    const auto t0 = std::chrono::steady_clock::now();
    m->fw_x = d_x;
    m->fw_scores = d_scores;
    m->fw_logits = d_logits;
    int rc = GNNVC_OK;
    // (every repeat takes the packing off at least one of the two exchanged stages, so the third attempt ships full rows everywhere.
    // Two attempts were one too few: a stage-0 overflow hands stage 1 a damaged input in the first attempt, so stage 1's own overflow
    // only shows in the second — fuzz_multi.py case 232 returned that attempt's lossy rows.)
    for (int attempt = 0; attempt < 3; ++attempt) {
        if (m->opt.poison && m->opt.only_part < 0) {   // (tests, fuzz; before any part starts: peers write into these buffers on their own streams)
            for (Part &p : m->parts) {
                if (hipSetDevice(p.device) != hipSuccess) continue;
                for (int b = 0; b < 2; ++b)
                    if (p.h[b].p) (void)hipMemsetAsync(p.h[b].p, 0xFF, (size_t)m->n * 16 * sizeof(float), p.stream);
                (void)hipStreamSynchronize(p.stream);
            }
        }
        ++m->epoch;
        rc = run_job(m, kForward, err);
        if (rc != GNNVC_OK) break;
        // lossless or repeated: a pack step raises its flag when a non-zero fits neither the dense columns nor the list
        bool again = false;
        if (m->opt.only_part < 0)
            for (int s = 0; s < 2; ++s) {
                if (!m->pk[s].on) continue;
                bool over = false;
                for (const Part &p : m->parts) over |= p.flag_pin.p && p.flag_pin.p[s] != 0;
                if (over) {   // full rows for this stage from now on (the lists were sized from this graph's own counts: it never fit)
                    m->pk[s].on = false;
                    layout_stage(m, s);
                    again = true;
                }
            }
        if (!again) break;
    }
    if (rc != GNNVC_OK) m->pk[0] = m->pk[1] = Packing();   // (a first forward may have failed between choosing and allocating)
    if (rc == GNNVC_OK && audit) {   // every part has drained: did any part's audit find a mismatch (in any attempt)?
        for (size_t r = 0; r < m->parts.size(); ++r) {
            long now = 0;
            if (gnnvc_get_info(m->parts[r].eng, "audit_failures", &now) != GNNVC_OK || now == failures[r]) continue;
            m->audit_last_part = (int)r;
            if (!m->opt.audit_repair) {
                err = "part " + std::to_string(r) + ": " + gnnvc_last_error(m->parts[r].eng);
                rc = GNNVC_ERR_AUDIT;
            }
            break;
        }
    }
    (void)hipSetDevice(m->parts[0].device);
    m->last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

int multi_synchronize(MultiState *m) {
    for (Part &p : m->parts) {
        if (hipSetDevice(p.device) != hipSuccess || hipStreamSynchronize(p.stream) != hipSuccess ||
            (p.copy && hipStreamSynchronize(p.copy) != hipSuccess))
            return GNNVC_ERR_DEVICE;
    }
    return GNNVC_OK;
}

}  // namespace gnnvc
