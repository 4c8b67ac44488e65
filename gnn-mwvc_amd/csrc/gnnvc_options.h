// gnnvc_options.h — what gnnvc_set_option can set on an engine: the values (struct Options, gnnvc_engine::opt), and ONE table
// that says for every key which member it writes, how the caller's value is clamped, and what else the engine has to do about
// it (gnnvc_set_option in gnnvc_engine.cpp applies those effects).  Plain data: nothing of HIP in here, a host-only program
// can exercise it (tests/support/options_host.cpp).  Internal.
#pragma once
#include <cstdint>
#include <cstring>

namespace gnnvc {

struct Options {
    int generic = 1;            // option "generic_stages": 0 = never, 1 = models that have no trained-shape stage list, 2 = every model that fits (tests)

    // column-blocked plan of the F = 1 stage (built per graph, see gnnvc_kernels.hip)
    int blocked = 1;            // option "blocked_stage0"
    uint32_t block_cols = 0;    // option "block_cols" (0 = default)
    uint32_t blocked_min_n = 1u << 20;  // below this x fits the L2s anyway
    uint32_t compact_min_n = 1u << 18;  // option "compact_min_n": the compact-table plan's own bound (the smaller of the two counts)
    uint64_t compact_min_nnz = 8u << 20;   // ... and its entries bound (default sizes only)
    uint64_t compact_first_entries = 48ull << 20;   // option "compact_first_forward_entries": graphs of this many entries build
                                               // the plan inside their FIRST forward (0 = never; otherwise it is built in the second).
                                               // Metric graph (200 M entries): first forward 10.96 -> 9.18 ms; ER-3M (60 M): 3.03 -> 2.69;
                                               // ER-1M (20 M): 0.92 -> 1.14
    uint32_t plan_chunk_rows = 0;       // != 0: cap on the rows per chunk of the LDS-table / compact-table plans
    // LDS-table plan of the F = 1 stage
    int lds_table = 1;          // 0 = off, 1 = when it applies, 2 = also on skewed graphs
    int lt_bits = 0;            // option "lds_table_bits" (tests, A/B): force a width (0 = by the graph)
    uint32_t lds_skewed_rows = 0;       // (0 = by the size of x) option "lds_table_skewed_rows": rows of at least this many entries stay outside the skewed-graph plan
    uint32_t lds_skewed_min_n = 1u << 21;
    int lds_skewed = 1;              // option "lds_table_skewed": 0 = skewed graphs keep the gathering F = 1 kernels
    uint32_t lt_min_chunks = 128;       // option "lds_table_min_chunks": a short row range is cut into at least this many chunks
    // compact-table plan of the 16-wide stages
    int compact = 1;            // 0 = off, 1 = when it applies, 2 = also on skewed graphs
    int overlap = 1;                  // last stage: dense layers of round k under the sums of round k + 1
    int dense_skip = 1;               // option "dense_skip_zeros" (A/B): the aggregate-only dense kernels take a clean row's <= 11 non-zero
                                      // first-layer terms from its sums and the input's compact table instead of the 32-term chain (k_dense_f16)
                                      // — and the VALU hidden layers of k_stage_f1 / k_dense_f16 leave out the units that are zero in a whole
                                      // wave (dense_live).  Both only in layers whose weights allow it (StagePlan::skip_ok); 0 = neither
    // pruned adjacency of the 16-wide stages
    int prune = 1;               // option "prune_zero_rows": 1 = the rows found all zero when the plan is built (or predicted at hand-off), 0 = off
    uint64_t prune_heavy_entries = 16u << 20;   // option "prune_heavy_entries": from this many entries left, rows up to the sorted threshold stay with the tile kernel
    uint64_t prune_early_nnz = 64u << 20;   // option "prune_early_entries": skewed graphs with at least this many entries build the plan in their first forward (0 = never)
    // option "prune_predict": 1 = large skewed graphs (the ones the filtered gather is offered to) get the first 16-wide stage's
    // pruned adjacency when they are HANDED OVER, from the predicted set — a graph scored once (the reference's driver,
    // src/GNN_VC.cpp:171-192) then runs its first forward on it, and the next stage borrows it until it has its own
    int prune_predict = 1;
    uint64_t predict_min_nnz = 48u << 20;   // option "prune_predict_min_entries"
    int prune_eff = 1;           // option "prune_class_by_entries_left" (A/B): 0 = rows keep the class their degree gives them
    int prune_giant = 1;         // option "prune_giant_rows" (A/B): 0 = the giant rows keep their full streams
    uint64_t prune_min_nnz = 1u << 20;   // option "prune_min_entries": smaller graphs are not worth a plan
    uint32_t prune_min_drop = 15;   // option "prune_min_drop_percent": build only if at least this share of the entries goes
    int giant_gather_first = -1; // option "giant_gather_first": the giant rows' gather on the main queue ahead of the tile kernel (1), on the side queue with the rest of their chain (0), -1 = by the graph (launch_side_rows)
    int long_on_main = -1;       // option "long_rows_on_main": -1 = by the graph (launch_side_rows), 0 = beside the giant rows on the side queue, 1 = ahead of the tile kernel
    // filtered gather (see gnnvc_engine::filter_bits)
    int filter = 1;              // option "filter_zero_rows" (A/B): 0 = plain gathers until the plan is there
    // which graphs (measured, scratch/experiments/first_ab2.sh + fuzz_large.py: first forward with / without): R-MAT from ~48 M
    // entries on gains 0.5 - 1.6 ms (R-MAT-22 4.61 -> 3.98, R-MAT-24 19.3 -> 17.7, scale 21 x 16: 2.84 -> 2.30); smaller graphs
    // lose 0.05 - 0.25 ms to the marks and look-ups, power-law graphs (41 - 58 % of the entries point to zero rows) 0.1 ms, nearly
    // uniform graphs with a few hubs (1 - 20 %) 0.2 ms — those have 1 - 3 % of their entries in long rows, R-MAT 35 - 58 %
    uint64_t filter_min_nnz = 48u << 20;   // option "filter_min_entries"
    uint32_t filter_min_long_pct = 25;     // option "filter_min_long_percent": only graphs whose long rows hold this share of the entries
    uint32_t filter_min_pct = 50;   // option "filter_min_percent": the share of the entries that has to point into the set (decided on the device)
    int filter_keep = 1;         // option "filter_keep_lists" (A/B): 0 = every filtered stage walks the whole adjacency

    // table tiles (k_stage_t4)
    int t4 = 1;                          // option "table_tiles"
    uint32_t t4_min_n = 49152;           // option "table_tiles_min_n": below, the 64-byte rows fit an XCD's L2 anyway
    uint64_t t4_max_bytes = 6ull << 20;  // option "table_tiles_max_bytes": the table has to (mostly) sit in a 4 MiB L2
    int t4_solo = 1;                     // option "table_tiles_solo" (A/B): 0 = always launch the gathering kernel behind the tiles
    int timing = 0;                      // option "forward_timing": 0 = a forward records no events (gnnvc_last_forward_ms is refused), 1 = its first and last, 2 = one per stage too
    int poison = 0;                      // option "poison_features" (tests, fuzz): a whole forward starts by filling the engine's feature buffers with NaN bit patterns — a row no kernel writes shows in the result instead of hiding behind an earlier forward's values
    uint32_t verdict_period = 8;         // option "verdict_period": calm verdicts are asked for every this-many forwards (1 = always)
    int wide = 1;                        // option "wide_tiles": graphs of up to "wide_tiles_max_n" vertices run their plain stages a workgroup per tile
    uint32_t wide_max_n = 49152;         // the F = 1 stage ("wide_tiles_max_n": where the table tiles start — feeding them from wide tiles was measured slower) ...
    uint32_t wide_max_n16 = 131072;      // ... and the 16-wide stages ("wide_tiles_max_n_f16") up to these many vertices (measured: small_sizes.py)

    // option "mfma_dense": dense layers on the matrix cores (bit-identical to the VALU path).
    // 0 = VALU everywhere, 1 = MFMA everywhere, 2 = MFMA in the F = 16 stages only (default:
    // the F = 1 stage's first layer has K = 5 and stays on the VALU, and sending its 32
    // activations through LDS just to reach the matrix layout costs more than it saves)
    int mfma = 2;

    // degree-sorted tile order (16-wide stages, skewed graphs)
    int sorted = -1;               // option "sorted_tiles": -1 auto (by measured waste), 0 off, 1 on
    uint64_t sorted_min_nnz = 4ull << 20;   // auto mode leaves smaller graphs on natural tiles
    uint32_t sorted_long_thresh = 1024;   // long-row threshold of the 16-wide stages when their tiles are sorted

    // long rows (degree >= long_thresh): one workgroup each, on aux_stream beside the tile kernel
    uint32_t long_thresh = 512;   // option "long_row_threshold" (0 = off)
    bool long_auto = true;        // no explicit threshold: 256 where few rows are that long, else 512
    int ktrace = 0;                  // option "kernel_trace": HIP events around every main-stream kernel of a forward
    uint32_t giant_thresh = 16384;   // option "giant_row_threshold" (0 = off: k_long_* take every long row)
    int side_streams = 1;            // option "side_streams": 0 = long / giant rows on the main stream, one after the other (profiling)
    uint32_t giant_f16 = 65536;     // option "giant_row_threshold_f16": the 16-wide stages send only rows from this degree on the giant way
    bool giant_f16_auto = true;     // no explicit giant threshold: by the graph (gnnvc_engine::giant_f16)
    int giant_segments = -1;  // option "giant_segments": 1 = a stream on several waves, 0 = one wave walks it, -1 = by the graph (default)
    // Plans at hand-off (round 3).  The reference's driver scores every graph exactly once (src/GNN_VC.cpp:171-192), so a plan
    // built inside a graph's second forward never serves it.  What depends on the graph alone is built when the graph is handed
    // over (upload / staged commit / attach): 1 (default) = the plans one use repays (degree-uniform graphs of at least
    // handoff_min_nnz entries: LDS table + compact table; every graph: the tile order and every buffer a forward would
    // otherwise allocate), 2 = every plan whatever its cost (callers who score a graph many times, or hide the build under a
    // copy), 0 = as in round 2 (inside the first two forwards).
    int handoff = 1;
    uint64_t handoff_min_nnz = 24ull << 20;   // (the builds cost ~20 ps per entry and plan, a first forward saves ~40: from ~20 Mi entries on one use repays them)
    // First use of the compact-table plan on a graph: a pilot over the first pilot_rows rows of the producing stage picks
    // the consumer's table columns, so the producer can write the table on its way (see launch_main)
    uint32_t pilot_rows = 65536;

    // On-device audit (options "audit_*"; k_audit_stage): every audit_period-th call of a forward entry point has each
    // fused stage it runs recomputed by code that uses none of the plans and compared bit for bit, right behind the stage and
    // before the next one is queued; the call reads the records back once, at its end (one stream synchronisation).
    uint32_t audit_period = 0;           // 0 = off
    int audit_repair = 0;                // 1 = the audit's values are written over mismatching ones, the call succeeds
    int audit_flip_stage = -1;           // test hook: in an audited call of this stage whose rows hold audit_flip_row, flip
    uint32_t audit_flip_row = 0;         // ... the lowest mantissa bit of output (row, 0) between the stage and its audit
    int audit_quiet = 0;                 // record mismatches without returning them (the parts of a multi-device handle)
    int audit_log = 0;                   // one stderr line per audited call with the counters (drivers that cannot read them)
};

// How a caller's value becomes the member's: clamped to lo .. hi (most keys), or by one of a few rules of their own.
struct Clamp {
    enum Rule { kRange, kNonZero, kSign, kFlipRow, kGiantThreshold, kTableBits, kMfma } rule;
    long lo = 0, hi = 0;
    constexpr long operator()(long v) const {
        switch (rule) {
        case kRange: return v < lo ? lo : (v > hi ? hi : v);
        case kNonZero: return v != 0 ? 1 : 0;
        case kSign: return v < 0 ? -1 : (v != 0 ? 1 : 0);
        case kFlipRow: return v < 0 || v > 0xFFFFFFFFl ? 0xFFFFFFFFl : v;   // out of range: no row
        case kGiantThreshold: return v > 0 ? (v < 64 ? 64 : v) : 0;         // 0 = off; also sets giant_f16 (apply_option)
        case kTableBits: return (v == 8 || v == 10 || v == 16) ? v : 0;     // anything else: by the graph
        case kMfma: return (v >= 0 && v <= 2) ? v : 2;                      // anything else: the default
        }
        return v;
    }
};
constexpr Clamp range(long lo, long hi) { return Clamp{Clamp::kRange, lo, hi}; }
constexpr long kNoCap = 0x7FFFFFFFFFFFFFFFl;      // (a value above the member's width is cut to it)
constexpr Clamp kBool{Clamp::kNonZero};           // != 0 -> 1
constexpr Clamp kTri{Clamp::kSign};               // < 0 -> -1 (by the graph), else != 0
constexpr Clamp kZeroToTwo = range(0, 2);
constexpr Clamp kPositive = range(0, kNoCap);     // > 0 -> the value, else 0
constexpr Clamp kPositiveOr1 = range(1, kNoCap);  // > 0 -> the value, else 1
constexpr Clamp kPercent = range(0, 101);         // (101: never reached)

// What setting a key does besides writing its member.
enum OptionEffect : uint32_t {
    kFxShortLists = 1u << 0,    // short_from = 0: lists a filtered stage left go by the thresholds and variants of the call that wrote them
    kFxForgetPruned = 1u << 1,  // the pruned adjacencies are built again
    kFxSortedStale = 1u << 2,   // the cached sorted row ranges are invalid
    kFxLongExplicit = 1u << 3,  // long_auto = false
    kFxGiantExplicit = 1u << 4, // giant_f16_auto = false
    kFxAuditRestart = 1u << 5,  // audit_calls = 0: calls are counted from here
    // a multi-device handle (exactly one of):
    kFxForward = 1u << 6,       // ... hands the key on after setting it on the front (gnnvc::multi_set_option)
    kFxFrontOnly = 1u << 7,     // ... keeps it to the front engine: its parts keep their kernels / the front prints for all of them
    kFxPartsElsewhere = 1u << 8,// ... decides per forward what its parts get (multi_forward_device)
    // a key that changes what a forward has cached
    kFxPlan = kFxShortLists | kFxForward,
};

// One row per key.  S = the struct the members are of (Options here, the exchange's options in gnnvc_multi.cpp).
template <class S>
struct OptionRow {
    const char *key;
    int S::*i = nullptr;
    uint32_t S::*u = nullptr;
    uint64_t S::*q = nullptr;
    Clamp clamp = kBool;
    uint32_t fx = 0;
    constexpr OptionRow(const char *k, int S::*m, Clamp c, uint32_t f) : key(k), i(m), clamp(c), fx(f) {}
    constexpr OptionRow(const char *k, uint32_t S::*m, Clamp c, uint32_t f) : key(k), u(m), clamp(c), fx(f) {}
    constexpr OptionRow(const char *k, uint64_t S::*m, Clamp c, uint32_t f) : key(k), q(m), clamp(c), fx(f) {}
    constexpr OptionRow(const char *k, uint32_t f) : key(k), fx(f) {}   // a key that is accepted and writes nothing here
    void store(S &s, long v) const {
        const long c = clamp(v);
        if (i) s.*i = (int)c;
        else if (u) s.*u = (uint32_t)c;
        else if (q) s.*q = (uint64_t)c;
    }
    long load(const S &s) const { return i ? (long)(s.*i) : (u ? (long)(s.*u) : (q ? (long)(s.*q) : 0)); }
};

template <class S, size_t N>
const OptionRow<S> *find_option(const OptionRow<S> (&rows)[N], const char *key) {
    for (const OptionRow<S> &r : rows)
        if (strcmp(r.key, key) == 0) return &r;
    return nullptr;
}

inline constexpr OptionRow<Options> kOptionRows[] = {
    // touch nothing a forward has cached.  The audit: a multi-device handle decides per forward whether its parts audit
    // (gnnvc_multi.cpp), the other audit keys go to every part
    {"poison_features", &Options::poison, kBool, kFxForward},
    {"verdict_period", &Options::verdict_period, range(1, 64), kFxForward},
    {"audit_period", &Options::audit_period, range(0, 0x7FFFFFFF), kFxAuditRestart | kFxPartsElsewhere},
    {"generic_stages", &Options::generic, kZeroToTwo, kFxFrontOnly},   // (k_stage_any: takes effect at once)
    {"audit_log", &Options::audit_log, kBool, kFxFrontOnly},
    {"audit_repair", &Options::audit_repair, kBool, kFxForward},
    {"audit_flip_stage", &Options::audit_flip_stage, range(-1, 64), kFxForward},
    {"audit_flip_row", &Options::audit_flip_row, Clamp{Clamp::kFlipRow}, kFxForward},
    {"audit_quiet", &Options::audit_quiet, kBool, kFxForward},
    {"forward_timing", &Options::timing, kZeroToTwo, kFxForward},
    // the plans, thresholds and kernel variants
    {"blocked_stage0", &Options::blocked, kZeroToTwo, kFxPlan},   // 2 = also on skewed graphs
    {"block_cols", &Options::block_cols, kPositive, kFxPlan},
    {"blocked_min_n", &Options::blocked_min_n, kPositive, kFxPlan},
    {"compact_min_n", &Options::compact_min_n, kPositive, kFxPlan},
    {"compact_first_forward_entries", &Options::compact_first_entries, kPositive, kFxPlan},
    {"plan_chunk_rows", &Options::plan_chunk_rows, kPositive, kFxPlan},
    {"overlap_dense", &Options::overlap, kBool, kFxPlan},
    {"long_row_threshold", &Options::long_thresh, kPositive, kFxPlan | kFxLongExplicit},
    // (an explicit threshold holds for every stage; "giant_row_threshold_f16" afterwards refines it)
    {"giant_row_threshold", &Options::giant_thresh, Clamp{Clamp::kGiantThreshold}, kFxPlan | kFxGiantExplicit},
    {"giant_row_threshold_f16", &Options::giant_f16, kPositiveOr1, kFxPlan | kFxGiantExplicit | kFxForgetPruned},
    {"giant_segments", &Options::giant_segments, kTri, kFxPlan},
    {"side_streams", &Options::side_streams, kBool, kFxPlan},
    {"kernel_trace", &Options::ktrace, kBool, kFxPlan},
    {"compact_gather", &Options::compact, kZeroToTwo, kFxPlan},
    {"prune_zero_rows", &Options::prune, range(0, 1), kFxPlan | kFxForgetPruned},
    {"prune_class_by_entries_left", &Options::prune_eff, kBool, kFxPlan | kFxForgetPruned},
    {"prune_heavy_entries", &Options::prune_heavy_entries, kPositive, kFxPlan | kFxForgetPruned},
    {"prune_early_entries", &Options::prune_early_nnz, kPositive, kFxPlan},
    {"prune_giant_rows", &Options::prune_giant, kBool, kFxPlan},
    {"prune_predict", &Options::prune_predict, kBool, kFxPlan},
    {"wide_tiles", &Options::wide, kBool, kFxPlan},
    {"wide_tiles_max_n", &Options::wide_max_n, kPositive, kFxPlan},
    {"wide_tiles_max_n_f16", &Options::wide_max_n16, kPositive, kFxPlan},
    {"dense_skip_zeros", &Options::dense_skip, kBool, kFxPlan},
    {"table_tiles", &Options::t4, kBool, kFxPlan},
    {"table_tiles_solo", &Options::t4_solo, kBool, kFxPlan},
    {"table_tiles_min_n", &Options::t4_min_n, kPositive, kFxPlan},
    {"table_tiles_max_bytes", &Options::t4_max_bytes, kPositive, kFxPlan},
    {"prune_predict_min_entries", &Options::predict_min_nnz, kPositive, kFxPlan},
    {"giant_gather_first", &Options::giant_gather_first, kTri, kFxPlan},
    {"long_rows_on_main", &Options::long_on_main, kTri, kFxPlan},
    {"filter_zero_rows", &Options::filter, kBool, kFxPlan},
    {"filter_keep_lists", &Options::filter_keep, kBool, kFxPlan},
    {"filter_min_entries", &Options::filter_min_nnz, kPositive, kFxPlan},
    {"filter_min_long_percent", &Options::filter_min_long_pct, kPercent, kFxPlan},
    {"filter_min_percent", &Options::filter_min_pct, kPercent, kFxPlan},
    {"prune_min_entries", &Options::prune_min_nnz, kPositive, kFxPlan},
    {"prune_min_drop_percent", &Options::prune_min_drop, range(0, 100), kFxPlan},
    {"lds_table_skewed", &Options::lds_skewed, kBool, kFxPlan},
    {"lds_table_skewed_rows", &Options::lds_skewed_rows, kPositive, kFxPlan},
    {"lds_table", &Options::lds_table, kZeroToTwo, kFxPlan},
    {"lds_table_min_chunks", &Options::lt_min_chunks, kPositiveOr1, kFxPlan},
    {"lds_table_bits", &Options::lt_bits, Clamp{Clamp::kTableBits}, kFxPlan},
    {"plans_at_handoff", &Options::handoff, kZeroToTwo, kFxPlan},
    {"handoff_min_entries", &Options::handoff_min_nnz, kPositive, kFxPlan},
    {"pilot_rows", &Options::pilot_rows, kPositive, kFxPlan},
    {"sorted_min_nnz", &Options::sorted_min_nnz, kPositive, kFxPlan},
    {"sorted_long_row_threshold", &Options::sorted_long_thresh, kPositiveOr1, kFxPlan | kFxLongExplicit},
    {"mfma_dense", &Options::mfma, Clamp{Clamp::kMfma}, kFxPlan},
    {"sorted_tiles", &Options::sorted, kTri, kFxPlan | kFxSortedStale},
};

// Sets `key` on `o`; *fx = what the engine has to do about it (OptionEffect).  false = no such key, nothing touched.
inline bool apply_option(Options &o, const char *key, long value, uint32_t *fx) {
    const OptionRow<Options> *r = find_option(kOptionRows, key);
    if (!r) return false;
    r->store(o, value);
    if (r->clamp.rule == Clamp::kGiantThreshold) o.giant_f16 = o.giant_thresh ? o.giant_thresh : 1u;
    if (r->fx & kFxLongExplicit) o.long_auto = false;
    if (r->fx & kFxGiantExplicit) o.giant_f16_auto = false;
    *fx = r->fx;
    return true;
}

// The value of `key` as set (gnnvc_get_info's keys that echo an option).
inline bool read_option(const Options &o, const char *key, long *value) {
    const OptionRow<Options> *r = find_option(kOptionRows, key);
    if (r) *value = r->load(o);
    return r != nullptr;
}

}  // namespace gnnvc
