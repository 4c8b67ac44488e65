// gnnvc_engine_state.h — the engine object behind include/gnnvc.h's opaque handle and what the translation units of
// libgnnvc_hip.so share about it.  Internal.
//   gnnvc_engine.cpp  the C ABI: model text, graph hand-off entry points, stage selection and launches, forwards
//   gnnvc_plans.cpp   what is built per GRAPH: row classes (long / giant rows, tile order), the LDS-table, compact-table and
//                     column-blocked plans, the pruned adjacency, and when (hand-off / first forwards)
//   gnnvc_multi.cpp   several devices behind one handle (public ABI only)
//   gnnvc_backward.cpp the backward pass: training forward, model- and layer-level backward (kernels: gnnvc_backward.hip), and the
//                     loss and the optimizer step around it (kernels: gnnvc_fit.hip)
//   gnnvc_kernels.hip the gfx950 kernels and their launchers
//   gnnvc_device_mem.h the owning handles every buffer, event and stream below is held by (DevBuf, PinBuf, Event, Stream)
//   gnnvc_options.h   what gnnvc_set_option sets (gnnvc_engine::opt) and the table of its keys — no HIP in it
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cctype>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/gnnvc.h"
#include "gnnvc_device_mem.h"
#include "gnnvc_kernels.h"
#include "gnnvc_multi.h"
#include "gnnvc_options.h"

using gnnvc::GraphDev;
using gnnvc::StagePlan;

namespace gnnvc_eng {

enum LayerKind { kLinear = 0, kGraph = 1, kRelu = 2, kSigmoid = 3 };

struct Layer {
    LayerKind kind;
    uint32_t k = 0, m = 0;          // linear: W is k x m
    std::vector<float> W, bias;     // host copies
    size_t w_off = 0, b_off = 0;    // float offsets in the device parameter buffer
};

}  // namespace gnnvc_eng

using gnnvc::DevBuf;
using gnnvc::PinBuf;
using gnnvc_eng::Layer;
using namespace gnnvc_eng;

struct gnnvc_engine {
    int device = 0;
    // gnnvc_create_multi: this handle is the FRONT of several devices — an ordinary engine on devices[0] (model, layer-level
    // entry points, staging memory, the assembled scores) whose graph hand-offs and forwards go to `multi` (gnnvc_multi.cpp)
    gnnvc::MultiState *multi = nullptr;
    std::string name;
    std::vector<Layer> layers;
    std::vector<StagePlan> stages;  // non-empty iff every stage is of a trained shape (gnnvc::stage_variant): the specialised kernels and plans
    // Generic stages (option "generic_stages", k_stage_any): the stage list of every model of the fused layer pattern whose
    // widths fit gnnvc::stage_any_fits — the trained shapes included, which only option value 2 sends there.
    std::vector<StagePlan> gstages;
    bool generic_ran = false;       // gnnvc_get_info "generic_stages_active": the last forward ran k_stage_any
    // gnnvc_set_generic_big_stages: 0 = off, else the LDS limit (65 536 .. 163 840 bytes) under which stages outside the default
    // bounds are admitted to gstages (gnnvc::stage_any_route; every plan in gstages carries the value it was derived under)
    uint32_t big_lds = 0;
    // gnnvc_set_generic_feature_width: 0 = off, else what f and a stage's last width may be (33 .. 64) instead of 32; carried by
    // every plan in gstages like big_lds
    uint32_t feat_width = 0;
    // gnnvc_set_generic_patterns: 0 = off, else the mask of GNNVC_PATTERN_PROLOGUE | GNNVC_PATTERN_OPEN_END (a dense stage in front
    // of the first graph layer; a model that ends in a ReLU or in its bare linear layer); carried by every plan in gstages too
    uint32_t patterns = 0;
    // gnnvc_set_generic_live_columns: 0 = off, else 1 .. 100 — inside a whole forward a graph stage with f >= 2 that does not end in
    // its bare linear layer gathers from the compact table of its input's live columns iff kept * 100 <= live_percent * f, decided
    // on the device (k_any_live_mask, k_any_live_pack).  Not carried by the plans: it changes no admission.  live_table = the
    // table (n x the widest eligible f, an engine buffer of its own), live_desc = a 16-byte descriptor per stage, zeroed by each
    // such forward, live_seen[s] = the last forward examined stage s (what the "generic_live_*_<s>" read-outs copy back).
    // (the buffers themselves are declared with the feature buffers below, behind the streams)
    uint32_t live_percent = 0;
    std::vector<uint8_t> live_seen;
    bool generic_on() const { return !gstages.empty() && (opt.generic == 2 || (opt.generic == 1 && stages.empty())); }
    const std::vector<StagePlan> &stage_list() const { return generic_on() ? gstages : stages; }   // what the ABI reports and runs
    // Heavy rows of generic stages (gnnvc_set_generic_heavy_rows): rows of at least heavy_from entries (0: none) get a workgroup
    // each for their sums (k_any_heavy_sums), beside or ahead of the light rows' k_stage_any.  The list and the sums are the
    // engine's; what is known about the current graph is in pg.heavy.
    uint32_t heavy_from = 512;      // the trained path's long-row threshold
    // Giant rows of generic stages (gnnvc_set_generic_giant_rows): the listed rows of at least max(ggiant_from, heavy_from) entries
    // (0: none) take the trained path's exact parallel scan instead of k_any_heavy_sums' one chain per column: k_any_giant_gather
    // into a slab of the engine's own (ag_* below; the classing: pg.ggiant), k_giant_segsum / k_giant_segmap / k_giant_sum, k_any_giant_place.
    uint32_t ggiant_from = 16384;   // the trained path's giant_row_threshold
    int ggiant_segments = -1;       // 1 = one stream on several waves, 0 = one wave walks each stream, -1 = by the graph (find_giant's rule)
    int in_width = 1, out_width = 1;
    int max_width = 1;
    bool ends_in_sigmoid = false;
    float ws = 120.0f;  // graph_layer::WEIGHT_SCALE default (reference include/gnn_inference.hpp:25)

    gnnvc::Options opt;             // everything gnnvc_set_option sets (gnnvc_options.h)
    // The streams this engine made, ahead of every buffer and event: members go in reverse order, so the streams outlive
    // what their work may refer to (gnnvc_destroy has waited for them before anything goes).  aux_stream = the side queue.
    gnnvc::Stream own_stream, aux_stream;
    hipStream_t stream = nullptr;   // the main stream in force: own_stream or the caller's (gnnvc_set_stream)
    std::vector<gnnvc::Event> ev;  // stage boundaries of the last forward
    int ev_count = 0;
    bool ev_stages = false;                  // the last forward recorded an event per stage (forward_timing 2)

    DevBuf<float> params;
    // Every member has one of three lifetimes, and where it is declared says which.  The ENGINE's: the model, options, streams and
    // events above and, below Call, every DevBuf / PinBuf, one struct per owner (blk, lt, c4, t4, srt, gi, prune_buf ...: buffers keep
    // their capacity across graphs on purpose), plus what is carried across graphs by design, each with its reason.  The RESIDENT
    // GRAPH's: PerGraph, a nested struct per owner, plain data without a buffer handle — reset_graph_state assigns a fresh one and
    // does nothing else, and each owner's builder (find_long, prepare_table_tiles, lt_begin, c4_begin, class_heavy_rows) begins by
    // assigning its own struct.  The CALL's or forward's at hand: Call, never reset as a whole (find_long and c4_begin restart
    // the member each owns: srt_cur, c4_emit_zero).
    //
    // A plan being put together (round 3): the expensive passes — counting and regrouping a slice's entries by column block — need
    // nothing but that slice's rows, so a hand-off runs them piece by piece on the second stream while the rest of the column array
    // is still crossing the bus (flat layouts only); begin / advance / finish: see lt_begin .. c4_finish below.
    struct PlanBuild {
        bool open = false, mapped = false;
        uint32_t base = 0, end = 0, slice_rows = 0, slices = 0, chunks = 0, rows = 0, nblocks = 0, bc = 0, slack = 0, done = 0;
        uint64_t entry_cap = 0, plan_nnz = 0;
        gnnvc::PlanMap pm;
    };
    // pruned adjacency of the 16-wide stages (kernels: k_prune_*), one per consumer stage: built from the input the stage
    // sees the second time the graph is scored; every later call proves on the device that its input still fits
    struct PrunePlan {
        bool tried = false, ready = false, deferred = false;
        // round 4: built at HAND-OFF from the set the graph alone predicts (k_predict_zero_f1: the reference driver's input is
        // x = W / ws, so the first 16-wide stage's zero rows follow from the weights) — proven per call like any other set;
        // verified: a forward has run with it and the host has seen that its check passed (if not, the plan is dropped and
        // rebuilt from the input the stage really sees)
        bool predicted = false, verified = false;
        bool from_prev = false;             // built from the previous stage's kept entries (its set is contained in this one)
        uint64_t kept = 0;                  // entries left
        uint64_t members = 0;               // vertices in the set
        uint32_t sn = 0;                    // rows of the list in PruneBufs::svertex
        bool slist = false;
        uint32_t eff_thresh = 0xFFFFFFFFu;   // entries left from which a row goes to the long-row kernel
    };
    // A few row ranges of the degree-sorted tile order are cached: a vertex-partitioned caller alternates between its own rows and
    // (for a replicated stage) the whole graph, or between the pieces of a pipelined stage — each range is sorted once per graph.
    struct SortedRange {
        bool valid = false, use = false;
        uint32_t lo = 0, hi = 0, n = 0;
        uint64_t stamp = 0;
    };
    static constexpr int kSortedRanges = 6;
    struct PerGraph {
        uint32_t graph_uses = 0;        // stage-0 executions on the current graph
        bool wide_used = false;         // a stage since the hand-off ran on wide tiles
        // memsets the plans' launches queued between kernels since the last whole forward on this graph began (gnnvc_get_info
        // "plan_memsets_last_forward": 1 in a steady forward on the plans, the LDS table's flag; no forward on this graph yet: 0)
        uint32_t plan_memsets = 0;
        double plan_build_ms = 0.0;     // host wall time spent building per-graph plans for the current graph (they end in stream syncs)
        double early_ms = 0.0;          // host time the hand-off spent classing the graph and queuing builds before the commit
        double handoff_build_ms = 0.0;  // ... and prepare_plans' share of plan_build_ms
        bool empty_slice = false;       // gnnvc_attach_graph_slice with no rows: every stage call is a no-op
        // the next graph derived from this one (gnnvc_derive_graph_begin / _commit); every hand-off ends an open derivation
        bool der_open = false;
        uint32_t der_n_new = 0;
        uint64_t der_nnz_new = 0, der_tail_total = 0;
        // row classes (find_long / find_giant).  Long rows (degree >= long_thresh): one workgroup each, on aux_stream beside the
        // tile kernel; giant rows (degree >= giant_thresh, a subset of them): CSR-order sums evaluated in parallel (exact_sum.h)
        struct Rows {
            uint32_t n_long = 0, long_thresh = 0xFFFFFFFFu;
            uint32_t thresh_f16 = 0xFFFFFFFFu;   // 16-wide stages: rows >= this go to k_long_f16 (>= long_thresh, the list's threshold)
            uint64_t long_entries = 0;           // entries of the listed rows
            uint32_t n_giant = 0, giant_thresh = 0xFFFFFFFFu, giant_blocks = 0, maxseg = 0;
            uint64_t giant_entries = 0;
            bool giant_walk_bound = false;       // (walk_bound: the longest stream's walk is what a stage waits for, find_giant)
            bool interleave = false;             // deal natural tiles round-robin (work is unevenly spread over the row range)
            bool sorted_wanted = false;          // degree-sorted tile order, decided from the measured tile waste
            double waste = 0.0, tail = 0.0;
        } rows;
        SortedRange sorted[kSortedRanges];       // (the lists themselves: srt.range[])
        // column-blocked plan of the F = 1 stage: built (ready) / build attempted (tried) — on the graph's SECOND forward: it costs
        // about as much as it saves on one, and the reference's driver uses every graph exactly once, src/GNN_VC.cpp:171-192
        struct Blk {
            bool ready = false, tried = false;
            uint32_t count = 0, cols = 0;
        } blk;
        // LDS-table plan of the F = 1 stage (same timing as the blocked plan).  LtPlan is what lt_begin starts afresh ...
        struct LtPlan {
            bool ready = false, tried = false;
            uint32_t bits = 8;              // width of the plan's table entries: 8, 10 or 16 bits per vertex (by the graph's largest weight)
            bool mapped = false;            // skewed graphs: rows dealt to slices (lt.rowmap), blocks of equal mass, rows below plan_thresh
            uint32_t plan_thresh = 0xFFFFFFFFu;
            uint32_t rows = 0, chunks = 0, blocks = 0, steps_total = 0, last_entry = 0;
            uint32_t base = 0, end = 0;     // the plan's row range: the rows this engine holds when it was built
            PlanBuild pb;
        };
        // ... and the rest outlives a rebuild on the same graph.  (round 4) The device's per-forward verdict on the byte table comes
        // back behind whole forwards like the compact table's: an input that is not k / ws leaves the plan's launches empty and — in
        // the skewed layout, whose rows below the giant ones are all the tile kernel's then — makes the stage several times slower
        // than without the plan; one miss there, three on the consecutive-row layout, switch it off for the graph
        struct Lt : LtPlan {
            bool used = false, off = false;
            uint32_t unfit_runs = 0;
        } lt;
        // compact-table plan of the 16-wide stages (built like the LDS-table plan); C4Plan is what c4_begin starts afresh
        struct C4Plan {
            bool ready = false, tried = false;
            int prepared_stage = -1;             // gnnvc_stage_input_ready: the table holds this stage's input ...
            const float *prepared_in = nullptr;  // ... as found at this address
            bool seeded[4] = {false, false, false, false};
            uint32_t rows = 0, chunks = 0, steps_total = 0, block = 0, last_entry = 0, nblocks = 0, nslices = 0;
            uint32_t base = 0, end = 0;          // the plan's row range: the whole graph, or the rows a multi-GPU rank computes
            uint32_t dirty_cap = 0;
            PlanBuild pb;
        };
        // Does the device keep finding a stage's input unfit for the plan (more than its tables' columns live: low-degree graphs)?
        // Whole forwards copy the verdicts out behind themselves (fit_pin); three misses in a row switch the plan off for that stage
        // of this graph — its counting, choosing and empty launches cost up to 17 % of a forward that then gathers anyway.
        struct C4 : C4Plan {
            bool range_mode = false;             // a driver asked for a range plan (gnnvc_stage_input_ready): no whole-graph plan any more
            bool fit_pending = false, fit_used[4] = {false, false, false, false}, stage_off[4] = {false, false, false, false};
            uint32_t unfit_runs[4] = {0, 0, 0, 0};
            uint32_t fit_calm = 0;               // verdicts in a row that changed nothing: from four on, only every eighth forward asks
            uint32_t fit_skip = 0;
            int last_desc = 0;                   // word offset in c4.desc of the plan's last launch (tests / tools)
            // Elided rows (gnnvc::CompactElide): elide_ok[s] = the last verdict seen for consumer stage s said that its producer's
            // table was taken as written — only then is the producer of its input allowed to leave out full rows; any other
            // verdict withdraws it until the stage fits again.  elided_last = producers launched that way in the last whole forward
            // ("elided_row_stages_last_forward").
            bool elide_ok[4] = {false, false, false, false};
            uint32_t elided_last = 0;
        } c4;
        // Table tiles (round 4; k_stage_t4): graphs too small for the compact-table plan and too large for their feature rows to sit
        // in an L2 (50 - 400 K vertices: BASELINE configs[1]) gather the 16-wide stages' neighbours from the 16-byte compact table of
        // the input — written by the kernel that produces the input, for the columns the previous forward chose — inside whole forwards.
        struct T4 {
            bool ok = false;                     // the current graph qualifies
            bool used = false;                   // the forward whose verdicts are on their way ran with the table tiles offered
            bool fit_seen[4] = {false, false, false, false};   // the stage's table fit in the last forward whose verdict has arrived
            uint32_t unfit_runs = 0;             // forwards in a row whose first 16-wide stage left the launch to the gathering kernel
        } t4;
        PrunePlan prune[4];
        // Filtered gather: while a skewed graph's 16-wide stage has no pruned adjacency (the graph's first forward: the reference's
        // driver never comes back for a second), its kernels look every entry's target up in the bitmap of THIS input's all-zero
        // rows, written just before them, and fetch the pad row instead (GraphDev::zero_bits; nothing to build, nothing to prove).
        struct Filter {
            bool filtered[4] = {false, false, false, false};   // the last call of the stage was offered the bitmap
            bool borrowed[4] = {false, false, false, false};   // the last call of the stage ran on the PREVIOUS stage's predicted plan (gather_view)
            // ... and the targets a filtered stage found outside its set, left per row in prune_buf[stage].pcol / .prp (the buffers of
            // the plan that is not built yet), are the adjacency of the NEXT 16-wide stage of the same forward when the device finds
            // that stage's input to keep the set all zero (GraphDev::keep_col / short_col)
            bool short_used[4] = {false, false, false, false};   // the last call of the stage was offered an earlier stage's lists
            uint32_t short_min = 0, short_max = 0;   // the degrees [min, max) of the rows that have a list
            int short_from = 0;                  // the stage whose filtered call left them (0 = none)
        } filter;
        // generic stages: the graph's heavy rows (class_heavy_rows) — known = classed, at the threshold thresh
        struct Heavy {
            bool known = false;
            uint32_t rows = 0, thresh = 0;
            uint64_t entries = 0;
        } heavy;
        // ... and the giant ones among them, classed with from / seg as set at the time: rows, gather blocks, segments of the
        // longest stream (0: one wave walks each stream), the degree from which a listed row is giant (0xFFFFFFFF: none)
        struct GGiant {
            uint32_t from = 0, rows = 0, blocks = 0, maxseg = 0, min = 0xFFFFFFFFu;
            int seg = -1;
            uint64_t entries = 0;
        } ggiant;
        // backward pass (gnnvc_backward.cpp): symmetric = is the adjacency symmetric with multiplicities (-1: not checked yet; the
        // check runs once per resident graph, on the device); saved = the engine's train buffers hold a training forward on THIS graph
        struct Train {
            int symmetric = -1;
            bool saved = false;
        } train;
    };
    PerGraph pg;
    uint32_t giant_f16() const {
        if (!pg.rows.n_giant) return 0xFFFFFFFFu;
        // by the graph: a 65 536-entry row's add chain in k_long_f16 is ~0.26 ms — lost in the stages of a graph with 64 M entries
        // and more (R-MAT-22 2.98 -> 2.88 ms, R-MAT-24 12.6 -> 11.6 ms), what the stages of a smaller one would wait for (R-MAT-20
        // 0.99 -> 1.05 ms, power-law 1.03 -> 1.30 ms).  (16 streams per row: three times a long row's traffic — worth it only for
        // the rows whose add chain a stage would wait for)
        if (opt.giant_f16_auto && g.nnz < (64ull << 20)) return pg.rows.giant_thresh;
        return std::max(pg.rows.giant_thresh, opt.giant_f16);
    }

    // the call's or forward's at hand: written by the call that reads it; no hand-off resets them (the read-outs below outlive one)
    struct AuditCheck {
        int stage;
        uint32_t lo, hi;
        std::string plan;                    // what produced the stage (StageChoice, views, side queues)
    };
    struct Call {
        int c4_fused_for = -1;          // stage whose input statistics (and table) the previous stage kernel of this forward produced
        int c4_elided_for = -1;         // ... and whose input that kernel was allowed to write without the full rows of unflagged vertices
        bool c4_emit_zero = false;      // the last thing queued on c4.emit_counts was a k_c4_choose that clears them behind its read
        int side_join = 0;              // what the stage at hand joins on: 0 nothing, 1 the long rows' queue, 2 the giant rows' queue
        bool stage_wide = false;        // the last launch_main ran the stage on wide tiles (audit reports)
        int srt_cur = -1;               // the entry of pg.sorted ensure_sorted selected for the call in progress
        bool t4_now = false;            // the forward at hand runs with the table tiles offered
        uint32_t heavy_last_rows = 0;   // gnnvc_get_info "generic_heavy_last_rows": listed rows of the last forward / stage call (0 = one launch)
        uint32_t ggiant_last_rows = 0;  // "generic_giant_last_rows": giant rows of the last forward / stage call
        bool ggiant_last_segmented = false;   // "generic_giant_last_segmented": that call used several waves per stream
        bool audit_now = false;         // the call at hand is audited
        std::vector<AuditCheck> audit_pending;   // the checks of the call at hand: record i of audit_rec is check i's
    };
    Call call;

    // the engine's again.  The resident graph itself: every hand-off writes g / have_graph before it resets pg
    GraphDev g;
    bool have_graph = false;
    DevBuf<uint32_t> rowptr, col, w, nw;
    // staged hand-off (gnnvc_graph_staging .. gnnvc_commit_staged_graph)
    PinBuf<uint32_t> pin_rowptr, pin_col, pin_w, pin_nw;
    PinBuf<uint32_t> pin_small;   // host side of small device<->host round trips
    // What describes a CANDIDATE graph on its way in and is consumed by its hand-off: the staging counters; early_* (handoff_early:
    // plans begun while the column array arrives; set while pg still describes the previous graph); pre / pre_armed (below)
    uint32_t staged_n = 0;
    uint64_t staged_nnz = 0, staged_sent = 0;   // columns [0, staged_sent) are already on their way
    bool staging = false;
    bool early_open = false, early_declined = false;
    struct PreClass {
        bool valid = false, cuts = false, waste = false, longs = false;
        uint32_t lo = 0, hi = 0, waste_thresh = 0, heavy_from = 0, long_thresh = 0;
        uint32_t cut[9] = {0};
        unsigned long long sums[2] = {0, 0};
        uint32_t found[4] = {0, 0, 0, 0};
    } pre;
    bool pre_armed = false;                  // set by the hand-off that ran classify_hand_off, right before ITS find_long (which clears it): no other find_long — the early hand-off's, a later graph's after a failed attach — may take what was learned about another candidate
    DevBuf<uint32_t> cls_dev;                // classify_graph's 16 words of device scratch
    PinBuf<uint32_t> cls_pin;                // ... and its 24 result words
    uint32_t *cls_pin_dev = nullptr;
    gnnvc::Event ev_piece;
    // the next graph derived from the resident one (pg.der_*)
    DevBuf<uint32_t> rowptr2, col2, der_old_row, der_new_of, der_tail, der_tailptr, der_tailcols;
    DevBuf<unsigned long long> hash_buf;
    std::vector<uint32_t> der_tail_host;
    // feature buffers
    DevBuf<float> x, h[2], scores, logits;
    DevBuf<float> scratch[2];  // layer-level entry points / unfused path / generic stages (ping-pong rows of up to 32 columns)
    DevBuf<float> live_table;                 // gnnvc_set_generic_live_columns: the compact table (above)
    DevBuf<unsigned long long> live_desc;     // ... and two words per generic stage: {mask, kept | used << 32}
    struct BlockedBufs {   // column-blocked plan (pg.blk; see gnnvc_kernels.hip)
        DevBuf<uint32_t> ptr, col, scratch, flag;
        DevBuf<float> acc;
    } blk;
    struct LdsTableBufs {   // LDS-table plan (pg.lt)
        DevBuf<uint32_t> rowmap, first, bstart;
        DevBuf<uint8_t> bytes;
        DevBuf<uint32_t> entries, segcnt, stepptr, stepcnt, bad;
        DevBuf<uint4> steps;
        // scratch of layout_skewed_plan (skewed graphs): the degree-sorted row list, released behind the dealing, and coarse = a
        // uint16 per 256 columns, their block
        DevBuf<uint32_t> skew_vertex, skew_coarse;
        DevBuf<uint4> skew_meta;
    } lt;
    struct CompactBufs {   // compact-table plan (pg.c4)
        DevBuf<uint32_t> entries, segcnt, stepptr, stepcnt, desc;
        DevBuf<uint4> steps;
        DevBuf<float> table, acc, agg16;
        DevBuf<uint32_t> round_counts;     // next dirty-row slot of each round of the aggregation grid (compact_rounds() words; set by k_c4_choose)
        DevBuf<uint32_t> dirty;
        DevBuf<unsigned long long> counts, emit_counts;
        DevBuf<uint32_t> elide;            // gnnvc::kElideWords words per consumer stage (k_c4_choose writes them, k_c4_compact and the verdicts read them)
    } c4;
    std::vector<gnnvc::Event> round_ev;    // "round k's sums are done" (main stream -> aux stream)
    static constexpr int kDescWords = 16;   // per consumer stage (see k_c4_choose); the build flag follows the last stage's
    PinBuf<uint32_t> fit_pin;                // the verdicts whole forwards copy out behind themselves (pg.c4.fit_*, pg.lt, pg.t4)
    uint32_t *fit_dev = nullptr;             // fit_pin as the device sees it (the verdict words are WRITTEN there by one small kernel)
    gnnvc::Event ev_fit;
    struct PruneBufs {   // pruned adjacency (pg.prune[])
        DevBuf<uint32_t> prp, pcol, heavy;
        DevBuf<uint32_t> svertex;            // skewed graphs: the engine's rows below the long-row threshold BY ENTRIES LEFT, heaviest first
        DevBuf<uint4> smeta;                 // ... with their pruned ranges
    } prune_buf[4];
    DevBuf<uint32_t> prune_flags, prune_scratch, prune_off;   // (off / mask: per chunk of 64 entries, while a plan is built)
    DevBuf<unsigned long long> prune_mask;   // flags: [stage] = this call's verdict (0 = the pruned adjacency applies), [3] = observe
    DevBuf<uint32_t> filter_bits[4];          // filtered gather (pg.filter)
    DevBuf<unsigned long long> filter_info;   // [4 * stage]: {degrees of the set's vertices, their number, verdict on an earlier stage's lists}
    struct TableTileBufs {   // table tiles (pg.t4)
        // Carried across graphs by design (prepare_table_tiles says why): choice_live = a forward with table tiles has run on this
        // engine, the descriptors hold a choice; parity = which of a stage's two descriptors the producers read in the forward at hand
        bool choice_live = false;
        uint32_t parity = 0;
        DevBuf<float> table[2];               // [0]: the table of stage 1's input, [1]: of stage 2's (a stage gathers from one while emitting the other)
        DevBuf<uint32_t> desc;                // [stage - 1][parity][16 words]
        DevBuf<unsigned long long> counts[2]; // the producers' per-column counters: [stage - 1], two sets of kEmitCounters each (by parity, like the descriptors)
        unsigned long long *counts_of(int stage, uint32_t par) { return counts[stage - 1].p + (size_t)par * gnnvc::kEmitCounters; }
        uint32_t *desc_of(int stage, uint32_t par) { return desc.p + ((size_t)(stage - 1) * 2 + par) * 16; }
    } t4;
    struct SortedBufs {   // degree-sorted tile order (16-wide stages, skewed graphs); built per row range on demand (pg.sorted[])
        struct {
            DevBuf<uint32_t> vertex;
            DevBuf<uint4> meta;
        } range[kSortedRanges];
        uint64_t clock = 0;                // stamps only order the ranges of one graph: it may run on
        DevBuf<uint32_t> hist;
        DevBuf<unsigned long long> sum;
    } srt;
    DevBuf<uint32_t> long_list, long_count;   // long rows (pg.rows)
    struct GiantBufs {   // giant rows (pg.rows): (segsum / segmap: one stream on several waves, see k_giant_segmap)
        DevBuf<uint4> meta, segmap;
        DevBuf<unsigned long long> off;
        DevBuf<float> slab, agg, segsum;
    } gi;
    // generic stages' heavy rows (heavy_from above): find_long_rows' list and count words, and the sums — rows x the widest stage input
    DevBuf<uint32_t> heavy_list, heavy_count;
    DevBuf<float> heavy_sum;
    // generic stages' giant rows: {row, first entry, degree, first gather block} heaviest first, each row's slab offset and position
    // in heavy_list, the slab (per row: the widest stage input x the degree rounded up to giant_window() floats), the aggregates
    // (rows x f of the stage at hand) and, with several waves per stream, the segments' sums and maps.  Not the trained path's gi.
    DevBuf<uint4> ag_meta, ag_segmap;
    DevBuf<unsigned long long> ag_off;
    DevBuf<uint32_t> ag_pos;
    DevBuf<float> ag_slab, ag_agg, ag_segsum;
    gnnvc::Event ev_fork, ev_join;
    // (the long rows' and the giant rows' stream handles: the side queue again, not owned — ensure_side_streams — with join events of their own)
    hipStream_t long_stream = nullptr;
    gnnvc::Event ev_long;
    int side_probes = 0;             // streams tried until one ran beside the main stream (info "side_queue_probes")
    bool side_beside = false;        // ... and whether one did (info "side_queue_runs_beside")
    hipStream_t giant_stream = nullptr;  // giant rows: three dependent launches, the side work's long pole -> a high-priority stream of its own
    gnnvc::Event ev_giant;
    // Backward pass (gnnvc_train_forward* / gnnvc_backward*, gnnvc_backward.cpp): the saved forward and the gradients' scratch, grown
    // on demand and kept across graphs like every buffer; whether they hold a forward of the resident graph is pg.train.saved.
    struct TrainBufs {
        DevBuf<float> params;            // the parameters the saved forward ran with (the model's own, or the caller's)
        DevBuf<float> acts;              // every layer's input and the last layer's output, back to back (act_off, in floats)
        std::vector<size_t> act_off;     // layers.size() + 2 offsets
        DevBuf<float> grad[2];           // gradient rows, ping-pong: n x the widest layer
        DevBuf<float> partials;          // k_bwd_linear_dw: row blocks x (k + 1) x m of the largest layer
        DevBuf<float> host_in, host_out; // the host forms' device side: scores gradient in, parameter gradient (+ grad_x) out
        DevBuf<uint8_t> row_ascends;     // the symmetry check's scratch
        DevBuf<uint32_t> sym_flag;
        DevBuf<float> fit_partials;      // k_mse_block: a loss partial per block of kGradBlockRows rows
        DevBuf<uint32_t> fit_counts;     // ... and its three counts
        size_t bytes() const {
            return (params.cap + acts.cap + grad[0].cap + grad[1].cap + partials.cap + host_in.cap + host_out.cap + sym_flag.cap +
                    fit_partials.cap + fit_counts.cap) * sizeof(float) + row_ascends.cap;
        }
    } train;
    gnnvc::KernelTraceSink ktrace;
    PinBuf<uint32_t> pin_info;  // small device -> host results that outlive the call that asked for them (never reallocated)
    DevBuf<uint32_t> dev_info;

    // on-device audit (options "audit_*", gnnvc_options.h): counters since the engine was made
    uint64_t audit_calls = 0;                // forward entry-point calls since the period was set
    DevBuf<unsigned long long> audit_rec;
    PinBuf<unsigned long long> audit_pin;
    uint64_t audit_runs = 0, audit_failures = 0, audit_repairs = 0, audit_nan_pairs = 0;
    long audit_last_stage = -1, audit_last_row = -1, audit_last_col = -1, audit_last_mismatches = 0;
    uint32_t audit_last_fused = 0, audit_last_plain = 0;

    std::string err;
};

static_assert(std::is_trivially_destructible_v<gnnvc_engine::PerGraph>);   // e->pg = PerGraph{} can neither free nor leak anything
static_assert(std::is_trivially_copyable_v<gnnvc_engine::PerGraph>);

namespace gnnvc_eng {

inline int fail(gnnvc_engine *e, int code, const char *fmt, ...) {
    if (e) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        e->err = buf;
    }
    return code;
}

#define HIP_TRY(e, call)                                                                   \
    do {                                                                                   \
        hipError_t rc_ = (call);                                                           \
        if (rc_ != hipSuccess)                                                             \
            return fail((e), rc_ == hipErrorOutOfMemory ? GNNVC_ERR_NOMEM : GNNVC_ERR_DEVICE, \
                        "%s: %s", #call, hipGetErrorString(rc_));                          \
    } while (0)

// entry points that read ONE device's resident graph have no meaning on the front of several devices
#define NOT_ON_MULTI(e, what)                                                                                          \
    do {                                                                                                               \
        if ((e)->multi) return fail((e), GNNVC_ERR_UNSUPPORTED, what " is not available on a multi-device handle (gnnvc_create_multi)"); \
    } while (0)

inline int hip_rc(gnnvc_engine *e, hipError_t rc) {
    if (rc == hipSuccess) return GNNVC_OK;
    return fail(e, rc == hipErrorOutOfMemory ? GNNVC_ERR_NOMEM : GNNVC_ERR_DEVICE, "%s", hipGetErrorString(rc));
}

inline int use_device(gnnvc_engine *e) {
    HIP_TRY(e, hipSetDevice(e->device));
    return GNNVC_OK;
}

// Generic stages' heavy rows: do the sums (k_any_heavy_sums) run on the side queue beside the light rows' k_stage_any, or do the
// three launches follow each other on the main stream?  The environment variable GNNVC_HEAVY_OVERLAP (0 | 1, read once per
// process) overrides the default, so that both orders can be measured with one library (profiles/generic_stages/README.md).
constexpr bool kHeavyOverlapDefault = true;
inline bool heavy_overlap() {
    static const bool on = [] {
        const char *s = getenv("GNNVC_HEAVY_OVERLAP");
        return s && *s ? atoi(s) != 0 : kHeavyOverlapDefault;
    }();
    return on;
}

// Generic stages' giant rows: does their gather (k_any_giant_gather, a throughput kernel) go to the main stream AHEAD of the fork —
// the trained path's giant_gather_first — instead of opening the chain on the side queue?  GNNVC_GIANT_GATHER_FIRST (0 | 1, read
// once per process) overrides the default; it means something only where the sums overlap (heavy_overlap()).  Both orders are
// measured in profiles/generic_stages/README.md, "Giant rows".
constexpr bool kGiantGatherFirstDefault = false;
inline bool giant_gather_first() {
    static const bool on = [] {
        const char *s = getenv("GNNVC_GIANT_GATHER_FIRST");
        return s && *s ? atoi(s) != 0 : kGiantGatherFirstDefault;
    }();
    return on;
}

// ---- gnnvc_backward.cpp: the backward pass's gnnvc_get_info keys ("graph_symmetric", "backward_workspace_bytes"); false = not one of them
bool backward_info(const gnnvc_engine *e, const std::string &key, long *value);
// ---- gnnvc_plans.cpp: the plans' read-outs that are spelled out there ("elided_row_stages_last_forward"); false = not one of them
bool plan_info(const gnnvc_engine *e, const std::string &key, long *value);

// ---- gnnvc_plans.cpp: what is built per graph -------------------------------------------------------------------------
int find_long(gnnvc_engine *e);                              // row classes of a new graph (long / giant rows, tile waste)
int class_heavy_rows(gnnvc_engine *e);                       // generic stages: the heavy rows of the current graph, once per graph and threshold
int ensure_sorted(gnnvc_engine *e, uint32_t lo, uint32_t hi);
int build_blocked(gnnvc_engine *e);
int build_lds_table(gnnvc_engine *e);
int build_compact(gnnvc_engine *e, uint32_t base = 0, uint32_t end = 0xFFFFFFFFu);
// a plan put together piece by piece (gnnvc_engine::PlanBuild): begin = eligibility, geometry, buffers; advance = count and
// regroup the slices up to a given one on a given stream; finish = the step records and the verdict
int lt_begin(gnnvc_engine *e);
int lt_advance(gnnvc_engine *e, uint32_t upto, hipStream_t stream);
int lt_finish(gnnvc_engine *e);
int c4_begin(gnnvc_engine *e, uint32_t base, uint32_t end);
int c4_advance(gnnvc_engine *e, uint32_t upto, hipStream_t stream);
int c4_finish(gnnvc_engine *e);
gnnvc::CompactPlan compact_plan(const gnnvc_engine *e);
gnnvc::LdsTablePlan lds_table_plan(const gnnvc_engine *e);
int ensure_side_streams(gnnvc_engine *e);
int reprobe_side_streams(gnnvc_engine *e);
int ensure_round_events(gnnvc_engine *e, size_t count);
int ensure_events(gnnvc_engine *e, size_t count);
int classify_hand_off(gnnvc_engine *e, const GraphDev &cand, uint32_t &bad);
int gather_view(gnnvc_engine *e, int stage, uint32_t lo, uint32_t hi, const float *in, bool gathering, bool sorted_tiles,
                GraphDev &gv, gnnvc::SortedOrder &so_p, bool matrix_cores = true, uint32_t long_from = 0xFFFFFFFFu);
int reserve_features(gnnvc_engine *e, uint32_t n);
int reserve_multi_front(gnnvc_engine *e, uint32_t n);
int prepare_plans(gnnvc_engine *e);                          // everything a forward needs that depends on the graph alone
int prepare_table_tiles(gnnvc_engine *e);                    // does the graph qualify for k_stage_t4, and its buffers
void reset_graph_state(gnnvc_engine *e);
int handoff_early(gnnvc_engine *e, uint32_t n, uint64_t nnz);
// host wall time of a plan build, added to pg.plan_build_ms (what was queued before is drained first: not the plan's cost)
template <class F>
int timed_build(gnnvc_engine *e, F &&f, bool may_build = true) {
    // (may_build false: the caller can already see that f will leave at its first test — a graph too small for the plan — and the
    // wait that keeps earlier work out of the build's time would only stall the forward: five of them made a small graph's SECOND
    // forward 60 us where its third takes 34)
    if (may_build) (void)hipStreamSynchronize(e->stream);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = f();
    e->pg.plan_build_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

}  // namespace gnnvc_eng
