/*
 * gnnvc.h — C ABI of the MI355X GNN-VC scoring engine (libgnnvc_hip.so).
 *
 * This is the drop-in boundary for the ONE hot path of KennethLangedal/GNN-MWVC:
 * the GNN forward `gnn::model::predict` and the layer `forward()`s it runs
 * (reference src/gnn_inference.cpp:20-81, include/gnn_inference.hpp:11-59) plus
 * the OpenBLAS seam `dot()` (reference src/matrix.cpp:106-122).  Plain
 * pointers and sizes only; no C++ or torch types.  Every entry point returns
 * GNNVC_OK (0) or a negative error code, never throws, and treats N = 0 as a
 * successful no-op (the reference calls predict with an empty graph at the end
 * of every run, src/GNN_VC.cpp:192 / SURVEY.md §3.2).
 *
 * There is no CPU fallback behind this ABI: without a HIP device every compute
 * entry point returns GNNVC_ERR_DEVICE.
 *
 * Numerics contract: logits — the input of the final sigmoid —
 * are bit-identical to the reference's on the same inputs (CSR-order fp32
 * neighbour sums, sequential-k fused-multiply-add chains, separately rounded
 * bias adds).  Device-side scores apply 1/(1+exp(-x)) with a device exp that is
 * a restatement of glibc's expf; hosts that need the reference's exact scores
 * apply their own libm to the logits (the C++ wrapper does).
 *
 * The reference-side binding a maintainer would add is shown in INTEGRATION.md.
 */
#ifndef GNNVC_H
#define GNNVC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNNVC_ABI_VERSION 1

enum {
    GNNVC_OK = 0,
    GNNVC_ERR_INVALID = -1,     /* bad argument / malformed model text */
    GNNVC_ERR_DEVICE = -2,      /* no HIP device, or a HIP call failed */
    GNNVC_ERR_NOMEM = -3,       /* host or device allocation failed */
    GNNVC_ERR_STATE = -4,       /* call out of order (e.g. forward before a graph) */
    GNNVC_ERR_UNSUPPORTED = -5, /* model / size outside what the engine handles */
    GNNVC_ERR_AUDIT = -6        /* the on-device audit (option "audit_period") found a fused stage's values wrong; the call
                                   completed, its outputs are as the fused path wrote them, gnnvc_last_error says where */
};

typedef struct gnnvc_engine gnnvc_engine;

int gnnvc_abi_version(void);
const char *gnnvc_strerror(int code);
/* Detail of the last failure on this engine (empty string if none). */
const char *gnnvc_last_error(const gnnvc_engine *e);

/* ---- model ----------------------------------------------------------------
 * gnnvc_create replaces `istream >> gnn::model` (reference
 * src/gnn_inference.cpp:120-139 + src/matrix.cpp:97-104): `model_text` is the
 * reference's text format (`<name> <n> Layers`, then Linear_Layer / Graph_Layer /
 * ReLU_Activation / Sigmoid_Activation records).  `device` is the HIP device
 * ordinal.  The parameters are uploaded once. */
int gnnvc_create(gnnvc_engine **out, const char *model_text, size_t len, int device);
void gnnvc_destroy(gnnvc_engine *e);

/* Several devices behind ONE handle (SURVEY.md §8b's `n_devices`; §5: "one process driving 8 devices").  The reference has one
 * call site, m.predict(x, out, g) on one thread (src/GNN_VC.cpp:192, include/gnn_inference.hpp:50): a drop-in that wants more
 * than one GPU has to partition behind that call, and this handle does.  devices[0 .. n_devices) are HIP ordinals (an ordinal
 * may repeat: several parts then share a device — how a one-GPU machine rehearses the path).  On such a handle
 *   gnnvc_upload_graph / the staged hand-off   cut the graph into n_devices contiguous row ranges of equal entry count (multiples
 *                         of 64 rows) and give device r the CSR slice of its rows (global column ids) — 1 / n_devices of the
 *                         graph's memory each — next to full-size replicated feature buffers;
 *   gnnvc_forward / gnnvc_forward_device        run every stage range by range — every device driven by a host thread of its own —
 *                         and, after the first and second stage, let each device send the rows it computed to every peer: in
 *                         pieces, packed to their live columns (gnnvc_pack_rows: 16 bytes a row on the metric graph; the
 *                         packing is chosen by the graph's first forward and checked lossless on every one), each piece stored
 *                         into the peers' receive buffers by one kernel (gnnvc_push_piece: a direct all-gather, one xGMI link
 *                         per peer, no ring, no host hop) under the next piece's kernels, and expanded there
 *                         (gnnvc_unpack_pieces); the scores (and logits) are assembled on devices[0].  gnnvc_forward_device
 *                         takes pointers on devices[0] and is complete when it returns — on an error too: every device is
 *                         drained first.  Options "multi_pieces" (pieces per part and stage; default 1 up to 4 devices, where
 *                         the per-range plans want whole ranges, 4 beyond), "multi_pack" 0 = full rows, "multi_push" 0 =
 *                         hipMemcpyPeerAsync per peer and piece, "multi_only_part" r = a forward runs part r's share only (a
 *                         timing rehearsal where parts share a device; its results are not complete), "multi_announce" -1|0|1 = a
 *                         part that runs a 16-wide stage as one piece announces the stage's complete input (compact table over
 *                         its rows: gnnvc_stage_input_ready; -1 = up to four devices).  A forward whose exception lists
 *                         overflow is repeated — up to three attempts, each with full rows for the stage that overflowed —
 *                         before it returns.  gnnvc_get_info: "multi_exchange_bytes_per_peer_stage0", "..._stage1" (bytes the
 *                         busiest part's pushes of the last forward wrote to one peer), "multi_packed_stage0", "..._stage1"
 *                         (is the stage's exchange packed), "multi_packed_columns_stage0", "..._stage1", "multi_pieces",
 *                         "multi_peer_stores" (every pair of devices can store into each other's memory),
 *                         "multi_part_span_us_<r>";
 *   gnnvc_set_weight_scale / gnnvc_set_option / gnnvc_synchronize / gnnvc_score_keys / gnnvc_last_forward_ms (total only)
 *                         and the layer-level entry points without a graph (linear, relu, sigmoid, sgemm, stream_sum) work
 *                         as on any handle; gnnvc_get_info adds "devices", "part_rows_<r>", "part_entries_<r>";
 *   the entry points that read ONE device's resident graph (attach_graph_device / _slice, stage_forward_device,
 *                         stage_input_ready, derive_graph_*, graph_row_hashes, reduction_flags, graph_layer_forward) return
 *                         GNNVC_ERR_UNSUPPORTED.
 * Results are those of a single device, bit for bit: a row is summed on one device in stored order.  n_devices = 1 is a
 * single engine behind the same code path. */
int gnnvc_create_multi(gnnvc_engine **out, const char *model_text, size_t len, const int *devices, int n_devices);

/* Generic-stage models on several devices behind one handle (opt-in).  gnnvc_create_multi keeps refusing every model but the
 * trained 32/32/16 one, and the gnnvc_set_generic_* calls keep returning GNNVC_ERR_UNSUPPORTED on its handle — so the opt-ins of
 * a generic model are made HERE, at creation, in *cfg (NULL = all defaults):
 *   size            sizeof(gnnvc_generic_config); anything else: GNNVC_ERR_INVALID;
 *   heavy_rows      as gnnvc_set_generic_heavy_rows;  GNNVC_GENERIC_DEFAULT (0xFFFFFFFF) = leave the engine's default (512);
 *   giant_rows      as gnnvc_set_generic_giant_rows;  GNNVC_GENERIC_DEFAULT = leave the default (16 384);
 *   giant_segments  as that call's `segments`; -1 = its rule;
 *   big_stages_lds  as gnnvc_set_generic_big_stages;    0 = off;
 *   feature_width   as gnnvc_set_generic_feature_width; 0 = off;
 *   patterns        as gnnvc_set_generic_patterns;      0 = off.
 * Null arguments, a wrong size or a value the matching single-device call would reject: GNNVC_ERR_INVALID with *out null, before
 * any device is touched.  Then
 *   a model of the trained shape               gives exactly the handle gnnvc_create_multi gives; cfg has no effect;
 *   a model that is a generic stage list under cfg   (option "generic_stages": gnnvc_is_fused on a single engine with the same
 *                         settings) runs the route below;
 *   a model that stays layer by layer under cfg      GNNVC_ERR_UNSUPPORTED, as is a stage list with a dense stage behind stage 0.
 * The config is applied to every part's engine before its stage list is read, and to the front handle: gnnvc_num_stages,
 * gnnvc_stage_widths, gnnvc_in_width, gnnvc_out_width, "generic_patterns", "generic_stage_layers_<s>" and their kin answer on the
 * handle as a single engine with the same settings would; "generic_heavy_rows", "generic_heavy_entries", "generic_giant_rows" and
 * "generic_giant_entries" are the parts' summed.  The gnnvc_set_generic_* calls stay refused on the handle.
 * The route: the graph is cut as for gnnvc_create_multi; every part holds x (n x in_width), two ping-pong buffers of n x wmax floats
 * (wmax: the widest intermediate stage output), scores and logits (n x out_width) — all reserved at hand-off, none inside a forward.
 * Every stage s runs piece by piece through gnnvc_stage_forward_device on the part's slice (k_stage_any: heavy and giant rows
 * included; the logits on the last stage), and after each piece of a stage that is not the last the piece's rows travel to every
 * peer as FULL rows of the stage's output width (1 .. 64 floats: no live-column codec, no first forward that chooses one), straight
 * into the peer's buffer of that stage: one kernel for all peers (gnnvc_push_rows; option "multi_push" 1, the default, and every
 * pair of devices with peer access — parts that share a device always have it) or one hipMemcpyPeerAsync per peer, on a stream of
 * its own under the next piece's kernels.  A graph stage waits for every peer's pieces of the stage before it; a dense stage 0
 * (GNNVC_PATTERN_PROLOGUE) waits for nothing; a model without a graph stage exchanges nothing; empty parts and empty pieces launch
 * and ship nothing.  Results are those of a single engine, bit for bit: a row is computed on one device in stored order.
 * Options: "multi_pieces", "multi_push" and "multi_only_part" (no earlier forward needed) keep their meaning, "poison_features"
 * fills n x wmax floats, "multi_pack" and "multi_announce" are accepted and change nothing.  gnnvc_forward_audited* audit every
 * part's rows (gnnvc_audit_stage_device, k_audit_any, right behind each piece's stage call; a mismatch is reported as
 * GNNVC_ERR_AUDIT once the job has drained; "audit_repair" is handed on); "audit_period" audits nothing on such a handle.
 * gnnvc_get_info: "multi_generic" (1 on this route, 0 on a trained handle), "multi_exchanges" (the number of exchanged stages: 0 with
 * one device), "multi_exchange_bytes_per_peer_stage<s>" (any exchanged stage s: the busiest part's rows x width x 4). */
#define GNNVC_GENERIC_DEFAULT 0xFFFFFFFFu
typedef struct gnnvc_generic_config {
    uint32_t size;            /* sizeof(gnnvc_generic_config); anything else: GNNVC_ERR_INVALID */
    uint32_t heavy_rows;      /* as gnnvc_set_generic_heavy_rows;  GNNVC_GENERIC_DEFAULT (0xFFFFFFFF) = leave the engine's default */
    uint32_t giant_rows;      /* as gnnvc_set_generic_giant_rows;  GNNVC_GENERIC_DEFAULT = leave the default */
    int32_t  giant_segments;  /* as that call's `segments`; -1 = its rule */
    uint32_t big_stages_lds;  /* as gnnvc_set_generic_big_stages;    0 = off */
    uint32_t feature_width;   /* as gnnvc_set_generic_feature_width; 0 = off */
    uint32_t patterns;        /* as gnnvc_set_generic_patterns;      0 = off */
} gnnvc_generic_config;
int gnnvc_create_multi_generic(gnnvc_engine **out, const char *model_text, size_t len,
                               const int *devices, int n_devices, const gnnvc_generic_config *cfg /* NULL = all defaults */);

/* model::set_weight_scale (reference src/gnn_inference.cpp:83-90): sets
 * graph_layer::WEIGHT_SCALE of every graph layer (default 120). */
int gnnvc_set_weight_scale(gnnvc_engine *e, float ws);

/* Run on a caller-owned hipStream_t (e.g. torch's current stream) instead of
 * the engine's own stream.  NULL restores the engine's stream.  Call it between forwards.  The engine's side queue (long and
 * giant rows, plan builders) has to sit on another hardware queue than the main stream; it is probed against the new one
 * (~0.3 ms) and replaced if the runtime put the two on the same queue: gnnvc_get_info "side_queue_runs_beside" says whether a
 * queue beside the main stream was found (0: skewed graphs' side work runs serialised — slower, never wrong). */
int gnnvc_set_stream(gnnvc_engine *e, void *hip_stream);
/* The stream the engine launches on at the moment (its own unless gnnvc_set_stream installed another): a caller orders its own
 * work behind the engine's asynchronous calls with it. */
int gnnvc_get_stream(gnnvc_engine *e, void **hip_stream);

/* Tuning options.  What a key decides about the graph itself — its row classes and thresholds, which plans it gets — is decided
 * when a graph is handed over (upload / staged commit / attach) and holds until the next one; what a key decides about the
 * launches — queues, kernel variants, when a plan that is still due is built — is read by the forward or stage call that follows.
 * A key may be set at any time, also under a resident graph with plans in force: every call that follows gives the same bits,
 * and the next hand-off leaves the engine as one that had the key set before its first graph — but for the table tiles' choice
 * of columns, which an engine carries from graph to graph and which changes time only (tests/test_gpu_option_flips.py
 * holds every key below to both, but the "audit_*" keys, "generic_stages" and "poison_features", which have tests of their own):
 *   "plans_at_handoff" 0|1|2  WHEN the per-graph plans below are built.  The reference's driver hands predict a new graph every
 *                         call and scores it once (src/GNN_VC.cpp:171-192), so what depends on the graph alone is built when
 *                         the graph is handed over (upload / staged commit / attach), not inside a later forward: 1 (default) =
 *                         the plans that ONE forward repays (degree-uniform graphs of at least "handoff_min_entries"
 *                         adjacency entries, default 24 Mi: LDS table + compact table; every graph: its tile order and
 *                         every buffer a forward would otherwise allocate), 2 = every plan the graph qualifies for whatever
 *                         it costs (callers who score a graph many times, or hide the build under a copy), 0 = inside the
 *                         graph's first two forwards (round 2's behaviour).  gnnvc_get_info "handoff_build_us" = what it took
 *   "pilot_rows"     n    first use of the compact-table plan on a graph: the producing stage's plain kernel over its first n
 *                         rows (default 65536, 0 = off) picks the next stage's table columns ahead of the real run, which
 *                         then writes the table on its way; the choice is re-made from the counts of all rows, so the pilot
 *                         changes time, never a result
 *   "filter_zero_rows" 0|1  a large skewed graph's FIRST forward (the reference's driver never comes back for a second): its
 *                         16-wide stages look every entry's target up in the bitmap of this input's all-zero rows and fetch the
 *                         pad row instead, the long rows walk lists a pass in front of them shortened — nothing is built, the
 *                         pruned adjacency ("prune_zero_rows") waits for a second forward (default 1; bit-identical either
 *                         way).  "filter_min_entries" (default 48 Mi) / "filter_min_long_percent" (25: the share of the
 *                         entries in long rows) say which graphs, "filter_min_percent" (50) from which share of the entries
 *                         pointing to zero rows the device uses the bitmap, "filter_keep_lists" 0 = every stage shortens the
 *                         full rows.  gnnvc_get_info: "filtered_stage1|2", "short_lists_stage2", "filter_mass_percent_stage1|2"
 *   "long_rows_on_main" -1|0|1  where the long rows' kernels run: the engine has ONE side queue beside its main stream (probed at
 *                         creation to sit on another hardware queue: gnnvc_get_info "side_queue_probes" / "side_queue_runs_beside");
 *                         the giant rows always take it, the long rows join them there (0) or run ahead of the tile kernel on the
 *                         main stream (1); -1 (default) = by the graph: on the main stream when the longest giant row's walk is
 *                         what a stage waits for.  "giant_gather_first" -1|0|1: the giant rows' gather on the main stream ahead
 *                         of the tile kernel (1) or on the side queue with the rest of their chain (0); -1 (default) = on the
 *                         main stream when it is small (at most 16 Mi giant entries) and the long rows are on the side queue
 *   "blocked_stage0" 0|1  column-blocked plan of the F = 1 stage (default 1; results are
 *                         bit-identical either way, it only changes memory traffic)
 *   "lds_table"      0|1|2  LDS-table plan of the F = 1 stage: when the input is x[v] = (float)W(v)/ws with integer
 *                         W(v) <= 65 535 (checked on the device at every forward), the neighbour values are read from a
 *                         table held slice by slice in LDS instead of gathered from memory — a byte per vertex for weights up
 *                         to 255, ten bits (three to a word) up to 1023, sixteen bits beyond (round 4; chosen per graph from
 *                         its largest weight and the weight scale: gnnvc_get_info "lds_table_bits"; "lds_table_bits" 8|10|16
 *                         forces a width, 0 = by the graph; "lds_table_min_chunks": how finely a short row range — a rank's
 *                         slice — is cut at least, default 128).  Default 1 = large graphs, skewed ones in their own layout
 *                         (byte table only); 2 = the consecutive-row layout on any large graph; 0 = off.
 *                         Takes precedence over "blocked_stage0"; bit-identical results
 *   "compact_gather" 0|1|2  compact-table plan of the 16-wide stages: when at most four feature columns carry
 *                         (nearly) all non-zeros of a stage's input — decided on the device at every forward —
 *                         neighbours are read from a 16-byte-per-vertex table swept block by block through L2
 *                         instead of 64-byte rows from memory (default 1 = large, non-skewed graphs); bit-identical
 *   "block_cols"     n    vertices per column block (default 524288 = 2 MiB of x)
 *   "blocked_min_n"  n    graphs with fewer vertices get none of the per-graph plans of the F = 1 stage (default 2^20)
 *   "compact_min_n"  n    ... nor the compact-table plan below the smaller of this (default 2^18) and "blocked_min_n"
 *                         (with default bounds the plans also want entries: 8 Mi for the compact table, 10 per row for the
 *                         F = 1 plans)
 *   "compact_first_forward_entries" n  the plans are built inside a graph's second forward; a graph with at least this
 *                         many adjacency entries builds the compact-table plan inside its FIRST forward, which one use
 *                         repays there (default 48 Mi; 0 = never) — what a caller gets who scores every graph once
 *   "overlap_dense"  0|1  last stage under the compact-table plan: dense layers of one round of the sums on a second
 *                         stream, under the next round's sums (default 1; bit-identical either way)
 *   "plan_chunk_rows" n   cap on the rows per chunk of the LDS-table and compact-table plans (default 0 = what
 *                         fits LDS); smaller chunks mean more rounds of the persistent grids — a test hook
 *   "long_row_threshold" d  rows of degree >= d get a workgroup of their own (0 = off); same CSR-order sums,
 *                         bit-identical results.  Default: by the graph — 256 where at most 16 Ki rows (and one row in
 *                         64) are that long, 512 otherwise; setting it (or "sorted_long_row_threshold") fixes it
 *   "lds_table_skewed" 0|1, "lds_table_skewed_rows" d  the LDS-table plan on SKEWED graphs (default 1): rows below d
 *                         entries dealt to slices of equal weight, column blocks of equal entry mass, giant rows (and
 *                         the rows from d on) beside it; d = 0 (default): 2048 while x (4 N bytes) fits the L2s
 *                         together, else everything below the giant rows.  Bit-identical
 *   "giant_row_threshold" d  long rows of degree >= d (default 16384, 0 = off) are summed by many waves at once:
 *                         their neighbour values are gathered by every CU into per-column streams and each stream's
 *                         sequential fp32 sum is evaluated with a parallel scan that reproduces the chain's
 *                         roundings (csrc/exact_sum.h); bit-identical results
 *   "giant_row_threshold_f16" d  the 16-wide stages send only rows of degree >= d the giant way.  Default: 65536 on graphs
 *                         of 64 Mi adjacency entries and more (sixteen streams per row are three times a long row's
 *                         traffic: worth it for the rows whose add chain a stage would wait for), "giant_row_threshold"
 *                         on smaller ones (there a 65 536-entry chain IS what a stage waits for); setting
 *                         "giant_row_threshold" sets this one too
 *   "giant_segments" -1|0|1  1 = a giant row's streams are cut into segments of 4096 addends summarised by many waves
 *                         at once (k_giant_segmap) and joined by one walk; 0 = one wave walks each stream; -1 (default) =
 *                         segments where the longest stream's walk would be what a stage waits for.  Same bits
 *   "side_streams"   0|1  1 (default) = long / giant rows on side streams beside the tile kernel; 0 = on the main
 *                         stream, one after the other (profiling: standalone kernel times)
 *   "kernel_trace"   0|1  HIP events around every main-stream kernel of a forward (gnnvc_kernel_trace)
 *   "mfma_dense"     0|1|2  dense layers on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, a
 *                         k-ordered fma chain: same bits as the VALU path): 0 = VALU, 1 = MFMA in
 *                         every stage, 2 = MFMA in the 16-wide stages only (default); immediate
 *   "sorted_tiles"   -1|0|1  16-wide stages take their 64-vertex tiles from a degree-sorted
 *                         vertex list instead of 64 consecutive rows (-1 = only when natural tiles
 *                         would spend more than twice the useful gather rounds, the default)
 *   "sorted_min_nnz" n     in auto mode, graphs with fewer adjacency entries keep natural tiles
 *                         (default 4 Mi: the sort costs more than it saves on a graph used once)
 *   "prune_zero_rows" 0|1  pruned adjacency of the 16-wide stages: adjacency entries whose target row is all zero in
 *                         the stage's input are left out of a second CSR (adding a row of zeros changes no bit of a
 *                         sum); EVERY call proves on the device that its input fits, else it uses the full adjacency.
 *                         1 (default) = the set of vertices is the rows found all zero when the plan is built (a
 *                         graph's stage inputs follow from its weights), 0 = off.  Bit-identical results
 *   "prune_predict"  0|1  (round 4) a large skewed graph — at least "prune_predict_min_entries" adjacency entries, default
 *                         48 Mi, "filter_min_long_percent" of them in long rows — gets the first 16-wide stage's pruned
 *                         adjacency when it is HANDED OVER, from the set of zero rows its own weights predict (the reference's
 *                         driver feeds x = W / ws, src/GNN_VC.cpp:189-191), proven per call like any other set; a graph scored
 *                         once runs its first forward on it and the next stage borrows it.  Default 1.  gnnvc_get_info:
 *                         "pruned_predicted_stage1", "pruned_borrowed_stage2"
 *   "dense_skip_zeros" 0|1  (round 4; A/B) the aggregate-only dense kernels of the compact-table plan leave out the first-layer
 *                         terms they know to be zero, and the hidden layers that run on the VALU (the 32 -> 32 and 32 -> 16
 *                         layers of the F = 1 stage kernel and of the aggregate-only dense kernels) leave out, wave by wave,
 *                         the terms whose input unit is zero in all 64 rows of the wave.  Bit-identical: a layer takes part
 *                         only if all its weights are finite and none of its biases has the bits of -0.0f, decided when
 *                         the model is loaded — gnnvc_get_info "dense_skip_layers": bit 3 s + l set = dense layer l + 1
 *                         of fused stage s may leave out zero terms (whatever this option says).  Default 1; 0 = every
 *                         chain runs all its terms
 *   "forward_timing" 0|1|2  (round 4) HIP events of a forward for gnnvc_last_forward_ms: 0 (default) = none — a record costs the
 *                         stream ~1.8 us, four of them were 5.5 us of a 30 - 80 us forward —, 1 = the forward's first and last
 *                         (total only), 2 = one per stage too
 *   "verdict_period" 1..64  (round 4) once four verdicts of the per-graph plans in a row have changed nothing, only every this-many
 *                         forwards ask for them (default 8; a verdict steers which kernels the NEXT forwards launch, never a result)
 *   "poison_features" 0|1  (tests, fuzz) a whole forward starts by filling the engine's own feature buffers (a multi-device
 *                         handle: every part's) with NaN bit patterns, so that a row no kernel writes — or no exchange delivers —
 *                         shows in the result instead of hiding behind what an earlier forward left there.  Default 0.
 *   "wide_tiles"     0|1  (round 4) graphs with fewer 64-vertex tiles than the chip has SIMDs — the reference CLI's later predict
 *                         calls — run a stage a WORKGROUP per tile (the gather on quads of lanes over four waves, each dense
 *                         layer's outputs a quarter per wave: the same fma chains, the same bits): the F = 1 stage up to
 *                         "wide_tiles_max_n" vertices (default 49 152), the 16-wide stages up to "wide_tiles_max_n_f16"
 *                         (default 131 072) where no plan has the stage; graphs without long rows.  Default 1.
 *                         gnnvc_get_info "wide_tiles_used"
 *   "table_tiles"    0|1  (round 4) graphs of "table_tiles_min_n" (default 49 152) vertices and more whose 16-byte-per-vertex
 *                         table fits "table_tiles_max_bytes" (default 6 MiB: n <= 393 K) and that are outside the compact-table
 *                         plan's range, without long rows: whole forwards gather the 16-wide stages' neighbours from an
 *                         L2-resident table of the input's four live columns, written by the kernel that produced the input
 *                         for the columns the previous forward chose (kept across graphs of one engine); vertices with
 *                         non-zeros elsewhere are flagged and their neighbours fetch those columns from the full rows —
 *                         bit-identical for any input.  Offered from a graph's second forward on, or its first when the
 *                         engine carries a choice over from its previous graph.  Default 1.  "table_tiles_solo" 0|1 (A/B):
 *                         0 = the gathering kernel is always launched behind the tiles.  gnnvc_get_info:
 *                         "table_tiles_active", "table_tiles_fit_stage1|2" (did the last forward's stage run on its table)
 *   "prune_min_entries" n  graphs with fewer adjacency entries do not prune (default 2^20);
 *   "prune_min_drop_percent" p  nor do graphs where less than p % of the entries would go (default 15);
 *   "prune_early_entries" n  skewed graphs with at least n entries build the plan in their first forward (default
 *                         2^26; 0 = always with the other plans, in the second)
 *   "prune_class_by_entries_left" 0|1, "prune_heavy_entries" n, "prune_giant_rows" 0|1  A/B switches of the plan: rows
 *                         classed by the entries they have left (default 1), the entry count from which the tile
 *                         kernel keeps rows of up to "sorted_long_row_threshold" entries (default 2^24; below: 512),
 *                         giant rows pruned too (default 1)
 *   "audit_period" k >= 0  on-device audit: every k-th call of a forward entry point on this engine (gnnvc_forward,
 *                         gnnvc_forward_device, gnnvc_stage_forward_device; counted from when the option was set, so calls k, 2k,
 *                         3k, ...) has each fused stage it runs recomputed right behind it — before the next stage is queued — by
 *                         a kernel that uses none of the plans (the CSR arrays only; sequential CSR-order sums, sequential fma
 *                         chains, separately rounded bias adds, as the layer-by-layer kernels state them) and compared bit for
 *                         bit with every value the fused path wrote (the stage output; the scores and logits of the last stage;
 *                         two NaNs count as equal).  A stage call checks its own row range, a sliced engine included.  An
 *                         audited call ends with one read-back of the records and SYNCHRONISES its stream; unaudited calls
 *                         launch, record and wait exactly as with the option off.  On a mismatch the call still runs all its
 *                         stages and returns GNNVC_ERR_AUDIT, gnnvc_last_error naming the stage, its row range, the number of
 *                         mismatching values, the first row and column with both bit patterns in hex, and the plan that produced
 *                         the stage; the engine stays usable.  Unfused models and generic-stage models (option "generic_stages")
 *                         audit nothing under the period: on a generic-stage model a call whose turn it is runs unaudited and
 *                         counts nothing.  The explicit calls audit them: gnnvc_forward_audited and
 *                         gnnvc_forward_audited_device audit every fused stage of one forward, whatever the period says and
 *                         without ticking its counter, and gnnvc_audit_stage_device checks rows the caller holds — for the
 *                         trained shapes and for generic stages alike (see "forward" below).  Default 0 (off).
 *   "audit_repair" 0|1    1 = the audit writes its own values over the mismatching ones: the call returns GNNVC_OK with correct
 *                         outputs (a repaired stage hands correct rows to the next one) and counts the repair.  Default 0.
 *   "audit_log" 0|1       1 = every audited call prints one stderr line, "gnnvc audit: audit_runs <n> audit_failures <n>
 *                         audit_repairs <n>" (the engine's totals; a multi-device handle's summed over its parts) followed by the
 *                         report of a failure — for drivers that cannot read gnnvc_get_info, e.g. through
 *                         GNNVC_OPTIONS=audit_period=1,audit_log=1.  Default 0.
 *   "audit_quiet" 0|1     1 = mismatches are recorded (counters, gnnvc_last_error) but not returned: the parts of a multi-device
 *                         handle, which reports them itself once the whole job has drained.  Default 0.
 *   "audit_flip_stage" -1|s, "audit_flip_row" r  (tests) in an audited call of stage s whose row range holds r, the lowest
 *                         mantissa bit of output value (r, 0) is flipped between the stage and its audit.  Unaudited calls are
 *                         never touched.  Default -1 (off).
 *                         gnnvc_get_info: "audit_runs" (stage checks done), "audit_failures" (checks with a mismatch),
 *                         "audit_repairs" (values repaired), "audit_nan_pairs" (NaN pairs taken as equal: with different bits
 *                         on the trained shapes, every pair on generic stages), and of the first
 *                         failing check of the last failing call: "audit_last_stage", "audit_last_row", "audit_last_col",
 *                         "audit_last_mismatches", "audit_last_fused_bits", "audit_last_plain_bits" (-1 / 0 before any).  A
 *                         multi-device handle decides per forward whether its parts audit; it sums their counters and reports
 *                         the last_* of the first failing part, its message prefixed "part <p>: ".
 *   "generic_stages" 0|1|2  models of other widths or depths than the trained one as fused stages (kernel k_stage_any; takes
 *                         effect at once).  The engine's specialised kernels and per-graph plans serve exactly the trained stage
 *                         shapes (5->32->32->16, 35->32->32->16, 35->32->16->1+sigmoid).  1 (default): a model of the pattern
 *                         stage+, a stage being Graph_Layer followed by d pairs (Linear_Layer, activation), 1 <= d <= 6 and d
 *                         free per stage, every activation a ReLU except the model's last, a sigmoid (a model that ends in a
 *                         ReLU stays layer by layer), whose widths fit 1 <= stage input width f <= 32 (first linear layer
 *                         k = 2 f + 3), every hidden width <= 64, a stage's last width <= 32, and whose every stage fits the
 *                         kernel's 64 KiB of LDS (transposed weights at one pitch per layer, biases, sixteen pairs of row
 *                         vectors; the kernel's LDS limit is not raised beyond that) — any number of stages, any input and
 *                         output width up to 32 — runs one fused kernel launch per stage with the layer-by-layer kernels'
 *                         arithmetic bit for bit: gnnvc_is_fused = 1, gnnvc_num_stages / gnnvc_stage_widths report its stages,
 *                         gnnvc_forward, gnnvc_forward_device and gnnvc_stage_forward_device run them (the pad row of d_in is
 *                         never read).  One stage outside the bounds leaves the whole model layer by layer.
 *                         A model whose every stage is of a trained shape is planned, launched and audited as ever.
 *                         0: such a model is not fused, has 0 stages and runs layer by layer (one launch per layer), as
 *                         before this option existed.  2 (tests): the trained shape is sent through the generic kernel as well,
 *                         none of its plans used.  Generic stages have no per-graph plan but the list of their heavy rows
 *                         (gnnvc_set_generic_heavy_rows below: rows of many entries get a workgroup each for their neighbour
 *                         sums, with the same bits) and, among those, of their giant rows (gnnvc_set_generic_giant_rows below:
 *                         rows of 16 384 entries and more are summed by the exact parallel scan, with the same bits; keys
 *                         "generic_giant_from", "generic_giant_segments", "generic_giant_rows", "generic_giant_entries",
 *                         "generic_giant_last_rows", "generic_giant_last_segmented").  The bounds above are the default ones:
 *                         gnnvc_set_generic_big_stages (below) admits, on request, stages with hidden widths up to 128 and
 *                         up to 160 KiB of LDS (keys "generic_big_lds", "generic_stage_lds_bytes_<s>",
 *                         "generic_stage_threads_<s>"), and gnnvc_set_generic_feature_width (below) input and last widths up
 *                         to 64 (key "generic_feature_width"), and gnnvc_set_generic_patterns (below) a dense stage in front
 *                         of the first graph layer and a model that ends in a ReLU or in a bare linear layer (keys
 *                         "generic_patterns", "generic_stage_dense_<s>", "generic_stage_end_<s>"), and gnnvc_set_generic_live_columns
 *                         (below) a gather from the compact table of a stage input's live columns, same bits (keys
 *                         "generic_live_columns", "generic_live_kept_<s>", "generic_live_used_<s>", "generic_live_mask_lo_<s>",
 *                         "generic_live_mask_hi_<s>").  "audit_period" audits nothing on
 *                         them, as on an unfused model: they are audited on demand, by gnnvc_forward_audited,
 *                         gnnvc_forward_audited_device and gnnvc_audit_stage_device (kernel k_audit_any: a wave per row, the
 *                         weights read as the model stores them — an implementation that shares nothing with k_stage_any; the
 *                         "audit_repair", "audit_quiet", "audit_log" and "audit_flip_*" options and every "audit_*" read-out
 *                         apply to it).  gnnvc_stage_input_ready, the row codec (16-column rows) and
 *                         gnnvc_create_multi with several devices keep returning GNNVC_ERR_UNSUPPORTED for them (several devices
 *                         are a call of their own for them, with the opt-ins made at creation: gnnvc_create_multi_generic).  On a
 *                         multi-device handle the option is stored and changes nothing.  gnnvc_get_info: "generic_stages",
 *                         "generic_stages_model" (1 = a forward would run the generic kernel now), "generic_stages_active"
 *                         (1 = the last forward did), "generic_stage_layers_<s>" (the dense-layer count d of stage s;
 *                         GNNVC_ERR_INVALID for a stage that does not exist or while the model is not generic),
 *                         "generic_max_dense_layers" (6).
 * gnnvc_get_info keys (further): "pruned_stage1|2", "pruned_entries_stage1|2", "pruned_vertices_stage1|2",
 * "pruned_last_ok_stage1|2" (did the last call of that stage use its pruned adjacency),
 * "compact_gather_last_ok", "compact_gather_last_passes", "compact_gather_last_dirty",
 * "compact_gather_blocks", "compact_gather_steps", "plan_build_us", "plan_memsets_last_forward" (the memsets the LDS-table and
 * compact-table plans queued between the kernels of the last gnnvc_forward_device, stage calls since included: 1 in a steady forward, the LDS table's flag),
 * "elided_row_stages_last_forward" (0, 1 or 2: the stage kernels of the last gnnvc_forward_device that were allowed to store a
 * wave's full 64-byte feature rows only where the compact table flags one of its vertices; results are the same either way).
 * gnnvc_get_info keys: "compact_gather_active", "compact_gather_chunks", "lds_table_active", "lds_table_chunks", "lds_table_steps", "mfma_dense", "sorted_tiles_active", "tile_waste_x100", "blocked_stage0_active", "blocked_blocks", "block_cols", "long_rows",
 * "long_row_threshold", "giant_rows", "giant_entries", "giant_row_threshold". */
int gnnvc_set_option(gnnvc_engine *e, const char *key, long value);
int gnnvc_get_info(const gnnvc_engine *e, const char *key, long *value);

/* Heavy rows of generic stages (option "generic_stages", kernel k_stage_any).  k_stage_any gives every row to sixteen lanes,
 * which walk a hub of tens of thousands of entries round by round while the rest of the device runs dry.  Rows of at least
 * from_degree entries therefore take another way: they are listed once per graph (at hand-off when the generic stage list is in
 * force, else by the first generic stage that runs on the graph: one pass over the row pointers and one 16-byte read-back), and
 * a stage call on a graph that has such rows is three launches — k_any_heavy_sums (a 256-thread workgroup per listed row: the
 * row's neighbour sums, one fp32 add per neighbour in stored order, one chain per column from +0.0f, as everywhere),
 * k_stage_any over the other rows, and k_stage_any over the listed rows with their sums read back.  Results are bit-identical
 * for every value.  A graph without such rows launches what it always did.
 *   from_degree 0      no row takes the heavy path: every row walks k_stage_any's loop, as before this call existed;
 *   from_degree >= 1   any value is legal; with 1 every non-empty row is heavy.  The default is 512, the long-row threshold of the
 *                      trained path.
 * The value takes effect at the next forward or stage call; an attached graph is classed again then.  On a model without a
 * generic stage list the value is stored and does nothing.  Listed rows of 16 384 entries and more leave k_any_heavy_sums'
 * one chain per column for the exact parallel scan (gnnvc_set_generic_giant_rows below).  A multi-device handle:
 * GNNVC_ERR_UNSUPPORTED; a null engine: GNNVC_ERR_INVALID.
 * gnnvc_get_info: "generic_heavy_from" (the threshold in force), "generic_heavy_rows" and "generic_heavy_entries" (the listed
 * rows of the attached graph or slice and their entries, from its last classing; 0 before one), "generic_heavy_last_rows" (the
 * listed rows the last forward or stage call sent down the heavy path — rows outside a stage call's range are skipped on the
 * device and still counted; 0 when it launched one kernel per stage). */
int gnnvc_set_generic_heavy_rows(gnnvc_engine *e, uint32_t from_degree);

/* Giant rows of generic stages.  k_any_heavy_sums adds a listed row with one fp32 chain per column, about 4 ns a neighbour: a hub
 * of several hundred thousand entries holds every stage for milliseconds.  Listed rows of at least from_degree entries therefore
 * take the route the trained model's giant rows take, for any stage input width f (1 .. 32; up to 64 under
 * gnnvc_set_generic_feature_width, a row's columns then in two launches): k_any_giant_gather (a 256-thread
 * workgroup per 256 entries) writes the row's neighbour values column-major into a slab of the engine's own, one stream of
 * floats per column in stored order; k_giant_sum — behind k_giant_segsum and k_giant_segmap when a stream is spread over several
 * waves — evaluates each stream's sequential fp32 sum with the exact parallel scan (bit for bit the chain's result, for any
 * data); k_any_giant_place puts the sums where the listed rows' k_stage_any launch reads them.  Results are bit-identical for
 * every pair of values.
 *   from_degree   0: no giant rows, every listed row is summed by k_any_heavy_sums.  The default is 16 384, the trained path's
 *                 "giant_row_threshold".  Giant rows are a subset of the heavy rows: a row is giant iff the heavy threshold is not
 *                 0 and its degree is at least max(from_degree, the heavy threshold); with heavy rows off there are none.
 *   segments      1: one stream on several waves (segments of 4096 addends, k_giant_segsum / k_giant_segmap); 0: one wave walks
 *                 each stream; -1 (default): by the graph, as the trained path's "giant_segments" — several waves where the longest
 *                 stream's walk is what a stage would wait for.  Any other value is stored: positive as 1, negative as -1.
 * Both values take effect at the next forward or stage call; an attached graph is classed again then (one more pass over the
 * heavy list, one read-back, the slab: the widest stage input x the rows' entries rounded up to 1024, in floats).  A slab that
 * does not fit in device memory leaves the graph without giant rows; that is not an error.  On a model without a generic stage
 * list the values are stored and do nothing.  A multi-device handle: GNNVC_ERR_UNSUPPORTED; a null engine: GNNVC_ERR_INVALID.
 * gnnvc_get_info: "generic_giant_from" and "generic_giant_segments" (as stored), "generic_giant_rows" and
 * "generic_giant_entries" (the giant rows of the attached graph or slice and their entries, from its last classing),
 * "generic_giant_last_rows" (the giant rows of the last forward or stage call; rows outside a stage call's range are skipped on
 * the device and still counted), "generic_giant_last_segmented" (1: that call ran k_giant_segsum and k_giant_segmap).
 * "generic_heavy_rows", "generic_heavy_entries" and "generic_heavy_last_rows" count every listed row, the giant ones included. */
int gnnvc_set_generic_giant_rows(gnnvc_engine *e, uint32_t from_degree, int segments);

/* Big stages of generic models (opt-in).  By default a generic stage is fused only within 64 KiB of LDS and hidden widths of at
 * most 64, and one stage outside these bounds sends the whole model back to one launch per layer.  gfx950 has 160 KiB of LDS per
 * CU and one workgroup may take all of it; this call lets k_stage_any use it.
 *   lds_bytes 0                    off (the default): the engine behaves exactly as if this call did not exist;
 *   lds_bytes 65 536 .. 163 840    on, with that LDS limit in bytes.  A generic stage is then admitted if 1 <= f <= 32, it has 1 .. 6
 *                                  dense layers, every hidden width is <= 128, its last width is <= 32, and its LDS layout AT 256
 *                                  THREADS (transposed weights, biases, sixteen pairs of row vectors) is <= lds_bytes;
 *   anything else                  GNNVC_ERR_INVALID.
 * A stage within the default bounds launches exactly the kernels it always did, at 256 threads.  Every other admitted stage
 * launches a "big" instantiation of the same kernel source — a hidden layer of more than 64 outputs is taken 64 outputs at a
 * time, with the same bits — at 1024, 512 or 256 threads a workgroup (64 / 32 / 16 rows a pass): the largest size whose own
 * layout fits lds_bytes.  Heavy and giant rows, gnnvc_stage_forward_device and the explicit audit calls (k_audit_any) serve a big
 * stage as they serve any generic stage.  Results are bit-identical to the layer-by-layer forward for every value.
 * The call takes effect at once, as option "generic_stages" does: the generic stage list is derived anew, and with it
 * gnnvc_is_fused, gnnvc_num_stages, gnnvc_stage_widths and "generic_stage_layers_<s>"; an attached graph's heavy and giant rows
 * are classed again by the next generic stage that runs.  A model that is still not admitted (a wider layer, a larger layout,
 * f or a last width above 32 — see gnnvc_set_generic_feature_width below) keeps running layer by layer.  The kernels' raised LDS limit is set here, once per device: if the
 * runtime refuses it the call returns GNNVC_ERR_UNSUPPORTED and the engine stays as it was — never a forward.  A multi-device
 * handle: GNNVC_ERR_UNSUPPORTED; a null engine: GNNVC_ERR_INVALID.
 * gnnvc_get_info: "generic_big_lds" (the value as set, 0 when off), "generic_stage_lds_bytes_<s>" (the LDS layout of stage s at 256
 * threads, in bytes) and "generic_stage_threads_<s>" (the workgroup size its launches use: 256, 512 or 1024 — 256 for every stage
 * within the default bounds); both per-stage keys follow "generic_stage_layers_<s>": GNNVC_ERR_INVALID for a stage that does
 * not exist or while the model is not generic. */
int gnnvc_set_generic_big_stages(gnnvc_engine *e, uint32_t lds_bytes);

/* Feature rows of generic models up to 64 wide (opt-in).  By default a generic stage is fused only if its feature width f — the
 * model's input width, and for later stages the previous stage's last layer — and its own last layer are at most 32: a model that
 * hands 48- or 64-wide rows from one graph layer to the next runs one launch per layer.  This call raises both bounds.
 *   max_width 0           off (the default): the bounds are 32 and the engine behaves exactly as if this call did not exist;
 *   max_width 33 .. 64    on: a generic stage is admitted if 1 <= f <= max_width and its last width is <= max_width — the model's
 *                         input width (stage 0's f) and its output width included — and it fits every other bound as before;
 *   anything else         GNNVC_ERR_INVALID, the engine unchanged.
 * The call is independent of gnnvc_set_generic_big_stages: an admitted stage must still fit the LDS and hidden-width bounds, the
 * default ones (64 KiB, hidden widths <= 64) or those that call allows; a stage with f = 64 and a 128-wide hidden layer needs both.
 * A stage whose f and last width are at most 32 launches exactly the kernels it always did.  A stage that uses the allowance
 * launches a "feat" instantiation of the same kernel source, in which a lane owns up to four neighbour-sum columns and up to four
 * outputs of the last layer: at 256 threads when the stage is within the default LDS and hidden-width bounds, else at the big
 * rule's 1024, 512 or 256.  Heavy rows (k_any_heavy_sums: groups of 64 lanes), giant rows (k_any_giant_gather: a row's columns in
 * two launches of at most 32), gnnvc_stage_forward_device and the explicit audit calls (k_audit_any) serve such a stage as they
 * serve any generic stage.  Results are bit-identical to the layer-by-layer forward for every value.
 * The call takes effect at once: the generic stage list is derived anew, and with it gnnvc_is_fused, gnnvc_num_stages,
 * gnnvc_stage_widths and "generic_stage_layers_<s>"; an attached graph's heavy and giant rows are classed again by the next generic
 * stage that runs (their buffers are sized by the widest f).  The kernels' raised LDS limit is set here, once per device: if the
 * runtime refuses it the call returns GNNVC_ERR_UNSUPPORTED and the engine stays as it was.  A multi-device handle:
 * GNNVC_ERR_UNSUPPORTED; a null engine: GNNVC_ERR_INVALID.
 * gnnvc_get_info: "generic_feature_width" (the value in force, 0 when off). */
int gnnvc_set_generic_feature_width(gnnvc_engine *e, uint32_t max_width);

/* Layer sequences of generic models beyond (Graph_Layer, (Linear_Layer, activation){1..6})+ with a last sigmoid (opt-in).  By default
 * a model with an input embedding in front of its first graph layer, a model cut after a stage (it ends in a ReLU) or a model that
 * ends in a bare Linear_Layer runs one launch per layer.  mask is a set of bits:
 *   GNNVC_PATTERN_PROLOGUE (1)   a DENSE stage — (Linear_Layer, activation){1..6} before the first Graph_Layer — is admitted as
 *                                stage 0 of the stage list (the graph stages then number from 1); a model of that stage alone, with
 *                                no graph layer, too.  Its bounds are a graph stage's with the first K equal to f where a graph
 *                                stage has 2 f + 3: f and its last width at most 32 (64 under gnnvc_set_generic_feature_width), hidden
 *                                widths at most 64 (128 under gnnvc_set_generic_big_stages), its LDS layout within the limit in force;
 *   GNNVC_PATTERN_OPEN_END (2)   the model's last activation may be a ReLU, or be missing, so that the model's last layer is the
 *                                Linear_Layer, whose outputs are stored as they are;
 *   0                            off (the default): the engine behaves exactly as if this call did not exist;
 *   any other bit                GNNVC_ERR_INVALID, the engine unchanged.
 * With the mask the admitted pattern is [P] S*, at least one stage in all: S today's graph stage, P the dense stage; every activation a
 * ReLU except the model's last.  A sigmoid inside the model, two Graph_Layers in a row, two Linear_Layers without an activation
 * between them, a block of seven dense layers keep the model layer by layer under every mask, silently and with the same bits; a model
 * of the trained shape keeps its own plans.  The call is independent of gnnvc_set_generic_big_stages and of
 * gnnvc_set_generic_feature_width: a 48-wide prologue needs the latter too, a 128-wide hidden layer in a prologue the former.
 * A dense stage is one k_stage_any launch over the call's rows (the kAnyDense instantiations: the row is the stage's own input row;
 * no array of the graph is read, no row is classed heavy or giant) — a graph must still be attached, it gives the number of rows.
 * d_logits is written by a stage that ends in the sigmoid and by no other.  gnnvc_forward, gnnvc_forward_device,
 * gnnvc_stage_forward_device and the explicit audit calls (k_audit_any, "audit_repair" included) serve these stages as they serve any
 * generic stage; "audit_period" goes on auditing nothing on generic models.  Results are bit-identical to the layer-by-layer forward
 * for every mask.
 * The call takes effect at once: the generic stage list is derived anew, and with it gnnvc_is_fused, gnnvc_num_stages,
 * gnnvc_stage_widths and "generic_stage_layers_<s>"; an attached graph's heavy and giant rows are classed again by the next generic
 * graph stage that runs.  A multi-device handle: GNNVC_ERR_UNSUPPORTED; a null engine: GNNVC_ERR_INVALID.
 * gnnvc_get_info: "generic_patterns" (the mask in force), "generic_stage_dense_<s>" (1 = stage s is a dense stage, else 0) and
 * "generic_stage_end_<s>" (0 = stage s ends in a ReLU, 1 = in the sigmoid, 2 = in its bare linear layer); both per-stage keys follow
 * "generic_stage_layers_<s>": GNNVC_ERR_INVALID for a stage that does not exist or while the model is not generic. */
#define GNNVC_PATTERN_PROLOGUE 1u
#define GNNVC_PATTERN_OPEN_END 2u
int gnnvc_set_generic_patterns(gnnvc_engine *e, uint32_t mask);

/* Live columns of generic stages (option "generic_stages", kernel k_stage_any), opt-in.  After a ReLU many columns of a stage's
 * input are +-0.0 in every row, and k_stage_any's gather loads them all the same, f floats per adjacency entry.  With this call
 * a graph stage gathers from a compact table of the LIVE columns instead:
 *   max_percent 0         off (the default): the engine launches exactly what it launches without this call;
 *   max_percent 1 .. 100  on.  Inside a whole forward every graph stage with f >= 2 has its input examined on the device
 *                         (k_any_live_mask: column c is dead iff (bits & 0x7fffffff) == 0 in all n rows — a denormal, or a value in a
 *                         row no edge refers to, makes it live), and gathers from the table (k_any_live_pack: n rows of `kept`
 *                         floats, kept = the number of live columns) iff kept * 100 <= max_percent * f.  The decision is the
 *                         device's, per forward and stage: nothing is copied back and nothing is waited for.  100 uses the
 *                         table for every such stage, also at kept == f; kept == 0 uses it under every value and gathers nothing;
 *   anything else         GNNVC_ERR_INVALID, the engine unchanged.
 * Results are bit-identical under every value: a neighbour sum is one fp32 add chain from +0.0f, a chain value is never -0.0f, and
 * adding +-0.0 to it returns the same bits — so a dead column's sum is +0.0f for every row and the live columns' chains are the ones
 * they were ("Live columns").  A row's own features, degree, W and NW are read as before.
 * It applies to gnnvc_forward, gnnvc_forward_device, gnnvc_forward_audited and gnnvc_forward_audited_device on a single engine whose
 * model runs as generic stages (the trained model under "generic_stages" 2 included); k_audit_any recomputes from the full rows, so an
 * audited forward checks the table's route independently.  It does NOT apply — same launches and bits as without it — to dense
 * stages, stages with f == 1, a last stage that ends in its bare linear layer, gnnvc_stage_forward_device and
 * gnnvc_audit_stage_device (d_in is the caller's, per range), sliced engines, and gnnvc_create_multi_generic.  Heavy and giant rows
 * (gnnvc_set_generic_heavy_rows, gnnvc_set_generic_giant_rows) keep reading full rows; the all-rows and light-rows launches read the
 * table.  The table is a buffer of the engine's own, n x the widest such f floats.
 * The call takes effect at the next forward.  It does not derive the stage list anew, so nothing is admitted or refused by it, and it
 * is independent of gnnvc_set_generic_big_stages, gnnvc_set_generic_feature_width and gnnvc_set_generic_patterns.  On a model without a
 * generic stage list the value is stored and does nothing.  A multi-device handle: GNNVC_ERR_UNSUPPORTED; a null engine:
 * GNNVC_ERR_INVALID.
 * gnnvc_get_info: "generic_live_columns" (the value in force) and, per stage and from the LAST forward, "generic_live_kept_<s>" (live
 * columns of its input), "generic_live_used_<s>" (1 = its launches gathered from the table), "generic_live_mask_lo_<s>" and
 * "generic_live_mask_hi_<s>" (the 64-bit column mask in two halves).  A stage the last forward did not examine — the call is off, the
 * stage is not one of those above, no forward yet, n == 0 — reads kept -1, used 0, mask 0.  The values live on the device: asking for
 * one of these keys costs one copy and one wait on the engine's stream.  The per-stage keys follow "generic_stage_layers_<s>":
 * GNNVC_ERR_INVALID for a stage that does not exist or while the model is not generic. */
int gnnvc_set_generic_live_columns(gnnvc_engine *e, uint32_t max_percent);

/* Model introspection (what model::layers holds). */
int gnnvc_num_layers(const gnnvc_engine *e);
/* 1 if the model runs as fused stages — the trained 3-stage shape, or (option "generic_stages", default on) any model of the
 * generic stage pattern within the generic kernel's width, depth and LDS bounds — 0 if it runs layer by layer. */
int gnnvc_is_fused(const gnnvc_engine *e);
/* Width of the forward's input / output rows. */
int gnnvc_in_width(const gnnvc_engine *e);
int gnnvc_out_width(const gnnvc_engine *e);

/* ---- graph hand-off ---------------------------------------------------------
 * What the forward reads from reduction_graph<uint32_t,uint32_t> (reference
 * include/reduction_graph.hpp: size() :141, begin(u)/end(u) :693-704, D :144,
 * W :147-151, NW :154-158): vertices 0..n-1, adj(u) = col[rowptr[u]..rowptr[u+1])
 * in the graph's stored order (that order is the fp32 summation order), the
 * vertex weights and the neighbourhood weights.  Host pointers; copied to the
 * device.  nnz = rowptr[n] must be < 2^32. */
int gnnvc_upload_graph(gnnvc_engine *e, uint32_t n, const uint64_t *rowptr,
                       const uint32_t *col, const uint32_t *w, const uint32_t *nw);

/* Zero-copy variant for callers whose CSR already lives in device memory
 * (multi-GPU shards, device-side generators): d_rowptr is uint32[n+1], d_col is
 * uint32[nnz + GNNVC_COL_PAD] (the pad entries may hold anything), d_w / d_nw are
 * uint32[n].  The caller keeps them alive until the next attach/upload/destroy. */
#define GNNVC_COL_PAD 64
int gnnvc_attach_graph_device(gnnvc_engine *e, uint32_t n, uint64_t nnz,
                              const uint32_t *d_rowptr, const uint32_t *d_col,
                              const uint32_t *d_w, const uint32_t *d_nw);

/* One rank's SLICE of a vertex-partitioned graph ("each GPU holds its rows' CSR slice with global
 * column ids, its slice of W / NW").  The engine then holds rows [row_lo, row_hi) of a graph of n_global vertices:
 *   d_rowptr_local  uint32[row_hi - row_lo + 1], relative to the slice (first = 0, last = nnz_local)
 *   d_col_local     uint32[nnz_local + GNNVC_COL_PAD], GLOBAL column ids, stored order
 *   d_w_local, d_nw_local  uint32[row_hi - row_lo]
 * — 1 / P of the graph's memory at P ranks; the feature matrices stay full-size and replicated (the caller's).  A
 * sliced engine is driven stage by stage with gnnvc_stage_forward_device on sub-ranges of its slice; the whole-graph
 * entry points (gnnvc_forward*, gnnvc_reduction_flags, gnnvc_graph_layer_forward) return GNNVC_ERR_STATE, and the
 * per-graph plans that index whole graphs stay off.  Results are those of the whole graph: a row is summed on one
 * GPU in stored order.  No reference counterpart (the reference is one process reading one graph,
 * src/gnn_inference.cpp:32-41).  The caller keeps the arrays alive until the next attach / upload / destroy. */
int gnnvc_attach_graph_slice(gnnvc_engine *e, uint32_t n_global, uint32_t row_lo, uint32_t row_hi, uint64_t nnz_local,
                             const uint32_t *d_rowptr_local, const uint32_t *d_col_local, const uint32_t *d_w_local,
                             const uint32_t *d_nw_local);

/* Staged hand-off (the caller is the pack loop over reduction_graph's
 * begin(u)/end(u) ranges, include/reduction_graph.hpp:693-704): instead of building a temporary
 * CSR and passing it to gnnvc_upload_graph, the caller writes the arrays straight into page-locked
 * memory owned by the engine.  Protocol:
 *   1. gnnvc_graph_staging(e, n, 0, &rowptr, NULL, &w, &nw): fill w[n], nw[n] and rowptr[n+1]
 *      (32-bit, rowptr[0] = 0, rowptr[n] = nnz);
 *   2. gnnvc_graph_staging(e, n, nnz, NULL, &col, NULL, NULL): the vertex arrays keep their contents;
 *      fill col[nnz] in any order;
 *   3. optionally, whenever a prefix-contiguous piece [first, first+count) of col is final,
 *      gnnvc_staged_columns_ready(e, first, count) starts its copy while the caller packs on
 *      (pieces must be announced in ascending order without gaps);
 *   4. gnnvc_commit_staged_graph(e) copies the rest, runs the same device-side checks as
 *      gnnvc_upload_graph and makes the graph current.
 * The pointers stay valid until the next gnnvc_graph_staging call with larger sizes.
 * An error from gnnvc_staged_columns_ready (e.g. GNNVC_ERR_INVALID for row pointers that are not monotone from 0 to nnz,
 * which a large hand-off checks before it starts building from them) ends the hand-off: no graph is current, begin again
 * at step 1. */
int gnnvc_graph_staging(gnnvc_engine *e, uint32_t n, uint64_t nnz, uint32_t **rowptr, uint32_t **col,
                        uint32_t **w, uint32_t **nw);
int gnnvc_staged_columns_ready(gnnvc_engine *e, uint64_t first, uint64_t count);
int gnnvc_commit_staged_graph(gnnvc_engine *e);

/* The NEXT graph derived from the one the device already holds.  Between two predict calls of the
 * reference's driver (src/GNN_VC.cpp:171-192) the graph shrinks — vertices leave, lists lose entries, survivors are
 * renumbered in order (include/reduction_graph.hpp:537-587) — and the only additions are the vertices its folds
 * create, which carry the largest ids and therefore sit at the END of their neighbours' lists (:335-398).  So a row of
 * the next graph is: the surviving entries of its old row, in order, renumbered — plus a short tail; a new vertex's
 * row is all tail.  Protocol (the resident graph must have come through gnnvc_upload_graph / the staged calls / a
 * previous derive, i.e. live in engine-owned memory):
 *   1. gnnvc_derive_graph_begin(e, n_new, old_row, rowptr_new, tail): old_row[u] = the row of the RESIDENT graph that
 *      vertex u of the next graph was, or GNNVC_NEW_VERTEX; rowptr_new = the next graph's 32-bit row pointers (n_new + 1).
 *      The device counts every row's surviving old entries and returns tail[u] = degree(u) - survivors: how many
 *      trailing entries of u's list it cannot derive.  An inconsistent mapping (a row with more survivors than its new
 *      degree, an old row claimed twice, ...) is GNNVC_ERR_INVALID and leaves the resident graph as it was;
 *   2. gnnvc_derive_graph_commit(e, tail_cols, n_tail, w, nw): the last tail[u] entries of every row, row after row
 *      (n_tail = their total), and the next graph's W / NW.  The engine assembles the CSR on the device, runs the same
 *      checks as an upload and makes it current.
 * What crosses the bus: 8 bytes per vertex + the tails, instead of 4 bytes per adjacency entry.  What the engine
 * cannot check is that the caller's lists really ARE "survivors + tail" (it never sees them): gnnvc_graph_row_hashes
 * returns a 64-bit FNV-1a hash of every resident row (column ids in stored order) for callers that want to compare. */
#define GNNVC_NEW_VERTEX 0xFFFFFFFFu
int gnnvc_derive_graph_begin(gnnvc_engine *e, uint32_t n_new, const uint32_t *old_row, const uint32_t *rowptr_new, uint32_t *tail);
int gnnvc_derive_graph_commit(gnnvc_engine *e, const uint32_t *tail_cols, uint64_t n_tail, const uint32_t *w, const uint32_t *nw);
int gnnvc_graph_row_hashes(gnnvc_engine *e, uint64_t *hashes);

/* ---- forward ----------------------------------------------------------------
 * gnnvc_forward replaces model::predict (reference src/gnn_inference.cpp:67-81)
 * for host callers: x is n x in_width (n x 1 for the shipped model:
 * x[u] = (float)W(u)/ws, reference src/GNN_VC.cpp:189-191), scores is
 * n x out_width.  `logits` (optional, may be NULL) receives the input of the
 * final sigmoid when the model ends in one. */
int gnnvc_forward(gnnvc_engine *e, const float *x, float *scores, float *logits);

/* Device-resident forward: all pointers are device memory; asynchronous on
 * the engine's stream (an audited call synchronises it: option "audit_period").  d_logits may be NULL. */
int gnnvc_forward_device(gnnvc_engine *e, const float *d_x, float *d_scores, float *d_logits);

/* The same two forwards with EVERY fused stage audited in this one call, whatever "audit_period" says (the period's call counter
 * is not ticked): each stage is recomputed right behind its launch, before the next stage is queued, and compared bit for bit
 * with every value the fused path wrote, as described under "audit_period".  A model of the trained shapes is audited by the
 * kernel the period uses (k_audit_stage); a generic-stage model (option "generic_stages"), which the period does not audit, by
 * k_audit_any.  The call synchronises its stream once, at its end.  GNNVC_OK: the audit was clean.  GNNVC_ERR_AUDIT: values
 * differ — the outputs are as the fused path wrote them, all stages have run, gnnvc_last_error carries the report and the engine
 * stays usable; with "audit_repair" 1 the values are repaired and the call returns GNNVC_OK.  The "audit_*" counters and
 * read-outs are updated as by any audited call, and "audit_quiet", "audit_log" and the "audit_flip_*" hooks apply.  A model that
 * runs layer by layer (gnnvc_is_fused = 0) has no stage to audit: GNNVC_ERR_UNSUPPORTED.  A graph of no vertices: GNNVC_OK,
 * nothing done.  A multi-device handle audits this forward on all its parts. */
int gnnvc_forward_audited(gnnvc_engine *e, const float *x, float *scores, float *logits);
int gnnvc_forward_audited_device(gnnvc_engine *e, const float *d_x, float *d_scores, float *d_logits);

/* One fused stage (graph layer + the dense layers up to the next graph
 * layer) over the vertex range [row_lo, row_hi) — the unit a 1-D
 * vertex-partitioned multi-GPU run executes between feature exchanges.
 * d_in is the full (n + 1) x in_width feature matrix whose LAST row is all
 * zeros (the gather reads it for masked lanes); d_out is the full
 * (n + 1) x out_width matrix of which only rows [row_lo, row_hi) are written.
 * d_logits (stage with a final sigmoid only, may be NULL) likewise.
 * Asynchronous on the engine's stream (an audited call synchronises it: option "audit_period"). */
int gnnvc_num_stages(const gnnvc_engine *e);
int gnnvc_stage_widths(const gnnvc_engine *e, int stage, int *in_width, int *out_width);
int gnnvc_stage_forward_device(gnnvc_engine *e, int stage, uint32_t row_lo, uint32_t row_hi,
                               const float *d_in, float *d_out, float *d_logits);

/* A pure check that runs no stage: are rows [row_lo, row_hi) of d_out what stage `stage` computes from d_in — and, on the stage
 * that ends in the sigmoid, those rows of d_logits too, when it is not NULL?  The buffers are laid out as for
 * gnnvc_stage_forward_device, and the same argument checks and slice rules hold (a sliced engine checks rows of its slice; an
 * empty range is GNNVC_OK).  Any fused model: the trained shapes (k_audit_stage) and generic stages (k_audit_any).  One
 * read-back; the call SYNCHRONISES the engine's stream.  Return codes, counters and read-outs as for gnnvc_forward_audited;
 * with "audit_repair" 1 the audit's values are written over the mismatching ones (hence d_out and d_logits are not const).  The
 * "audit_flip_*" hooks do not apply — the caller owns the buffers — and the period's call counter is not ticked.  A multi-device
 * handle: GNNVC_ERR_UNSUPPORTED. */
int gnnvc_audit_stage_device(gnnvc_engine *e, int stage, uint32_t row_lo, uint32_t row_hi,
                             const float *d_in, float *d_out, float *d_logits);

/* ---- feature-row codec for the exchange between vertex-partitioned GPUs --------
 * No reference counterpart (the reference is single-process).  After the ReLU that ends a fused
 * stage most entries of the N x 16 feature matrix are zero: on the metric graph two columns are
 * non-zero in every row, two in about a tenth of the rows, five in a handful of rows and seven in
 * none (which columns, and how dense, depends on the graph).  A piece of rows [row_lo, row_hi)
 * travels as
 *   d_dense  (row_hi - row_lo) x kp floats: the columns of `mask` in ascending order, zero padded
 *            (kp = 4, 8 or 12), and
 *   d_exc    an exception list for non-zeros in any other column: word 0 = count, then entries of
 *            four words {row - row_lo, column, value bits, 0} from word 4 on, room for exc_cap
 *            entries (4 + 4 * exc_cap words); may be NULL.
 * gnnvc_unpack_rows rebuilds the 16-float rows, writing +0.0f where nothing was shipped — exactly
 * the rows a full exchange would have delivered.  gnnvc_pack_rows ORs into *d_flag: bit 0 if a
 * non-zero fell outside `mask` and there was no list, bit 1 if the list overflowed; the caller then
 * falls back to full rows.  gnnvc_column_counts gives the per-column non-zero counts from which
 * the caller chooses mask, kp and exc_cap (synchronous); the other calls are asynchronous on the
 * engine's stream.  All pointers are device memory. */
int gnnvc_live_columns(gnnvc_engine *e, const float *d_feat, uint32_t rows, uint32_t width, uint32_t *mask);
int gnnvc_column_counts(gnnvc_engine *e, const float *d_feat, uint32_t rows, uint32_t width, uint64_t *counts /*[16]*/);
int gnnvc_pack_rows(gnnvc_engine *e, const float *d_feat, uint32_t width, uint32_t row_lo, uint32_t row_hi,
                    uint32_t mask, uint32_t kp, float *d_dense, uint32_t *d_exc, uint32_t exc_cap, uint32_t *d_flag);
int gnnvc_unpack_rows(gnnvc_engine *e, const float *d_dense, const uint32_t *d_exc, uint32_t exc_cap, uint32_t width,
                      uint32_t row_lo, uint32_t row_hi, uint32_t mask, uint32_t kp, float *d_feat);

/* One all-gathered piece, every peer's region in one launch: d_buf holds `world` regions of
 * piece_words words (dense part of dense_rows rows, then the exception list), region r carrying rows
 * [r * rows_per_rank + row_off, + rows) of rank r (cut at the end of its shard and at n);
 * skip_rank's region (the caller's own rows, already in place) is left alone. */
int gnnvc_unpack_gathered(gnnvc_engine *e, const float *d_buf, uint32_t world, uint32_t skip_rank, uint64_t piece_words,
                          uint32_t dense_rows, uint32_t exc_cap, uint32_t width, uint32_t rows_per_rank, uint32_t row_off,
                          uint32_t rows, uint32_t n, uint32_t mask, uint32_t kp, float *d_feat);

/* One packed piece to several destinations, and several packed pieces expanded, in ONE launch each (round 4; what
 * gnnvc_create_multi's devices exchange).  A piece REGION = rows x kp dense floats (gnnvc_pack_rows' d_dense) directly followed
 * by its exception list (4 + 4 * exc_cap words).
 *   gnnvc_push_piece     stores the dense part and the USED part of the list into each of d_dst[0 .. n_dst) (n_dst <= 64): device
 *                        pointers this engine's device can store to — its own memory, or a peer's once peer access is enabled
 *                        (hipDeviceEnablePeerAccess: the stores then cross the xGMI link to that peer) — on hip_stream (NULL =
 *                        the engine's stream; the region must be complete in that stream's order);
 *   gnnvc_unpack_pieces  expands pieces[0 .. n_pieces) (n_pieces <= 64) — region i holding rows [row_lo, row_hi) — into the
 *                        16-column rows of d_feat exactly as gnnvc_unpack_rows would, on the engine's stream. */
typedef struct gnnvc_piece {
    const float *d_region;
    uint32_t row_lo, row_hi;
} gnnvc_piece;
int gnnvc_push_piece(gnnvc_engine *e, const float *d_region, uint32_t rows, uint32_t kp, uint32_t exc_cap, uint32_t n_dst,
                     float *const *d_dst, void *hip_stream);
int gnnvc_unpack_pieces(gnnvc_engine *e, const gnnvc_piece *pieces, uint32_t n_pieces, uint32_t exc_cap, uint32_t width, uint32_t mask,
                        uint32_t kp, float *d_feat);

/* Full rows to several destinations in ONE launch (what gnnvc_create_multi_generic's devices exchange: rows of any width, no
 * codec).  Rows [r0, r1) of a row-major n x f matrix are one run of (r1 - r0) * f floats at word offset r0 * f, so the run starts
 * and ends at any 4-byte boundary.
 *   gnnvc_push_rows      stores the `words` floats at d_src into each of d_dst[0 .. n_dst) (n_dst <= 64): device pointers this
 *                        engine's device can store to — its own memory, or a peer's once peer access is enabled — on hip_stream
 *                        (NULL = the engine's stream; the run must be complete in that stream's order).  Asynchronous.  Kernel
 *                        k_push_rows: up to three head words as scalars until the source is 16-byte aligned, the body 16 bytes
 *                        per lane, up to three tail words as scalars — where every destination has the source's 16-byte phase
 *                        (pointer mod 16), as the same rows of equally wide, equally aligned matrices have; one destination of
 *                        another phase sends the launch through a 4-bytes-per-lane instantiation, never a misaligned 16-byte
 *                        store.  words = 0 or n_dst = 0: GNNVC_OK, nothing launched.  n_dst > 64, a null destination, a null
 *                        source or a pointer that is not 4-byte aligned: GNNVC_ERR_INVALID, nothing launched. */
int gnnvc_push_rows(gnnvc_engine *e, const float *d_src, uint64_t words, uint32_t n_dst, float *const *d_dst, void *hip_stream);

/* A multi-GPU rank that computes rows [row_lo, row_hi) of `stage` (1 or 2) in several gnnvc_stage_forward_device
 * calls announces the stage's complete input once: "d_in is final and will not change until those calls are done".
 * The engine then builds the compact-table plan over that row range — once per graph and range —
 * and writes the table for this input, so that each of the calls (if it covers enough rows to fill the GPU) reads
 * its neighbours from the table instead of gathering 64-byte rows.  Purely an optimisation hint: results are
 * bit-identical with or without it, and it does nothing on graphs or inputs the plan does not fit.  The
 * announcement is forgotten at the next gnnvc_stage_input_ready / gnnvc_forward(_device) / graph change. */
int gnnvc_stage_input_ready(gnnvc_engine *e, int stage, const float *d_in, uint32_t row_lo, uint32_t row_hi);

/* ---- reduction-rule candidates ------------------------------------
 * One vertex-parallel pass over the uploaded graph that evaluates which local rules of the
 * reference's reduce_graph (include/mwvc_reductions.hpp:335-380) would fire on each vertex as
 * the graph stands: flags[u] bit r for rule r of its switch — 0 neighborhood_reduction,
 * 1 twin_fold, 2 domination_reduction, 3 isolated_fold, 4 independent_fold, 5 neighbor_meta_reduction,
 * 6 neighborhood_meta_reduction — exact predicates, the last two with the covers of their <= 8-vertex
 * subgraphs enumerated the way include/small_solve.hpp does.  Vertices with D(u) > max_degree get 0
 * (reduce_graph skips them, :344; pass 20).
 * Needs ascending neighbour lists.  The host keeps applying reductions in the reference's own
 * stack order and merely skips clean vertices whose bit is 0. */
int gnnvc_reduction_flags(gnnvc_engine *e, uint32_t max_degree, uint8_t *flags);

/* ---- score consumer keys ------------------------------------------------
 * What the driver's sort and selection loop read from the scores (reference src/GNN_VC.cpp:194-206,
 * 213, 220): keys[u] = std::min(s, 1.0f - s), above_half[u] = s > 0.5f, computed on the device from
 * d_scores (n floats; NULL = the scores the last gnnvc_forward left there) and copied to the host.
 * The comparator itself (its 1e-4 tie band is not a strict weak order) must stay the host's
 * std::sort for the order to stay the reference's. */
int gnnvc_score_keys(gnnvc_engine *e, const float *d_scores, uint32_t n, float *keys, uint8_t *above_half);

/* Wait for everything queued on the engine's stream. */
int gnnvc_synchronize(gnnvc_engine *e);

/* hipEvent timings of the last gnnvc_forward / gnnvc_forward_device on the
 * engine's stream: total and per stage, in milliseconds (waits for them).  A forward records
 * events only when option "forward_timing" asks for them: 0 (the default) -> GNNVC_ERR_STATE,
 * 1 -> the total (stage_ms[] = -1), 2 -> total and stages. */
int gnnvc_last_forward_ms(gnnvc_engine *e, float *total_ms, float *stage_ms, int max_stages);

/* Per-kernel HIP-event timings of the gnnvc_forward_device calls made since the last call of this function, when
 * option "kernel_trace" is 1 (bench.py's roofline block): every kernel those forwards launched on the engine's
 * stream, in launch order — names[i] (static strings: the kernel as written at its launch site) and ms[i];
 * *count = how many there were (may exceed max; at most 16384 are kept).  Reading clears the records.
 * Kernels on the engine's side streams (long / giant rows, overlapped dense rounds) are not listed.  Waits. */
int gnnvc_kernel_trace(gnnvc_engine *e, int max, const char **names, float *ms, int *count);

/* ---- layer-level entry points (host pointers) ------------------------------
 * One call per reference layer forward(); used by the C++ mirror of the
 * reference's layer structs and by the per-layer parity tests. */

/* graph_layer::forward (reference src/gnn_inference.cpp:27-42) on the graph
 * currently uploaded: in is n x f, out is n x (2f+3), ws as set. */
int gnnvc_graph_layer_forward(gnnvc_engine *e, uint32_t f, const float *in, float *out);

/* linear_layer::forward (reference src/gnn_inference.cpp:20-25): out = in*W + bias,
 * in n x k, W k x m row-major, bias m. */
int gnnvc_linear_forward(gnnvc_engine *e, uint32_t n, uint32_t k, uint32_t m,
                         const float *in, const float *W, const float *bias, float *out);

/* ReLU::forward / sigmoid::forward (reference src/gnn_inference.cpp:44-52). */
int gnnvc_relu_forward(gnnvc_engine *e, size_t count, const float *in, float *out);
int gnnvc_sigmoid_forward(gnnvc_engine *e, size_t count, const float *in, float *out);

/* The neighbour sum of graph_layer::forward (reference src/gnn_inference.cpp:33-36) on explicit data:
 * sums[i] = (((0 + v[i][0]) + v[i][1]) + ...) + v[i][len-1], one rounded fp32 add per element, for `streams`
 * rows of `len` floats (host pointers, row-major).  Both modes evaluate that chain with the engine's parallel
 * giant-row kernels and return its exact bits whatever the data holds — the layer-level handle on the path rows of degree
 * >= "giant_row_threshold" take.  mode 0 runs a stream on several waves (segments of 4096 addends, each with its own parity
 * map relative to an estimated binade, used by the final walk only where the exact accumulator confirms it); mode 2 is the
 * same result with one wave walking the whole stream ("giant_segments" 0 for the engine's own rows).  (Rounds 1 - 3 had a
 * tolerance mode 1 — tree sums; it is gone: GNNVC_ERR_INVALID.) */
int gnnvc_stream_sum(gnnvc_engine *e, const float *values, uint32_t streams, uint32_t len, int mode, float *sums);

/* dot() (reference src/matrix.cpp:106-122, the cblas_sgemm seam):
 * C = op(A) * op(B) + beta * C, row-major, op = transpose when the flag is set;
 * m, n, k are the dimensions AFTER op.  Each output is one sequential-k fmaf
 * chain from +0.0f; with beta != 0 the old C is then added as fma(beta, C, acc). */
int gnnvc_sgemm(gnnvc_engine *e, int trans_a, int trans_b, uint32_t m, uint32_t n, uint32_t k,
                const float *A, uint32_t lda, const float *B, uint32_t ldb, float beta,
                float *C, uint32_t ldc);

/* ---- backward -----------------------------------------------------------------
 * Input and parameter gradients of the function the engine computes — the column layout of the graph layer included (DESIGN.md
 * §3) — for callers that retrain: the reference's weights came from a backprop-and-SGD trainer (reference
 * old_files/src/lib/gnn_training.cpp).  Every sum has one stated order, so a gradient depends on neither the device, the grid nor
 * the run ("Backward"):
 *   ReLU          grad_in = (z >= 0.0f) ? grad_out : 0.0f on the layer's input z (-0.0 passes, NaN gives 0: the trainer's rule);
 *   sigmoid       grad_in = (s * (1.0f - s)) * grad_out, rounded in that order, on the layer's OUTPUT s;
 *   linear        grad_in[i][kk]: one fmaf chain over j = 0 .. m - 1 of grad_out[i][j] * W[kk][j] from +0.0f (gnnvc_sgemm with
 *                 trans_b).  grad_W[kk][j]: rows are cut into blocks of GNNVC_GRAD_BLOCK_ROWS; a block's partial is one fmaf chain
 *                 over its rows in ascending order of in[i][kk] * grad_out[i][j] from +0.0f; the partials are added in ascending
 *                 block order, one rounded add each, from +0.0f; with `accumulate` that total is then added to the old value in
 *                 one rounded add.  grad_bias[j]: the same with in = 1.  Up to GNNVC_GRAD_BLOCK_ROWS rows this is gnnvc_sgemm with
 *                 trans_a and beta = accumulate ? 1 : 0 bit for bit (but where a chain underflows to -0.0f, which the add to
 *                 +0.0f turns into +0.0f);
 *   graph layer   (in n x f, out n x (2f+3)) grad_in[v][j] = (sum over u in adj(v) of grad_out[u][j], stored order, one rounded
 *                 add each from +0.0f) + own, own = grad_out[v][f + j] — but +0.0f where column f + j is one of f+1 .. f+3, which
 *                 the forward overwrites with the degree and the weights: h[1 .. min(3, f-1)] get no own term.  Degree, W / ws
 *                 and NW / ws are constants.  (This departs from the old trainer's graph_layer_training::backward, which hands
 *                 every own column its gradient as if the forward had not overwritten three of them: the gradient here is that
 *                 of the forward that runs.)  The neighbour term is the transposed sum written over adj(v): right only for a
 *                 SYMMETRIC adjacency (every graph of the reference is).  The engine checks that exactly, with multiplicities,
 *                 once per resident graph, on the device (gnnvc_get_info "graph_symmetric": -1 before the check, then 0 or 1;
 *                 the first call that needs the answer waits for its stream; neighbour lists that ascend are searched, others are
 *                 scanned, and a graph with a list of more than 65 536 entries that does not ascend is refused like one that is
 *                 not symmetric, its answer left at -1: sort the lists); a graph that is not symmetric gets
 *                 GNNVC_ERR_UNSUPPORTED from gnnvc_backward, gnnvc_backward_device and gnnvc_graph_layer_backward.  At the model
 *                 level the check is made, and the refusal given, only when a graph layer lies in the range of layers the call
 *                 walks: a model without one, or a call without grad_x whose first linear layer lies above every graph layer,
 *                 runs on any graph and leaves the answer as it was.
 * GNNVC_GRAD_BLOCK_ROWS is part of the ABI: changing it changes bits. */
#define GNNVC_GRAD_BLOCK_ROWS 4096

/* The model's parameters in the order of the model text: per Linear_Layer, W as k x m row-major, then the bias of m floats.
 * `params` holds *count floats.  These work on any handle. */
int gnnvc_num_params(const gnnvc_engine *e, uint64_t *count);
int gnnvc_get_params(const gnnvc_engine *e, float *params);

/* The model level.  A training forward runs the model layer by layer on the resident graph and keeps, in a workspace of the
 * engine's own (gnnvc_get_info "backward_workspace_bytes"), every layer's input, the output and a copy of the parameters it ran
 * with; gnnvc_backward then gives the gradient of sum(grad_scores * scores) for that forward.
 *   params / d_params   the parameters to run with, in gnnvc_get_params' order; NULL = the model's own.  The engine's inference
 *                       parameters and plans are never touched: a trainer keeps its weights on its side and holds one engine
 *                       with a resident graph.  With NULL the scores are the bits of gnnvc_forward's;
 *   x, scores           n x in_width, n x out_width;
 *   grad_scores         n x out_width;  grad_params: gnnvc_num_params floats, written — or, with accumulate != 0, added to (may be
 *                       NULL: only grad_x is wanted);  grad_x: n x in_width, optional (NULL), never accumulated.
 * The saved forward belongs to the resident graph: every hand-off (upload, staged commit, attach, derive) discards it.
 * gnnvc_backward* without a training forward on the resident graph: GNNVC_ERR_STATE (no graph at all: too).  A sliced engine or a
 * multi-device handle: GNNVC_ERR_UNSUPPORTED.  n = 0: GNNVC_OK, the parameter gradients are +0.0f (untouched when accumulating).
 * Ordinary forwards between a training forward and its backward change neither.  The _device forms take device pointers and are
 * asynchronous on the engine's stream (but for the one wait of the symmetry check, above); several backwards may follow one
 * training forward. */
int gnnvc_train_forward(gnnvc_engine *e, const float *params, const float *x, float *scores);
int gnnvc_train_forward_device(gnnvc_engine *e, const float *d_params, const float *d_x, float *d_scores);
int gnnvc_backward(gnnvc_engine *e, const float *grad_scores, float *grad_params, float *grad_x, int accumulate);
int gnnvc_backward_device(gnnvc_engine *e, const float *d_grad_scores, float *d_grad_params, float *d_grad_x, int accumulate);

/* The layer level (host pointers, like the layer-level forwards above).  gnnvc_graph_layer_backward runs on the resident graph:
 * grad_out n x (2f+3), grad_in n x f; errors as at the model level.  gnnvc_linear_backward: in n x k, W k x m, grad_out n x m;
 * grad_in (n x k), grad_W (k x m) and grad_bias (m) may each be NULL; accumulate applies to grad_W and grad_bias; n = 0 gives +0.0f
 * (untouched when accumulating).  gnnvc_relu_backward takes the ReLU's input z, gnnvc_sigmoid_backward the sigmoid's output s. */
int gnnvc_graph_layer_backward(gnnvc_engine *e, uint32_t f, const float *grad_out, float *grad_in);
int gnnvc_linear_backward(gnnvc_engine *e, uint32_t n, uint32_t k, uint32_t m, const float *in, const float *W,
                          const float *grad_out, float *grad_in, float *grad_W, float *grad_bias, int accumulate);
int gnnvc_relu_backward(gnnvc_engine *e, size_t count, const float *z, const float *grad_out, float *grad_in);
int gnnvc_sigmoid_backward(gnnvc_engine *e, size_t count, const float *s, const float *grad_out, float *grad_in);

/* ---- loss and step --------------------------------------------------------------
 * What the reference's old trainer does between a forward and the next one (reference old_files/src/lib/gnn_training.cpp: MSE_grad,
 * MSE_loss, SGD_step; old_files/src/apps/gnn_train.cpp: run_model's counters), on the device, so that a training step can stay
 * there.  Every operation is one fp32 operation rounded on its own, in the order written: no fused multiply-add, no reciprocal in
 * place of a division ("Loss and step").  Neither call needs a resident graph.
 *
 * gnnvc_mse: scores x and target y are rows x width.
 *   grad (optional)   grad[i][j] = (2.0f * (x[i][j] - y[i][j])) / (float)width — MSE_grad: not divided by the number of rows.  grad
 *                     may be the scores or the target buffer itself (the gradient in place: every element is read before it is
 *                     written); it must not overlap either in any other way.
 *   stats (optional)  every call ADDS to *stats; zero it to start a read-out.  The row value is se_i / (float)width, se_i one chain
 *                     over j = 0 .. width - 1 from +0.0f of se = se + d * d with d = x[i][j] - y[i][j].  Rows are cut into blocks of
 *                     GNNVC_GRAD_BLOCK_ROWS; a block's partial is one chain over its row values in ascending order from +0.0f, one
 *                     rounded add each; the call's total is one chain over the partials in ascending block order from +0.0f, and
 *                     loss_sum = loss_sum + (double)total.  Up to GNNVC_GRAD_BLOCK_ROWS rows the total is MSE_loss's own chain,
 *                     loss += se / width over the rows, before its division by the height, bit for bit.  The counts are run_model's,
 *                     on column 0 alone: positives = rows with y[i][0] > 0.5f (num_true), positive_hits = those of them with
 *                     x[i][0] > 0.5f (true_accuracy), negative_hits = rows with !(y[i][0] > 0.5f) and x[i][0] < 0.5f
 *                     (total_accuracy); a NaN counts where these comparisons put it.  rows = the rows seen.  From them run_model
 *                     reports loss_sum / rows, (positive_hits + negative_hits) / rows and positive_hits / positives.
 * gnnvc_sgd_step: SGD_step over count parameters, per element
 *                     g = grad[i];  if (weight_decay > 0.0f) g = g + ((2.0f * weight_decay) * w[i]);
 *                     v = (momentum * vel[i]) + (g / (float)batch);  vel[i] = v;  w[i] = w[i] - (lr * v);
 *                     with zero_grad != 0 then grad[i] = +0.0f, else grad is not written (the decayed value is not stored back).
 *                     params, vel and grad must not overlap.
 * Checks, in this order: a NULL engine, width == 0, batch == 0, grad and stats both NULL: GNNVC_ERR_INVALID.  A multi-device handle:
 * GNNVC_ERR_UNSUPPORTED.  rows == 0 or count == 0: GNNVC_OK, nothing is read or written.  Then a NULL scores, target, params, vel
 * or grad buffer: GNNVC_ERR_INVALID.  The _device forms take device pointers (the stats too: 8-byte aligned device memory), are
 * asynchronous on the engine's stream and never wait; no atomics are used, so a result depends on neither the grid nor the run.
 * The host forms copy in and out (the stats as found, so they add up across calls too) and wait for the stream. */
typedef struct gnnvc_fit_stats {     /* 40 bytes; zero it to start a read-out; every call adds to it */
    double   loss_sum;               /* sum of the calls' fp32 totals, each the sum over rows of se / width */
    uint64_t rows, positives, positive_hits, negative_hits;
} gnnvc_fit_stats;

int gnnvc_mse_device(gnnvc_engine *e, uint32_t rows, uint32_t width, const float *d_scores, const float *d_target,
                     float *d_grad /* may be NULL */, gnnvc_fit_stats *d_stats /* device memory, may be NULL */);
int gnnvc_mse(gnnvc_engine *e, uint32_t rows, uint32_t width, const float *scores, const float *target,
              float *grad, gnnvc_fit_stats *stats);            /* host pointers; waits for the stream */
int gnnvc_sgd_step_device(gnnvc_engine *e, uint64_t count, float *d_params, float *d_vel, float *d_grad,
                          uint64_t batch, float lr, float momentum, float weight_decay, int zero_grad);
int gnnvc_sgd_step(gnnvc_engine *e, uint64_t count, float *params, float *vel, float *grad,
                   uint64_t batch, float lr, float momentum, float weight_decay, int zero_grad);

#ifdef __cplusplus
}
#endif
#endif /* GNNVC_H */
