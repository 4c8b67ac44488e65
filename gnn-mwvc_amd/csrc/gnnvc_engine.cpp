// gnnvc_engine.cpp — host side of libgnnvc_hip.so: the C ABI of include/gnnvc.h.
//
// Holds the parsed model (the reference's text format, reference
// src/gnn_inference.cpp:120-139), the device copy of the graph view, the
// feature buffers, and sequences the stages like model::predict does
// (reference src/gnn_inference.cpp:67-81).  All arithmetic happens in the HIP
// kernels of gnnvc_kernels.hip; there is no CPU fallback here.
#include <cmath>

#include "gnnvc_engine_state.h"

namespace {

// ---- model text ------------------------------------------------------------
struct Cursor {
    const char *p, *end;
    bool token(std::string &out) {
        while (p < end && isspace((unsigned char)*p)) ++p;
        if (p >= end) return false;
        const char *s = p;
        while (p < end && !isspace((unsigned char)*p)) ++p;
        out.assign(s, p);
        return true;
    }
    bool size(uint32_t &v) {
        std::string t;
        if (!token(t)) return false;
        char *q = nullptr;
        unsigned long x = strtoul(t.c_str(), &q, 10);
        if (!q || *q) return false;
        v = (uint32_t)x;
        return true;
    }
    // matrix text: "<h> <w>" then h*w numbers (reference src/matrix.cpp:97-104)
    bool matrix(uint32_t &h, uint32_t &w, std::vector<float> &d) {
        if (!size(h) || !size(w)) return false;
        if ((uint64_t)h * w > (1u << 26)) return false;
        d.resize((size_t)h * w);
        std::string t;
        for (auto &v : d) {
            if (!token(t)) return false;
            v = strtof(t.c_str(), nullptr);  // same rounding as istream >> float
        }
        return true;
    }
};

int parse_model(gnnvc_engine *e, const char *text, size_t len) {
    Cursor c{text, text + len};
    std::string t;
    uint32_t n = 0;
    if (!c.token(e->name) || !c.size(n) || !c.token(t))
        return fail(e, GNNVC_ERR_INVALID, "model header: expected '<name> <n> Layers'");
    if (n > 4096) return fail(e, GNNVC_ERR_INVALID, "implausible layer count %u", n);
    for (uint32_t i = 0; i < n; ++i) {
        if (!c.token(t)) return fail(e, GNNVC_ERR_INVALID, "model text ends after %u of %u layers", i, n);
        Layer l;
        if (t == "Linear_Layer") {
            uint32_t bh = 0, bw = 0;
            l.kind = kLinear;
            if (!c.token(t) || !c.matrix(l.k, l.m, l.W))
                return fail(e, GNNVC_ERR_INVALID, "layer %u: malformed weight matrix", i);
            if (!c.token(t) || !c.matrix(bh, bw, l.bias) || bh != 1 || bw != l.m)
                return fail(e, GNNVC_ERR_INVALID, "layer %u: malformed bias", i);
        } else if (t == "Graph_Layer") {
            l.kind = kGraph;
        } else if (t == "ReLU_Activation") {
            l.kind = kRelu;
        } else if (t == "Sigmoid_Activation") {
            l.kind = kSigmoid;
        } else {
            continue;  // the reference's if-chain ignores unknown records
        }
        e->layers.push_back(std::move(l));
    }
    // zero layers is allowed: an engine used only for the layer-level entry points
    return GNNVC_OK;
}

// May a term whose input is +-0 be left out of this layer's fma chains bit for bit?  fma(+-0, w, acc) == acc needs a finite w
// (0 x inf is NaN) and an acc other than -0.0f; a chain that starts from +0.0f reaches -0.0f only by underflow, and a -0 / +0
// difference in acc survives the separately rounded bias add only if the bias is -0.0f itself.
bool zero_terms_may_go(const Layer &l) {
    for (float w : l.W)
        if (!std::isfinite(w)) return false;
    for (float b : l.bias) {
        uint32_t bits;
        memcpy(&bits, &b, sizeof bits);
        if (bits == 0x80000000u) return false;
    }
    return true;
}

void plan_generic(gnnvc_engine *e);

// Widths through the network; decides fused vs layer-by-layer.
int plan_model(gnnvc_engine *e) {
    // input width: a leading graph layer accepts any width; a leading linear fixes it.
    int wd = 1;
    for (const auto &l : e->layers) {
        if (l.kind == kLinear) { wd = (int)l.k; break; }
        if (l.kind == kGraph) { wd = 1; break; }
    }
    // walk back from the first linear through graph layers: k = 2*w + 3
    {
        int first_lin = -1, graphs_before = 0;
        for (size_t i = 0; i < e->layers.size(); ++i) {
            if (e->layers[i].kind == kLinear) { first_lin = (int)i; break; }
            if (e->layers[i].kind == kGraph) ++graphs_before;
        }
        if (first_lin >= 0) {
            int k = (int)e->layers[first_lin].k;
            for (int gq = 0; gq < graphs_before; ++gq) {
                if ((k - 3) % 2 != 0 || k < 5) return fail(e, GNNVC_ERR_INVALID, "inconsistent layer widths");
                k = (k - 3) / 2;
            }
            wd = k;
        }
    }
    e->in_width = wd;
    e->max_width = wd;
    size_t off = 0;
    for (auto &l : e->layers) {
        if (l.kind == kLinear) {
            if ((int)l.k != wd) return fail(e, GNNVC_ERR_INVALID, "linear layer expects %u inputs, gets %d", l.k, wd);
            wd = (int)l.m;
            l.w_off = off; off += l.W.size();
            l.b_off = off; off += l.bias.size();
        } else if (l.kind == kGraph) {
            wd = 2 * wd + 3;
        }
        e->max_width = std::max(e->max_width, wd);
    }
    e->out_width = wd;
    e->ends_in_sigmoid = !e->layers.empty() && e->layers.back().kind == kSigmoid;

    // fused plan: (Graph, Linear, ReLU, Linear, ReLU, Linear, ReLU|Sigmoid)+
    std::vector<StagePlan> st;
    size_t i = 0;
    int f = e->in_width;
    bool ok = !e->layers.empty() && e->layers.size() % 7 == 0;
    while (ok && i < e->layers.size()) {
        const Layer *L = &e->layers[i];
        ok = L[0].kind == kGraph && L[1].kind == kLinear && L[2].kind == kRelu &&
             L[3].kind == kLinear && L[4].kind == kRelu && L[5].kind == kLinear &&
             (L[6].kind == kRelu || L[6].kind == kSigmoid);
        if (!ok) break;
        StagePlan sp;
        sp.f = f;
        sp.n1 = (int)L[1].m; sp.n2 = (int)L[3].m; sp.n3 = (int)L[5].m;
        sp.sigmoid_last = L[6].kind == kSigmoid;
        sp.param_offset = L[1].w_off;
        // the parameter buffer is laid out in layer order, so W1 b1 W2 b2 W3 b3 are contiguous
        sp.variant = gnnvc::stage_variant(sp.f, sp.n1, sp.n2, sp.n3, sp.sigmoid_last);
        sp.nd = 3;
        sp.wn[0] = sp.n1; sp.wn[1] = sp.n2; sp.wn[2] = sp.n3;
        for (int l = 0; l < 3; ++l)
            if (zero_terms_may_go(L[1 + 2 * l])) sp.skip_ok |= 1u << l;
        const bool last = (i + 7 == e->layers.size());
        ok = sp.variant >= 0 && (int)L[1].k == 2 * f + 3 && (sp.sigmoid_last ? last : true) &&
             (last || sp.n3 == 16);
        st.push_back(sp);
        f = sp.n3;
        i += 7;
    }
    if (ok && !st.empty() && st.back().sigmoid_last) e->stages = std::move(st);
    plan_generic(e);
    return GNNVC_OK;
}

// generic stages (k_stage_any): (Graph, (Linear, activation){d})+ with 1 <= d <= kMaxDenseLayers, d free per stage, any widths
// within stage_any_fits (which knows the LDS bounds too: the default one, and the opt-in one of gnnvc_set_generic_big_stages, which
// each stage carries as big_lds, and the feature width of gnnvc_set_generic_feature_width, carried as feat_width); every activation a ReLU but the model's last, a sigmoid (a model that ends in a ReLU stays layer
// by layer, as for the trained shapes).  One stage outside the bounds leaves the whole model layer by layer.  Derives e->gstages
// anew from the layers (their parameter offsets are plan_model's): at model load, and when the opt-in's limit moves.
//
// With gnnvc_set_generic_patterns (e->patterns, carried by every stage as `patterns`) the pattern is [P] S*, at least one stage: P, a
// DENSE stage (Linear, activation){1..6} in front of the first graph layer (stage 0 of the list), and a last activation that may
// also be a ReLU or be missing.  This function only reads the layer sequence into stages — a sigmoid inside the model, two graph
// layers in a row, two linear layers without an activation between them or a block of seven dense layers is no sequence of
// stages under any mask — and says of each whether it is dense, how it ends and whether it is the model's last; whether the mask
// admits that is stage_any_route's decision, like every bound.
void plan_generic(gnnvc_engine *e) {
    e->gstages.clear();
    e->live_seen.clear();   // ("generic_live_*_<s>" speak of the stages of the list that ran)
    std::vector<StagePlan> gs;
    bool gok = !e->layers.empty();
    int f = e->in_width;
    for (size_t i = 0; gok && i < e->layers.size();) {
        const Layer *L = &e->layers[i];
        const size_t left = e->layers.size() - i;
        StagePlan sp;
        sp.dense = i == 0 && L[0].kind == kLinear;   // (only the model's first stage may lack its graph layer)
        gok = sp.dense || L[0].kind == kGraph;
        if (!gok) break;
        sp.f = f;
        sp.nd = 0;
        sp.patterns = e->patterns;
        int k = sp.dense ? f : 2 * f + 3;
        size_t at = sp.dense ? 0 : 1;
        while (gok && at < left && L[at].kind == kLinear) {
            // what follows the linear layer: its ReLU, the model's last sigmoid, or nothing — the model's last layer is this one
            const bool bare = at + 1 == left;
            const bool model_end = bare || at + 2 == left;
            const int end = bare ? gnnvc::kEndNone : L[at + 1].kind == kRelu ? gnnvc::kEndRelu
                            : (L[at + 1].kind == kSigmoid && model_end) ? gnnvc::kEndSigmoid : -1;
            gok = sp.nd < gnnvc::kMaxDenseLayers && (int)L[at].k == k && end >= 0;
            if (!gok) break;
            if (sp.nd == 0) sp.param_offset = L[at].w_off;   // (the parameter buffer is in layer order: W b W b ... are contiguous)
            sp.wn[sp.nd++] = k = (int)L[at].m;
            sp.end = end;
            sp.model_last = model_end;
            sp.sigmoid_last = end == gnnvc::kEndSigmoid;
            at += bare ? 1 : 2;
        }
        gok = gok && sp.nd >= 1 && (at == left || L[at].kind == kGraph);
        if (!gok) break;
        sp.n3 = sp.wn[sp.nd - 1];
        if (sp.nd == 3) { sp.n1 = sp.wn[0]; sp.n2 = sp.wn[1]; }
        sp.big_lds = e->big_lds;
        sp.feat_width = e->feat_width;
        gok = gnnvc::stage_any_fits(sp);
        gs.push_back(sp);
        f = sp.n3;
        i += at;
    }
    if (gok && !gs.empty()) e->gstages = std::move(gs);
}

int upload_params(gnnvc_engine *e) {
    std::vector<float> flat;
    for (const auto &l : e->layers)
        if (l.kind == kLinear) {
            flat.insert(flat.end(), l.W.begin(), l.W.end());
            flat.insert(flat.end(), l.bias.begin(), l.bias.end());
        }
    HIP_TRY(e, e->params.reserve(flat.size() + 64));
    if (!flat.empty())
        HIP_TRY(e, hipMemcpy(e->params.p, flat.data(), flat.size() * sizeof(float), hipMemcpyHostToDevice));
    return GNNVC_OK;
}

// ---------------------------------------------------------------- one stage call = plan selection, then launches
//
// choose_stage  decides WHAT a call runs: which of the per-graph plans serves the neighbour sums (building a plan the
//               first time it is due), whether the previous stage kernel of this forward already left the column
//               statistics, whether this stage's kernel produces them for the next one, sorted or natural tiles.
//               It launches nothing.
// launch_side_rows / launch_main  put the chosen kernels on the streams.  A new plan variant adds an enumerator, its
//               eligibility rule in choose_stage and its launches in launch_main.
struct StageChoice {
    enum Sums {
        kGather,            // the tile kernel gathers full rows itself (always correct; the fallback of every plan)
        kLdsTable,          // F = 1: byte table in LDS (k_lt_agg), the tile kernel only runs the dense layers
        kBlocked,           // F = 1: column-blocked partial sums (k_blk_accumulate)
        kCompactPrepared,   // F = 16: compact table written by gnnvc_stage_input_ready for exactly this input
        kCompactWhole,      // F = 16: compact table over the whole graph, decided per forward on the device
        kTableTiles         // F = 16, mid-size graphs: the tile kernel gathers the input's L2-resident compact table (k_stage_t4), or — decided
                            // on the device — leaves the launch to the gathering kernel behind it
    } sums = kGather;
    bool mfma = false;          // dense layers of the gathering kernel on the matrix cores
    bool fused_counts = false;  // kCompactWhole: the producing stage kernel of this forward left counts (and perhaps the table)
    bool rounds = false;        // kCompactWhole, last stage: sums one round at a time, dense kernel of round k under round k + 1
    bool emit = false;          // this stage's VALU epilogue counts / compacts its output rows for stage `stage + 1`
    bool emit_t4 = false;       // ... for the table tiles of stage `stage + 1` (k_stage_t4)
    bool elide = false;         // emit, and the kernel may leave out the full rows of waves whose table rows carry no flag (gnnvc::kSkipElide)
    bool elided_in = false;     // kCompactWhole: this stage's input was produced that way in this forward (gnnvc::CompactElide, kSkipRebuild)
    uint32_t long_thresh = 0xFFFFFFFFu;   // rows of at least this degree belong to the side streams
    gnnvc::SortedOrder sorted;  // n != 0: tiles from the degree-sorted list of this row range
};

int choose_stage(gnnvc_engine *e, int stage, uint32_t lo, uint32_t hi, const float *in, const float *out, bool in_forward,
                 StageChoice &c) {
    const bool longs = e->pg.rows.n_long > 0;
    const gnnvc::StagePlan &sp = e->stages[stage];
    // An announcement (gnnvc_stage_input_ready) covers the calls for ITS stage that follow it.  A call for any other
    // stage means the caller has moved on — the next forward has begun, or the announced buffer is about to be
    // rewritten — and a call that writes into the announced buffer ends it too: the table must never outlive its input.
    if (e->pg.c4.prepared_stage != -1 && (stage != e->pg.c4.prepared_stage || out == e->pg.c4.prepared_in)) e->pg.c4.prepared_stage = -1;
    // Producer side of the compact-table plan: inside a whole forward (engine-owned feature buffers nobody else
    // writes) the stage kernel that produces the next 16-wide stage's input also counts its non-zeros and writes
    // its compact rows, so that stage can skip its two passes over the input.  Only the VALU variants emit.
    const int fused_in = in_forward ? e->call.c4_fused_for : -1;   // is THIS stage's input covered by the previous kernel?
    const bool elided_in = in_forward && fused_in == stage && e->call.c4_elided_for == stage;
    e->call.c4_fused_for = -1;
    e->call.c4_elided_for = -1;
    const bool may_emit = in_forward && e->pg.c4.ready && !e->pg.c4.range_mode && e->pg.c4.base == 0 && e->pg.c4.end == e->g.n && !longs &&
                          (size_t)stage + 1 < e->stages.size() && e->stages[stage + 1].f == 16 && lo == 0 && hi == e->g.n &&
                          e->opt.mfma != 1 && !e->pg.c4.stage_off[stage + 1];
    // Elided rows: the producer may leave out full rows only if everything that runs on them in this forward is the compact-table
    // route of a whole forward on the engine's own buffers — whose kernels read a vertex's full row only where its table row is
    // flagged, and whose preparation puts the rows back on the device if it does not take the table as written.  So: may_emit
    // (a whole forward, the whole-graph plan, no long rows, the consumer's plan not switched off), no audit in this call (it
    // compares full rows), the consumer's first layer may leave out zero terms (else its dense kernel is handed no table), no
    // slice, no table tiles and no sorted tiles in this forward (the consumer's choice below would not be kCompactWhole — which
    // also means no pruned or filtered view and no plan builder that reads features, gather_view), and the last verdict seen for
    // the consumer said that its table was taken as written.  The consumer's choice is checked below: elided_in.
    const bool may_elide = may_emit && gnnvc::compact_elides_rows() && !e->call.audit_now && !e->call.t4_now && !e->g.sliced() && !e->pg.rows.sorted_wanted &&
                           e->opt.dense_skip && (e->stages[stage + 1].skip_ok & 1u) && e->pg.c4.elide_ok[stage + 1];
    c.long_thresh = (sp.f == 16) ? e->pg.rows.thresh_f16 : e->pg.rows.long_thresh;
    c.mfma = e->opt.mfma == 1 || (e->opt.mfma == 2 && sp.f == 16);
    const bool t4 = in_forward && e->call.t4_now && lo == 0 && hi == e->g.n;   // table tiles: whole forwards on a graph that qualifies
    c.emit_t4 = t4 && (size_t)stage + 1 < e->stages.size();
    if (stage == 0) {
        // The LDS-table plan works in chunks of ~19.5 K rows, one workgroup each: a call that covers fewer than
        // three quarters of a GPU's worth of chunks (the pieces of a pipelined multi-GPU run) would leave most CUs
        // idle for the time one chunk takes — such calls use the column-blocked plan instead.
        if (e->pg.graph_uses >= 1 && !e->pg.lt.tried) {
            int rc = build_lds_table(e);
            if (rc) return rc;
        }
        // (a skewed graph's plan sums all of its rows at once: whole-graph calls only)
        // (consecutive-row layout: any call that covers at least three quarters of the chunks a full GPU takes — or of the plan's
        // own, where the plan is a rank's slice of fewer)
        const uint32_t lt_need = std::min(192u, e->pg.lt.chunks - e->pg.lt.chunks / 4u);
        const bool lt_fits = e->pg.lt.ready && !e->pg.lt.off && hi > lo &&
                             (e->pg.lt.mapped ? (lo == 0 && hi == e->g.n)
                                           : (lo >= e->pg.lt.base && hi <= e->pg.lt.end &&
                                              ((hi - 1 - e->pg.lt.base) / e->pg.lt.rows - (lo - e->pg.lt.base) / e->pg.lt.rows + 1) >= lt_need));
        if (e->pg.graph_uses >= 1 && !lt_fits && !e->pg.blk.tried) {
            int rc = build_blocked(e);
            if (rc) return rc;
        }
        ++e->pg.graph_uses;
        c.sums = lt_fits ? StageChoice::kLdsTable : (e->pg.blk.ready ? StageChoice::kBlocked : StageChoice::kGather);
        if (lt_fits && in_forward) e->pg.lt.used = true;
        if (lt_fits && e->pg.lt.mapped) c.long_thresh = e->pg.lt.plan_thresh;   // the plan holds every row below the giant ones
        c.emit = may_emit;
        c.elide = may_elide;
        if (c.sums != StageChoice::kGather) return GNNVC_OK;   // (those two bring their own tile order)
    } else if (sp.f == 16 && t4) {
        c.sums = StageChoice::kTableTiles;
    } else if (sp.f == 16) {
        // (the second forward on a graph builds the plan; a graph whose plain 16-wide stages cost well above the build — the
        // option's bound — builds it in its first, which is all a score-once caller ever runs)
        const bool first_too = e->opt.compact_first_entries && e->g.nnz >= e->opt.compact_first_entries && lo == 0 && hi == e->g.n && in_forward;
        if (!e->pg.c4.range_mode && (e->pg.graph_uses >= 2 || first_too) && !e->pg.c4.tried) {
            int rc = build_compact(e);
            if (rc) return rc;
        }
        const bool whole_plan = e->pg.c4.ready && e->pg.c4.base == 0 && e->pg.c4.end == e->g.n && !e->pg.c4.stage_off[stage];
        const bool prepared = e->pg.c4.ready && e->pg.c4.prepared_stage == stage && e->pg.c4.prepared_in == in &&
                              lo >= e->pg.c4.base && hi <= e->pg.c4.end && hi > lo;
        if (prepared && !longs) {
            // gnnvc_stage_input_ready wrote the table for this input: any call that fills at least half the
            // GPU with chunks takes the sums from it (smaller ones would leave most CUs idle for a chunk's time)
            const uint32_t nchunks = (hi - 1 - e->pg.c4.base) / e->pg.c4.rows - (lo - e->pg.c4.base) / e->pg.c4.rows + 1;
            if (nchunks >= 128u) c.sums = StageChoice::kCompactPrepared;
        } else if (!e->pg.c4.range_mode && whole_plan && !longs && (uint64_t)(hi - lo) * 2 >= e->g.n) {
            // worth its fixed cost (count + compact the whole input) only when this call covers most of the rows
            c.sums = StageChoice::kCompactWhole;
            c.fused_counts = fused_in == stage;
            // Last stage: k_c4_agg is a persistent grid that holds nearly all LDS of its CUs but leaves most VALU
            // cycles idle, and the dense-only sigmoid kernel that follows is VALU-bound and needs no LDS.  So the sums
            // are launched one round (256 chunks) at a time and the dense kernel of round k goes to the aux stream,
            // under the sums of round k + 1.  Metric graph: 1.71 -> 1.58 ms.  (Not for the feature stages: their dense
            // kernels store 64-byte rows and slow the co-running sums by more than is gained.)
            // (a call of more rounds than there are round counters — "plan_chunk_rows" 16 on 300 K rows: 74 — runs its sums in
            // one launch, as with "overlap_dense" 0: it used to be refused by launch_main, tools/optionflips.py random_2)
            const uint32_t nrounds = ((hi - 1 - e->pg.c4.base) / e->pg.c4.rows - (lo - e->pg.c4.base) / e->pg.c4.rows) / 256u + 1u;
            c.rounds = e->opt.overlap && sp.variant == 2 && e->opt.mfma != 1 && nrounds <= gnnvc::compact_rounds();
            c.emit = may_emit;   // this stage's own (aggregate-only, VALU) kernel produces for the next one
            c.elide = may_elide;
            c.elided_in = elided_in;
        }
    }
    if (elided_in && !c.elided_in)   // (the rule above is this choice, made a stage early: they must agree)
        return fail(e, GNNVC_ERR_STATE, "stage %d: its input was written without full rows, but the compact-table plan does not run it", stage);
    // degree-sorted tiles on skewed graphs (every stage; the list is cached per row range)
    int rc = ensure_sorted(e, lo, hi);
    if (rc) return rc;
    if (e->call.srt_cur >= 0 && e->pg.sorted[e->call.srt_cur].use) {
        c.sorted.n = e->pg.sorted[e->call.srt_cur].n;
        c.sorted.vertex = e->srt.range[e->call.srt_cur].vertex.p;
        c.sorted.meta = e->srt.range[e->call.srt_cur].meta.p;
        c.rounds = false;   // (the plan forced onto a graph with sorted tiles: the gathering kernel does the stage)
    }
    return GNNVC_OK;
}

// stage sp over rows [lo, hi) of the engine's graph, on its stream
gnnvc::StageCall stage_call(const gnnvc_engine *e, const gnnvc::StagePlan &sp, const float *in, float *out, float *logits, uint32_t lo,
                            uint32_t hi) {
    return {.sp = &sp, .g = &e->g, .ws = e->ws, .params = e->params.p, .in = in, .out = out, .logits = logits, .row_lo = lo,
            .row_hi = hi, .stream = e->stream, .skip = e->opt.dense_skip ? sp.skip_ok : 0u};
}

// fork: the long (and giant) rows of this stage beside the tile kernel
int launch_side_rows(gnnvc_engine *e, const gnnvc::StageCall &call, uint32_t thr, bool plain_f1) {
    const GraphDev &gv = *call.g;
    // One side queue beside the main one (ensure_side_streams).  The giant rows' walk is a latency chain on a few waves and
    // always goes there; the long rows join it — unless that walk is what a stage waits for (find_giant: the power-law graph),
    // then they run ahead of the tile kernel on the main queue instead: power-law 1 M 0.89 ms (long rows beside the giant
    // walk: 1.15), R-MAT-22 2.62 ms (long rows on the main queue: 2.79).
    const bool side = e->opt.side_streams != 0;
    const bool long_on_main = side && (e->opt.long_on_main < 0 ? (e->pg.rows.n_giant != 0 && e->pg.rows.giant_walk_bound) : e->opt.long_on_main != 0);
    const bool side_long = side && !long_on_main;
    hipStream_t s_long = side_long ? e->long_stream : e->stream;
    hipStream_t s_giant = !side ? e->stream : (long_on_main ? e->giant_stream : e->long_stream);
    e->call.side_join = !side ? 0 : (long_on_main ? 2 : 1);
    // rows from this degree on go the giant way in this stage
    const uint32_t giant_from = call.sp->f == 16 ? e->giant_f16() : e->pg.rows.giant_thresh;
    gnnvc::StageCall giant = call;   // (on the main queue until the fork; the pruned view only where the option asks for it)
    if (!e->opt.prune_giant) giant.g = &e->g;
    gnnvc::GiantRows gr;
    bool gather_first = false;
    if (e->pg.rows.n_giant) {
        gr.n = e->pg.rows.n_giant;
        gr.blocks = e->pg.rows.giant_blocks;
        gr.meta = e->gi.meta.p;
        gr.off = e->gi.off.p;
        gr.slab = e->gi.slab.p;
        gr.agg = e->gi.agg.p;
        if (e->pg.rows.maxseg > 1) {
            gr.segsum = e->gi.segsum.p;
            gr.segmap = e->gi.segmap.p;
            gr.maxseg = e->pg.rows.maxseg;
        }
        // The giant rows' gather on the main queue, ahead of the fork (see launch_giant_stage) — where it is small (a throughput
        // kernel that delays the tile kernel by what it takes alone: R-MAT-22's 7.5 M giant entries 0.03 - 0.05 ms, R-MAT-24's
        // 64 M 0.3 - 0.6 ms) and the long rows are on the side queue behind the walk.  Measured: R-MAT-20 0.89 -> 0.83 ms
        // (first forward 1.32 -> 1.20), R-MAT-22 first forward 3.75 -> 3.57 (steady the same); R-MAT-24 9.5 -> 10.8 and
        // power-law 0.84 -> 0.87 the wrong way, hence the two conditions.
        // ... or, however large, in an F = 1 stage that has no plan (a graph's first forward): every long row's chain is on the
        // side queue there and the gather at its head waited for slots for as long as the tile kernel ran (R-MAT-24: 3.1 ms
        // for a kernel that takes 0.6 alone; the stage 6.1 ms against the tile kernel's 3.3)
        gather_first = side && (e->opt.giant_gather_first < 0 ? (!long_on_main && (e->pg.rows.giant_entries <= (16ull << 20) || plain_f1))
                                                               : e->opt.giant_gather_first != 0);
        if (gather_first) HIP_TRY(e, gnnvc::launch_giant_stage(giant, gr, giant_from, gnnvc::GiantPart::kGather));
    }
    if (side) {
        HIP_TRY(e, hipEventRecord(e->ev_fork, e->stream));
        if (side_long) HIP_TRY(e, hipStreamWaitEvent(e->long_stream, e->ev_fork, 0));
    }
    if (e->pg.rows.n_giant) {   // the heaviest rows: beside the tile kernel
        if (long_on_main) HIP_TRY(e, hipStreamWaitEvent(e->giant_stream, e->ev_fork, 0));
        giant.stream = s_giant;
        HIP_TRY(e, gnnvc::launch_giant_stage(giant, gr, giant_from, gather_first ? gnnvc::GiantPart::kAfterGather : gnnvc::GiantPart::kAll));
        if (long_on_main) HIP_TRY(e, hipEventRecord(e->ev_giant, e->giant_stream));
    }
    // (with rows classed by the entries they have left, k_long_* takes rows from gv.eff_thresh entries on whatever their degree)
    const uint32_t long_from = gv.prune_eff ? std::min(thr, gv.eff_thresh) : thr;
    if ((e->pg.rows.n_giant < e->pg.rows.n_long || giant_from > e->pg.rows.giant_thresh) && long_from < giant_from) {   // (equal: a plan or the giant kernels have every row in between)
        gnnvc::StageCall lng = call;
        lng.stream = s_long;
        HIP_TRY(e, gnnvc::launch_long_stage(lng, {.list = e->long_list.p, .n = e->pg.rows.n_long, .min_deg = thr, .max_deg = giant_from}));
    }
    if (side_long) HIP_TRY(e, hipEventRecord(e->ev_long, e->long_stream));
    return GNNVC_OK;
}

// call: the stage on the view of the graph the gathering kernels take (gather_view); the plans' launches see the graph itself
int launch_main(gnnvc_engine *e, const StageChoice &c, const gnnvc::StageCall &call_in, const gnnvc::SortedOrder &so_p, int stage) {
    gnnvc::StageCall call = call_in;   // (with the two bits of `skip` that belong to elided rows: every launch below copies this one)
    if (c.emit && c.elide) call.skip |= gnnvc::kSkipElide;
    if (c.elided_in) call.skip |= gnnvc::kSkipRebuild;
    const gnnvc::StagePlan &sp = *call.sp;
    const GraphDev &gv = *call.g;
    const uint32_t lo = call.row_lo, hi = call.row_hi;
    const float *in = call.in;
    gnnvc::StageCall plain = call;
    plain.g = &e->g;
    gnnvc::EmitArgs emit;
    // (the counters are zeroed only AFTER this stage's own k_c4_choose has read what the previous stage kernel left in them: by
    // that kernel itself where it read them — c4_emit_zero says whether the last thing queued on them was such a launch — and
    // by a memset here otherwise)
    auto arm_emit = [&]() -> int {
        if (!c.emit) return GNNVC_OK;
        const bool zero = e->call.c4_emit_zero;
        e->call.c4_emit_zero = false;   // (the kernel armed here counts into them)
        if (!zero) {
            ++e->pg.plan_memsets;
            HIP_TRY(e, hipMemsetAsync(e->c4.emit_counts.p, 0, gnnvc::kEmitCounters * sizeof(unsigned long long), e->stream));
        }
        emit.spec = e->c4.desc.p + gnnvc_engine::kDescWords * stage;   // consumer stage `stage + 1`: its descriptor words
        emit.table = e->c4.table.p;
        emit.counts = e->c4.emit_counts.p;
        e->call.c4_fused_for = stage + 1;
        if (c.elide) {
            e->call.c4_elided_for = stage + 1;
            ++e->pg.c4.elided_last;
        }
        return GNNVC_OK;
    };
    // First use of the compact-table plan on this graph: no earlier forward has said which four columns the NEXT stage's
    // table holds, so this stage's kernel could only count, and the consumer would make a pass of its own over its whole
    // input to write the table (k_c4_compact: 0.25 ms per stage on the metric graph — what a graph scored ONCE pays in full).
    // A pilot — the plain gathering kernel over the first rows of this very stage — makes that choice ahead of the real
    // run, which then writes the table on its way.  The consumer's k_c4_choose still decides from the counts of ALL rows
    // and has the table rewritten if the pilot chose otherwise: the pilot changes time, never a result.
    auto pilot = [&]() -> int {
        if (!c.emit || e->pg.c4.seeded[stage + 1] || !e->opt.pilot_rows) return GNNVC_OK;
        e->pg.c4.seeded[stage + 1] = true;
        const uint32_t rows = std::min(e->opt.pilot_rows, hi - lo);
        if ((uint64_t)rows * 8 > (uint64_t)(hi - lo)) return GNNVC_OK;   // (a graph this small is its own pilot: not worth a launch)
        uint32_t *cons = e->c4.desc.p + gnnvc_engine::kDescWords * stage;   // consumer stage `stage + 1`
        e->call.c4_emit_zero = false;
        ++e->pg.plan_memsets;
        HIP_TRY(e, hipMemsetAsync(e->c4.emit_counts.p, 0, gnnvc::kEmitCounters * sizeof(unsigned long long), e->stream));
        gnnvc::EmitArgs pe;
        pe.spec = e->c4.desc.p + 2 * gnnvc_engine::kDescWords + 4;   // a word that is always 0: count, do not write table rows
        pe.table = e->c4.table.p;
        pe.counts = e->c4.emit_counts.p;
        gnnvc::StageCall first = plain;   // (every row of them on VALU tiles, no logits)
        first.row_hi = lo + rows;
        first.logits = nullptr;
        HIP_TRY(e, gnnvc::launch_stage(first, {.interleave = true, .emit = pe}));
        HIP_TRY(e, gnnvc::compact_choose(e->c4.emit_counts.p, 64, rows, cons, 1u, e->stream, /*clear_counts=*/true));
        e->call.c4_emit_zero = true;
        return GNNVC_OK;
    };
    if (c.emit_t4) {   // this stage's epilogue counts its output's columns and writes the next stage's table (for that stage's last choice)
        const int cons = stage + 1;
        emit.spec = e->t4.desc_of(cons, e->t4.parity);
        emit.table = e->t4.table[cons - 1].p;
        emit.counts = e->t4.counts_of(cons, e->t4.parity);   // (cleared by the consumer's launch of the previous forward: k_stage_t4)
    }
    if (c.sums == StageChoice::kTableTiles) {
        uint32_t *d_in = e->t4.desc_of(stage, e->t4.parity), *d_out = e->t4.desc_of(stage, e->t4.parity ^ 1u);
        const bool solo = e->pg.t4.fit_seen[stage] && e->opt.t4_solo;
        HIP_TRY(e, gnnvc::launch_stage_t4(plain, {.table_in = e->t4.table[stage - 1].p,
                                                  .counts_in = e->t4.counts_of(stage, e->t4.parity),
                                                  .counts_zero = e->t4.counts_of(stage, e->t4.parity ^ 1u),
                                                  .desc_in = d_in, .desc_out = d_out, .emit = emit, .interleave = e->pg.rows.interleave, .solo = solo}));
        if (solo) return GNNVC_OK;
        // ... and the gathering kernel, which leaves at once when the table tiles did the rows (d_out[8]: decided on the device)
        return hip_rc(e, gnnvc::launch_stage(call, {.long_thresh = c.long_thresh, .mfma = c.mfma, .interleave = e->pg.rows.interleave,
                                                    .skip_flag = d_out + 8}));
    }
    if (c.sums == StageChoice::kLdsTable || c.sums == StageChoice::kBlocked) {
        int rc = pilot();
        if (rc) return rc;
        rc = arm_emit();
        if (rc) return rc;
    }
    if (c.sums == StageChoice::kLdsTable) {   // (the sums share the blocked plan's buffer)
        ++e->pg.plan_memsets;   // (the flag "this input does not match the table": cleared by a memset ahead of k_lt_bytes_x)
        return hip_rc(e, gnnvc::launch_stage0_lds_table(plain, lds_table_plan(e), e->lt.bytes.p, e->blk.acc.p, e->lt.bad.p,
                                                        {.long_thresh = c.long_thresh, .mfma = e->opt.mfma == 1,
                                                         .interleave = e->pg.rows.interleave, .emit = emit}));
    }
    if (c.sums == StageChoice::kBlocked)
        return hip_rc(e, gnnvc::launch_stage0_blocked(plain,
                                                      {.nblocks = e->pg.blk.count, .bp = e->blk.ptr.p, .colb = e->blk.col.p, .acc = e->blk.acc.p},
                                                      {.long_thresh = e->pg.rows.long_thresh, .mfma = e->opt.mfma == 1,
                                                       .interleave = e->pg.rows.interleave, .emit = emit}));
    gnnvc::CompactSums sums;   // (all null: the compact-table plan is not in this call)
    uint32_t *desc = nullptr;
    if (c.sums == StageChoice::kCompactPrepared || c.sums == StageChoice::kCompactWhole) {
        desc = e->c4.desc.p + gnnvc_engine::kDescWords * (stage - 1);
        e->pg.c4.last_desc = gnnvc_engine::kDescWords * (stage - 1);
        if (c.sums == StageChoice::kCompactWhole) e->pg.c4.fit_used[stage] = true;
        sums = {.acc4 = e->c4.acc.p, .c4desc = desc, .agg16 = e->c4.agg16.p, .table_in = (call.skip & 1u) ? e->c4.table.p : nullptr};   // (without the table: route C, the full chain)
        const bool whole = c.sums == StageChoice::kCompactWhole;
        if (whole && !c.fused_counts) HIP_TRY(e, gnnvc::column_counts(in, e->g.n, e->c4.counts.p, e->stream));
        const bool fused = whole && c.fused_counts;
        // what: 1 = choose the columns + write the table, 2 = the sums; the prepared table only needs its sums, a call
        // that runs its sums round by round (below) only the preparation
        const int what = !whole ? 2 : (c.rounds ? 1 : 3);
        // (its k_c4_choose clears what this stage counts into: desc[5], the rounds' counters, and the producer's counters
        // where it is the one that reads them)
        if (fused) e->call.c4_emit_zero = false;
        if (!(what & 1)) ++e->pg.plan_memsets;   // (no k_c4_choose in this call: launch_compact_gather clears desc[5] with a memset)
        // (a forward's own rows: k_c4_choose leaves its verdict on the producer's table, and has elided rows put back where it
        // does not take that table — `in` is e->h[] then, written by nobody else)
        gnnvc::CompactElide el;
        if (fused && stage >= 1 && stage <= 2 && e->c4.elide.p)
            el = {.words = e->c4.elide.p + gnnvc::kElideWords * (stage - 1), .rows = const_cast<float *>(in), .elided = c.elided_in};
        if (c.elided_in && !el.words) return fail(e, GNNVC_ERR_STATE, "stage %d: elided rows without their words", stage);
        HIP_TRY(e, gnnvc::launch_compact_gather(e->g, compact_plan(e), in, fused ? e->c4.emit_counts.p : e->c4.counts.p, fused ? 64 : 1,
                                                desc, e->c4.table.p, e->c4.acc.p, lo, hi, e->c4.dirty.p, e->pg.c4.dirty_cap,
                                                e->c4.agg16.p, e->stream, what, c.rounds ? e->c4.round_counts.p : nullptr, 256u * e->pg.c4.rows, fused, el));
        if (fused) e->call.c4_emit_zero = true;
    }
    if (c.sums != StageChoice::kLdsTable && c.sums != StageChoice::kBlocked) {
        int rc = pilot();
        if (rc) return rc;
        rc = arm_emit();
        if (rc) return rc;
    }
    const gnnvc::SortedOrder *sop = c.sorted.n ? &c.sorted : nullptr;
    // Wide tiles (k_stage_w*): a graph with fewer tiles than the chip has SIMDs — the reference CLI's later predict calls — and
    // nothing but the plain gather to run (no plan, no long rows, no pruned adjacency, nothing to emit): a workgroup per tile
    if (c.sums == StageChoice::kGather && e->opt.wide && e->g.n <= (sp.f == 16 ? e->opt.wide_max_n16 : e->opt.wide_max_n) && !e->g.sliced() && e->pg.rows.n_long == 0 && !sop &&
        !sums.acc4 && !emit.counts && gv.prune_bad == nullptr && gv.zero_bits == nullptr && sp.variant >= 0 && sp.variant <= 2) {
        e->pg.wide_used = true;
        e->call.stage_wide = true;
        return hip_rc(e, gnnvc::launch_stage_wide(plain));
    }
    HIP_TRY(e, gnnvc::launch_stage(call, {.long_thresh = c.long_thresh, .mfma = c.mfma, .so = sop, .interleave = e->pg.rows.interleave,
                                          .sums = sums, .mfma_agg = e->opt.mfma == 1, .emit = emit, .dense_part = !c.rounds,
                                          .so_pruned = so_p.vertex ? &so_p : nullptr}));
    if (!c.rounds) return GNNVC_OK;
    // (desc[5] is zero and each round's counter at the round's first slot: k_c4_choose, what = 1 above)
    const uint32_t rows = e->pg.c4.rows, c0 = (lo - e->pg.c4.base) / rows, c1 = (hi - 1 - e->pg.c4.base) / rows;
    const uint32_t nrounds = (c1 - c0) / 256u + 1u;
    if (nrounds > gnnvc::compact_rounds()) return fail(e, GNNVC_ERR_UNSUPPORTED, "too many rounds of the compact-table plan");
    {
        int rc = ensure_round_events(e, nrounds);
        if (rc) return rc;
    }
    for (uint32_t k = 0; k < nrounds; ++k) {
        const uint32_t ca = c0 + 256u * k, cb = std::min(c1 + 1u, ca + 256u);
        const uint32_t ra = std::max(lo, e->pg.c4.base + ca * rows);
        const uint32_t rb = (uint32_t)std::min<uint64_t>(hi, (uint64_t)e->pg.c4.base + (uint64_t)cb * rows);
        // round k hands out its dirty-row slots from word k, which starts at its first chunk's row offset within the call:
        // rows are done by whole chunks, so the round's dirty rows fit below the next round's first slot, and below c4_dirty_cap
        uint32_t *const count = e->c4.round_counts.p + k;
        const uint32_t slot_base = 256u * k * rows;
        HIP_TRY(e, gnnvc::compact_sums(e->g, compact_plan(e), desc, e->c4.table.p, e->c4.acc.p, ra, rb, e->c4.dirty.p, e->pg.c4.dirty_cap,
                                       e->stream, count));
        const bool last = k + 1 == nrounds;
        hipStream_t ds = last ? e->stream : e->aux_stream;
        if (!last) {
            HIP_TRY(e, hipEventRecord(e->round_ev[k], e->stream));
            HIP_TRY(e, hipStreamWaitEvent(e->aux_stream, e->round_ev[k], 0));
        }
        HIP_TRY(e, gnnvc::compact_fix(e->g, in, desc, e->c4.dirty.p, e->pg.c4.dirty_cap, e->c4.agg16.p, count, slot_base, ds,
                                      /*blocks=*/64, c.elided_in ? e->c4.table.p : nullptr));
        gnnvc::StageCall round = plain;
        round.row_lo = ra;
        round.row_hi = rb;
        round.stream = ds;
        HIP_TRY(e, gnnvc::launch_dense_sigmoid(round, sums, /*long_thresh=*/0xFFFFFFFFu));
    }
    if (nrounds > 1) {
        HIP_TRY(e, hipEventRecord(e->ev_join, e->aux_stream));
        HIP_TRY(e, hipStreamWaitEvent(e->stream, e->ev_join, 0));
    }
    return GNNVC_OK;
}

// what produced a stage (the audit's report): the plan that served its sums and everything that ran beside it
std::string describe_stage(const gnnvc_engine *e, const StageChoice &c, const GraphDev &gv) {
    static const char *const kSums[] = {"gather", "lds_table", "blocked", "compact_prepared", "compact_whole", "table_tiles"};
    char buf[320];
    int at = snprintf(buf, sizeof buf, "sums=%s%s mfma=%d sorted_tiles=%d rounds=%d emit=%d pruned=%d filtered=%d short_lists=%d",
                      kSums[c.sums], e->call.stage_wide ? " (wide tiles)" : "", c.mfma ? 1 : 0, c.sorted.n ? 1 : 0, c.rounds ? 1 : 0,
                      (c.emit || c.emit_t4) ? 1 : 0, gv.prune_bad ? 1 : 0, gv.zero_bits ? 1 : 0, gv.short_col ? 1 : 0);
    if (e->pg.rows.n_long > 0 && at > 0 && at < (int)sizeof buf) {
        // (launch_side_rows: side_join 0 = everything on the main queue, 1 = long and giant rows on the side queue, 2 = long rows
        // on the main queue, giant rows on a queue of their own)
        const char *lq = e->call.side_join == 1 ? "side" : "main";
        const char *gq = e->call.side_join == 0 ? "main" : (e->call.side_join == 1 ? "side" : "giant");
        at += snprintf(buf + at, sizeof buf - at, " long_rows=%u (from degree %u, %s queue)", e->pg.rows.n_long, c.long_thresh, lq);
        if (e->pg.rows.n_giant && at < (int)sizeof buf) snprintf(buf + at, sizeof buf - at, " giant_rows=%u (%s queue)", e->pg.rows.n_giant, gq);
    }
    return buf;
}

int run_stage(gnnvc_engine *e, int stage, uint32_t lo, uint32_t hi, const float *in, float *out, float *logits,
              bool in_forward = false, std::string *plan = nullptr) {
    e->call.stage_wide = false;
    StageChoice c;
    int rc = choose_stage(e, stage, lo, hi, in, out, in_forward, c);
    if (rc) return rc;
    const bool longs = e->pg.rows.n_long > 0;
    GraphDev gv;   // (the check behind a pruned adjacency is queued before the fork to the side streams)
    gnnvc::SortedOrder so_p;
    rc = gather_view(e, stage, lo, hi, in, c.sums == StageChoice::kGather, c.sorted.n != 0, gv, so_p, c.mfma, c.long_thresh);
    if (rc) return rc;
    gnnvc::StageCall call = stage_call(e, e->stages[stage], in, out, logits, lo, hi);
    call.g = &gv;
    if (longs) {
        rc = launch_side_rows(e, call, c.long_thresh, /*plain_f1=*/call.sp->f == 1 && c.sums == StageChoice::kGather);
        if (rc) return rc;
    }
    rc = launch_main(e, c, call, so_p, stage);
    if (rc) return rc;
    if (longs && e->call.side_join) {   // join: the side queue's last kernel of this stage
        if (e->call.side_join == 1) HIP_TRY(e, hipStreamWaitEvent(e->stream, e->ev_long, 0));
        else if (e->pg.rows.n_giant) HIP_TRY(e, hipStreamWaitEvent(e->stream, e->ev_giant, 0));
    }
    // (every writer of out / logits is now ordered before whatever follows on e->stream: the side queues through the join above,
    // the rounds' dense kernels on the aux stream through launch_main's wait on ev_join)
    if (plan) *plan = describe_stage(e, c, gv);
    return GNNVC_OK;
}

// ---------------------------------------------------------------- the audit (options "audit_*", k_audit_stage / k_audit_any)
// Is this call of a forward entry point audited?  (calls k, 2k, 3k, ... since the period was set)
bool audit_tick(gnnvc_engine *e) {
    if (!e->opt.audit_period) return false;
    return ++e->audit_calls % e->opt.audit_period == 0;
}

// right behind the launches of `stage` (of e->stage_list()) over [lo, hi), on e->stream: the test hook (hook: not when the
// caller owns the buffers, gnnvc_audit_stage_device), then the audit into the call's next record — k_audit_stage for the trained
// shapes, k_audit_any for a generic stage
int audit_stage(gnnvc_engine *e, int stage, uint32_t lo, uint32_t hi, const float *in, float *out, float *logits, std::string &plan,
                bool hook = true) {
    const std::vector<StagePlan> &st = e->stage_list();
    const size_t slot = e->call.audit_pending.size();
    if (slot == 0) {   // the call's first check: its records
        HIP_TRY(e, e->audit_rec.reserve(std::max<size_t>(st.size(), 1) * gnnvc::kAuditWords));
        HIP_TRY(e, hipMemsetAsync(e->audit_rec.p, 0, e->audit_rec.cap * sizeof(unsigned long long), e->stream));
    }
    if (slot >= st.size()) return fail(e, GNNVC_ERR_STATE, "more audited stages than the model has");
    const gnnvc::StagePlan &sp = st[stage];
    if (hook && e->opt.audit_flip_stage == stage && e->opt.audit_flip_row >= lo && e->opt.audit_flip_row < hi)
        HIP_TRY(e, gnnvc::launch_audit_flip(out, (size_t)e->opt.audit_flip_row * (size_t)sp.n3, e->stream));
    const gnnvc::StageCall call = stage_call(e, sp, in, out, sp.sigmoid_last ? logits : nullptr, lo, hi);
    unsigned long long *rec = e->audit_rec.p + slot * gnnvc::kAuditWords;
    if (e->generic_on()) HIP_TRY(e, gnnvc::launch_audit_any(call, rec, /*repair=*/e->opt.audit_repair != 0));
    else HIP_TRY(e, gnnvc::launch_audit_stage(call, rec, /*repair=*/e->opt.audit_repair != 0));
    e->call.audit_pending.push_back(gnnvc_engine::AuditCheck{stage, lo, hi, std::move(plan)});
    return GNNVC_OK;
}

// end of an audited call: one read-back of the records, one stream synchronisation, the verdict
int audit_finish(gnnvc_engine *e, int rc) {
    if (!e->call.audit_now) return rc;
    e->call.audit_now = false;
    std::vector<gnnvc_engine::AuditCheck> checks;
    checks.swap(e->call.audit_pending);
    if (rc != GNNVC_OK || checks.empty()) return rc;
    const size_t words = checks.size() * gnnvc::kAuditWords;
    HIP_TRY(e, e->audit_pin.reserve(std::max(e->stage_list().size(), checks.size()) * gnnvc::kAuditWords));
    HIP_TRY(e, hipMemcpyAsync(e->audit_pin.p, e->audit_rec.p, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    std::string report;
    for (size_t i = 0; i < checks.size(); ++i) {
        const unsigned long long *r = e->audit_pin.p + i * gnnvc::kAuditWords;
        ++e->audit_runs;
        e->audit_nan_pairs += r[1];
        e->audit_repairs += r[2];
        if (r[0] == 0) continue;
        ++e->audit_failures;
        const unsigned long long kc = ~r[3], kf = ~r[4], kp = ~r[5];
        const uint32_t code = (uint32_t)kc;
        if (!report.empty()) continue;   // (the counters take every check; the last_* read-outs and the message the first failing one)
        e->audit_last_stage = checks[i].stage;
        e->audit_last_row = (long)(kc >> 32);
        e->audit_last_col = (long)(code & 63u);
        e->audit_last_mismatches = (long)r[0];
        e->audit_last_fused = (uint32_t)kf;
        e->audit_last_plain = (uint32_t)kp;
        char buf[256];
        snprintf(buf, sizeof buf, "audit: stage %d rows [%u, %u): %llu mismatching values%s; first at row %u column %u%s: fused 0x%08x, audit 0x%08x; ",
                 checks[i].stage, checks[i].lo, checks[i].hi, r[0], r[2] ? " (repaired)" : "", (uint32_t)(kc >> 32), code & 63u,
                 code >= 64u ? " of the logits" : "", (uint32_t)kf, (uint32_t)kp);
        report = std::string(buf) + "plan: " + checks[i].plan;
    }
    if (report.empty()) return GNNVC_OK;
    e->err = report;   // (also where a quiet engine's owner reads it)
    if (e->opt.audit_repair || e->opt.audit_quiet) return GNNVC_OK;
    return GNNVC_ERR_AUDIT;
}

// Layer-by-layer forward on device buffers (any model).
int forward_unfused(gnnvc_engine *e, const float *d_x, float *d_out, float *d_logits) {
    const uint32_t n = e->g.n;
    const size_t cap = ((size_t)n + 1) * (size_t)e->max_width;
    for (auto &s : e->scratch) HIP_TRY(e, s.reserve(cap));
    const float *cur = d_x;
    int wd = e->in_width, pp = 0;
    for (size_t i = 0; i < e->layers.size(); ++i) {
        const Layer &l = e->layers[i];
        const bool last = i + 1 == e->layers.size();
        float *dst = last ? d_out : e->scratch[pp].p;
        switch (l.kind) {
        case kGraph:
            HIP_TRY(e, gnnvc::launch_graph_layer(e->g, e->ws, (uint32_t)wd, cur, dst, e->stream));
            wd = 2 * wd + 3;
            break;
        case kLinear:
            HIP_TRY(e, gnnvc::launch_linear(n, l.k, l.m, cur, e->params.p + l.w_off,
                                            e->params.p + l.b_off, dst, e->stream));
            wd = (int)l.m;
            break;
        case kRelu:
            HIP_TRY(e, gnnvc::launch_relu((size_t)n * wd, cur, dst, e->stream));
            break;
        case kSigmoid:
            if (last && d_logits)
                HIP_TRY(e, hipMemcpyAsync(d_logits, cur, (size_t)n * wd * sizeof(float),
                                          hipMemcpyDeviceToDevice, e->stream));
            HIP_TRY(e, gnnvc::launch_sigmoid((size_t)n * wd, cur, dst, e->stream));
            break;
        }
        cur = dst;
        pp ^= 1;
    }
    return GNNVC_OK;
}

// One generic stage over [lo, hi): one k_stage_any launch — or, on a graph with heavy rows (gnnvc_set_generic_heavy_rows,
// class_heavy_rows), three: the heavy rows' sums a workgroup per row (k_any_heavy_sums), k_stage_any over the light rows, and
// k_stage_any over the listed rows with their sums read back.  Where some of the listed rows are giant
// (gnnvc_set_generic_giant_rows) their chain comes first — k_any_giant_gather, [k_giant_segsum, k_giant_segmap,] k_giant_sum,
// k_any_giant_place, which leaves their sums where the listed rows' launch reads them — and k_any_heavy_sums skips them.  The
// giant chain and then the heavy sums go to the side queue beside the light rows (fork / join as launch_side_rows) or ahead of
// them on the main stream (heavy_overlap()); the listed rows' launch follows all of them.
// live_stage >= 0 (forward_generic only, for a stage live_eligible accepts): the stage's input is examined first — k_any_live_mask,
// k_any_live_pack, on the main stream — and the all-rows / light-rows launch may gather from the table; the heavy and giant rows'
// kernels, on whichever queue, read full rows as ever.
static bool live_eligible(const gnnvc_engine *e, const StagePlan &sp) {
    return e->live_percent != 0 && !sp.dense && sp.f >= 2 && sp.end != gnnvc::kEndNone;
}

int run_generic_stage(gnnvc_engine *e, const StagePlan &sp, const float *in, float *out, float *logits, uint32_t lo, uint32_t hi,
                      int live_stage = -1) {
    if (sp.dense) {   // a dense stage (gnnvc_set_generic_patterns): no neighbour sums, so no row is classed and nothing is split — one launch
        HIP_TRY(e, gnnvc::launch_stage_any(stage_call(e, sp, in, out, logits, lo, hi)));
        return GNNVC_OK;
    }
    {   // (lazily: option "generic_stages" set after the attach, or a threshold that has moved)
        const int rc = class_heavy_rows(e);
        if (rc) return rc;
    }
    gnnvc::StageCall call = stage_call(e, sp, in, out, logits, lo, hi);
    if (live_stage >= 0) {
        call.live_table = e->live_table.p;
        call.live_desc = e->live_desc.p + 2 * (size_t)live_stage;
        HIP_TRY(e, gnnvc::launch_any_live(call, e->live_percent));
    }
    const gnnvc_engine::PerGraph &pg = e->pg;
    e->call.heavy_last_rows = pg.heavy.rows;
    e->call.ggiant_last_rows = pg.heavy.rows ? pg.ggiant.rows : 0;
    e->call.ggiant_last_segmented = e->call.ggiant_last_rows && pg.ggiant.maxseg > 1;
    if (!pg.heavy.rows) {
        HIP_TRY(e, gnnvc::launch_stage_any(call));
        return GNNVC_OK;
    }
    const gnnvc::AnyHeavyRows hr{.list = e->heavy_list.p, .n = pg.heavy.rows, .from = pg.heavy.thresh, .hsum = e->heavy_sum.p,
                                 .below = pg.ggiant.rows ? pg.ggiant.min : 0xFFFFFFFFu};
    const bool side = heavy_overlap() && e->aux_stream;
    gnnvc::StageCall sums = call;
    gnnvc::AnyGiantRows ar;
    if (pg.ggiant.rows) {
        ar.gr.n = pg.ggiant.rows;
        ar.gr.blocks = pg.ggiant.blocks;
        ar.gr.meta = e->ag_meta.p;
        ar.gr.off = e->ag_off.p;
        ar.gr.slab = e->ag_slab.p;
        ar.gr.agg = e->ag_agg.p;
        ar.gr.segsum = pg.ggiant.maxseg > 1 ? e->ag_segsum.p : nullptr;
        ar.gr.segmap = pg.ggiant.maxseg > 1 ? e->ag_segmap.p : nullptr;
        ar.gr.maxseg = pg.ggiant.maxseg;
        ar.pos = e->ag_pos.p;
    }
    const bool gather_first = side && pg.ggiant.rows && giant_gather_first();   // (the gather on the main stream, ahead of the fork)
    if (gather_first) HIP_TRY(e, gnnvc::launch_any_giant(call, ar, hr.hsum, gnnvc::AnyGiantPart::kGather));
    if (side) {
        HIP_TRY(e, hipEventRecord(e->ev_fork, e->stream));
        HIP_TRY(e, hipStreamWaitEvent(e->aux_stream, e->ev_fork, 0));
        sums.stream = e->aux_stream;
    }
    if (pg.ggiant.rows) {
        if (!gather_first) HIP_TRY(e, gnnvc::launch_any_giant(sums, ar, hr.hsum, gnnvc::AnyGiantPart::kGather));
        HIP_TRY(e, gnnvc::launch_giant_sums(ar.gr, (uint32_t)sp.f, lo, hi, sums.stream));
        HIP_TRY(e, gnnvc::launch_any_giant(sums, ar, hr.hsum, gnnvc::AnyGiantPart::kPlace));
    }
    HIP_TRY(e, gnnvc::launch_any_heavy_sums(sums, hr));
    if (side) HIP_TRY(e, hipEventRecord(e->ev_join, e->aux_stream));
    HIP_TRY(e, gnnvc::launch_stage_any(call, gnnvc::AnyRows::kLight, hr));
    if (side) HIP_TRY(e, hipStreamWaitEvent(e->stream, e->ev_join, 0));
    HIP_TRY(e, gnnvc::launch_stage_any(call, gnnvc::AnyRows::kListed, hr));
    return GNNVC_OK;
}

// Forward of a generic-stage model (option "generic_stages"): one k_stage_any launch per stage (three on a graph with heavy rows,
// run_generic_stage), rows ping-ponging through the scratch buffers.  No pad row (the kernels read rows of neighbours only),
// nothing cached between calls but the list of heavy rows.  In an audited call (gnnvc_forward_audited*) each stage's check
// (k_audit_any) is queued right behind its launches.
int forward_generic(gnnvc_engine *e, const float *d_x, float *d_out, float *d_logits) {
    const uint32_t n = e->g.n;
    const std::vector<StagePlan> &st = e->gstages;
    int wmax = 1;
    for (size_t s = 0; s + 1 < st.size(); ++s) wmax = std::max(wmax, st[s].n3);
    if (st.size() > 1)
        for (auto &b : e->scratch) HIP_TRY(e, b.reserve(((size_t)n + 1) * (size_t)wmax));
    // gnnvc_set_generic_live_columns: the table is as wide as the widest eligible stage input; the descriptors start from zero
    // (live_seen[s] is set behind stage s's launches: a forward that fails part-way leaves the stages it never reached unexamined)
    e->live_seen.assign(st.size(), 0);
    int live_wmax = 0;
    for (size_t s = 0; s < st.size(); ++s)
        if (live_eligible(e, st[s])) live_wmax = std::max(live_wmax, st[s].f);
    if (live_wmax) {   // (a descriptor is two 64-bit words of live_desc: sizeof(AnyLiveDesc) == 16, asserted beside the struct)
        HIP_TRY(e, e->live_table.reserve((size_t)n * (size_t)live_wmax));
        HIP_TRY(e, e->live_desc.reserve(2 * st.size()));
        HIP_TRY(e, hipMemsetAsync(e->live_desc.p, 0, 2 * st.size() * sizeof(unsigned long long), e->stream));
        if (e->opt.poison) HIP_TRY(e, hipMemsetAsync(e->live_table.p, 0xFF, (size_t)n * (size_t)live_wmax * sizeof(float), e->stream));
    }
    const float *cur = d_x;
    for (size_t s = 0; s < st.size(); ++s) {
        const bool last = s + 1 == st.size();
        float *dst = last ? d_out : e->scratch[s & 1].p;
        {
            const bool live = live_eligible(e, st[s]);
            const int rc = run_generic_stage(e, st[s], cur, dst, last ? d_logits : nullptr, 0, n, live ? (int)s : -1);
            if (rc != GNNVC_OK) return rc;
            e->live_seen[s] = live ? 1 : 0;
        }
        if (e->call.audit_now) {   // (gnnvc_forward_audited* only: "audit_period" never sets it for a generic-stage model)
            std::string plan = st[s].dense ? "k_stage_any (dense rows)"
                               : e->call.heavy_last_rows ? "k_stage_any (light rows, listed rows) + k_any_heavy_sums" : "k_stage_any";
            if (!st[s].dense && e->call.ggiant_last_rows)
                plan += e->call.ggiant_last_segmented ? " + k_any_giant_gather, k_giant_segsum, k_giant_segmap, k_giant_sum, k_any_giant_place"
                                                 : " + k_any_giant_gather, k_giant_sum, k_any_giant_place";
            if (e->live_seen[s]) plan += " + k_any_live_mask, k_any_live_pack (the live-column table, where the device chose it)";
            const int rc = audit_stage(e, (int)s, 0, n, cur, dst, last ? d_logits : nullptr, plan);
            if (rc != GNNVC_OK) return rc;
        }
        cur = dst;
    }
    return GNNVC_OK;
}

}  // namespace


// ============================================================================ ABI

extern "C" {

int gnnvc_abi_version(void) { return GNNVC_ABI_VERSION; }

const char *gnnvc_strerror(int code) {
    switch (code) {
    case GNNVC_OK: return "ok";
    case GNNVC_ERR_INVALID: return "invalid argument or malformed model";
    case GNNVC_ERR_DEVICE: return "HIP device unavailable or HIP call failed";
    case GNNVC_ERR_NOMEM: return "out of memory";
    case GNNVC_ERR_STATE: return "call out of order";
    case GNNVC_ERR_UNSUPPORTED: return "unsupported model or size";
    case GNNVC_ERR_AUDIT: return "on-device audit found values that differ from the plain recomputation";
    default: return "unknown error";
    }
}

const char *gnnvc_last_error(const gnnvc_engine *e) { return e ? e->err.c_str() : ""; }

int gnnvc_create(gnnvc_engine **out, const char *model_text, size_t len, int device) {
    if (!out || !model_text) return GNNVC_ERR_INVALID;
    *out = nullptr;
    gnnvc_engine *e = new (std::nothrow) gnnvc_engine();
    if (!e) return GNNVC_ERR_NOMEM;
    int rc = GNNVC_OK;
    try {
        e->device = device;
        rc = parse_model(e, model_text, len);
        if (rc == GNNVC_OK) rc = plan_model(e);
        if (rc == GNNVC_OK) {
            int count = 0;
            if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
                rc = fail(e, GNNVC_ERR_DEVICE, "no HIP device %d (found %d) — this engine has no CPU path", device, count);
        }
        if (rc == GNNVC_OK) rc = use_device(e);
        if (rc == GNNVC_OK) {
            if (e->own_stream.create(hipStreamNonBlocking) != hipSuccess)
                rc = fail(e, GNNVC_ERR_DEVICE, "hipStreamCreate failed");
            e->stream = e->own_stream;
        }
        // (creating a stream takes ~10 ms on this stack: the side queues are made here, once per engine, not inside the first
        // hand-off or forward that wants them)
        if (rc == GNNVC_OK) rc = ensure_round_events(e, 0);
        if (rc == GNNVC_OK) rc = upload_params(e);
        // (the page-locked words a forward's verdicts are written to: a pinned allocation is tens of microseconds — here, not in
        // the first forward that asks)
        if (rc == GNNVC_OK && (e->fit_pin.reserve(8) != hipSuccess ||
                               hipHostGetDevicePointer(reinterpret_cast<void **>(&e->fit_dev), e->fit_pin.p, 0) != hipSuccess))
            rc = fail(e, GNNVC_ERR_NOMEM, "page-locked verdict words");
        if (rc == GNNVC_OK && e->ev_fit.create(hipEventDisableTiming) != hipSuccess)
            rc = fail(e, GNNVC_ERR_DEVICE, "hipEventCreate failed");
    } catch (const std::bad_alloc &) {
        rc = GNNVC_ERR_NOMEM;
    } catch (...) {
        rc = GNNVC_ERR_INVALID;
    }
    if (rc != GNNVC_OK) {
        // keep the message reachable for the caller through stderr: there is no engine to ask
        if (!e->err.empty()) fprintf(stderr, "gnnvc_create: %s\n", e->err.c_str());
        gnnvc_destroy(e);
        return rc;
    }
    *out = e;
    return GNNVC_OK;
}

int gnnvc_create_multi(gnnvc_engine **out, const char *model_text, size_t len, const int *devices, int n_devices) {
    if (!out || !model_text || !devices || n_devices < 1) return GNNVC_ERR_INVALID;
    *out = nullptr;
    gnnvc_engine *e = nullptr;
    int rc = gnnvc_create(&e, model_text, len, devices[0]);
    if (rc != GNNVC_OK) return rc;
    std::string err;
    try {
        rc = gnnvc::multi_create(&e->multi, model_text, len, devices, n_devices, /*generic=*/false, nullptr, err);
    } catch (const std::bad_alloc &) {
        rc = GNNVC_ERR_NOMEM;
    } catch (...) {
        rc = GNNVC_ERR_INVALID;
    }
    if (rc != GNNVC_OK) {
        if (!err.empty()) fprintf(stderr, "gnnvc_create_multi: %s\n", err.c_str());
        gnnvc_destroy(e);
        return rc;
    }
    (void)hipSetDevice(devices[0]);
    *out = e;
    return GNNVC_OK;
}

void gnnvc_destroy(gnnvc_engine *e) {
    if (!e) return;
    if (e->multi) {
        gnnvc::multi_destroy(e->multi);
        e->multi = nullptr;
    }
    // nothing of this engine's is in flight any more when its members (gnnvc_device_mem.h) free what they hold
    if (e->own_stream) {
        (void)hipSetDevice(e->device);
        (void)hipStreamSynchronize(e->own_stream);
        if (e->aux_stream) (void)hipStreamSynchronize(e->aux_stream);
    }
    delete e;
}

int gnnvc_set_weight_scale(gnnvc_engine *e, float ws) {
    if (!e) return GNNVC_ERR_INVALID;
    e->ws = ws;
    if (e->multi) return gnnvc::multi_set_weight_scale(e->multi, ws);
    return GNNVC_OK;
}

int gnnvc_set_stream(gnnvc_engine *e, void *hip_stream) {
    if (!e) return GNNVC_ERR_INVALID;
    hipStream_t want = hip_stream ? (hipStream_t)hip_stream : e->own_stream;
    if (want == e->stream) return GNNVC_OK;
    e->stream = want;
    if (e->multi) return GNNVC_OK;
    int rc = use_device(e);
    if (rc) return rc;
    return reprobe_side_streams(e);   // (the side queue has to sit on another hardware queue than THIS stream)
}

int gnnvc_get_stream(gnnvc_engine *e, void **hip_stream) {
    if (!e || !hip_stream) return GNNVC_ERR_INVALID;
    *hip_stream = e->stream;
    return GNNVC_OK;
}

int gnnvc_set_option(gnnvc_engine *e, const char *key, long value) {
    if (!e || !key) return GNNVC_ERR_INVALID;
    if (strncmp(key, "multi_", 6) == 0) {   // the exchange of a multi-device handle (gnnvc_multi.cpp): "multi_pieces", "multi_pack", "multi_push", "multi_only_part"
        if (!e->multi) return fail(e, GNNVC_ERR_INVALID, "option '%s' needs a multi-device handle (gnnvc_create_multi)", key);
        const int rc = gnnvc::multi_set_option(e->multi, key, value);
        return rc ? fail(e, rc, "unknown option '%s'", key) : GNNVC_OK;
    }
    uint32_t fx = 0;   // (the keys, their clamps and their effects: gnnvc_options.h)
    if (!gnnvc::apply_option(e->opt, key, value, &fx)) return fail(e, GNNVC_ERR_INVALID, "unknown option '%s'", key);
    if (fx & gnnvc::kFxShortLists) e->pg.filter.short_from = 0;
    if (fx & gnnvc::kFxForgetPruned)
        for (auto &pp : e->pg.prune) pp = {};
    if (fx & gnnvc::kFxSortedStale)
        for (auto &r : e->pg.sorted) r.valid = false;
    if (fx & gnnvc::kFxAuditRestart) e->audit_calls = 0;
    return (fx & gnnvc::kFxForward) && e->multi ? gnnvc::multi_set_option(e->multi, key, value) : GNNVC_OK;
}

// The bodies of gnnvc_set_generic_big_stages / _feature_width / _patterns behind their refusal on a multi-device handle:
// gnnvc_create_multi_generic applies its config to the front handle through these, never through the public setters.
static int set_big_stages(gnnvc_engine *e, uint32_t lds_bytes);
static int set_feature_width(gnnvc_engine *e, uint32_t max_width);
static int set_patterns(gnnvc_engine *e, uint32_t mask);

int gnnvc_set_generic_heavy_rows(gnnvc_engine *e, uint32_t from_degree) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_set_generic_heavy_rows");
    e->heavy_from = from_degree;   // (the attached graph is classed again by the next generic stage that runs: class_heavy_rows)
    return GNNVC_OK;
}

int gnnvc_set_generic_giant_rows(gnnvc_engine *e, uint32_t from_degree, int segments) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_set_generic_giant_rows");
    e->ggiant_from = from_degree;   // (as above: class_heavy_rows classes the attached graph again when either value has moved)
    e->ggiant_segments = segments;
    return GNNVC_OK;
}

int gnnvc_set_generic_big_stages(gnnvc_engine *e, uint32_t lds_bytes) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_set_generic_big_stages");
    return set_big_stages(e, lds_bytes);
}

static int set_big_stages(gnnvc_engine *e, uint32_t lds_bytes) {
    if (lds_bytes != 0 && (lds_bytes < 65536u || lds_bytes > 163840u))
        return fail(e, GNNVC_ERR_INVALID, "gnnvc_set_generic_big_stages: %u is neither 0 nor within 65536 .. 163840", lds_bytes);
    if (lds_bytes == e->big_lds) return GNNVC_OK;
    if (lds_bytes) {   // the big instantiations' LDS limit on this device: refused here, never inside a forward
        const int rc = use_device(e);
        if (rc) return rc;
        if (gnnvc::allow_big_stages() != hipSuccess) {
            (void)hipGetLastError();
            return fail(e, GNNVC_ERR_UNSUPPORTED, "gnnvc_set_generic_big_stages: the runtime refuses k_stage_any 160 KiB of dynamic LDS on device %d", e->device);
        }
    }
    e->big_lds = lds_bytes;
    plan_generic(e);                // (at once, as option "generic_stages": the stage list and everything the ABI reports of it)
    e->pg.heavy.known = false;      // an attached graph is classed again by the next generic stage that runs (class_heavy_rows)
    return GNNVC_OK;
}

int gnnvc_set_generic_feature_width(gnnvc_engine *e, uint32_t max_width) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_set_generic_feature_width");
    return set_feature_width(e, max_width);
}

static int set_feature_width(gnnvc_engine *e, uint32_t max_width) {
    if (max_width != 0 && (max_width <= (uint32_t)gnnvc::kAnyMaxF || max_width > (uint32_t)gnnvc::kAnyFeatMax))
        return fail(e, GNNVC_ERR_INVALID, "gnnvc_set_generic_feature_width: %u is neither 0 nor within %d .. %d", max_width,
                    gnnvc::kAnyMaxF + 1, gnnvc::kAnyFeatMax);
    if (max_width == e->feat_width) return GNNVC_OK;
    if (max_width) {   // the feat instantiations' LDS limit on this device (a wide stage may be a big one too): refused here, never inside a forward
        const int rc = use_device(e);
        if (rc) return rc;
        if (gnnvc::allow_feat_stages() != hipSuccess) {
            (void)hipGetLastError();
            return fail(e, GNNVC_ERR_UNSUPPORTED, "gnnvc_set_generic_feature_width: the runtime refuses k_stage_any 160 KiB of dynamic LDS on device %d", e->device);
        }
    }
    e->feat_width = max_width;
    plan_generic(e);                // (at once, as gnnvc_set_generic_big_stages)
    e->pg.heavy.known = false;      // an attached graph is classed again by the next generic stage that runs (class_heavy_rows): hsum and the giant slab follow the widest f
    return GNNVC_OK;
}

int gnnvc_set_generic_patterns(gnnvc_engine *e, uint32_t mask) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_set_generic_patterns");
    return set_patterns(e, mask);
}

static int set_patterns(gnnvc_engine *e, uint32_t mask) {
    if (mask & ~(uint32_t)(GNNVC_PATTERN_PROLOGUE | GNNVC_PATTERN_OPEN_END))
        return fail(e, GNNVC_ERR_INVALID, "gnnvc_set_generic_patterns: 0x%x has bits other than GNNVC_PATTERN_PROLOGUE | GNNVC_PATTERN_OPEN_END", mask);
    static_assert(GNNVC_PATTERN_PROLOGUE == gnnvc::kPatternPrologue && GNNVC_PATTERN_OPEN_END == gnnvc::kPatternOpenEnd, "one mask");
    if (mask == e->patterns) return GNNVC_OK;
    e->patterns = mask;             // (no LDS limit to raise: a dense stage outside the default bounds needs the big or feat call, which raise theirs)
    plan_generic(e);                // (at once, as gnnvc_set_generic_big_stages)
    e->pg.heavy.known = false;      // an attached graph is classed again by the next generic graph stage that runs (class_heavy_rows)
    return GNNVC_OK;
}

int gnnvc_set_generic_live_columns(gnnvc_engine *e, uint32_t max_percent) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_set_generic_live_columns");
    if (max_percent > 100u)
        return fail(e, GNNVC_ERR_INVALID, "gnnvc_set_generic_live_columns: %u is not within 0 .. 100", max_percent);
    e->live_percent = max_percent;   // (the next forward's; the stage list is not derived again: nothing is admitted or refused by it)
    return GNNVC_OK;
}

// "generic_live_{kept,used,mask_lo,mask_hi}_<s>": stage s's descriptor of the last forward, copied back now — one copy and one
// wait on the engine's stream; a forward itself copies nothing back.  A stage that forward did not examine: kept -1, used 0, mask 0.
static int live_readout(const gnnvc_engine *e, long s, char what, long *value) {
    unsigned long long d[2] = {0ull, 0ull};
    const bool seen = (size_t)s < e->live_seen.size() && e->live_seen[(size_t)s] && e->live_desc.p;
    if (seen) {
        if (hipSetDevice(e->device) != hipSuccess ||
            hipMemcpyAsync(d, e->live_desc.p + 2 * (size_t)s, sizeof d, hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
            hipStreamSynchronize(e->stream) != hipSuccess) {
            (void)hipGetLastError();
            return GNNVC_ERR_DEVICE;
        }
    }
    switch (what) {
    case 'k': *value = seen ? (long)(uint32_t)d[1] : -1; break;
    case 'u': *value = (long)(uint32_t)(d[1] >> 32); break;
    case 'l': *value = (long)(uint32_t)d[0]; break;
    default: *value = (long)(uint32_t)(d[0] >> 32); break;
    }
    return GNNVC_OK;
}

// gnnvc_create_multi with the generic opt-ins made at creation (the setters stay refused on the handle).  Everything that can be
// refused without a device is refused before one is touched.
int gnnvc_create_multi_generic(gnnvc_engine **out, const char *model_text, size_t len, const int *devices, int n_devices,
                               const gnnvc_generic_config *cfg) {
    if (out) *out = nullptr;
    if (!out || !model_text || !devices || n_devices < 1) return GNNVC_ERR_INVALID;
    gnnvc_generic_config c{(uint32_t)sizeof(gnnvc_generic_config), GNNVC_GENERIC_DEFAULT, GNNVC_GENERIC_DEFAULT, -1, 0, 0, 0};
    if (cfg) {
        if (cfg->size != sizeof(gnnvc_generic_config)) return GNNVC_ERR_INVALID;
        c = *cfg;
    }
    // (what the matching single-device setter would reject; the heavy and giant thresholds and the segments take any value)
    if (c.big_stages_lds != 0 && (c.big_stages_lds < 65536u || c.big_stages_lds > 163840u)) return GNNVC_ERR_INVALID;
    if (c.feature_width != 0 && (c.feature_width <= (uint32_t)gnnvc::kAnyMaxF || c.feature_width > (uint32_t)gnnvc::kAnyFeatMax)) return GNNVC_ERR_INVALID;
    if (c.patterns & ~(uint32_t)(GNNVC_PATTERN_PROLOGUE | GNNVC_PATTERN_OPEN_END)) return GNNVC_ERR_INVALID;
    gnnvc_engine *e = nullptr;
    int rc = gnnvc_create(&e, model_text, len, devices[0]);
    if (rc != GNNVC_OK) return rc;
    // the front handle answers gnnvc_num_stages, gnnvc_stage_widths, "generic_patterns", "generic_stage_layers_<s>" ... as a single
    // engine with the same settings would (a model of the trained shape keeps its own plans: the config has no effect on it)
    if (e->stages.empty()) {
        if (c.heavy_rows != GNNVC_GENERIC_DEFAULT) e->heavy_from = c.heavy_rows;
        if (c.giant_rows != GNNVC_GENERIC_DEFAULT) e->ggiant_from = c.giant_rows;
        e->ggiant_segments = c.giant_segments;
        if (rc == GNNVC_OK && c.big_stages_lds) rc = set_big_stages(e, c.big_stages_lds);
        if (rc == GNNVC_OK && c.feature_width) rc = set_feature_width(e, c.feature_width);
        if (rc == GNNVC_OK && c.patterns) rc = set_patterns(e, c.patterns);
    }
    std::string err;
    if (rc == GNNVC_OK) {
        try {
            rc = gnnvc::multi_create(&e->multi, model_text, len, devices, n_devices, /*generic=*/true, &c, err);
        } catch (const std::bad_alloc &) {
            rc = GNNVC_ERR_NOMEM;
        } catch (...) {
            rc = GNNVC_ERR_INVALID;
        }
    } else {
        err = e->err;
    }
    if (rc != GNNVC_OK) {
        if (!err.empty()) fprintf(stderr, "gnnvc_create_multi_generic: %s\n", err.c_str());
        gnnvc_destroy(e);
        return rc;
    }
    (void)hipSetDevice(devices[0]);
    *out = e;
    return GNNVC_OK;
}

// "<prefix><s>" of a generic model: the stage index, or -1 (no such stage, not a number, the model is not generic)
static long generic_stage_index(const gnnvc_engine *e, const std::string &k, size_t prefix_len) {
    const char *num = k.c_str() + prefix_len;
    char *end = nullptr;
    const long s = strtol(num, &end, 10);
    if (!e->generic_on() || *num < '0' || *num > '9' || *end != 0 || s >= (long)e->gstages.size()) return -1;
    return s;
}

int gnnvc_get_info(const gnnvc_engine *e, const char *key, long *value) {
    if (!e || !key || !value) return GNNVC_ERR_INVALID;
    const std::string k(key);
    if (k == "devices") *value = e->multi ? gnnvc::multi_devices(e->multi) : 1;
    else if (e->multi && (k.rfind("part_rows_", 0) == 0 || k.rfind("part_entries_", 0) == 0)) {   // "part_rows_<r>", "part_entries_<r>"
        const int r = atoi(k.c_str() + k.rfind('_') + 1);
        uint32_t lo = 0, hi = 0;
        uint64_t en = 0;
        if (gnnvc::multi_part_info(e->multi, r, &lo, &hi, &en) != GNNVC_OK) return GNNVC_ERR_INVALID;
        *value = k[5] == 'r' ? (long)(hi - lo) : (long)en;
    }
    else if (e->multi && k.rfind("audit_", 0) == 0) {   // the parts' audits (gnnvc_multi.cpp)
        if (!gnnvc::multi_audit_info(e->multi, key, value)) return GNNVC_ERR_INVALID;
    }
    else if (e->multi && gnnvc::multi_is_generic(e->multi) &&   // the parts' classings summed (the front itself holds no graph)
             (k == "generic_heavy_rows" || k == "generic_heavy_entries" || k == "generic_giant_rows" || k == "generic_giant_entries")) {
        if (!gnnvc::multi_sum_info(e->multi, key, value)) return GNNVC_ERR_INVALID;
    }
    else if (k == "generic_stages" || k == "plans_at_handoff" || k == "mfma_dense") (void)gnnvc::read_option(e->opt, key, value);   // (as set)
    else if (backward_info(e, k, value)) {}   // the backward pass's read-outs, spelled out where it lives (gnnvc_backward.cpp)
    else if (plan_info(e, k, value)) {}       // ... and the plans' (gnnvc_plans.cpp)
    else if (k == "generic_stages_model") *value = e->generic_on() ? 1 : 0;   // would a forward run k_stage_any now
    else if (k == "generic_stages_active") *value = e->generic_ran ? 1 : 0;   // did the last one
    else if (k == "generic_max_dense_layers") *value = gnnvc::kMaxDenseLayers;
    else if (k == "generic_heavy_from") *value = (long)e->heavy_from;                 // gnnvc_set_generic_heavy_rows
    else if (k == "generic_heavy_rows") *value = (long)e->pg.heavy.rows;              // the attached graph's last classing
    else if (k == "generic_heavy_entries") *value = (long)e->pg.heavy.entries;
    else if (k == "generic_heavy_last_rows") *value = (long)e->call.heavy_last_rows;       // 0: the last call launched one kernel a stage
    else if (k == "generic_giant_from") *value = (long)e->ggiant_from;                // gnnvc_set_generic_giant_rows
    else if (k == "generic_giant_segments") *value = (long)e->ggiant_segments;        // as stored: -1 | 0 | 1 (or whatever was passed)
    else if (k == "generic_giant_rows") *value = (long)e->pg.ggiant.rows;              // the attached graph's last classing
    else if (k == "generic_giant_entries") *value = (long)e->pg.ggiant.entries;
    else if (k == "generic_giant_last_rows") *value = (long)e->call.ggiant_last_rows;
    else if (k == "generic_giant_last_segmented") *value = e->call.ggiant_last_segmented ? 1 : 0;
    else if (k.rfind("generic_stage_layers_", 0) == 0) {   // "generic_stage_layers_<s>": dense layers of stage s of a generic model
        const long s = generic_stage_index(e, k, sizeof("generic_stage_layers_") - 1);
        if (s < 0) return GNNVC_ERR_INVALID;
        *value = e->gstages[(size_t)s].nd;
    }
    else if (k == "generic_big_lds") *value = (long)e->big_lds;                       // gnnvc_set_generic_big_stages, as set
    else if (k == "generic_feature_width") *value = (long)e->feat_width;              // gnnvc_set_generic_feature_width, as set
    else if (k == "generic_patterns") *value = (long)e->patterns;                     // gnnvc_set_generic_patterns, as set
    else if (k == "generic_live_columns") *value = (long)e->live_percent;             // gnnvc_set_generic_live_columns, as set
    else if (k.rfind("generic_live_kept_", 0) == 0 || k.rfind("generic_live_used_", 0) == 0 || k.rfind("generic_live_mask_lo_", 0) == 0 ||
             k.rfind("generic_live_mask_hi_", 0) == 0) {      // the last forward's verdict on stage s, read back from the device
        const char what = k[13] == 'k' ? 'k' : k[13] == 'u' ? 'u' : k[18] == 'l' ? 'l' : 'h';
        const size_t prefix = what == 'k' ? sizeof("generic_live_kept_") - 1 : what == 'u' ? sizeof("generic_live_used_") - 1
                              : sizeof("generic_live_mask_lo_") - 1;   // (mask_lo and mask_hi: the same length)
        const long s = generic_stage_index(e, k, prefix);
        if (s < 0) return GNNVC_ERR_INVALID;
        return live_readout(e, s, what, value);
    }
    else if (k.rfind("generic_stage_dense_", 0) == 0) {       // "generic_stage_dense_<s>": 1 = stage s has no graph layer (a prologue)
        const long s = generic_stage_index(e, k, sizeof("generic_stage_dense_") - 1);
        if (s < 0) return GNNVC_ERR_INVALID;
        *value = e->gstages[(size_t)s].dense ? 1 : 0;
    }
    else if (k.rfind("generic_stage_end_", 0) == 0) {         // "generic_stage_end_<s>": 0 = it ends in a ReLU, 1 = in the sigmoid, 2 = in its bare linear layer
        const long s = generic_stage_index(e, k, sizeof("generic_stage_end_") - 1);
        if (s < 0) return GNNVC_ERR_INVALID;
        *value = e->gstages[(size_t)s].end;
    }
    else if (k.rfind("generic_stage_lds_bytes_", 0) == 0) {   // "generic_stage_lds_bytes_<s>": the stage's LDS layout at 256 threads
        const long s = generic_stage_index(e, k, sizeof("generic_stage_lds_bytes_") - 1);
        if (s < 0) return GNNVC_ERR_INVALID;
        *value = (long)gnnvc::stage_any_route(e->gstages[(size_t)s]).lds256;
    }
    else if (k.rfind("generic_stage_threads_", 0) == 0) {     // "generic_stage_threads_<s>": the workgroup size its launches use
        const long s = generic_stage_index(e, k, sizeof("generic_stage_threads_") - 1);
        if (s < 0) return GNNVC_ERR_INVALID;
        *value = gnnvc::stage_any_route(e->gstages[(size_t)s]).threads;
    }
    else if (k == "audit_runs") *value = (long)e->audit_runs;
    else if (k == "audit_failures") *value = (long)e->audit_failures;
    else if (k == "audit_repairs") *value = (long)e->audit_repairs;
    else if (k == "audit_nan_pairs") *value = (long)e->audit_nan_pairs;
    else if (k == "audit_last_stage") *value = e->audit_last_stage;
    else if (k == "audit_last_row") *value = e->audit_last_row;
    else if (k == "audit_last_col") *value = e->audit_last_col;
    else if (k == "audit_last_mismatches") *value = e->audit_last_mismatches;
    else if (k == "audit_last_fused_bits") *value = (long)e->audit_last_fused;
    else if (k == "audit_last_plain_bits") *value = (long)e->audit_last_plain;
    else if (k == "multi_last_forward_us") *value = e->multi ? (long)(gnnvc::multi_last_forward_ms(e->multi) * 1000.0) : 0;
    else if (k.rfind("multi_", 0) == 0) {
        if (!e->multi || !gnnvc::multi_get_info(e->multi, key, value)) return GNNVC_ERR_INVALID;
    }
    else if (k == "dense_skip_layers") {   // bit 3 s + l: dense layer l + 1 of fused stage s may leave out its zero terms (the model's weights allow it)
        *value = 0;
        for (size_t s = 0; s < e->stages.size() && s < 10; ++s) *value |= (long)(e->stages[s].skip_ok & 7u) << (3 * s);
    }
    else if (k == "compact_gather_active") *value = e->pg.c4.ready ? 1 : 0;
    else if (k == "compact_gather_chunks") *value = e->pg.c4.ready ? (long)e->pg.c4.chunks : 0;
    else if (k == "compact_gather_block_cols") *value = e->pg.c4.ready ? (long)e->pg.c4.block : 0;
    else if (k == "compact_gather_rows_per_chunk") *value = e->pg.c4.ready ? (long)e->pg.c4.rows : 0;
    else if (k == "compact_gather_steps") *value = e->pg.c4.ready ? (long)e->pg.c4.steps_total : 0;
    else if (k == "pruned_stage1" || k == "pruned_stage2") *value = e->pg.prune[k.back() - '0'].ready ? 1 : 0;
    else if (k == "side_queue_probes") *value = e->side_probes;
    else if (k == "side_queue_runs_beside") *value = e->side_beside ? 1 : 0;
    else if (k == "long_entries_percent") *value = e->pg.rows.n_long && e->g.nnz ? (long)(e->pg.rows.long_entries * 100ull / e->g.nnz) : 0;
    else if (k == "filtered_stage1" || k == "filtered_stage2") *value = e->pg.filter.filtered[k.back() - '0'] ? 1 : 0;
    else if (k == "short_lists_stage1" || k == "short_lists_stage2") *value = e->pg.filter.short_used[k.back() - '0'] ? 1 : 0;
    else if (k == "filter_mass_percent_stage1" || k == "filter_mass_percent_stage2") {   // (diagnostic: reads the device's counters back)
        const int st = k.back() - '0';
        *value = -1;
        if (e->pg.filter.filtered[st] && e->filter_info.p && e->g.nnz) {
            unsigned long long info[2] = {0, 0};
            if (hipStreamSynchronize(e->stream) != hipSuccess ||
                hipMemcpy(info, e->filter_info.p + 4 * st, sizeof info, hipMemcpyDeviceToHost) != hipSuccess)
                return GNNVC_ERR_DEVICE;
            *value = (long)(info[0] * 100ull / e->g.nnz);
        }
    }
    else if (k == "pruned_vertices_stage1" || k == "pruned_vertices_stage2") *value = e->pg.prune[k.back() - '0'].ready ? (long)e->pg.prune[k.back() - '0'].members : 0;
    else if (k == "pruned_entries_stage1" || k == "pruned_entries_stage2") *value = e->pg.prune[k.back() - '0'].ready ? (long)e->pg.prune[k.back() - '0'].kept : 0;
    else if (k == "pruned_predicted_stage1") *value = e->pg.prune[1].ready && e->pg.prune[1].predicted ? 1 : 0;
    else if (k == "pruned_borrowed_stage2") *value = e->pg.filter.borrowed[2] ? 1 : 0;
    else if (k == "pruned_from_previous_stage2") *value = e->pg.prune[2].ready && e->pg.prune[2].from_prev ? 1 : 0;
    else if (k == "pruned_last_ok_stage1" || k == "pruned_last_ok_stage2") {
        // did the last call of that stage use its pruned adjacency?  (waits for the stream; tests and tools)
        const int st = k.back() - '0';
        *value = 0;
        if (e->pg.prune[st].ready || e->pg.filter.borrowed[st]) {
            uint32_t bad = 1;
            if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess ||
                hipMemcpy(&bad, e->prune_flags.p + st, sizeof bad, hipMemcpyDeviceToHost) != hipSuccess)
                return GNNVC_ERR_DEVICE;
            *value = bad == 0 ? 1 : 0;
        }
    }
    else if (k == "wide_tiles_used") *value = e->pg.wide_used ? 1 : 0;   // (did any stage since the graph was handed over run on wide tiles)
    else if (k == "table_tiles_active") *value = e->pg.t4.ok ? 1 : 0;
    else if (k == "table_tiles_fit_stage1" || k == "table_tiles_fit_stage2") {   // did the last forward's stage run on the table?  (waits for the stream)
        *value = 0;
        if (e->pg.t4.ok && e->t4.desc.p) {
            uint32_t fit = 0;
            gnnvc_engine *m = const_cast<gnnvc_engine *>(e);
            if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess ||
                hipMemcpy(&fit, m->t4.desc_of(k.back() - '0', e->t4.parity) + 8, sizeof fit, hipMemcpyDeviceToHost) != hipSuccess)
                return GNNVC_ERR_DEVICE;
            *value = (long)fit;
        }
    }
    else if (k == "lds_table_off") *value = e->pg.lt.off ? 1 : 0;
    else if (k == "lds_table_bits") *value = e->pg.lt.ready ? (long)e->pg.lt.bits : 0;
    else if (k == "compact_gather_off_stage1" || k == "compact_gather_off_stage2") *value = e->pg.c4.stage_off[k.back() - '0'] ? 1 : 0;
    else if (k == "compact_gather_blocks") *value = e->pg.c4.ready ? (long)e->pg.c4.nblocks : 0;
    else if (k == "compact_gather_last_ok" || k == "compact_gather_last_dirty" || k == "compact_gather_last_passes" ||
             k == "compact_table_written_by_producer") {
        // what the device decided at the last launch of the plan (waits for the stream; for tests and tools)
        *value = 0;
        if (e->pg.c4.ready && e->c4.desc.p) {
            uint32_t d[8] = {0};
            if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess ||
                hipMemcpy(d, e->c4.desc.p + e->pg.c4.last_desc, sizeof d, hipMemcpyDeviceToHost) != hipSuccess)
                return GNNVC_ERR_DEVICE;
            if (k == "compact_table_written_by_producer") *value = (d[0] && !d[6]) ? 1 : 0;   // (no compaction pass was needed)
            else *value = k == "compact_gather_last_ok" ? (d[0] ? 1 : 0) : (k == "compact_gather_last_passes" ? (long)d[0] : (long)d[5]);
        }
    }
    else if (k == "plan_memsets_last_forward") *value = (long)e->pg.plan_memsets;
    else if (k == "lds_table_active") *value = e->pg.lt.ready ? 1 : 0;
    else if (k == "lds_table_last_ok") {   // did the last forward's input fit the table?  (waits for the stream; tests and tools)
        *value = 0;
        if (e->pg.lt.ready && e->lt.bad.p) {
            uint32_t bad = 1;
            if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess ||
                hipMemcpy(&bad, e->lt.bad.p, sizeof bad, hipMemcpyDeviceToHost) != hipSuccess)
                return GNNVC_ERR_DEVICE;
            *value = bad == 0 ? 1 : 0;
        }
    }
    else if (k == "lds_table_mapped") *value = e->pg.lt.ready && e->pg.lt.mapped ? 1 : 0;
    else if (k == "lds_table_blocks") *value = e->pg.lt.ready ? (long)e->pg.lt.blocks : 0;
    else if (k == "lds_table_chunks") *value = e->pg.lt.ready ? (long)e->pg.lt.chunks : 0;
    else if (k == "lds_table_steps") *value = e->pg.lt.ready ? (long)e->pg.lt.steps_total : 0;
    else if (k == "blocked_stage0_active") *value = e->pg.blk.ready ? 1 : 0;
    else if (k == "blocked_blocks") *value = e->pg.blk.ready ? (long)e->pg.blk.count : 0;
    else if (k == "block_cols") *value = e->pg.blk.ready ? (long)e->pg.blk.cols : 0;
    else if (k == "long_rows") *value = (long)e->pg.rows.n_long;
    else if (k == "plan_build_us") *value = (long)(e->pg.plan_build_ms * 1000.0);
    else if (k == "handoff_build_us") *value = (long)(e->pg.handoff_build_ms * 1000.0);
    else if (k == "handoff_early_us") *value = (long)(e->pg.early_ms * 1000.0);
    else if (k == "graph_uses") *value = (long)e->pg.graph_uses;
    else if (k == "slice_rows") *value = e->pg.empty_slice ? 0 : (long)(e->g.hi() - e->g.lo());
    else if (k == "slice_entries") *value = (long)e->g.nnz;
    else if (k == "giant_rows") *value = (long)e->pg.rows.n_giant;
    else if (k == "giant_segments") *value = e->pg.rows.n_giant ? (long)e->pg.rows.maxseg : 0;
    else if (k == "giant_entries") *value = (long)e->pg.rows.giant_entries;
    else if (k == "giant_row_threshold") *value = e->pg.rows.n_giant ? (long)e->pg.rows.giant_thresh : 0;
    else if (k == "sorted_tiles_active") *value = e->pg.rows.sorted_wanted ? 1 : 0;
    else if (k == "tile_waste_x100") *value = (long)(e->pg.rows.waste * 100.0);
    else if (k == "heavy_tail_x1000") *value = (long)(e->pg.rows.tail * 1000.0);
    else if (k == "interleaved_tiles") *value = e->pg.rows.interleave ? 1 : 0;
    else if (k == "long_row_threshold") *value = e->pg.rows.n_long ? (long)e->pg.rows.long_thresh : 0;
    else return GNNVC_ERR_INVALID;
    return GNNVC_OK;
}

int gnnvc_num_layers(const gnnvc_engine *e) { return e ? (int)e->layers.size() : GNNVC_ERR_INVALID; }
int gnnvc_is_fused(const gnnvc_engine *e) { return e ? (e->stage_list().empty() ? 0 : 1) : GNNVC_ERR_INVALID; }
int gnnvc_in_width(const gnnvc_engine *e) { return e ? e->in_width : GNNVC_ERR_INVALID; }
int gnnvc_out_width(const gnnvc_engine *e) { return e ? e->out_width : GNNVC_ERR_INVALID; }
int gnnvc_num_stages(const gnnvc_engine *e) { return e ? (int)e->stage_list().size() : GNNVC_ERR_INVALID; }

int gnnvc_stage_widths(const gnnvc_engine *e, int stage, int *in_width, int *out_width) {
    if (!e || stage < 0 || stage >= (int)e->stage_list().size()) return GNNVC_ERR_INVALID;
    if (in_width) *in_width = e->stage_list()[stage].f;
    if (out_width) *out_width = e->stage_list()[stage].n3;
    return GNNVC_OK;
}

// Common tail of the host hand-offs: device-side sanity checks of the arrays now in
// e->rowptr/col/w/nw, then make them the engine's graph.
// Slices of an open plan build whose rows' column entries lie inside the first `sent` entries of the column array (rp: the
// HOST copy of the row pointers the hand-off was given).
extern "C++" {
template <class RP>
static uint32_t slices_arrived(const gnnvc_engine::PlanBuild &pb, const RP *rp, uint32_t n, uint64_t sent) {
    uint32_t lo = 0, hi = pb.slices;   // largest s with rp[min(n, base + s * slice_rows)] <= sent
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        const uint64_t row = std::min<uint64_t>(n, (uint64_t)pb.base + (uint64_t)mid * pb.slice_rows);
        if ((uint64_t)rp[row] <= sent) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
}   // extern "C++"


// the first `sent` column entries are on their way (queued on e->stream): regroup the slices they complete, on the second stream
extern "C++" {
template <class RP>
static int handoff_progress(gnnvc_engine *e, const RP *rp, uint32_t n, uint64_t sent) {
    if (!e->early_open || (!e->pg.lt.pb.open && !e->pg.c4.pb.open)) return GNNVC_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t lt_to = e->pg.lt.pb.open ? slices_arrived(e->pg.lt.pb, rp, n, sent) : 0u;
    const uint32_t c4_to = e->pg.c4.pb.open ? slices_arrived(e->pg.c4.pb, rp, n, sent) : 0u;
    if ((e->pg.lt.pb.open && lt_to > e->pg.lt.pb.done) || (e->pg.c4.pb.open && c4_to > e->pg.c4.pb.done)) {
        HIP_TRY(e, hipEventRecord(e->ev_piece, e->stream));
        HIP_TRY(e, hipStreamWaitEvent(e->aux_stream, e->ev_piece, 0));
        int rc = lt_advance(e, lt_to, e->aux_stream);
        if (rc == GNNVC_OK) rc = c4_advance(e, c4_to, e->aux_stream);
        if (rc) return rc;
    }
    e->pg.early_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GNNVC_OK;
}
}   // extern "C++"

static int adopt_uploaded(gnnvc_engine *e, uint32_t n, uint64_t nnz) {
    if (e->early_open) {   // whatever the second stream still regroups has to be done before the plans are finished on this one
        HIP_TRY(e, hipEventRecord(e->ev_piece, e->aux_stream));
        HIP_TRY(e, hipStreamWaitEvent(e->stream, e->ev_piece, 0));
    }
    {
        const GraphDev cand{n, nnz, e->rowptr.p, e->col.p, e->w.p, e->nw.p};
        uint32_t bad = 0;
        if (e->early_open) {   // (the graph was classed when its row pointers arrived: only the checks are left)
            HIP_TRY(e, gnnvc::validate_graph(cand, e->blk.flag.p, e->stream));
            HIP_TRY(e, hipMemcpyAsync(&bad, e->blk.flag.p, sizeof bad, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(e, hipStreamSynchronize(e->stream));
        } else {
            const int rc0 = classify_hand_off(e, cand, bad);
            if (rc0) return rc0;
        }
        if (bad) {
            e->have_graph = false;
            if (e->early_open) {   // plans begun from this graph's arrays: worthless
                e->early_open = false;
                reset_graph_state(e);
            }
            return fail(e, GNNVC_ERR_INVALID, "%s", (bad & 1u) ? "a column id is not a vertex of this graph (col[i] >= n)"
                                                                 : "row pointers are not monotone from 0 to nnz");
        }
    }
    const bool early = e->early_open;   // the graph was classed and its plans begun while the column array was arriving
    e->early_open = false;
    e->g = GraphDev{n, nnz, e->rowptr.p, e->col.p, e->w.p, e->nw.p};
    e->have_graph = true;
    e->pg.empty_slice = false;
    e->pg.der_open = false;   // (a derivation begun against the previous graph must not be committed against this one)
    int rc = reserve_features(e, n);
    if (rc) return rc;
    if (!early) {
        reset_graph_state(e);
        e->pre_armed = true;
        rc = find_long(e);
        if (rc) return rc;
    }
    return prepare_plans(e);   // ... which is why what depends on the graph alone is built here, not in a later forward
}

int gnnvc_upload_graph(gnnvc_engine *e, uint32_t n, const uint64_t *rowptr, const uint32_t *col,
                       const uint32_t *w, const uint32_t *nw) {
    if (!e) return GNNVC_ERR_INVALID;
    if (n && (!rowptr || !w || !nw)) return fail(e, GNNVC_ERR_INVALID, "null graph arrays");
    int rc = use_device(e);
    if (rc) return rc;
    if (e->multi) {
        if (n && rowptr[n] && !col) return fail(e, GNNVC_ERR_INVALID, "null column array");
        std::string err;
        rc = gnnvc::multi_upload(e->multi, n, rowptr, nullptr, col, w, nw, err);
        (void)hipSetDevice(e->device);
        if (rc) return fail(e, rc, "%s", err.c_str());
        e->have_graph = false;   // (the front itself holds no graph: the parts do)
        return reserve_multi_front(e, n);
    }
    const uint64_t nnz = n ? rowptr[n] : 0;
    if (nnz >= 0xFFFFFFFFull - GNNVC_COL_PAD)
        return fail(e, GNNVC_ERR_UNSUPPORTED, "nnz %llu does not fit 32-bit row pointers", (unsigned long long)nnz);
    if (nnz && !col) return fail(e, GNNVC_ERR_INVALID, "null column array");
    e->pg.der_open = false;
    HIP_TRY(e, e->rowptr.reserve((size_t)n + 1));
    HIP_TRY(e, e->col.reserve(nnz + GNNVC_COL_PAD));
    HIP_TRY(e, e->w.reserve(n));
    HIP_TRY(e, e->nw.reserve(n));
    HIP_TRY(e, e->blk.flag.reserve(1));
    // stream-ordered behind earlier forwards; the uint64 row pointers are staged in the scratch
    // buffer and narrowed on the device, and the sanity checks run there too (a host pass over
    // 2e8 column ids costs more than the copy)
    HIP_TRY(e, e->scratch[0].reserve(((size_t)n + 1) * 2));
    if (n) {
        HIP_TRY(e, hipMemcpyAsync(e->scratch[0].p, rowptr, ((size_t)n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(e, gnnvc::narrow_rowptr(e->scratch[0].p, e->rowptr.p, (size_t)n + 1, e->stream));
        HIP_TRY(e, hipMemcpyAsync(e->w.p, w, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(e, hipMemcpyAsync(e->nw.p, nw, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    } else {
        HIP_TRY(e, hipMemsetAsync(e->rowptr.p, 0, sizeof(uint32_t), e->stream));
    }
    e->early_open = e->early_declined = false;
    rc = handoff_early(e, n, nnz);   // (large graphs: classed now, plans begun — see handoff_early)
    if (rc) {
        e->early_open = false;
        reset_graph_state(e);
        return rc;
    }
    if (e->early_open && (e->pg.lt.pb.open || e->pg.c4.pb.open)) {
        // the column array in pieces: while piece k + 1 crosses the bus the second stream regroups the slices piece k completed
        const uint64_t piece = 16ull << 20;
        for (uint64_t at = 0; at < nnz; at += piece) {
            const uint64_t cnt = std::min(piece, nnz - at);
            HIP_TRY(e, hipMemcpyAsync(e->col.p + at, col + at, cnt * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
            rc = handoff_progress(e, rowptr, n, at + cnt);
            if (rc) return rc;
        }
    } else if (nnz) {
        HIP_TRY(e, hipMemcpyAsync(e->col.p, col, nnz * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    }
    HIP_TRY(e, hipMemsetAsync(e->col.p + nnz, 0, GNNVC_COL_PAD * sizeof(uint32_t), e->stream));
    return adopt_uploaded(e, n, nnz);
}

/* ---- staged hand-off --------------------------------------------------------
 * The reference's driver hands predict a freshly mutated graph every call (src/GNN_VC.cpp:171-192)
 * whose adjacency lives in scattered ranges of one big array (include/reduction_graph.hpp:29-36),
 * so the host has to pack it.  Packing straight into page-locked memory owned by the engine saves
 * the allocation + zero fill + page faults of a temporary CSR and the bounce copy of a pageable
 * upload, and finished pieces of the column array go out while the host packs the next. */
int gnnvc_graph_staging(gnnvc_engine *e, uint32_t n, uint64_t nnz, uint32_t **rowptr, uint32_t **col,
                        uint32_t **w, uint32_t **nw) {
    if (!e) return GNNVC_ERR_INVALID;
    if (nnz >= 0xFFFFFFFFull - GNNVC_COL_PAD)
        return fail(e, GNNVC_ERR_UNSUPPORTED, "nnz %llu does not fit 32-bit row pointers", (unsigned long long)nnz);
    int rc = use_device(e);
    if (rc) return rc;
    if (e->staging && e->staged_sent && (n != e->staged_n || nnz != e->staged_nnz))
        return fail(e, GNNVC_ERR_STATE, "staging resized after columns were sent");
    HIP_TRY(e, e->pin_rowptr.reserve((size_t)n + 1));
    HIP_TRY(e, e->pin_w.reserve(n));
    HIP_TRY(e, e->pin_nw.reserve(n));
    HIP_TRY(e, e->pin_col.reserve(nnz));
    e->staged_n = n;
    e->staged_nnz = nnz;
    if (!e->staging) {
        e->staged_sent = 0;
        e->early_open = e->early_declined = false;
    }
    e->staging = true;
    if (rowptr) *rowptr = e->pin_rowptr.p;
    if (col) *col = e->pin_col.p;
    if (w) *w = e->pin_w.p;
    if (nw) *nw = e->pin_nw.p;
    return GNNVC_OK;
}

int gnnvc_staged_columns_ready(gnnvc_engine *e, uint64_t first, uint64_t count) {
    if (!e) return GNNVC_ERR_INVALID;
    if (!e->staging) return fail(e, GNNVC_ERR_STATE, "no graph is being staged");
    if (first != e->staged_sent || first + count > e->staged_nnz)
        return fail(e, GNNVC_ERR_INVALID, "column pieces must be announced in order (expected offset %llu)",
                    (unsigned long long)e->staged_sent);
    if (!count) return GNNVC_OK;
    if (e->multi) {   // (the slices are cut when the whole graph is known: nothing leaves before the commit)
        e->staged_sent = first + count;
        return GNNVC_OK;
    }
    int rc = use_device(e);
    if (rc) return rc;
    if (!e->staged_sent) {   // first piece: the device array is about to be overwritten
        e->have_graph = false;
        e->pg.der_open = false;
        HIP_TRY(e, e->col.reserve(e->staged_nnz + GNNVC_COL_PAD));
    }
    HIP_TRY(e, hipMemcpyAsync(e->col.p + first, e->pin_col.p + first, count * sizeof(uint32_t), hipMemcpyHostToDevice,
                              e->stream));
    e->staged_sent = first + count;
    // Large graphs: the row pointers and weights are final by now (step 1 of the protocol) — they go out, the graph is classed
    // and its plans begun, and from here on every announced piece lets the second stream regroup the slices it completes.
    if (!e->early_open && !e->early_declined && e->opt.handoff && e->staged_n &&
        (e->opt.handoff >= 2 || e->staged_nnz >= e->opt.handoff_min_nnz) && e->pin_rowptr.p[e->staged_n] == e->staged_nnz) {
        const uint32_t n = e->staged_n;
        HIP_TRY(e, e->rowptr.reserve((size_t)n + 1));
        HIP_TRY(e, e->w.reserve(n));
        HIP_TRY(e, e->nw.reserve(n));
        HIP_TRY(e, hipMemcpyAsync(e->rowptr.p, e->pin_rowptr.p, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(e, hipMemcpyAsync(e->w.p, e->pin_w.p, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(e, hipMemcpyAsync(e->nw.p, e->pin_nw.p, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        rc = handoff_early(e, n, e->staged_nnz);
    }
    if (rc == GNNVC_OK) rc = handoff_progress(e, e->pin_rowptr.p, e->staged_n, e->staged_sent);
    if (rc) {   // (e.g. row pointers the early builders must not see: the hand-off is over, the staging memory can be reused)
        e->staging = false;
        e->staged_sent = 0;
        e->early_open = false;
        reset_graph_state(e);
    }
    return rc;
}

int gnnvc_commit_staged_graph(gnnvc_engine *e) {
    if (!e) return GNNVC_ERR_INVALID;
    if (!e->staging) return fail(e, GNNVC_ERR_STATE, "no graph is being staged");
    int rc = use_device(e);
    if (rc) return rc;
    const uint32_t n = e->staged_n;
    const uint64_t nnz = e->staged_nnz;
    e->staging = false;
    e->have_graph = false;
    if (n && e->pin_rowptr.p[n] != nnz) return fail(e, GNNVC_ERR_INVALID, "staged rowptr[n] differs from the staged nnz");
    if (e->multi) {
        e->staged_sent = 0;
        std::string err;
        rc = gnnvc::multi_upload(e->multi, n, nullptr, e->pin_rowptr.p, e->pin_col.p, e->pin_w.p, e->pin_nw.p, err);
        (void)hipSetDevice(e->device);
        if (rc) return fail(e, rc, "%s", err.c_str());
        return reserve_multi_front(e, n);
    }
    HIP_TRY(e, e->rowptr.reserve((size_t)n + 1));
    HIP_TRY(e, e->col.reserve(nnz + GNNVC_COL_PAD));
    HIP_TRY(e, e->w.reserve(n));
    HIP_TRY(e, e->nw.reserve(n));
    HIP_TRY(e, e->blk.flag.reserve(1));
    if (n && !e->early_open) {   // (an early hand-off sent them with its first piece)
        HIP_TRY(e, hipMemcpyAsync(e->rowptr.p, e->pin_rowptr.p, ((size_t)n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(e, hipMemcpyAsync(e->w.p, e->pin_w.p, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(e, hipMemcpyAsync(e->nw.p, e->pin_nw.p, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    } else if (!n) {
        HIP_TRY(e, hipMemsetAsync(e->rowptr.p, 0, sizeof(uint32_t), e->stream));
    }
    if (nnz > e->staged_sent)
        HIP_TRY(e, hipMemcpyAsync(e->col.p + e->staged_sent, e->pin_col.p + e->staged_sent,
                                  (nnz - e->staged_sent) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    e->staged_sent = 0;
    HIP_TRY(e, hipMemsetAsync(e->col.p + nnz, 0, GNNVC_COL_PAD * sizeof(uint32_t), e->stream));
    return adopt_uploaded(e, n, nnz);
}

static int attach_common(gnnvc_engine *e, const GraphDev &cand) {
    {   // a column id >= n would send the gather to a wild address: check before accepting the graph — and, in the same pass of
        // the stream, learn what find_long is about to ask (classify_hand_off: one wait instead of four)
        uint32_t bad = 0;
        const int rc0 = classify_hand_off(e, cand, bad);
        if (rc0) return rc0;
        if (bad) {
            e->have_graph = false;
            return fail(e, GNNVC_ERR_INVALID, "%s", (bad & 1u) ? "a column id is not a vertex of this graph (col[i] >= n)"
                                                                 : "row pointers are not monotone from 0 to nnz");
        }
    }
    e->g = cand;
    e->have_graph = true;
    e->pg.empty_slice = false;
    e->pg.der_open = false;
    int rc = reserve_features(e, cand.n);
    if (rc) return rc;
    // (a staged hand-off that opened the early builders may have been abandoned or refused before its commit: nothing of it —
    // open plan builds with the OLD graph's geometry least of all — may reach prepare_plans with this graph)
    reset_graph_state(e);
    e->early_open = e->early_declined = false;
    e->pre_armed = true;
    rc = find_long(e);
    if (rc) return rc;
    return prepare_plans(e);   // ... which is why what depends on the graph alone is built here, not in a later forward
}

/* ---- the next graph derived from the resident one ---------------------------------------------
 * See the k_derive_* kernels: the device keeps the CSR of the last hand-off; the caller says which old row every vertex
 * of the next graph was (or that it is new) and how long its list is now, learns how many trailing entries per row the
 * device cannot derive, ships exactly those, and the engine assembles the next CSR in place of an upload of all of it. */
int gnnvc_derive_graph_begin(gnnvc_engine *e, uint32_t n_new, const uint32_t *old_row, const uint32_t *rowptr_new, uint32_t *tail) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_derive_graph_begin");
    e->pg.der_open = false;
    if (!e->have_graph || e->g.rowptr != e->rowptr.p || e->g.col != e->col.p || e->g.sliced() || e->pg.empty_slice)
        return fail(e, GNNVC_ERR_STATE, "no engine-owned whole graph is resident (hand one over with gnnvc_upload_graph or the staged calls first)");
    if (n_new && (!old_row || !rowptr_new || !tail)) return fail(e, GNNVC_ERR_INVALID, "null arrays");
    int rc = use_device(e);
    if (rc) return rc;
    const uint64_t nnz_new = n_new ? rowptr_new[n_new] : 0;
    if (n_new && rowptr_new[0] != 0) return fail(e, GNNVC_ERR_INVALID, "rowptr_new[0] != 0");
    if (nnz_new >= 0xFFFFFFFFull - GNNVC_COL_PAD) return fail(e, GNNVC_ERR_UNSUPPORTED, "nnz too large");
    HIP_TRY(e, e->der_old_row.reserve(n_new));
    HIP_TRY(e, e->rowptr2.reserve((size_t)n_new + 1));
    HIP_TRY(e, e->der_new_of.reserve(std::max<uint32_t>(e->g.n, 1u)));
    HIP_TRY(e, e->der_tail.reserve(n_new));
    HIP_TRY(e, e->blk.flag.reserve(1));
    if (n_new) {
        HIP_TRY(e, hipMemcpyAsync(e->der_old_row.p, old_row, (size_t)n_new * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(e, hipMemcpyAsync(e->rowptr2.p, rowptr_new, ((size_t)n_new + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    } else {
        HIP_TRY(e, hipMemsetAsync(e->rowptr2.p, 0, sizeof(uint32_t), e->stream));
    }
    HIP_TRY(e, gnnvc::derive_tails(e->g, e->der_old_row.p, n_new, e->rowptr2.p, e->der_new_of.p, e->der_tail.p, e->blk.flag.p, e->stream));
    uint32_t bad = 0;
    if (n_new) HIP_TRY(e, hipMemcpyAsync(tail, e->der_tail.p, (size_t)n_new * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(&bad, e->blk.flag.p, sizeof bad, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if (bad)
        return fail(e, GNNVC_ERR_INVALID, "%s", (bad & 1u) ? "old_row[] names a row the resident graph does not have"
                                                 : (bad & 2u) ? "two vertices of the next graph claim the same old row"
                                                              : "a row has more surviving old neighbours than its new degree: not derived from the resident graph");
    e->der_tail_host.assign(tail, tail + n_new);
    uint64_t total = 0;
    for (uint32_t u = 0; u < n_new; ++u) total += tail[u];
    e->pg.der_n_new = n_new;
    e->pg.der_nnz_new = nnz_new;
    e->pg.der_tail_total = total;
    e->pg.der_open = true;
    return GNNVC_OK;
}

int gnnvc_derive_graph_commit(gnnvc_engine *e, const uint32_t *tail_cols, uint64_t n_tail, const uint32_t *w, const uint32_t *nw) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_derive_graph_commit");
    if (!e->pg.der_open) return fail(e, GNNVC_ERR_STATE, "gnnvc_derive_graph_begin first");
    e->pg.der_open = false;
    e->early_open = e->early_declined = false;   // (an abandoned staged hand-off must not pass for this graph's)
    if (!e->have_graph || e->g.rowptr != e->rowptr.p || e->g.col != e->col.p || e->g.sliced() || e->pg.empty_slice)
        return fail(e, GNNVC_ERR_STATE, "the resident graph changed since gnnvc_derive_graph_begin");
    const uint32_t n = e->pg.der_n_new;
    if (n_tail != e->pg.der_tail_total) return fail(e, GNNVC_ERR_INVALID, "expected %llu tail entries, got %llu",
                                                 (unsigned long long)e->pg.der_tail_total, (unsigned long long)n_tail);
    if ((n_tail && !tail_cols) || (n && (!w || !nw))) return fail(e, GNNVC_ERR_INVALID, "null arrays");
    int rc = use_device(e);
    if (rc) return rc;
    std::vector<uint32_t> tptr((size_t)n + 1, 0);
    for (uint32_t u = 0; u < n; ++u) tptr[u + 1] = tptr[u] + e->der_tail_host[u];
    HIP_TRY(e, e->der_tailptr.reserve((size_t)n + 1));
    HIP_TRY(e, e->der_tailcols.reserve(std::max<uint64_t>(n_tail, 1)));
    HIP_TRY(e, e->col2.reserve(e->pg.der_nnz_new + GNNVC_COL_PAD));
    HIP_TRY(e, hipMemcpy(e->der_tailptr.p, tptr.data(), tptr.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (n_tail) HIP_TRY(e, hipMemcpyAsync(e->der_tailcols.p, tail_cols, n_tail * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, gnnvc::derive_fill(e->g, e->der_old_row.p, e->der_new_of.p, e->rowptr2.p, e->der_tailptr.p, e->der_tailcols.p, n,
                                  e->col2.p, e->stream));
    HIP_TRY(e, hipMemsetAsync(e->col2.p + e->pg.der_nnz_new, 0, GNNVC_COL_PAD * sizeof(uint32_t), e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));   // (the old arrays are about to change hands)
    std::swap(e->rowptr, e->rowptr2);
    std::swap(e->col, e->col2);
    e->have_graph = false;
    HIP_TRY(e, e->w.reserve(n));
    HIP_TRY(e, e->nw.reserve(n));
    if (n) {
        HIP_TRY(e, hipMemcpyAsync(e->w.p, w, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(e, hipMemcpyAsync(e->nw.p, nw, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    }
    return adopt_uploaded(e, n, e->pg.der_nnz_new);
}

int gnnvc_graph_row_hashes(gnnvc_engine *e, uint64_t *hashes) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_graph_row_hashes");
    if (!e->have_graph || e->pg.empty_slice) return fail(e, GNNVC_ERR_STATE, "no graph attached");
    const uint32_t rows = e->g.hi() - e->g.lo();
    if (!rows) return GNNVC_OK;
    if (!hashes) return fail(e, GNNVC_ERR_INVALID, "null output");
    int rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(e, e->hash_buf.reserve(rows));
    HIP_TRY(e, gnnvc::row_hashes(e->g, e->hash_buf.p, e->stream));
    HIP_TRY(e, hipMemcpyAsync(hashes, e->hash_buf.p, (size_t)rows * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return GNNVC_OK;
}

int gnnvc_attach_graph_device(gnnvc_engine *e, uint32_t n, uint64_t nnz, const uint32_t *d_rowptr,
                              const uint32_t *d_col, const uint32_t *d_w, const uint32_t *d_nw) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_attach_graph_device");
    if (n && (!d_rowptr || !d_col || !d_w || !d_nw)) return fail(e, GNNVC_ERR_INVALID, "null device graph arrays");
    if (nnz >= 0xFFFFFFFFull - GNNVC_COL_PAD) return fail(e, GNNVC_ERR_UNSUPPORTED, "nnz too large");
    int rc = use_device(e);
    if (rc) return rc;
    return attach_common(e, GraphDev{n, nnz, d_rowptr, d_col, d_w, d_nw});
}

int gnnvc_attach_graph_slice(gnnvc_engine *e, uint32_t n_global, uint32_t row_lo, uint32_t row_hi, uint64_t nnz_local,
                             const uint32_t *d_rowptr_local, const uint32_t *d_col_local, const uint32_t *d_w_local,
                             const uint32_t *d_nw_local) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_attach_graph_slice");
    if (row_lo > row_hi || row_hi > n_global) return fail(e, GNNVC_ERR_INVALID, "slice [%u, %u) outside a graph of %u vertices", row_lo, row_hi, n_global);
    if (!d_rowptr_local || !d_col_local || (row_hi > row_lo && (!d_w_local || !d_nw_local)))
        return fail(e, GNNVC_ERR_INVALID, "null device graph arrays");
    if (nnz_local >= 0xFFFFFFFFull - GNNVC_COL_PAD) return fail(e, GNNVC_ERR_UNSUPPORTED, "nnz too large");
    int rc = use_device(e);
    if (rc) return rc;
    // the kernels index rowptr / w / nw by GLOBAL row id: bias the slice's arrays so that they can (only rows of the
    // slice are ever touched — every whole-graph pass of the engine walks [row_base, row_end))
    GraphDev cand{n_global, nnz_local, d_rowptr_local - row_lo, d_col_local, d_w_local - row_lo, d_nw_local - row_lo};
    cand.row_base = row_lo;
    cand.row_end = row_hi ? row_hi : 0;
    if (row_lo == 0 && row_hi == n_global) cand.row_end = 0;   // the whole graph after all
    e->pg.der_open = false;
    if (row_hi == row_lo) {   // an empty slice: nothing to compute, nothing to index — and nothing of the previous graph's
        e->g = cand;
        e->g.row_end = row_hi;
        if (row_hi == 0) e->g.nnz = 0;   // (at the front)
        e->have_graph = true;
        reset_graph_state(e);
        e->pg.empty_slice = true;
        return GNNVC_OK;
    }
    return attach_common(e, cand);
}

static void audit_log_line(const gnnvc_engine *e, int rc);

int gnnvc_stage_forward_device(gnnvc_engine *e, int stage, uint32_t row_lo, uint32_t row_hi,
                               const float *d_in, float *d_out, float *d_logits) {
    if (!e) return GNNVC_ERR_INVALID;
    const bool audit = audit_tick(e);
    NOT_ON_MULTI(e, "gnnvc_stage_forward_device");
    if (!e->have_graph) return fail(e, GNNVC_ERR_STATE, "no graph attached");
    if (stage < 0 || stage >= (int)e->stage_list().size()) return fail(e, GNNVC_ERR_INVALID, "stage %d out of range", stage);
    if (row_lo > row_hi || row_hi > e->g.n) return fail(e, GNNVC_ERR_INVALID, "row range [%u,%u) outside graph of %u", row_lo, row_hi, e->g.n);
    if (row_lo == row_hi) return GNNVC_OK;
    if (e->pg.empty_slice || row_lo < e->g.lo() || row_hi > e->g.hi())
        return fail(e, GNNVC_ERR_INVALID, "rows [%u,%u) are not in the slice [%u,%u) this engine holds", row_lo, row_hi, e->g.lo(),
                    e->pg.empty_slice ? e->g.lo() : e->g.hi());
    if (!d_in || !d_out) return fail(e, GNNVC_ERR_INVALID, "null feature buffers");
    int rc = use_device(e);
    if (rc) return rc;
    e->call.heavy_last_rows = 0;
    e->call.ggiant_last_rows = 0;
    e->call.ggiant_last_segmented = false;
    if (e->generic_on()) {   // (k_stage_any, with k_any_heavy_sums on a graph with heavy rows; a generic stage audits nothing)
        const StagePlan &sp = e->gstages[stage];
        return run_generic_stage(e, sp, d_in, d_out, sp.sigmoid_last ? d_logits : nullptr, row_lo, row_hi);
    }
    if (!audit) return run_stage(e, stage, row_lo, row_hi, d_in, d_out, d_logits);
    e->call.audit_now = true;
    std::string plan;
    rc = run_stage(e, stage, row_lo, row_hi, d_in, d_out, d_logits, false, &plan);
    if (rc == GNNVC_OK) rc = audit_stage(e, stage, row_lo, row_hi, d_in, d_out, d_logits, plan);
    rc = audit_finish(e, rc);
    if (e->opt.audit_log) audit_log_line(e, rc);
    return rc;
}

// A pure check of the caller's buffers: no stage runs, the test hook does not apply, the period's counter is not ticked
int gnnvc_audit_stage_device(gnnvc_engine *e, int stage, uint32_t row_lo, uint32_t row_hi, const float *d_in, float *d_out,
                             float *d_logits) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_audit_stage_device");
    if (!e->have_graph) return fail(e, GNNVC_ERR_STATE, "no graph attached");
    if (stage < 0 || stage >= (int)e->stage_list().size()) return fail(e, GNNVC_ERR_INVALID, "stage %d out of range", stage);
    if (row_lo > row_hi || row_hi > e->g.n) return fail(e, GNNVC_ERR_INVALID, "row range [%u,%u) outside graph of %u", row_lo, row_hi, e->g.n);
    if (row_lo == row_hi) return GNNVC_OK;
    if (e->pg.empty_slice || row_lo < e->g.lo() || row_hi > e->g.hi())
        return fail(e, GNNVC_ERR_INVALID, "rows [%u,%u) are not in the slice [%u,%u) this engine holds", row_lo, row_hi, e->g.lo(),
                    e->pg.empty_slice ? e->g.lo() : e->g.hi());
    if (!d_in || !d_out) return fail(e, GNNVC_ERR_INVALID, "null feature buffers");
    int rc = use_device(e);
    if (rc) return rc;
    e->call.audit_pending.clear();
    e->call.audit_now = true;
    std::string plan = e->generic_on() ? "the caller's buffers (k_stage_any's, if gnnvc_stage_forward_device filled them)" : "the caller's buffers";
    rc = audit_stage(e, stage, row_lo, row_hi, d_in, d_out, d_logits, plan, /*hook=*/false);
    rc = audit_finish(e, rc);
    if (e->opt.audit_log) audit_log_line(e, rc);
    return rc;
}

static int forward_single(gnnvc_engine *e, const float *d_x, float *d_scores, float *d_logits);

// option "audit_log": one stderr line per audited call with the engine's counters (for drivers that cannot read them)
static void audit_log_line(const gnnvc_engine *e, int rc) {
    long runs = 0, failures = 0, repairs = 0;
    (void)gnnvc_get_info(e, "audit_runs", &runs);
    (void)gnnvc_get_info(e, "audit_failures", &failures);
    (void)gnnvc_get_info(e, "audit_repairs", &repairs);
    fprintf(stderr, "gnnvc audit: audit_runs %ld audit_failures %ld audit_repairs %ld%s%s\n", runs, failures, repairs,
            rc == GNNVC_ERR_AUDIT ? " — " : "", rc == GNNVC_ERR_AUDIT ? e->err.c_str() : "");
}

// gnnvc_forward_device (audit = this call's turn by "audit_period") and gnnvc_forward_audited_device (explicit = true: every
// fused stage audited in this call, generic stages included)
static int forward_device_impl(gnnvc_engine *e, const float *d_x, float *d_scores, float *d_logits, bool audit, bool explicit_audit) {
    if (e->multi) {   // pointers on the first device; complete (every device drained) when it returns
        if (!gnnvc::multi_has_graph(e->multi)) return fail(e, GNNVC_ERR_STATE, "no graph attached");
        if (gnnvc::multi_vertices(e->multi) == 0) return GNNVC_OK;
        if (!d_x || !d_scores) return fail(e, GNNVC_ERR_INVALID, "null feature buffers");
        int rc = use_device(e);
        if (rc) return rc;
        HIP_TRY(e, hipStreamSynchronize(e->stream));   // (whatever produced d_x on this handle's stream)
        std::string err;
        // (generic parts audit on demand only, as a single generic engine: "audit_period" audits nothing on such a handle)
        if (gnnvc::multi_is_generic(e->multi)) audit = explicit_audit;
        rc = gnnvc::multi_forward_device(e->multi, d_x, d_scores, d_logits, audit, err);
        (void)hipSetDevice(e->device);
        if (rc) rc = fail(e, rc, "%s", err.c_str());
        if (audit && e->opt.audit_log) audit_log_line(e, rc);
        return rc;
    }
    if (explicit_audit) {
        if (!e->have_graph) return fail(e, GNNVC_ERR_STATE, "no graph attached");
        if (e->layers.empty()) return fail(e, GNNVC_ERR_STATE, "engine was created without a model");
        if (e->stage_list().empty()) return fail(e, GNNVC_ERR_UNSUPPORTED, "model is not fused into stages: there is nothing to audit");
        e->call.audit_now = true;
    } else {
        // (an unfused model runs the layer-by-layer kernels, a generic-stage model k_stage_any: the period audits nothing)
        e->call.audit_now = audit && !e->stages.empty() && !e->generic_on();
    }
    const int rc = audit_finish(e, forward_single(e, d_x, d_scores, d_logits));
    if (audit && e->opt.audit_log) audit_log_line(e, rc);
    return rc;
}

int gnnvc_forward_device(gnnvc_engine *e, const float *d_x, float *d_scores, float *d_logits) {
    if (!e) return GNNVC_ERR_INVALID;
    return forward_device_impl(e, d_x, d_scores, d_logits, audit_tick(e), /*explicit_audit=*/false);
}

int gnnvc_forward_audited_device(gnnvc_engine *e, const float *d_x, float *d_scores, float *d_logits) {
    if (!e) return GNNVC_ERR_INVALID;
    return forward_device_impl(e, d_x, d_scores, d_logits, /*audit=*/true, /*explicit_audit=*/true);   // (the period's counter is not ticked)
}

static int forward_single(gnnvc_engine *e, const float *d_x, float *d_scores, float *d_logits) {
    if (!e->have_graph) return fail(e, GNNVC_ERR_STATE, "no graph attached");
    const uint32_t n = e->g.n;
    e->ev_count = 0;
    e->live_seen.clear();   // ("generic_live_*_<s>": what THIS forward examines, forward_generic)
    if (e->layers.empty()) return fail(e, GNNVC_ERR_STATE, "engine was created without a model");
    if (n == 0) return GNNVC_OK;
    if (e->g.sliced() || e->pg.empty_slice)
        return fail(e, GNNVC_ERR_STATE, "this engine holds a slice of the graph: run it stage by stage (gnnvc_stage_forward_device)");
    if (!d_x || !d_scores) return fail(e, GNNVC_ERR_INVALID, "null feature buffers");
    int rc = use_device(e);
    if (rc) return rc;
    e->pg.plan_memsets = 0;
    e->pg.c4.elided_last = 0;
    e->generic_ran = e->generic_on();
    e->call.heavy_last_rows = 0;
    e->call.ggiant_last_rows = 0;
    e->call.ggiant_last_segmented = false;   // (run_generic_stage sets it)
    if (e->generic_ran || e->stages.empty()) {
        rc = ensure_events(e, 2);
        if (rc) return rc;
        if (e->opt.timing >= 1) HIP_TRY(e, hipEventRecord(e->ev[0], e->stream));
        rc = e->generic_ran ? forward_generic(e, d_x, d_scores, d_logits) : forward_unfused(e, d_x, d_scores, d_logits);
        if (rc) return rc;
        if (e->opt.timing >= 1) HIP_TRY(e, hipEventRecord(e->ev[1], e->stream));
        e->ev_count = e->opt.timing >= 1 ? 2 : 0;
        e->ev_stages = false;
        return GNNVC_OK;
    }
    const size_t ns = e->stages.size();
    rc = ensure_events(e, ns + 1);
    if (rc) return rc;
    const float *cur = d_x;   // (the pad rows of e->h were zeroed when the graph was handed over: reserve_features)
    e->call.c4_fused_for = -1;
    e->pg.c4.prepared_stage = -1;
    if (e->pg.c4.fit_pending && hipEventQuery(e->ev_fit) == hipSuccess) {   // the previous forward's verdicts have arrived
        e->pg.c4.fit_pending = false;
        const uint32_t before = e->pg.lt.unfit_runs + e->pg.t4.unfit_runs + e->pg.c4.unfit_runs[1] + e->pg.c4.unfit_runs[2];
        const bool seen1 = e->pg.t4.fit_seen[1], seen2 = e->pg.t4.fit_seen[2];
        if (e->pg.lt.used && e->pg.lt.ready) {
            e->pg.lt.unfit_runs = e->fit_pin.p[2] != 0u ? e->pg.lt.unfit_runs + 1 : 0u;
            if (e->pg.lt.unfit_runs >= (e->pg.lt.mapped ? 1u : 3u)) e->pg.lt.off = true;
        }
        if (e->pg.t4.used && e->pg.t4.ok) {
            // table tiles: a graph whose first 16-wide stage keeps missing (more than four live columns: sparse graphs) stops paying
            // for the counters, the choice and the launches that leave at once — the first forward on a graph always misses (nobody
            // has chosen columns yet), hence four in a row
            e->pg.t4.unfit_runs = e->fit_pin.p[3] == 0u ? e->pg.t4.unfit_runs + 1 : 0u;
            if (e->pg.t4.unfit_runs >= 4u) e->pg.t4.ok = false;
            // a stage whose table fit the last forward seen gets no gathering kernel behind it (k_stage_t4's solo mode copes with
            // the rare forward that does not fit after all)
            e->pg.t4.fit_seen[1] = e->fit_pin.p[3] != 0u;
            e->pg.t4.fit_seen[2] = e->fit_pin.p[4] != 0u;
        }
        bool elide_moved = false;
        for (int s = 1; s <= 2; ++s) {
            if (!e->pg.c4.fit_used[s]) continue;
            // (elided rows: was the producer's table taken as written?  k_c4_choose's word, whatever else became of the stage)
            const bool ok = e->fit_pin.p[4 + s] != 0u;
            elide_moved = elide_moved || ok != e->pg.c4.elide_ok[s];
            e->pg.c4.elide_ok[s] = ok;
            // (a stage whose statistics were to come from a producer that itself fell back had no chance: not its miss)
            if (s == 2 && e->pg.c4.fit_used[1] && e->fit_pin.p[0] == 0u) continue;
            e->pg.c4.unfit_runs[s] = e->fit_pin.p[s - 1] == 0u ? e->pg.c4.unfit_runs[s] + 1 : 0u;
            if (e->pg.c4.unfit_runs[s] >= 3u) e->pg.c4.stage_off[s] = true;
        }
        const uint32_t after = e->pg.lt.unfit_runs + e->pg.t4.unfit_runs + e->pg.c4.unfit_runs[1] + e->pg.c4.unfit_runs[2];
        const bool calm = after == 0u && before == 0u && seen1 == e->pg.t4.fit_seen[1] && seen2 == e->pg.t4.fit_seen[2] && !elide_moved;
        e->pg.c4.fit_calm = calm ? e->pg.c4.fit_calm + 1u : 0u;
    }
    if (!e->pg.c4.fit_pending) {
        for (int s = 0; s < 4; ++s) e->pg.c4.fit_used[s] = false;
        e->pg.lt.used = false;
        e->pg.t4.used = false;
    }
    struct SinkGuard {   // the thread-local sink never outlives this call, whichever way it returns
        ~SinkGuard() { gnnvc::set_kernel_trace(nullptr); }
    } sink_guard;
    if (e->opt.ktrace && e->ktrace.used < 16384) {   // records pile up over forwards until gnnvc_kernel_trace reads them
        e->ktrace.stream = e->stream;
        gnnvc::set_kernel_trace(&e->ktrace);
    }
    // Table tiles are offered from a graph's SECOND forward on — or from its first, when the engine carries a choice of columns
    // over from its previous graph: a fresh engine's first forward on a graph has no table to gather from, and the counting, the
    // choice and the launches that leave at once would only cost the caller who scores the graph once (ER-100K: 0.14 vs 0.11 ms).
    e->call.t4_now = e->pg.t4.ok && (e->t4.choice_live || e->pg.graph_uses >= 1);
    // Events (option "forward_timing"): none by default — a record costs the stream ~1.8 us, four of them were 5.5 us of a small
    // graph's 31 - 82 us forward (scratch/experiments/r4_gaps.sh) — 1 = the forward's first and last, 2 = one per stage as well.
    // (ev[0] is also what the first-forward plan build on the second stream waits for, below.)
    const bool build_under_stage0 = ns >= 2 && !e->pg.c4.tried && !e->pg.c4.range_mode && e->aux_stream && e->pg.rows.n_long == 0 && !e->pg.rows.sorted_wanted &&
                                    e->opt.compact_first_entries && e->g.nnz >= e->opt.compact_first_entries;
    if (e->opt.timing >= 1 || build_under_stage0) HIP_TRY(e, hipEventRecord(e->ev[0], e->stream));
    if (e->opt.poison)   // (tests, fuzz: rows 0 .. n - 1 of both feature buffers; the pad row n stays zero)
        for (size_t b = 0; b + 1 < ns && b < 2; ++b) HIP_TRY(e, hipMemsetAsync(e->h[b].p, 0xFF, (size_t)n * 16 * sizeof(float), e->stream));
    for (size_t s = 0; s < ns; ++s) {
        const bool last = s + 1 == ns;
        float *dst = last ? d_scores : e->h[s & 1].p;
        std::string plan;
        rc = run_stage(e, (int)s, 0, n, cur, dst, last ? d_logits : nullptr, /*in_forward=*/true, e->call.audit_now ? &plan : nullptr);
        if (rc) break;
        if (e->call.audit_now && (rc = audit_stage(e, (int)s, 0, n, cur, dst, last ? d_logits : nullptr, plan)) != GNNVC_OK) break;
        if ((e->opt.timing >= 2 || (last && e->opt.timing == 1)) && hipEventRecord(e->ev[s + 1], e->stream) != hipSuccess) { rc = fail(e, GNNVC_ERR_DEVICE, "hipEventRecord failed"); break; }
        if (s == 0 && build_under_stage0 && !e->pg.c4.tried) {
            // A large graph's first forward: the compact-table plan of the stages to come depends on the graph alone — it is
            // built now, on the second stream, under the kernels of stage 0 that were just queued (the build synchronises with
            // its own stream only; it is complete when it returns).
            // (behind whatever the caller had queued before this forward — it may still be writing the graph's arrays)
            HIP_TRY(e, hipStreamWaitEvent(e->aux_stream, e->ev[0], 0));
            hipStream_t main_stream = e->stream;
            e->stream = e->aux_stream;
            rc = build_compact(e);
            e->stream = main_stream;
            if (rc) break;
        }
        cur = dst;
    }
    gnnvc::set_kernel_trace(nullptr);
    if (rc) return rc;
    if (e->call.t4_now) {   // (the descriptors this forward's table tiles wrote are the next forward's specs)
        e->t4.parity ^= 1u;
        e->t4.choice_live = true;
    }
    e->ev_count = e->opt.timing >= 1 ? (int)ns + 1 : 0;
    e->ev_stages = e->opt.timing >= 2;
    const bool c4_verdicts = (e->pg.c4.fit_used[1] || e->pg.c4.fit_used[2]) && e->pg.c4.ready && e->c4.desc.p;
    const bool lt_verdict = e->pg.lt.used && e->pg.lt.ready && e->lt.bad.p;
    const bool t4_verdict = e->call.t4_now && e->t4.desc.p;
    if (t4_verdict && !e->pg.c4.fit_pending) e->pg.t4.used = true;
    if (!e->pg.c4.fit_pending && (c4_verdicts || lt_verdict || t4_verdict)) {   // this forward's verdicts, written out behind it
        // ONE small kernel stores the words into page-locked host memory (round 4: they were up to five 4-byte hipMemcpyAsync, ~20 us
        // of a small graph's forward + wait, scratch/experiments/r4_gaps.sh), and once four verdicts in a row have changed nothing
        // only every eighth forward asks — a verdict steers which kernels the NEXT forwards launch, never a result: every plan
        // proves its input on the device in every call.
        const bool ask = e->pg.c4.fit_calm < 4u || (++e->pg.c4.fit_skip % e->opt.verdict_period) == 0u;
        if (!ask) {
            if (!c4_verdicts) for (int s = 1; s <= 2; ++s) e->pg.c4.fit_used[s] = false;
            return GNNVC_OK;
        }
        if (!e->ev_fit) HIP_TRY(e, e->ev_fit.create(hipEventDisableTiming));
        if (!e->fit_dev) {
            HIP_TRY(e, e->fit_pin.reserve(8));
            HIP_TRY(e, hipHostGetDevicePointer(reinterpret_cast<void **>(&e->fit_dev), e->fit_pin.p, 0));
        }
        gnnvc::VerdictWords vw;
        if (c4_verdicts)
            for (int s = 1; s <= 2; ++s) {
                vw.src[s - 1] = e->c4.desc.p + gnnvc_engine::kDescWords * (s - 1);
                if (e->c4.elide.p) vw.src[4 + s] = e->c4.elide.p + gnnvc::kElideWords * (s - 1) + 5;
            }
        else
            for (int s = 1; s <= 2; ++s) e->pg.c4.fit_used[s] = false;
        if (lt_verdict) vw.src[2] = e->lt.bad.p;
        if (t4_verdict)   // (the parity has flipped: the descriptors this forward wrote are the current ones)
            for (int s = 1; s <= 2; ++s) vw.src[2 + s] = e->t4.desc_of(s, e->t4.parity) + 8;
        HIP_TRY(e, gnnvc::write_verdicts(vw, e->fit_dev, e->stream));
        HIP_TRY(e, hipEventRecord(e->ev_fit, e->stream));
        e->pg.c4.fit_pending = true;
    }
    return GNNVC_OK;
}

int gnnvc_stage_input_ready(gnnvc_engine *e, int stage, const float *d_in, uint32_t row_lo, uint32_t row_hi) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_stage_input_ready");
    if (!e->have_graph) return fail(e, GNNVC_ERR_STATE, "no graph attached");
    if (e->stages.empty()) return fail(e, GNNVC_ERR_UNSUPPORTED, "model is not fused into stages");
    if (stage < 1 || stage >= (int)e->stages.size()) return fail(e, GNNVC_ERR_INVALID, "stage %d has no 16-wide input", stage);
    if (row_lo > row_hi || row_hi > e->g.n) return fail(e, GNNVC_ERR_INVALID, "row range [%u, %u) outside the graph", row_lo, row_hi);
    e->pg.c4.prepared_stage = -1;
    if (e->g.n == 0 || row_lo == row_hi || e->pg.empty_slice) return GNNVC_OK;
    if (!d_in) return fail(e, GNNVC_ERR_INVALID, "null feature buffer");
    int rc = use_device(e);
    if (rc) return rc;
    const bool same_range = e->pg.c4.range_mode && e->pg.c4.tried && e->pg.c4.base == row_lo && e->pg.c4.end == row_hi;
    e->pg.c4.range_mode = true;
    if (!same_range) {
        rc = build_compact(e, row_lo, row_hi);
        if (rc) return rc;
        if (!e->pg.c4.ready) {   // remember what was tried, so that the next forward does not try again
            e->pg.c4.base = row_lo;
            e->pg.c4.end = row_hi;
        }
    }
    if (!e->pg.c4.ready || e->pg.rows.n_long > 0) return GNNVC_OK;   // the plan does not apply to this graph: nothing to prepare
    uint32_t *desc = e->c4.desc.p + gnnvc_engine::kDescWords * (stage - 1);
    e->pg.c4.last_desc = gnnvc_engine::kDescWords * (stage - 1);
    HIP_TRY(e, gnnvc::column_counts(d_in, e->g.n, e->c4.counts.p, e->stream));
    HIP_TRY(e, gnnvc::launch_compact_gather(e->g, compact_plan(e), d_in, e->c4.counts.p, 1, desc, e->c4.table.p, e->c4.acc.p, e->pg.c4.base,
                                            e->pg.c4.end, e->c4.dirty.p, e->pg.c4.dirty_cap, e->c4.agg16.p, e->stream, /*what=*/1));
    e->pg.c4.prepared_stage = stage;
    e->pg.c4.prepared_in = d_in;
    return GNNVC_OK;
}

// gnnvc_forward, and gnnvc_forward_audited (audited = true)
static int forward_host(gnnvc_engine *e, const float *x, float *scores, float *logits, bool audited) {
    const auto device_forward = audited ? gnnvc_forward_audited_device : gnnvc_forward_device;
    if (e->multi) {
        if (!gnnvc::multi_has_graph(e->multi)) return fail(e, GNNVC_ERR_STATE, "no graph attached");
        const uint32_t n = gnnvc::multi_vertices(e->multi);
        if (n == 0) return GNNVC_OK;
        if (!x || !scores) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
        int rc = use_device(e);
        if (rc) return rc;
        const size_t in_b = (size_t)n * e->in_width * sizeof(float);   // (1 x 1 for the trained model; a generic model's own widths)
        const size_t out_b = (size_t)n * e->out_width * sizeof(float);
        HIP_TRY(e, hipMemcpyAsync(e->x.p, x, in_b, hipMemcpyHostToDevice, e->stream));
        const bool want_logits = logits && e->ends_in_sigmoid;
        rc = device_forward(e, e->x.p, e->scores.p, want_logits ? e->logits.p : nullptr);
        if (rc && rc != GNNVC_ERR_AUDIT) return rc;   // (a failed audit: the outputs as the fused path wrote them, and the error)
        HIP_TRY(e, hipMemcpyAsync(scores, e->scores.p, out_b, hipMemcpyDeviceToHost, e->stream));
        if (want_logits) HIP_TRY(e, hipMemcpyAsync(logits, e->logits.p, out_b, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(e, hipStreamSynchronize(e->stream));
        return rc;
    }
    if (!e->have_graph) return fail(e, GNNVC_ERR_STATE, "no graph attached");
    const uint32_t n = e->g.n;
    if (e->layers.empty()) return fail(e, GNNVC_ERR_STATE, "engine was created without a model");
    if (audited && e->stage_list().empty()) return fail(e, GNNVC_ERR_UNSUPPORTED, "model is not fused into stages: there is nothing to audit");
    if (n == 0) {
        e->live_seen.clear();   // (a forward that examined no stage: "generic_live_*_<s>")
        return GNNVC_OK;
    }
    // (before the copy below: a sliced engine has no feature buffers of its own — e->x may be null or sized for an earlier graph)
    if (e->g.sliced() || e->pg.empty_slice)
        return fail(e, GNNVC_ERR_STATE, "this engine holds a slice of the graph: run it stage by stage (gnnvc_stage_forward_device)");
    if (!x || !scores) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
    int rc = use_device(e);
    if (rc) return rc;
    if (e->x.cap < ((size_t)n + 1) * (size_t)e->in_width) return fail(e, GNNVC_ERR_STATE, "feature buffers are not sized for this graph");
    const size_t in_b = (size_t)n * e->in_width * sizeof(float);
    const size_t out_b = (size_t)n * e->out_width * sizeof(float);
    HIP_TRY(e, hipMemcpyAsync(e->x.p, x, in_b, hipMemcpyHostToDevice, e->stream));
    const bool want_logits = logits && e->ends_in_sigmoid;
    rc = device_forward(e, e->x.p, e->scores.p, want_logits ? e->logits.p : nullptr);
    if (rc && rc != GNNVC_ERR_AUDIT) return rc;   // (a failed audit: the outputs as the fused path wrote them, and the error)
    HIP_TRY(e, hipMemcpyAsync(scores, e->scores.p, out_b, hipMemcpyDeviceToHost, e->stream));
    if (want_logits)
        HIP_TRY(e, hipMemcpyAsync(logits, e->logits.p, out_b, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return rc;
}

int gnnvc_forward(gnnvc_engine *e, const float *x, float *scores, float *logits) {
    if (!e) return GNNVC_ERR_INVALID;
    return forward_host(e, x, scores, logits, /*audited=*/false);
}

int gnnvc_forward_audited(gnnvc_engine *e, const float *x, float *scores, float *logits) {
    if (!e) return GNNVC_ERR_INVALID;
    return forward_host(e, x, scores, logits, /*audited=*/true);
}

int gnnvc_reduction_flags(gnnvc_engine *e, uint32_t max_degree, uint8_t *flags) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_reduction_flags");
    if (!e->have_graph) return fail(e, GNNVC_ERR_STATE, "no graph attached");
    const uint32_t n = e->g.n;
    if (n == 0) return GNNVC_OK;
    if (e->g.sliced() || e->pg.empty_slice) return fail(e, GNNVC_ERR_STATE, "this engine holds a slice of the graph");
    if (!flags) return fail(e, GNNVC_ERR_INVALID, "null flags buffer");
    int rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(e, e->scratch[1].reserve((size_t)n / 4 + 2));   // n bytes
    uint8_t *d = reinterpret_cast<uint8_t *>(e->scratch[1].p);
    HIP_TRY(e, gnnvc::launch_reduction_flags(e->g, max_degree, d, e->stream));
    HIP_TRY(e, hipMemcpyAsync(flags, d, n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return GNNVC_OK;
}

// ---- feature-row codec of the inter-GPU exchange (device pointers, asynchronous except live_columns)
int gnnvc_live_columns(gnnvc_engine *e, const float *d_feat, uint32_t rows, uint32_t width, uint32_t *mask) {
    if (!e || !mask) return GNNVC_ERR_INVALID;
    if (width != 16) return fail(e, GNNVC_ERR_UNSUPPORTED, "the row codec handles 16-column feature rows");
    *mask = 0;
    if (!rows) return GNNVC_OK;
    if (!d_feat) return fail(e, GNNVC_ERR_INVALID, "null feature buffer");
    int rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(e, e->blk.flag.reserve(1));
    HIP_TRY(e, e->pin_small.reserve(16));
    HIP_TRY(e, gnnvc::live_columns(d_feat, rows, e->blk.flag.p, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->pin_small.p, e->blk.flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    *mask = e->pin_small.p[0];
    return GNNVC_OK;
}

int gnnvc_column_counts(gnnvc_engine *e, const float *d_feat, uint32_t rows, uint32_t width, uint64_t *counts) {
    if (!e || !counts) return GNNVC_ERR_INVALID;
    if (width != 16) return fail(e, GNNVC_ERR_UNSUPPORTED, "the row codec handles 16-column feature rows");
    for (int c = 0; c < 16; ++c) counts[c] = 0;
    if (!rows) return GNNVC_OK;
    if (!d_feat) return fail(e, GNNVC_ERR_INVALID, "null feature buffer");
    int rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(e, e->srt.sum.reserve(16));
    HIP_TRY(e, e->pin_small.reserve(64));
    HIP_TRY(e, gnnvc::column_counts(d_feat, rows, e->srt.sum.p, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->pin_small.p, e->srt.sum.p, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    std::memcpy(counts, e->pin_small.p, 16 * sizeof(uint64_t));
    return GNNVC_OK;
}

static int codec_args(gnnvc_engine *e, uint32_t width, uint32_t row_lo, uint32_t row_hi, uint32_t mask, uint32_t kp) {
    if (width != 16) return fail(e, GNNVC_ERR_UNSUPPORTED, "the row codec handles 16-column feature rows");
    if (row_lo > row_hi) return fail(e, GNNVC_ERR_INVALID, "row range [%u, %u)", row_lo, row_hi);
    if (mask >> 16) return fail(e, GNNVC_ERR_INVALID, "column mask has bits beyond the row width");
    if (kp < 4 || kp > 16 || kp % 4 || (uint32_t)__builtin_popcount(mask) > kp)
        return fail(e, GNNVC_ERR_INVALID, "packed width %u cannot hold %d live columns", kp, __builtin_popcount(mask));
    return GNNVC_OK;
}

int gnnvc_pack_rows(gnnvc_engine *e, const float *d_feat, uint32_t width, uint32_t row_lo, uint32_t row_hi,
                    uint32_t mask, uint32_t kp, float *d_dense, uint32_t *d_exc, uint32_t exc_cap, uint32_t *d_flag) {
    if (!e) return GNNVC_ERR_INVALID;
    int rc = codec_args(e, width, row_lo, row_hi, mask, kp);
    if (rc) return rc;
    if (!d_flag || (row_lo != row_hi && (!d_feat || !d_dense))) return fail(e, GNNVC_ERR_INVALID, "null device buffers");
    rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(e, gnnvc::pack_rows(d_feat, row_lo, row_hi, mask, kp, d_dense, d_exc, d_exc ? exc_cap : 0, d_flag, e->stream));
    return GNNVC_OK;
}

int gnnvc_unpack_rows(gnnvc_engine *e, const float *d_dense, const uint32_t *d_exc, uint32_t exc_cap, uint32_t width,
                      uint32_t row_lo, uint32_t row_hi, uint32_t mask, uint32_t kp, float *d_feat) {
    if (!e) return GNNVC_ERR_INVALID;
    int rc = codec_args(e, width, row_lo, row_hi, mask, kp);
    if (rc) return rc;
    if (row_lo == row_hi) return GNNVC_OK;
    if (!d_feat || !d_dense) return fail(e, GNNVC_ERR_INVALID, "null device buffers");
    rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(e, gnnvc::unpack_rows(d_dense, d_exc, d_exc ? exc_cap : 0, row_lo, row_hi, mask, kp, d_feat, e->stream));
    return GNNVC_OK;
}

int gnnvc_unpack_gathered(gnnvc_engine *e, const float *d_buf, uint32_t world, uint32_t skip_rank, uint64_t piece_words,
                          uint32_t dense_rows, uint32_t exc_cap, uint32_t width, uint32_t rows_per_rank, uint32_t row_off,
                          uint32_t rows, uint32_t n, uint32_t mask, uint32_t kp, float *d_feat) {
    if (!e) return GNNVC_ERR_INVALID;
    int rc = codec_args(e, width, 0, rows, mask, kp);
    if (rc) return rc;
    if (!world || !rows) return GNNVC_OK;
    if (!d_buf || !d_feat) return fail(e, GNNVC_ERR_INVALID, "null device buffers");
    if (rows > dense_rows || piece_words < (uint64_t)dense_rows * kp + (exc_cap ? 4 + 4ull * exc_cap : 0) ||
        (uint64_t)row_off + rows > rows_per_rank)
        return fail(e, GNNVC_ERR_INVALID, "piece geometry: %u rows at offset %u of %u per rank, dense part %u rows, %llu words",
                    rows, row_off, rows_per_rank, dense_rows, (unsigned long long)piece_words);
    rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(e, gnnvc::unpack_gathered(d_buf, world, skip_rank, (size_t)piece_words, dense_rows, exc_cap, rows_per_rank, row_off,
                                      rows, n, mask, kp, d_feat, e->stream));
    return GNNVC_OK;
}

int gnnvc_push_piece(gnnvc_engine *e, const float *d_region, uint32_t rows, uint32_t kp, uint32_t exc_cap, uint32_t n_dst,
                     float *const *d_dst, void *hip_stream) {
    if (!e) return GNNVC_ERR_INVALID;
    if (!n_dst) return GNNVC_OK;
    if (n_dst > 64 || kp < 4 || kp > 16 || kp % 4) return fail(e, GNNVC_ERR_INVALID, "push of %u destinations, packed width %u", n_dst, kp);
    if (!d_region || !d_dst) return fail(e, GNNVC_ERR_INVALID, "null device buffers");
    for (uint32_t i = 0; i < n_dst; ++i)
        if (!d_dst[i]) return fail(e, GNNVC_ERR_INVALID, "null destination %u", i);
    int rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(e, gnnvc::push_piece(d_region, rows, kp, exc_cap, n_dst, d_dst, hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream));
    return GNNVC_OK;
}

int gnnvc_push_rows(gnnvc_engine *e, const float *d_src, uint64_t words, uint32_t n_dst, float *const *d_dst, void *hip_stream) {
    if (!e) return GNNVC_ERR_INVALID;
    if (n_dst > 64) return fail(e, GNNVC_ERR_INVALID, "push of %u destinations (at most 64)", n_dst);
    if (n_dst && !d_dst) return fail(e, GNNVC_ERR_INVALID, "null device buffers");
    for (uint32_t i = 0; i < n_dst; ++i)
        if (!d_dst[i] || (reinterpret_cast<uintptr_t>(d_dst[i]) & 3u)) return fail(e, GNNVC_ERR_INVALID, "destination %u is null or not 4-byte aligned", i);
    if (!n_dst || !words) return GNNVC_OK;
    if (!d_src || (reinterpret_cast<uintptr_t>(d_src) & 3u)) return fail(e, GNNVC_ERR_INVALID, "the source is null or not 4-byte aligned");
    int rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(e, gnnvc::push_rows(d_src, (size_t)words, n_dst, d_dst, hip_stream ? static_cast<hipStream_t>(hip_stream) : e->stream));
    return GNNVC_OK;
}

int gnnvc_unpack_pieces(gnnvc_engine *e, const gnnvc_piece *pieces, uint32_t n_pieces, uint32_t exc_cap, uint32_t width, uint32_t mask,
                        uint32_t kp, float *d_feat) {
    if (!e) return GNNVC_ERR_INVALID;
    int rc = codec_args(e, width, 0, 0, mask, kp);
    if (rc) return rc;
    if (!n_pieces) return GNNVC_OK;
    if (n_pieces > 64 || !pieces || !d_feat) return fail(e, GNNVC_ERR_INVALID, "%u pieces (1 .. 64), null buffers", n_pieces);
    gnnvc::UnpackPiece up[64];
    for (uint32_t i = 0; i < n_pieces; ++i) {
        if (pieces[i].row_lo > pieces[i].row_hi || (pieces[i].row_lo != pieces[i].row_hi && !pieces[i].d_region))
            return fail(e, GNNVC_ERR_INVALID, "piece %u: rows [%u, %u)", i, pieces[i].row_lo, pieces[i].row_hi);
        up[i] = gnnvc::UnpackPiece{pieces[i].d_region, pieces[i].row_lo, pieces[i].row_hi};
    }
    rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(e, gnnvc::unpack_pieces(up, n_pieces, exc_cap, mask, kp, d_feat, e->stream));
    return GNNVC_OK;
}

int gnnvc_score_keys(gnnvc_engine *e, const float *d_scores, uint32_t n, float *keys, uint8_t *above_half) {
    if (!e) return GNNVC_ERR_INVALID;
    if (!d_scores) {   // the scores the last gnnvc_forward left on the device
        const bool have = e->multi ? gnnvc::multi_has_graph(e->multi) : e->have_graph;
        const uint32_t cur = e->multi ? gnnvc::multi_vertices(e->multi) : e->g.n;
        if (!have || e->out_width != 1) return fail(e, GNNVC_ERR_STATE, "no single-column scores on the device");
        if (n != cur) return fail(e, GNNVC_ERR_INVALID, "n = %u, the current graph has %u vertices", n, cur);
        d_scores = e->scores.p;
    }
    if (!n) return GNNVC_OK;
    if (!keys || !above_half) return fail(e, GNNVC_ERR_INVALID, "null output buffers");
    int rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(e, e->scratch[0].reserve(n));
    HIP_TRY(e, e->scratch[1].reserve((size_t)n / 4 + 2));
    uint8_t *d_cls = reinterpret_cast<uint8_t *>(e->scratch[1].p);
    HIP_TRY(e, gnnvc::score_keys(d_scores, n, e->scratch[0].p, d_cls, e->stream));
    HIP_TRY(e, hipMemcpyAsync(keys, e->scratch[0].p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(above_half, d_cls, n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return GNNVC_OK;
}

int gnnvc_synchronize(gnnvc_engine *e) {
    if (!e) return GNNVC_ERR_INVALID;
    int rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if (e->multi) {
        rc = gnnvc::multi_synchronize(e->multi);
        (void)hipSetDevice(e->device);
        if (rc) return fail(e, rc, "a device of the multi-device handle failed to synchronise");
    }
    return GNNVC_OK;
}

int gnnvc_last_forward_ms(gnnvc_engine *e, float *total_ms, float *stage_ms, int max_stages) {
    if (!e) return GNNVC_ERR_INVALID;
    if (e->multi) {   // (host wall time of the last forward over all devices; no per-stage split)
        const double ms = gnnvc::multi_last_forward_ms(e->multi);
        if (ms <= 0.0) return fail(e, GNNVC_ERR_STATE, "no timed forward yet");
        if (total_ms) *total_ms = (float)ms;
        for (int s = 0; stage_ms && s < max_stages; ++s) stage_ms[s] = 0.0f;
        return GNNVC_OK;
    }
    if (e->ev_count < 2)
        return fail(e, GNNVC_ERR_STATE, e->opt.timing ? "no timed forward yet" : "no timed forward: option forward_timing is 0 (1 = total, 2 = per stage)");
    int rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(e, hipEventSynchronize(e->ev[e->ev_count - 1]));
    if (total_ms) HIP_TRY(e, hipEventElapsedTime(total_ms, e->ev[0], e->ev[e->ev_count - 1]));
    for (int s = 0; stage_ms && s < max_stages && s + 1 < e->ev_count; ++s) {
        if (e->ev_stages) HIP_TRY(e, hipEventElapsedTime(&stage_ms[s], e->ev[s], e->ev[s + 1]));
        else stage_ms[s] = -1.0f;   // (forward_timing 1: the stages' events were not recorded)
    }
    return GNNVC_OK;
}

int gnnvc_kernel_trace(gnnvc_engine *e, int max, const char **names, float *ms, int *count) {
    if (!e || !count) return GNNVC_ERR_INVALID;
    *count = 0;
    if (!e->opt.ktrace) return fail(e, GNNVC_ERR_STATE, "option kernel_trace is off");
    int rc = use_device(e);
    if (rc) return rc;
    const size_t used = e->ktrace.used;
    for (size_t i = 0; i < used; ++i) {
        const auto &r = e->ktrace.recs[i];
        HIP_TRY(e, hipEventSynchronize(r.b));
        if ((int)i < max) {
            float t = 0.0f;
            HIP_TRY(e, hipEventElapsedTime(&t, r.a, r.b));
            if (names) names[i] = r.name;
            if (ms) ms[i] = t;
        }
    }
    *count = (int)used;
    e->ktrace.used = 0;
    return GNNVC_OK;
}

// ---- layer-level entry points (host pointers in, host pointers out) ------------

static int run_host_op(gnnvc_engine *e, size_t in_count, const float *in, size_t out_count,
                       float *out, bool out_is_input,
                       hipError_t (*op)(gnnvc_engine *, const float *, float *, void *), void *ctx) {
    int rc = use_device(e);
    if (rc) return rc;
    HIP_TRY(e, e->scratch[0].reserve(in_count));
    HIP_TRY(e, e->scratch[1].reserve(out_count));
    if (in_count)
        HIP_TRY(e, hipMemcpyAsync(e->scratch[0].p, in, in_count * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if (out_is_input && out_count)
        HIP_TRY(e, hipMemcpyAsync(e->scratch[1].p, out, out_count * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, op(e, e->scratch[0].p, e->scratch[1].p, ctx));
    if (out_count)
        HIP_TRY(e, hipMemcpyAsync(out, e->scratch[1].p, out_count * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return GNNVC_OK;
}

int gnnvc_graph_layer_forward(gnnvc_engine *e, uint32_t f, const float *in, float *out) {
    if (!e) return GNNVC_ERR_INVALID;
    NOT_ON_MULTI(e, "gnnvc_graph_layer_forward");
    if (!e->have_graph) return fail(e, GNNVC_ERR_STATE, "no graph attached");
    if (f == 0) return fail(e, GNNVC_ERR_INVALID, "zero feature width");
    const uint32_t n = e->g.n;
    if (n == 0) return GNNVC_OK;
    if (e->g.sliced() || e->pg.empty_slice) return fail(e, GNNVC_ERR_STATE, "this engine holds a slice of the graph");
    if (!in || !out) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
    struct Ctx { uint32_t f; } ctx{f};
    return run_host_op(e, (size_t)n * f, in, (size_t)n * (2 * f + 3), out, false,
                       [](gnnvc_engine *en, const float *di, float *dout, void *c) {
                           return gnnvc::launch_graph_layer(en->g, en->ws, ((Ctx *)c)->f, di, dout, en->stream);
                       }, &ctx);
}

int gnnvc_linear_forward(gnnvc_engine *e, uint32_t n, uint32_t k, uint32_t m, const float *in,
                         const float *W, const float *bias, float *out) {
    if (!e) return GNNVC_ERR_INVALID;
    if ((size_t)n * m == 0) return GNNVC_OK;
    if (!in || !W || !bias || !out) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
    int rc = use_device(e);
    if (rc) return rc;
    DevBuf<float> dW;   // (freed when the call returns: run_host_op has waited for the stream by then)
    HIP_TRY(e, dW.reserve((size_t)k * m + m));
    hipError_t h1 = hipMemcpy(dW.p, W, (size_t)k * m * sizeof(float), hipMemcpyHostToDevice);
    hipError_t h2 = hipMemcpy(dW.p + (size_t)k * m, bias, (size_t)m * sizeof(float), hipMemcpyHostToDevice);
    if (h1 != hipSuccess || h2 != hipSuccess) return fail(e, GNNVC_ERR_DEVICE, "parameter upload failed");
    struct Ctx { uint32_t n, k, m; const float *W; } ctx{n, k, m, dW.p};
    return run_host_op(e, (size_t)n * k, in, (size_t)n * m, out, false,
                       [](gnnvc_engine *en, const float *di, float *dout, void *c) {
                           auto *x = (Ctx *)c;
                           return gnnvc::launch_linear(x->n, x->k, x->m, di, x->W, x->W + (size_t)x->k * x->m, dout, en->stream);
                       }, &ctx);
}

int gnnvc_relu_forward(gnnvc_engine *e, size_t count, const float *in, float *out) {
    if (!e) return GNNVC_ERR_INVALID;
    if (!count) return GNNVC_OK;
    if (!in || !out) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
    struct Ctx { size_t n; } ctx{count};
    return run_host_op(e, count, in, count, out, false,
                       [](gnnvc_engine *en, const float *di, float *dout, void *c) {
                           return gnnvc::launch_relu(((Ctx *)c)->n, di, dout, en->stream);
                       }, &ctx);
}

int gnnvc_sigmoid_forward(gnnvc_engine *e, size_t count, const float *in, float *out) {
    if (!e) return GNNVC_ERR_INVALID;
    if (!count) return GNNVC_OK;
    if (!in || !out) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
    struct Ctx { size_t n; } ctx{count};
    return run_host_op(e, count, in, count, out, false,
                       [](gnnvc_engine *en, const float *di, float *dout, void *c) {
                           return gnnvc::launch_sigmoid(((Ctx *)c)->n, di, dout, en->stream);
                       }, &ctx);
}

int gnnvc_stream_sum(gnnvc_engine *e, const float *values, uint32_t streams, uint32_t len, int mode, float *sums) {
    if (!e) return GNNVC_ERR_INVALID;
    if (!streams) return GNNVC_OK;
    if (!sums || (len && !values)) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
    if (mode != 0 && mode != 2) return fail(e, GNNVC_ERR_INVALID, "mode %d (0 = a stream on several waves, 2 = on one wave; the same exact sum)", mode);
    if (len == 0) {
        for (uint32_t i = 0; i < streams; ++i) sums[i] = 0.0f;
        return GNNVC_OK;
    }
    int rc = use_device(e);
    if (rc) return rc;
    const uint32_t win = gnnvc::giant_window();
    const size_t lpad = ((size_t)len + win - 1) / win * win;
    DevBuf<float> slab, agg, segsum;
    DevBuf<uint4> meta, segmap;
    DevBuf<unsigned long long> off;
    const size_t segs = (size_t)streams * gnnvc::giant_segments(len);
    hipError_t h = slab.reserve(lpad * streams);
    if (h == hipSuccess && mode == 0) h = segsum.reserve(segs);
    if (h == hipSuccess && mode == 0) h = segmap.reserve(segs);
    if (h == hipSuccess) h = agg.reserve((size_t)streams * 16);
    if (h == hipSuccess) h = meta.reserve((size_t)streams + 1);
    if (h == hipSuccess) h = off.reserve(streams);
    if (h == hipSuccess) h = hipMemsetAsync(slab.p, 0, lpad * streams * sizeof(float), e->stream);
    if (h == hipSuccess)
        h = hipMemcpy2DAsync(slab.p, lpad * sizeof(float), values, (size_t)len * sizeof(float), (size_t)len * sizeof(float), streams,
                             hipMemcpyHostToDevice, e->stream);
    if (h == hipSuccess) h = gnnvc::stream_sums(slab.p, streams, len, meta.p, off.p, agg.p, mode, e->stream, segsum.p, segmap.p);
    std::vector<float> host((size_t)streams * 16);
    if (h == hipSuccess) h = hipMemcpyAsync(host.data(), agg.p, host.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream);
    if (h == hipSuccess) h = hipStreamSynchronize(e->stream);
    if (h != hipSuccess) return fail(e, h == hipErrorOutOfMemory ? GNNVC_ERR_NOMEM : GNNVC_ERR_DEVICE, "stream sum: %s", hipGetErrorString(h));
    for (uint32_t i = 0; i < streams; ++i) sums[i] = host[(size_t)i * 16];
    return GNNVC_OK;
}

int gnnvc_sgemm(gnnvc_engine *e, int trans_a, int trans_b, uint32_t m, uint32_t n, uint32_t k,
                const float *A, uint32_t lda, const float *B, uint32_t ldb, float beta, float *C,
                uint32_t ldc) {
    if (!e) return GNNVC_ERR_INVALID;
    if ((size_t)m * n == 0) return GNNVC_OK;
    if (!C || (k && (!A || !B))) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
    const size_t a_rows = trans_a ? k : m, b_rows = trans_b ? n : k;
    const size_t a_cols = trans_a ? m : k, b_cols = trans_b ? k : n;
    if (lda < a_cols || ldb < b_cols || ldc < n) return fail(e, GNNVC_ERR_INVALID, "leading dimension too small");
    int rc = use_device(e);
    if (rc) return rc;
    // BLAS guarantees only (rows - 1) * ld + cols elements of a matrix with a padded leading dimension: copy exactly
    // that much in either direction (the last row's padding is not the caller's memory)
    const size_t a_elems = a_rows ? (a_rows - 1) * lda + a_cols : 0;
    const size_t b_elems = b_rows ? (b_rows - 1) * ldb + b_cols : 0;
    const size_t c_elems = (size_t)(m - 1) * ldc + n;
    DevBuf<float> dB;
    HIP_TRY(e, dB.reserve(b_elems + 1));
    if (b_elems && hipMemcpy(dB.p, B, b_elems * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return fail(e, GNNVC_ERR_DEVICE, "B upload failed");
    struct Ctx { int ta, tb; uint32_t m, n, k, lda, ldb, ldc; float beta; const float *B; } ctx{
        trans_a, trans_b, m, n, k, lda, ldb, ldc, beta, dB.p};
    return run_host_op(e, a_elems, A, c_elems, C, true,
                       [](gnnvc_engine *en, const float *dA, float *dC, void *c) {
                           auto *x = (Ctx *)c;
                           return gnnvc::launch_sgemm(x->ta, x->tb, x->m, x->n, x->k, dA, x->lda, x->B, x->ldb,
                                                      x->beta, dC, x->ldc, en->stream);
                       }, &ctx);
}

}  // extern "C"
