// Host program over gnn-mwvc_amd/csrc/gnnvc_options.h (nothing of HIP) for tests/test_options_host.py: every key of the
// option table is fed a fixed set of values; per key, one line with what was written to which member of gnnvc::Options
// and the effects the engine is told to apply.  Every trial starts from an Options whose members all hold a value no
// clamp produces, so a member that is written shows, whatever is written to it.
#include <cstdio>
#include <string>
#include <vector>

#include "../../gnn-mwvc_amd/csrc/gnnvc_options.h"

#define MEMBERS(X)                                                                                                              \
    X(generic) X(blocked) X(block_cols) X(blocked_min_n) X(compact_min_n) X(compact_min_nnz) X(compact_first_entries)           \
    X(plan_chunk_rows) X(lds_table) X(lt_bits) X(lds_skewed_rows) X(lds_skewed_min_n) X(lds_skewed) X(lt_min_chunks) X(compact) \
    X(overlap) X(dense_skip) X(prune) X(prune_heavy_entries) X(prune_early_nnz) X(prune_predict) X(predict_min_nnz)             \
    X(prune_eff) X(prune_giant) X(prune_min_nnz) X(prune_min_drop) X(giant_gather_first) X(long_on_main) X(filter)              \
    X(filter_min_nnz) X(filter_min_long_pct) X(filter_min_pct) X(filter_keep) X(t4) X(t4_min_n) X(t4_max_bytes) X(t4_solo)      \
    X(timing) X(poison) X(verdict_period) X(wide) X(wide_max_n) X(wide_max_n16) X(mfma) X(sorted) X(sorted_min_nnz)             \
    X(sorted_long_thresh) X(long_thresh) X(long_auto) X(ktrace) X(giant_thresh) X(side_streams) X(giant_f16) X(giant_f16_auto)  \
    X(giant_segments) X(handoff) X(handoff_min_nnz) X(pilot_rows) X(audit_period) X(audit_repair) X(audit_flip_stage)           \
    X(audit_flip_row) X(audit_quiet) X(audit_log)

static const std::vector<long> kValues = {-5, 0, 1, 2, 3, 64, 101, 65536, 1L << 40};
// the one key whose accepted values are none of those: the three it takes and one between them, on a line of its own
static const char *const kBitsKey = "lds_table_bits";
static const std::vector<long> kBitsValues = {8, 10, 12, 16};
static const long kUntouched = 77;   // (bool members: true)

static std::string effects(uint32_t fx) {
    static const struct { uint32_t bit; const char *name; } names[] = {
        {gnnvc::kFxShortLists, "short_lists"}, {gnnvc::kFxForgetPruned, "forget_pruned"}, {gnnvc::kFxSortedStale, "sorted_stale"},
        {gnnvc::kFxLongExplicit, "long_explicit"}, {gnnvc::kFxGiantExplicit, "giant_explicit"}, {gnnvc::kFxAuditRestart, "audit_restart"},
        {gnnvc::kFxForward, "multi_forward"}, {gnnvc::kFxFrontOnly, "multi_front_only"}, {gnnvc::kFxPartsElsewhere, "multi_parts_elsewhere"}};
    std::string s;
    for (const auto &n : names)
        if (fx & n.bit) {
            fx &= ~n.bit;
            s += (s.empty() ? "" : "+") + std::string(n.name);
        }
    if (fx) s += "+unknown";
    return s.empty() ? "none" : s;
}

// One line: `label`, then every member some value of `values` wrote with what it then held, then the effects.
static bool print_key(const gnnvc::Options &fresh, const char *key, const std::vector<long> &values, const std::string &label) {
    struct Seen { const char *name; std::string values; bool any; };
    std::vector<Seen> seen;
#define X(m) seen.push_back(Seen{#m, "", false});
    MEMBERS(X)
#undef X
    std::string fxs;
    bool fx_same = true;
    for (size_t t = 0; t < values.size(); ++t) {
        gnnvc::Options o = fresh;
        uint32_t fx = 0;
        if (!gnnvc::apply_option(o, key, values[t], &fx)) {
            printf("%s: refused\n", key);
            return false;
        }
        size_t i = 0;
#define X(m)                                                                                        \
    {                                                                                               \
        const bool hit = (long long)o.m != (long long)fresh.m;                                       \
        seen[i].any |= hit;                                                                         \
        seen[i].values += (t ? "," : "") + (hit ? std::to_string((long long)o.m) : std::string("-")); \
        ++i;                                                                                        \
    }
        MEMBERS(X)
#undef X
        const std::string f = effects(fx);
        if (t && f != fxs) fx_same = false;
        fxs = f;
    }
    printf("%s", label.c_str());
    for (const Seen &s : seen)
        if (s.any) printf(" %s=%s", s.name, s.values.c_str());
    printf(" fx=%s\n", fx_same ? fxs.c_str() : "varies");
    return true;
}

int main() {
    gnnvc::Options fresh;
#define X(m) fresh.m = (decltype(fresh.m))kUntouched;
    MEMBERS(X)
#undef X
    uint32_t fx = 0;
    if (gnnvc::apply_option(fresh, "no_such_option", 1, &fx) || gnnvc::apply_option(fresh, "", 1, &fx)) {
        printf("an unknown key was accepted\n");
        return 1;
    }
    for (const auto &row : gnnvc::kOptionRows)
        if (!print_key(fresh, row.key, kValues, row.key)) return 1;
    return print_key(fresh, kBitsKey, kBitsValues, std::string(kBitsKey) + "@8,10,12,16") ? 0 : 1;
}
