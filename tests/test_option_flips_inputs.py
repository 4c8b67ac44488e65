"""tools/optionflips.py, the case table of tests/test_gpu_option_flips.py, on the CPU: conditions that keep those tests from passing
vacuously, not measurements.

  a. the table is pinned: a SHA-256 over repr(case(i)) of every case, the counts of each kind;
  b. coverage: the directed cases' keys and EXCLUDED are together exactly the keys of gnnvc_options.h's table, EXCLUDED holds only
     keys that have tests of their own or change no kernel, and none that forgets pruned adjacencies, invalidates the sorted row
     ranges or switches an automatic threshold off;
  c. every directed case moves its key across its graph — shown in numpy on the CSR: a threshold has rows (vertices, entries,
     bytes) on both sides of its values, a key of a plan runs on a graph on which that plan is engaged under the case's options;
  d. the random cases' value choices are tests/test_gpu_fuzz.py::_options';
  e. the expected values are the oracle's: what tests/test_gpu_models.py::want_of caches for every (model, graph, weight scale)
     the cases use is OracleModel.predict's output, bit for bit."""
import hashlib
import re

import numpy as np
import pytest

from oracle import oracle_py
from tools import optionflips as of
from tests import flip_harness as fh
from tests import test_gpu_models as tm
from tests.generic_harness import bits
from tests.test_gpu_fuzz import _options
from tests.test_option_docs import ROOT, _table_keys

TABLE_SHA256 = "cabd6e2d2d0eb4976347f5aa6503f48204bbf6af8f93b63aaff5cbb6c325debb"
ALLOWED_EXCLUSIONS = {"audit_period", "audit_repair", "audit_flip_stage", "audit_flip_row", "audit_quiet", "audit_log",
                      "generic_stages", "poison_features", "forward_timing", "kernel_trace", "verdict_period"}
CASES = [of.case(i) for i in range(of.N)]


# ---------------------------------------------------------------- a. the pinned table

def test_the_table_is_the_pinned_one():
    assert of.N == 105 and len(of.DIRECTED) == 71 and of.N_RANDOM == 24 and len(of.MULTI) == 6 and len(of.SCALE) == 4
    assert [c.kind for c in CASES] == ["directed"] * 71 + ["random"] * 24 + ["multi"] * 6 + ["scale"] * 4
    assert [c.index for c in CASES] == of.directed_indices() + of.random_indices() + of.multi_indices() + of.scale_indices()
    assert len({c.name for c in CASES}) == of.N
    h = hashlib.sha256()
    for c in CASES:
        h.update(repr(c).encode())
    assert h.hexdigest() == TABLE_SHA256
    assert all(12 <= len(c.steps) <= 20 for c in CASES if c.kind == "random"), [len(c.steps) for c in CASES if c.kind == "random"]
    assert all(c.options["poison_features"] == 1 for c in CASES)
    assert set(of.REGRESSIONS.values()) <= set(range(of.N))
    # random_2: the compact table in chunks of 16 rows on 300 K vertices, the last stage round by round — more than 64 rounds of 256 chunks
    c = CASES[of.REGRESSIONS["more rounds of the compact-table plan than round counters"]]
    assert (c.name, c.graph, c.options["plan_chunk_rows"], c.options["blocked_min_n"]) == ("random_2", "er300k", 16, 0)
    assert c.options.get("overlap_dense", 1) == 1 and c.options.get("mfma_dense", 2) != 1 and c.steps[:3] == (("forward", "x"),) * 3
    assert (of.GRAPH_N["er300k"] + 15) // 16 > 64 * 256


def test_the_graphs_and_models_are_the_named_ones():
    from tests.test_modelgen import GRAPHS
    from tools import modelgen as mg
    assert list(of.GRAPH_N) == list(GRAPHS) and all(tm.graph_of(k).n == n for k, n in of.GRAPH_N.items())
    assert sorted(sum(of.CLASSES.values(), [])) == sorted(GRAPHS)
    assert of.MODELS == ["trained", "dense_3_0.35", "live_four"] and set(of.MODELS[1:]) | {of.PREDICTED_MODEL} <= set(mg.FAMILY)
    assert of.PLANNED == tm.PLANNED and of.PREDICT == tm.PREDICT
    assert {c.model for c in CASES} == set(of.MODELS) | {of.PREDICTED_MODEL} and {c.graph for c in CASES} == set(GRAPHS)
    assert {c.key for c in CASES if c.model == of.PREDICTED_MODEL} == {"prune_predict", "prune_predict_min_entries"}
    # the weight scales: the largest weight times 1, 3, 9 falls into the byte, the ten-bit and the sixteen-bit table
    assert [int(tm.graph_of("er300k").ws) * m for m in of.SCALES] == [120, 360, 1080]
    for c in CASES:
        n, graph = of.GRAPH_N[c.graph], c.graph
        for s in c.steps:
            if s[0] == "graph":
                graph, n = s[1], of.GRAPH_N[s[1]]
            if s[0] == "stage":
                _, st, lo, hi = s
                assert st in (0, 1, 2) and lo % 64 == 0 and lo < hi <= n and (hi % 64 == 0 or hi == n), (c.name, s, graph)
            if s[0] == "weight_scale":
                assert s[1] in of.SCALES


# ---------------------------------------------------------------- b. coverage

def _rows():
    """{key: the text of its row} of kOptionRows."""
    src = (ROOT / "gnn-mwvc_amd" / "csrc" / "gnnvc_options.h").read_text()
    body = src[src.index(" kOptionRows[] = {"):]
    body = body[:body.index("\n};")]
    return {m.group(1): m.group(0) for m in re.finditer(r'^\s*\{"([a-z0-9_]+)",.*$', body, flags=re.M)}


def test_every_key_is_covered_or_excluded_by_name():
    keys = set(_table_keys("gnnvc_options.h", "kOptionRows"))
    covered = of.covered_keys()
    assert covered | set(of.EXCLUDED) == keys, (sorted(keys - covered - set(of.EXCLUDED)), sorted((covered | set(of.EXCLUDED)) - keys))
    assert not covered & set(of.EXCLUDED)
    assert set(of.EXCLUDED) <= ALLOWED_EXCLUSIONS and all(reason for reason in of.EXCLUDED.values())
    rows = _rows()
    assert set(rows) == keys
    for k in of.EXCLUDED:
        assert not re.search(r"kFx(ForgetPruned|SortedStale|LongExplicit|GiantExplicit)", rows[k]), k
    # each key: every value of its domain but the first is flipped to, in every one of its cases
    for c in CASES[: len(of.DIRECTED)]:
        first, domain, _, _ = of.KEYS[c.key]
        sets = [s[2] for s in c.steps if s[0] == "set" and s[1] == c.key]
        assert c.options[c.key] == first and list(c.options)[-1] == c.key, c.name
        others = [v for v in domain if v != first]
        assert set(others) <= set(sets) and sets[-1] == first and c.steps[-1] == ("reupload",), c.name
        # ... once more between a hand-off and its first forward, and across a hand-off
        assert [c.steps[j + 1][2] for j, s in enumerate(c.steps) if s == ("reupload", "plain")] == others, c.name
        assert [c.steps[j - 1][2] for j, s in enumerate(c.steps[:-1]) if s == ("reupload",) and c.steps[j - 1][0] == "set"][-len(others):] == others, c.name
        for j, s in enumerate(c.steps):   # after every flip: two forwards, the other input, a call of each 16-wide stage
            if s[0] == "set" and s[2] != first and c.steps[j + 1: j + 4] == (("forward", "x"), ("forward", "x"), ("forward", "other")):
                assert [t[:2] for t in c.steps[j + 4: j + 6]] == [("stage", 1), ("stage", 2)], (c.name, j)
        assert sum(1 for j, s in enumerate(c.steps) if s[0] == "set" and [t[:2] for t in c.steps[j + 4: j + 6]] == [("stage", 1), ("stage", 2)]) \
            == len([v for v in domain if v != first]), c.name
    # a multi-device handle: the keys it hands on to its parts (kFxForward, which kFxPlan contains)
    for k in of.MULTI:
        assert re.search(r"kFx(Forward|Plan)", rows[k]), k


# ---------------------------------------------------------------- c. every directed case moves its key

DEFAULTS = {"long_row_threshold": 512, "giant_row_threshold": 16384, "table_tiles": 1, "table_tiles_min_n": 49152, "table_tiles_max_bytes": 6 << 20,
            "compact_gather": 1, "mfma_dense": 2, "blocked_min_n": 1 << 20, "compact_min_n": 1 << 18, "lds_table": 1, "blocked_stage0": 1,
            "wide_tiles": 1, "wide_tiles_max_n": 49152, "wide_tiles_max_n_f16": 131072}   # gnnvc_options.h: struct Options
# where a key's FIRST value has to lie for its plan to be engaged when the case begins
ENGAGED_WHEN = {"table_tiles_min_n": "n >=", "compact_min_n": "n >=", "blocked_min_n": "n >=", "wide_tiles_max_n": "n <=", "wide_tiles_max_n_f16": "n <=",
                "table_tiles_max_bytes": "bytes <=", "handoff_min_entries": "entries >=", "compact_first_forward_entries": "entries >="}


def _engaged(plan, g, o):
    """Is `plan` in force on graph g under options o (gnnvc_plans.cpp's conditions, restated on the CSR)?"""
    opt = lambda k: o.get(k, DEFAULTS[k])
    deg = np.diff(g.rowptr.astype(np.int64))
    long_from = opt("long_row_threshold")
    has_long = long_from > 0 and bool((deg >= long_from).any())
    in_plan_range = g.n >= min(opt("blocked_min_n"), opt("compact_min_n")) and (opt("blocked_min_n") < (1 << 20) or g.nnz >= (8 << 20))
    if plan == "long rows":
        return has_long
    if plan == "giant rows":
        return has_long and opt("giant_row_threshold") > 0 and bool((deg >= max(opt("giant_row_threshold"), long_from)).any())
    if plan == "table tiles":
        return (opt("table_tiles") and opt("compact_gather") and opt("mfma_dense") != 1 and g.n >= opt("table_tiles_min_n")
                and (g.n + 1) * 16 <= opt("table_tiles_max_bytes") and not has_long and not in_plan_range)
    if plan == "wide tiles":
        return bool(opt("wide_tiles")) and g.n <= min(opt("wide_tiles_max_n"), opt("wide_tiles_max_n_f16")) and not has_long
    if plan == "lds table":
        return bool(opt("lds_table")) and g.n >= opt("blocked_min_n") and not has_long and (opt("blocked_min_n") < (1 << 20) or g.nnz >= 10 * g.n)
    if plan == "compact gather":
        return bool(opt("compact_gather")) and in_plan_range and not has_long
    if plan == "blocked":   # (at least two column blocks of x)
        return bool(opt("blocked_stage0")) and not opt("lds_table") and g.n >= opt("blocked_min_n") and not has_long and g.n > (o.get("block_cols") or 512 << 10)
    raise KeyError(plan)


def _share_into(g, rows):
    """The share of the graph's entries that point into the set `rows` (a mask over the vertices)."""
    return float(rows[g.col].mean())


def _zero_rows(c, g):
    """The first 16-wide stage's input has zero rows that hold a share of the entries worth a pruned adjacency under the case's options,
    and the graph has the long rows that make it "skewed" for the engine."""
    h1 = fh.want(c.model, c.graph, "h1")
    zero = ~(h1 != 0).any(axis=1)
    return _engaged("long rows", g, c.options) and _share_into(g, zero) * 100 >= max(15, c.options.get("prune_min_drop_percent", 15))


def _prediction(c, g):
    """The set the hand-off predicts (tests/test_modelgen.py::_predicted restates k_predict_zero_f1) holds a share of the entries."""
    from tests.test_modelgen import _predicted
    fh.model_text(c.model)
    om = tm.oracle_of(c.model)
    om.set_weight_scale(g.ws)
    ptop, pscale = _predicted(om, g)
    in_set = (np.diff(g.rowptr.astype(np.int64)) > 0) & (ptop <= -1e-3 * (1.0 + pscale))
    return _engaged("long rows", g, c.options) and _share_into(g, in_set) * 100 >= 15 and c.options.get("prune_predict_min_entries", 48 << 20) <= g.nnz


@pytest.mark.parametrize("key", sorted(of.covered_keys()))
def test_a_directed_case_moves_its_key_across_its_graph(key):
    first, domain, places, shows = of.KEYS[key]
    values = sorted(set(domain) | {first})
    for c in (c for c in CASES[: len(of.DIRECTED)] if c.key == key):
        g = tm.graph_of(c.graph)
        deg = np.diff(g.rowptr.astype(np.int64))
        if shows == "degree":
            assert any(v > 0 and (deg < v).any() and (deg >= v).any() for v in values), (c.name, values, int(deg.max()))
            assert _engaged("long rows", g, c.options) or key == "long_row_threshold", c.name
        elif shows in ("n", "entries", "bytes"):
            count = {"n": g.n, "entries": g.nnz, "bytes": (g.n + 1) * 16}[shows]
            assert any(v <= count for v in values) and any(v > count for v in values), (c.name, values, count)
            if key in ENGAGED_WHEN:
                what, op = ENGAGED_WHEN[key].split()
                assert what == shows and (count >= first if op == ">=" else count <= first), (c.name, first, count)
                if key == "compact_first_forward_entries":
                    assert first > 0
        else:
            special = {"zero rows": _zero_rows, "prediction": _prediction}
            assert any(special[p](c, g) if p in special else _engaged(p, g, c.options) for p in shows.split(" or ")), (c.name, shows)
        if key.startswith("prune_predict"):
            assert _prediction(c, g), c.name
        if c.graph in ("er100k", "er300k", "er1933"):   # a case on a graph of the tables: one of them is in force when it begins
            assert any(_engaged(p, g, c.options) for p in ("table tiles", "wide tiles", "lds table", "compact gather", "blocked")), c.name


def test_the_expectations_name_real_readouts_and_the_harness_keeps_the_full_list():
    assert fh.AT_HANDOFF == ["long_rows", "giant_rows", "giant_entries", "giant_segments", "lds_table_active", "compact_gather_active",
                             "table_tiles_active", "pruned_predicted_stage1"]
    assert fh.AFTER_FORWARDS == ["wide_tiles_used", "lds_table_last_ok", "compact_gather_last_ok", "pruned_last_ok_stage1",
                                 "pruned_entries_stage1", "table_tiles_fit_stage1", "table_tiles_fit_stage2"]
    src = (ROOT / "gnn-mwvc_amd" / "csrc" / "gnnvc_engine.cpp").read_text()
    named = set(fh.AT_HANDOFF + fh.AFTER_FORWARDS) | {s[1] for c in CASES for s in c.steps if s[0] == "expect"}
    assert all(f'"{k}"' in src for k in named), sorted(k for k in named if f'"{k}"' not in src)
    assert all(set(k for k, _ in c.left_out) <= set(fh.AT_HANDOFF + fh.AFTER_FORWARDS) and all(r for _, r in c.left_out) for c in CASES)
    # the cases that show their transition by a read-out: wide tiles and table tiles among them
    shown = {(c.key, c.graph) for c in CASES if any(s[0] == "expect" for s in c.steps)}
    assert {("wide_tiles", "er1933"), ("table_tiles", "er100k")} <= shown


# ---------------------------------------------------------------- d. the random cases' values

def test_the_value_choices_are_the_plan_fuzzs():
    seen = {}
    for case in range(400):
        for k, v in _options(np.random.default_rng(90_000 + case)).items():
            seen.setdefault(k, set()).add(v)
    for k in ("blocked_min_n", "prune_min_entries", "poison_features"):   # (constants there)
        assert len(seen.pop(k)) == 1
    assert {k: sorted(v) for k, v in seen.items()} == {k: sorted(set(v)) for k, v in of.CHOICES.items()}
    keys = set(_table_keys("gnnvc_options.h", "kOptionRows"))
    assert set(of.CHOICES_MORE) <= keys - set(of.CHOICES)
    random = [c for c in CASES if c.kind == "random"]
    kinds = {s[0] for c in random for s in c.steps}
    assert kinds == {"set", "forward", "stage", "weight_scale", "reupload", "graph", "stream"}, kinds
    for c in random:   # graph changes go round the classes: uniform, skewed, tiny, uniform ...
        cls = lambda name: next(k for k, v in of.CLASSES.items() if name in v)
        seq = [cls(c.graph)] + [cls(s[1]) for s in c.steps if s[0] == "graph"]
        assert all(of.CLASS_ORDER.index(b) == (of.CLASS_ORDER.index(a) + 1) % 3 for a, b in zip(seq, seq[1:])), (c.name, seq)
    assert sum(1 for c in random for s in c.steps if s[0] == "graph") >= 12
    assert len({s[1] for c in random for s in c.steps if s[0] == "set"}) >= 24


# ---------------------------------------------------------------- e. the expected values are the oracle's

NEEDED = sorted({need for c in CASES for need in fh.needs(c)})


@pytest.mark.parametrize("gname", list(of.GRAPH_N))
def test_the_expected_values_are_predicts(gname):
    g = tm.graph_of(gname)
    mine = [t for t in NEEDED if t[1] == gname]
    assert mine
    for name, _, scale in mine:
        om = oracle_py.OracleModel(fh.model_text(name))
        om.set_weight_scale(float(np.float32(g.ws * scale)))
        for what, x in (("logits", g.x()), ("other", tm.other_input(g))):
            got = fh.want(name, gname, what, scale)
            assert got.shape == (g.n,) and np.isfinite(got).all(), (name, gname, scale, what)
            assert np.array_equal(bits(got), bits(om.predict(g, x, stop_after=om.n_layers - 2)[:, 0])), (name, gname, scale, what)
        for st, stop in ((1, 6), (2, 13)):   # the stage calls' inputs and expectations: the ReLU outputs behind layers 6 and 13
            assert np.array_equal(bits(fh.want(name, gname, f"h{st}", scale)), bits(om.predict(g, g.x(), stop_after=stop)[:, :16])), (name, gname, scale, st)
        if scale != 1:   # another scale is another result: a forward that ignored gnnvc_set_weight_scale would show
            assert not np.array_equal(bits(fh.want(name, gname, "logits", scale)), bits(fh.want(name, gname, "logits", 1))), (name, gname, scale)
