"""The case table of the trained path's option-flip tests (tests/test_gpu_option_flips.py, tests/flip_harness.py): what a caller
may do to ONE engine between forwards — set options under the resident graph, hand the same graph over again, hand over a graph of
another class, move the weight scale, change the stream — and still read the oracle's bits.  CPU only, no graph is built here:
tests/test_option_flips_inputs.py pins the table with a hash and shows on the graphs' CSR that every directed case moves its key
across its graph.

case(i) -> Case, deterministic (numpy's default_rng(SEED + i), as tests/test_gpu_fuzz.py seeds its cases):

  0 .. len(DIRECTED) - 1   directed, one key on one graph: settle, flip the key to every other value of its domain under the
                           resident graph — two forwards, the other input and a call of each 16-wide stage after every flip;
                           every value once more between a hand-off and its first forward, and across a hand-off; then the key
                           back at its first value, two forwards, the same graph again
  then RANDOM cases        12 to 20 steps: sets of one to three keys (values as tests/test_gpu_fuzz.py::_options draws them),
                           forwards, stage calls, the same graph again, a graph of the next class (uniform, skewed, tiny, uniform
                           ...), the weight scale, the stream
  then len(MULTI) cases    one key each on hub4096 behind a three-part handle: sets and whole forwards only
  then len(SCALE) cases    the weight scale moves under a resident graph whose stage 0 runs on the LDS table, across the table's
                           entry widths and back; every move is followed by forwards, stage calls and the same graph again

Steps (tests/flip_harness.py runs them):
  ("set", key, value)          gnnvc_set_option under the resident graph
  ("forward", "x" | "other")   a whole forward of the driver's input g.x(), or of g.x() * 0.37f
  ("stage", st, lo, hi)        gnnvc_stage_forward_device over rows [lo, hi) (lo a multiple of 64; hi one, or n), fed the oracle's input
  ("weight_scale", m)          gnnvc_set_weight_scale(m * g.ws): 1 = the driver's own; 3 and 9 move the scale — which the LDS table's
                               entry width follows as it follows the largest weight — from a byte's range into ten and sixteen bits
                               (tests/test_gpu_parity.py::test_lds_table_entry_width_follows_the_weights: 120 x 1 | 3 | 9)
  ("reupload",)                the same graph again (the harness alternates gnnvc_upload_graph and the staged route), then both state
                               checks of tests/flip_harness.py, which run three forwards
  ("reupload", "plain")        the same graph again and the hand-off read-outs alone: the steps that follow fall between a hand-off and
                               its first forward, where the filtered gather, the first-forward builds and the pilot read their keys
  ("graph", name)              another graph of GRAPH_N on the same engine
  ("stream", "caller" | "own") gnnvc_set_stream to a stream of the caller's, and back
  ("expect", info_key, value)  a gnnvc_get_info read-out that shows the case reached the transition it is named for"""
import collections

import numpy as np

SEED = 97_000
# left_out: ((read-out, reason), ...) of the harness's lists that are not defined on the case's graph — no case needs one so far
# (what the table tiles carry from graph to graph is the harness's own rule: tests/flip_harness.py, CARRIED_BY_TABLE_TILES)
Case = collections.namedtuple("Case", "index name kind key graph model options steps left_out")

MODELS = ["trained", "dense_3_0.35", "live_four"]   # tools/modelgen.py's members light the columns and lanes the trained weights leave dark
PREDICTED_MODEL = "zero_rows_heavy"                 # ... and the one whose zero rows the hand-off predicts ("prune_predict*" only)
GRAPH_N = {"er1933": 1933, "er100k": 100000, "er300k": 300000, "rmat13": 8192, "hub4096": 20000}   # tests/test_modelgen.py::GRAPHS
CLASSES = {"uniform": ["er100k", "er300k"], "skewed": ["rmat13", "hub4096"], "tiny": ["er1933"]}
CLASS_ORDER = ["uniform", "skewed", "tiny"]
SCALES = [1, 3, 9]

# the options that engage the plans on these graphs, as the suite already sets them (tests/test_gpu_models.py: PLANNED, PREDICT,
# test_long_and_giant_rows) — poison_features 1 everywhere: a row that no kernel writes shows in the result
PLANNED = {"blocked_min_n": 0, "compact_min_n": 0, "plans_at_handoff": 2}
PREDICT = {"blocked_min_n": 0, "long_row_threshold": 256, "sorted_long_row_threshold": 512, "giant_row_threshold": 4096,
           "prune_min_entries": 0, "prune_predict_min_entries": 0, "filter_min_long_percent": 0, "prune_min_drop_percent": 1}
HUBS = {"long_row_threshold": 8, "giant_row_threshold": 1000}
BASES = {
    "plain": {},
    "planned": PLANNED,
    "in_forwards": dict(PLANNED, plans_at_handoff=0),          # the plans are built inside the first forwards
    "handoff_1": dict(PLANNED, plans_at_handoff=1),            # ... at hand-off only where one use repays them (handoff_min_entries)
    "blocked": dict(PLANNED, lds_table=0, block_cols=65536),   # stage 0 on the column-blocked plan (five blocks of x)
    "compact_bound": {"blocked_min_n": 1 << 19, "plans_at_handoff": 2},   # compact_min_n alone decides on a graph of 300 K vertices
    "predict": PREDICT,
    "sorted": dict(PREDICT, sorted_tiles=1),
    "giant_rmat": dict(PREDICT, long_row_threshold=64, giant_row_threshold=300, sorted_tiles=1),   # rmat13: ~70 giant rows
    "hubs": HUBS,
}

BOOL, TRI, ZERO_TO_TWO = (0, 1), (-1, 0, 1), (0, 1, 2)

# key -> (first value, the other values of its domain, [(graph, base, model)], what the CPU test shows of the case).  The first
# value is set before the graph is handed over, so "back at its first value" is the state of an engine that never flipped it —
# also for the keys that switch an automatic choice off for good ("long_row_threshold", "giant_row_threshold" ...).
# shows: "degree" = rows on both sides of a flipped value; "n" / "entries" / "bytes" = the graph's count on both sides of the
# flipped values; otherwise the plan that has to be engaged under the initial options for the flips to matter.
KEYS = {
    # ---- row classes and the side queue: hub4096 and rmat13
    "long_row_threshold": (8, (0, 4, 64, 5000), [("hub4096", "hubs", "trained"), ("rmat13", "predict", "dense_3_0.35")], "degree"),
    "giant_row_threshold": (1000, (0, 64, 3000, 5000), [("hub4096", "hubs", "dense_3_0.35"), ("rmat13", "giant_rmat", "trained")], "degree"),
    "giant_row_threshold_f16": (65536, (1, 500, 2000, 5000), [("hub4096", "hubs", "live_four"), ("rmat13", "giant_rmat", "dense_3_0.35")], "degree"),
    "giant_segments": (-1, TRI, [("hub4096", "hubs", "trained"), ("rmat13", "giant_rmat", "live_four")], "giant rows"),
    "side_streams": (1, BOOL, [("hub4096", "hubs", "dense_3_0.35"), ("rmat13", "giant_rmat", "trained")], "giant rows"),
    "giant_gather_first": (-1, TRI, [("hub4096", "hubs", "live_four"), ("rmat13", "giant_rmat", "dense_3_0.35")], "giant rows"),
    "long_rows_on_main": (-1, TRI, [("hub4096", "hubs", "trained"), ("rmat13", "giant_rmat", "live_four")], "giant rows"),
    "prune_giant_rows": (1, BOOL, [("hub4096", "hubs", "dense_3_0.35"), ("rmat13", "giant_rmat", "trained")], "giant rows"),
    "sorted_tiles": (-1, TRI, [("rmat13", "predict", "trained"), ("hub4096", "hubs", "live_four")], "long rows"),
    "sorted_min_nnz": (0, (1, 100_000, 1 << 30), [("rmat13", "predict", "dense_3_0.35")], "entries"),
    "sorted_long_row_threshold": (512, (1, 64, 300, 100_000), [("rmat13", "sorted", "trained"), ("hub4096", dict(HUBS, sorted_tiles=1), "dense_3_0.35")], "degree"),
    # ---- the pruned adjacency and the filtered gather: rmat13 with the prediction at hand-off
    "prune_zero_rows": (1, BOOL, [("rmat13", "predict", "trained"), ("hub4096", "hubs", "trained")], "zero rows or long rows"),
    "prune_class_by_entries_left": (1, BOOL, [("rmat13", "sorted", "trained"), ("rmat13", "giant_rmat", "trained")], "zero rows"),
    "prune_heavy_entries": (16 << 20, (0, 1, 50_000), [("rmat13", "sorted", "trained")], "entries"),
    "prune_early_entries": (64 << 20, (0, 1, 50_000), [("rmat13", dict(PREDICT, filter_zero_rows=0), "trained")], "entries"),
    # (the prediction needs weights that zero whole rows by the vertices' own weights: tools/modelgen.py's zero_rows_heavy, as
    # tests/test_gpu_models.py::test_zero_row_prediction_holds — under the three models above no set is predicted on these graphs)
    "prune_predict": (1, BOOL, [("rmat13", "predict", "zero_rows_heavy")], "prediction"),
    "prune_predict_min_entries": (0, (1, 100_000, 1 << 30), [("rmat13", "predict", "zero_rows_heavy")], "entries"),
    "prune_min_entries": (0, (1, 100_000, 1 << 30), [("rmat13", "predict", "trained")], "entries"),
    "prune_min_drop_percent": (1, (0, 50, 100), [("rmat13", "predict", "trained")], "zero rows"),
    "filter_zero_rows": (1, BOOL, [("rmat13", dict(PREDICT, filter_min_entries=0, prune_predict=0), "trained")], "zero rows"),
    "filter_keep_lists": (1, BOOL, [("rmat13", dict(PREDICT, filter_min_entries=0, prune_predict=0), "trained")], "zero rows"),
    "filter_min_entries": (0, (1, 100_000, 1 << 30), [("rmat13", dict(PREDICT, prune_predict=0), "trained")], "entries"),
    "filter_min_long_percent": (0, (50, 101), [("rmat13", dict(PREDICT, filter_min_entries=0, prune_predict=0), "trained")], "zero rows"),
    "filter_min_percent": (50, (0, 101), [("rmat13", dict(PREDICT, filter_min_entries=0, prune_predict=0), "trained")], "zero rows"),
    "lds_table_skewed": (1, BOOL, [("rmat13", "predict", "trained"), ("hub4096", dict(HUBS, blocked_min_n=0), "live_four")], "long rows"),
    "lds_table_skewed_rows": (0, (64, 512, 16384), [("rmat13", "predict", "live_four"), ("hub4096", dict(HUBS, blocked_min_n=0), "trained")], "degree"),
    # ---- the tables: er100k (table tiles) and er300k (LDS table, compact gather)
    "table_tiles": (1, BOOL, [("er100k", "plain", "live_four")], "table tiles"),
    "table_tiles_solo": (1, BOOL, [("er100k", "plain", "live_four")], "table tiles"),
    "table_tiles_min_n": (49152, (0, 100_000, 100_001, 1 << 30), [("er100k", "plain", "trained")], "n"),
    "table_tiles_max_bytes": (6 << 20, (0, 1_600_015, 1_600_016, 1 << 40), [("er100k", "plain", "live_four")], "bytes"),
    "compact_gather": (1, ZERO_TO_TWO, [("er300k", "planned", "live_four"), ("er100k", "plain", "trained")], "compact gather or table tiles"),
    "compact_min_n": (0, (300_000, 300_001, 1 << 30), [("er300k", "compact_bound", "trained")], "n"),
    "compact_first_forward_entries": (1, (0, 1_000_000, 100_000_000), [("er300k", "in_forwards", "live_four")], "entries"),
    "plan_chunk_rows": (0, (16, 48, 4096), [("er300k", "planned", "trained")], "lds table"),
    "overlap_dense": (1, BOOL, [("er300k", "planned", "live_four")], "compact gather"),
    "lds_table": (1, ZERO_TO_TWO, [("er300k", "planned", "dense_3_0.35"), ("rmat13", "predict", "trained")], "lds table or long rows"),
    "lds_table_bits": (0, (8, 10, 16), [("er300k", "planned", "trained")], "lds table"),
    "lds_table_min_chunks": (128, (1, 100_000), [("er300k", "planned", "live_four")], "lds table"),
    "blocked_stage0": (1, ZERO_TO_TWO, [("er300k", "blocked", "trained")], "blocked"),
    "block_cols": (65536, (0, 1024, 1 << 22), [("er300k", "blocked", "dense_3_0.35")], "blocked"),
    "blocked_min_n": (0, (300_000, 300_001, 1 << 30), [("er300k", "planned", "trained")], "n"),
    "plans_at_handoff": (2, ZERO_TO_TWO, [("er300k", "planned", "live_four")], "lds table"),
    "handoff_min_entries": (0, (1, 1_000_000, 100_000_000), [("er300k", "handoff_1", "trained")], "entries"),
    "pilot_rows": (65536, (0, 64, 1 << 30), [("er300k", "planned", "live_four")], "compact gather"),
    "dense_skip_zeros": (1, BOOL, [("er300k", "planned", "trained"), ("er100k", "plain", "dense_3_0.35")], "compact gather or table tiles"),
    "mfma_dense": (2, ZERO_TO_TWO, [("er300k", "planned", "live_four"), ("er100k", "plain", "trained"), ("hub4096", "hubs", "dense_3_0.35")],
                   "compact gather or table tiles or giant rows"),
    "kernel_trace": (0, BOOL, [("er100k", "plain", "trained")], "table tiles"),
    "forward_timing": (0, ZERO_TO_TWO, [("er300k", "planned", "trained")], "lds table"),
    "verdict_period": (8, (1, 64), [("er300k", "planned", "dense_3_0.35")], "compact gather"),
    # ---- wide tiles: er1933
    "wide_tiles": (1, BOOL, [("er1933", "plain", "trained")], "wide tiles"),
    "wide_tiles_max_n": (49152, (0, 1932, 1933, 1 << 30), [("er1933", "plain", "dense_3_0.35")], "n"),
    "wide_tiles_max_n_f16": (131072, (0, 1932, 1933, 1 << 30), [("er1933", "plain", "live_four")], "n"),
}

# the keys of kOptionRows that no directed case flips, one reason each
EXCLUDED = {
    "audit_period": "the audit's own tests flip it between forwards (tests/test_gpu_audit.py)",
    "audit_repair": "tests/test_gpu_audit.py",
    "audit_flip_stage": "a test hook that makes a forward wrong on purpose (tests/test_gpu_audit.py)",
    "audit_flip_row": "as audit_flip_stage",
    "audit_quiet": "tests/test_gpu_audit.py",
    "audit_log": "writes to stderr only (tests/test_gpu_audit.py)",
    "generic_stages": "the generic path has its own lifecycle tests (tests/test_gpu_generic_lifecycle.py)",
    "poison_features": "1 in every case: the tests depend on it, flipping it off would only hide an unwritten row",
}

# Read-outs that show a case reached its transition.  after[(key, graph)] = {flip value: [expect steps behind that flip's forwards]};
# "table_tiles" and "wide_tiles" run the sequence of _transition_steps instead: a key read at hand-off shows at the next one.
AFTER_SETTLE = {
    ("wide_tiles", "er1933"): [("expect", "wide_tiles_used", 1)],
    ("table_tiles", "er100k"): [("expect", "table_tiles_active", 1)],
    ("lds_table", "er300k"): [("expect", "lds_table_active", 1), ("expect", "lds_table_last_ok", 1)],
    ("compact_gather", "er300k"): [("expect", "compact_gather_active", 1)],
    ("giant_row_threshold", "hub4096"): [("expect", "giant_rows", 3)],
    ("blocked_stage0", "er300k"): [("expect", "blocked_stage0_active", 1)],
    ("block_cols", "er300k"): [("expect", "blocked_stage0_active", 1)],
    ("prune_predict", "rmat13"): [("expect", "pruned_predicted_stage1", 1), ("expect", "pruned_last_ok_stage1", 1)],
    ("prune_zero_rows", "rmat13"): [("expect", "pruned_stage1", 1), ("expect", "pruned_last_ok_stage1", 1)],
    ("sorted_long_row_threshold", "rmat13"): [("expect", "sorted_tiles_active", 1), ("expect", "pruned_stage1", 1)],
}


def _transition_steps(key, graph):
    """Steps in front of the flip back: the withdrawal and the engagement the case is named for, shown by read-outs."""
    if (key, graph) == ("wide_tiles", "er1933"):
        # read inside every stage call: off, the same graph again (the read-out says "since the graph was handed over"), two forwards
        # without wide tiles — then on under the resident graph, and the next forward runs on them
        return [("set", key, 0), ("reupload",), ("forward", "x"), ("forward", "x"), ("expect", "wide_tiles_used", 0),
                ("set", key, 1), ("forward", "x"), ("expect", "wide_tiles_used", 1)]
    if (key, graph) == ("table_tiles", "er100k"):
        # read when a graph is handed over: a resident graph keeps its tiles, the next hand-off withdraws them
        return [("set", key, 0), ("forward", "x"), ("expect", "table_tiles_active", 1), ("reupload",), ("expect", "table_tiles_active", 0),
                ("forward", "x"), ("forward", "x"), ("set", key, 1), ("forward", "x"), ("expect", "table_tiles_active", 0)]
    if (key, graph) == ("lds_table", "er300k"):
        return [("set", key, 0), ("forward", "x"), ("reupload",), ("expect", "lds_table_active", 0), ("forward", "x"), ("forward", "x")]
    if (key, graph) == ("compact_gather", "er300k"):
        return [("set", key, 0), ("forward", "x"), ("reupload",), ("expect", "compact_gather_active", 0), ("forward", "x"), ("forward", "x")]
    if (key, graph) == ("giant_row_threshold", "hub4096"):
        return [("set", key, 5000), ("forward", "x"), ("expect", "giant_rows", 3), ("reupload",), ("expect", "giant_rows", 0), ("forward", "x")]
    if (key, graph) == ("prune_predict", "rmat13"):
        return [("set", key, 0), ("forward", "x"), ("reupload",), ("expect", "pruned_predicted_stage1", 0), ("forward", "x")]
    return []


def _base(b):
    return dict(BASES[b]) if isinstance(b, str) else dict(b)


def _range(rng, n, whole):
    """A 64-aligned row range of a graph of n rows: the whole graph, or a sub-range of at least 64 rows that ends at a multiple of 64 or at n."""
    if whole or n < 192:
        return 0, n
    tiles = (n + 63) // 64
    a = int(rng.integers(0, tiles - 1))
    b = int(rng.integers(a + 1, tiles + 1))
    return 64 * a, min(n, 64 * b)


def _directed_list():
    out = []
    for key, (first, domain, places, _) in KEYS.items():
        for graph, base, model in places:
            out.append((key, graph, base, model))
    return out


DIRECTED = _directed_list()
N_RANDOM = 24
# the keys a multi-device handle hands on to its parts (kFxForward) that touch row classes or queues: hub4096 behind three parts
MULTI = ["long_row_threshold", "giant_row_threshold", "side_streams", "long_rows_on_main", "prune_zero_rows", "mfma_dense"]
# cases kept by name after they showed a defect of the engine: what it was -> index
#   random_2: "plan_chunk_rows" 16 on er300k gives the compact table 18 750 chunks; the last stage, run round by round (256 chunks a
#   round, "overlap_dense"), needed 74 round counters of 64 and the forward was refused with GNNVC_ERR_UNSUPPORTED
REGRESSIONS = {"more rounds of the compact-table plan than round counters": len(DIRECTED) + 2}
# the weight scale under the LDS table: (graph, base, model) — er300k's table follows the scale to ten and sixteen bits, the skewed
# graphs' (dealt from the degree-sorted list, a byte per entry or none) steps aside
SCALE = [("er300k", "planned", "trained"), ("er300k", "planned", "live_four"), ("rmat13", "predict", "dense_3_0.35"),
         ("hub4096", dict(HUBS, blocked_min_n=0), "trained")]
N = len(DIRECTED) + N_RANDOM + len(MULTI) + len(SCALE)


def _directed(i):
    key, graph, base, model = DIRECTED[i]
    first, domain, _, _ = KEYS[key]
    rng = np.random.default_rng(SEED + i)
    n = GRAPH_N[graph]
    options = _base(base)
    options.pop(key, None)
    options["poison_features"] = 1
    options[key] = first          # (last: an explicit threshold holds whatever was set before it)
    settle = int(rng.integers(3, 11))
    steps = [("forward", "x")] * settle + list(AFTER_SETTLE.get((key, graph), []))
    for j, v in enumerate(v for v in domain if v != first):
        steps += [("set", key, int(v)), ("forward", "x"), ("forward", "x"), ("forward", "other")]
        for st in (1, 2):   # one call per 16-wide stage: the whole graph (where the whole-graph plans apply) and a sub-range in turn
            steps.append(("stage", st) + _range(rng, n, whole=(j + st) % 2 == 0))
    steps += _transition_steps(key, graph)
    others = [int(v) for v in domain if v != first]
    for j, v in enumerate(others):   # between a hand-off and its first forward: the key moves there and back under the plans of the first forwards
        steps += [("set", key, int(first)), ("reupload", "plain"), ("set", key, v), ("forward", "x"), ("forward", "other"),
                  ("stage", 1 + j % 2) + _range(rng, n, whole=j % 2 == 1)]
    for v in others:                 # across a hand-off: the engine is a fresh one's with the same set calls, whatever the value
        steps += [("set", key, v), ("reupload",), ("forward", "other")]
    steps += [("set", key, int(first)), ("forward", "x"), ("forward", "x"), ("reupload",)]
    again = sum(1 for k, g, _, _ in DIRECTED[:i] if (k, g) == (key, graph))   # (a key twice on one graph: under another base)
    name = f"directed_{key}_{graph}" + (f"_{again + 1}" if again else "")
    return Case(i, name, "directed", key, graph, model, options, tuple(steps), ())


# tests/test_gpu_fuzz.py::_options' value choices (tests/test_option_flips_inputs.py holds this table to that function)
CHOICES = {
    "prune_min_drop_percent": list(range(30)),
    "long_row_threshold": [0, 8, 40, 64, 128, 256, 512],
    "sorted_long_row_threshold": [64, 256, 512, 1024, 2048],
    "giant_row_threshold": [0, 64, 300, 1000, 4096, 16384],
    "giant_row_threshold_f16": [64, 1000, 5000, 65536],
    "giant_segments": [-1, 0, 1],
    "sorted_tiles": [-1, 0, 1],
    "prune_zero_rows": [0, 1],
    "prune_class_by_entries_left": [0, 1],
    "prune_giant_rows": [0, 1],
    "prune_heavy_entries": [1, 1 << 24],
    "lds_table": [0, 1],
    "lds_table_skewed_rows": [0, 64, 512, 2048, 16384],
    "compact_gather": [0, 1],
    "mfma_dense": [0, 1, 2],
    "overlap_dense": [0, 1],
    "plan_chunk_rows": [16, 48, 256, 4096],
    "table_tiles": [0, 1],
    "table_tiles_min_n": [0, 49152],
    "table_tiles_solo": [0, 1],
    "wide_tiles": [0, 1],
}
# ... and the keys read inside a forward that _options leaves alone, over their whole domains
CHOICES_MORE = {"side_streams": [0, 1], "long_rows_on_main": [-1, 0, 1], "giant_gather_first": [-1, 0, 1], "dense_skip_zeros": [0, 1],
                "filter_zero_rows": [0, 1], "filter_keep_lists": [0, 1], "prune_predict": [0, 1], "pilot_rows": [0, 64, 65536],
                "plans_at_handoff": [0, 1, 2], "blocked_stage0": [0, 1, 2], "lds_table_skewed": [0, 1]}


def _draw_sets(rng, count):
    table = dict(CHOICES, **CHOICES_MORE)
    keys = sorted(table)
    picked = [keys[int(k)] for k in rng.choice(len(keys), count, replace=False)]
    return [("set", k, int(table[k][int(rng.integers(len(table[k])))])) for k in picked]


def _random(i):
    rng = np.random.default_rng(SEED + i)
    cls = int(rng.integers(len(CLASS_ORDER)))
    pick = lambda c: CLASSES[CLASS_ORDER[c % 3]][int(rng.integers(len(CLASSES[CLASS_ORDER[c % 3]])))]
    graph = first_graph = pick(cls)
    model = MODELS[int(rng.integers(len(MODELS)))]
    options = dict(PLANNED if rng.random() < 0.5 else PREDICT)
    options["prune_min_entries"] = 0
    for _, k, v in _draw_sets(rng, int(rng.integers(3, 9))):
        options[k] = v
    options["poison_features"] = 1
    steps = [("forward", "x")] * int(rng.integers(1, 4))
    length = int(rng.integers(12, 21))
    while len(steps) < length - 2:
        r = rng.random()
        if r < 0.34:
            steps += _draw_sets(rng, int(rng.integers(1, 4)))
            steps.append(("forward", "x" if rng.random() < 0.7 else "other"))
        elif r < 0.54:
            steps.append(("forward", "x" if rng.random() < 0.6 else "other"))
        elif r < 0.66:
            steps.append(("stage", int(rng.integers(0, 3))) + _range(rng, GRAPH_N[graph], whole=rng.random() < 0.4))
        elif r < 0.76:
            steps.append(("reupload",))
        elif r < 0.88:
            cls += 1
            graph = pick(cls)
            steps.append(("graph", graph))
        elif r < 0.94:
            steps.append(("weight_scale", SCALES[int(rng.integers(len(SCALES)))]))
            steps.append(("forward", "x"))
        else:
            steps.append(("stream", "caller"))
            steps.append(("forward", "x"))
            steps.append(("stream", "own"))
    steps += [("forward", "x"), ("forward", "other")]
    return Case(i, f"random_{i - len(DIRECTED)}", "random", None, first_graph, model, options, tuple(steps), ())


def _multi(i):
    key = MULTI[i - len(DIRECTED) - N_RANDOM]
    first, domain, _, _ = KEYS[key]
    options = dict(HUBS)
    options.pop(key, None)
    options["poison_features"] = 1
    options[key] = first
    steps = [("forward", "x")] * 3
    for v in domain:
        if v != first:
            steps += [("set", key, int(v)), ("forward", "x"), ("forward", "x"), ("forward", "other")]
    steps += [("set", key, int(first)), ("forward", "x"), ("forward", "x")]
    model = MODELS[(i - len(DIRECTED) - N_RANDOM) % len(MODELS)]
    return Case(i, f"multi_{key}_hub4096", "multi", key, "hub4096", model, options, tuple(steps), ())


def _scale(i):
    j = i - len(DIRECTED) - N_RANDOM - len(MULTI)
    graph, base, model = SCALE[j]
    rng = np.random.default_rng(SEED + i)
    n = GRAPH_N[graph]
    options = _base(base)
    options["poison_features"] = 1
    uniform = graph in CLASSES["uniform"]
    steps = [("forward", "x")] * 3 + [("expect", "lds_table_active", 1), ("expect", "lds_table_bits", 8), ("expect", "lds_table_last_ok", 1)]
    for m, bits in ((3, 10), (9, 16), (1, 8), (9, 16), (3, 10), (1, 8)):
        steps += [("weight_scale", m), ("forward", "x"), ("forward", "x"), ("forward", "other"), ("stage", 0, 0, n),
                  ("stage", 1) + _range(rng, n, whole=False), ("stage", 2, 0, n), ("reupload",)]
        steps += [("expect", "lds_table_bits", bits)] if uniform else [("expect", "lds_table_active", 1 if bits == 8 else 0)]
        steps += [("forward", "x"), ("forward", "other")]
    return Case(i, f"scale_{graph}_{model}", "scale", None, graph, model, options, tuple(steps), ())


_cases = {}


def case(i):
    if i not in _cases:
        if not 0 <= i < N:
            raise IndexError(i)
        first_multi = len(DIRECTED) + N_RANDOM
        _cases[i] = (_directed(i) if i < len(DIRECTED) else _random(i) if i < first_multi else _multi(i) if i < first_multi + len(MULTI)
                     else _scale(i))
    return _cases[i]


def long_case(seed):
    """A random case beyond the pinned ones (python -m tests.flip_harness --from A --to B): seed >= N."""
    c = _random(seed)
    return c._replace(name=f"long_{seed}")


def directed_indices():
    return list(range(len(DIRECTED)))


def random_indices():
    return list(range(len(DIRECTED), len(DIRECTED) + N_RANDOM))


def multi_indices():
    return list(range(len(DIRECTED) + N_RANDOM, len(DIRECTED) + N_RANDOM + len(MULTI)))


def scale_indices():
    return list(range(len(DIRECTED) + N_RANDOM + len(MULTI), N))


def covered_keys():
    return {k for k, _, _, _ in DIRECTED}


def describe(c):
    return f"case {c.index} {c.name}: {c.kind}, graph {c.graph}, model {c.model}, options {c.options}"
