"""Every option key gnnvc_set_option accepts (single engines and the multi-device handle's own) is described in include/gnnvc.h —
the header is the ABI's documentation, and an option nobody can look up is a knob nobody can trust."""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parents[1]

# the keys, as they were when an if-chain in gnnvc_set_option held them: a table row added or lost shows here
KEYS = [
    "audit_flip_row", "audit_flip_stage", "audit_log", "audit_period", "audit_quiet", "audit_repair", "block_cols",
    "blocked_min_n", "blocked_stage0", "compact_first_forward_entries", "compact_gather", "compact_min_n",
    "dense_skip_zeros", "filter_keep_lists", "filter_min_entries", "filter_min_long_percent", "filter_min_percent",
    "filter_zero_rows", "forward_timing", "generic_stages", "giant_gather_first", "giant_row_threshold",
    "giant_row_threshold_f16", "giant_segments", "handoff_min_entries", "kernel_trace", "lds_table",
    "lds_table_bits", "lds_table_min_chunks", "lds_table_skewed", "lds_table_skewed_rows", "long_row_threshold",
    "long_rows_on_main", "mfma_dense", "multi_announce", "multi_only_part", "multi_pack", "multi_pieces",
    "multi_push", "overlap_dense", "pilot_rows", "plan_chunk_rows", "plans_at_handoff", "poison_features",
    "prune_class_by_entries_left", "prune_early_entries", "prune_giant_rows", "prune_heavy_entries",
    "prune_min_drop_percent", "prune_min_entries", "prune_predict", "prune_predict_min_entries", "prune_zero_rows",
    "side_streams", "sorted_long_row_threshold", "sorted_min_nnz", "sorted_tiles", "table_tiles",
    "table_tiles_max_bytes", "table_tiles_min_n", "table_tiles_solo", "verdict_period", "wide_tiles",
    "wide_tiles_max_n", "wide_tiles_max_n_f16",
]


def _table_keys(path, table):
    """The first field of every row of `static const ... <table>[] = { {"key", ...}, ... };` in `path`."""
    src = (ROOT / "gnn-mwvc_amd" / "csrc" / path).read_text()
    body = src[src.index(f" {table}[] = {{"):]
    body = body[:body.index("\n};")]
    return re.findall(r'^\s*\{"([a-z0-9_]+)",', body, flags=re.M)


def _set_option_keys():
    return _table_keys("gnnvc_options.h", "kOptionRows") + _table_keys("gnnvc_multi.cpp", "kMultiRows")


def test_every_settable_option_is_in_the_header():
    header = (ROOT / "include" / "gnnvc.h").read_text()
    keys = _set_option_keys()
    assert sorted(set(keys)) == sorted(KEYS)
    missing = [k for k in keys if f'"{k}"' not in header]
    assert not missing, missing


def test_no_key_has_two_rows():
    for path, table in (("gnnvc_options.h", "kOptionRows"), ("gnnvc_multi.cpp", "kMultiRows")):
        keys = _table_keys(path, table)
        assert len(keys) == len(set(keys)), sorted(k for k in keys if keys.count(k) > 1)
