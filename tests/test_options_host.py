"""gnnvc_set_option's table (gnn-mwvc_amd/csrc/gnnvc_options.h) on the host: tests/support/options_host.cpp, a program of its
own built with the address and undefined-behaviour sanitizers, feeds every key the values -5, 0, 1, 2, 3, 64, 101, 65536 and
2^40 and prints, per key, what each written member of gnnvc::Options then holds ("-" = left alone) and the effects the engine is
told to apply.  EXPECTED is what the if-chain this table replaced did with the same inputs: the members, and the effects that show
on an engine (short lists dropped, pruned plans forgotten, sorted ranges invalidated, audit calls recounted, the long / giant
thresholds made explicit), were printed by a program linked against that library, run on a default-constructed engine (no
multi-device handle: gnnvc_set_option then makes no HIP call); what a multi-device handle does with the key (multi_*) was read
off the chain — every key below its "forward_timing" branch and the ones that returned multi_set_option's code forward.
"lds_table_bits" takes none of those nine values, so the program feeds it 8, 10, 12 and 16 besides (the last line; expected values
printed the same way)."""
import pathlib
import subprocess

import pytest

HERE = pathlib.Path(__file__).resolve().parent
SRC = HERE / "support" / "options_host.cpp"
HDR = HERE.parent / "gnn-mwvc_amd" / "csrc" / "gnnvc_options.h"
EXE = HERE / "support" / "options_host"

EXPECTED = """\
poison_features poison=1,0,1,1,1,1,1,1,1 fx=multi_forward
verdict_period verdict_period=1,1,1,2,3,64,64,64,64 fx=multi_forward
audit_period audit_period=0,0,1,2,3,64,101,65536,2147483647 fx=audit_restart+multi_parts_elsewhere
generic_stages generic=0,0,1,2,2,2,2,2,2 fx=multi_front_only
audit_log audit_log=1,0,1,1,1,1,1,1,1 fx=multi_front_only
audit_repair audit_repair=1,0,1,1,1,1,1,1,1 fx=multi_forward
audit_flip_stage audit_flip_stage=-1,0,1,2,3,64,64,64,64 fx=multi_forward
audit_flip_row audit_flip_row=4294967295,0,1,2,3,64,101,65536,4294967295 fx=multi_forward
audit_quiet audit_quiet=1,0,1,1,1,1,1,1,1 fx=multi_forward
forward_timing timing=0,0,1,2,2,2,2,2,2 fx=multi_forward
blocked_stage0 blocked=0,0,1,2,2,2,2,2,2 fx=short_lists+multi_forward
block_cols block_cols=0,0,1,2,3,64,101,65536,0 fx=short_lists+multi_forward
blocked_min_n blocked_min_n=0,0,1,2,3,64,101,65536,0 fx=short_lists+multi_forward
compact_min_n compact_min_n=0,0,1,2,3,64,101,65536,0 fx=short_lists+multi_forward
compact_first_forward_entries compact_first_entries=0,0,1,2,3,64,101,65536,1099511627776 fx=short_lists+multi_forward
plan_chunk_rows plan_chunk_rows=0,0,1,2,3,64,101,65536,0 fx=short_lists+multi_forward
overlap_dense overlap=1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
long_row_threshold long_thresh=0,0,1,2,3,64,101,65536,0 long_auto=0,0,0,0,0,0,0,0,0 fx=short_lists+long_explicit+multi_forward
giant_row_threshold giant_thresh=0,0,64,64,64,64,101,65536,0 giant_f16=1,1,64,64,64,64,101,65536,1 giant_f16_auto=0,0,0,0,0,0,0,0,0 fx=short_lists+giant_explicit+multi_forward
giant_row_threshold_f16 giant_f16=1,1,1,2,3,64,101,65536,0 giant_f16_auto=0,0,0,0,0,0,0,0,0 fx=short_lists+forget_pruned+giant_explicit+multi_forward
giant_segments giant_segments=-1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
side_streams side_streams=1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
kernel_trace ktrace=1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
compact_gather compact=0,0,1,2,2,2,2,2,2 fx=short_lists+multi_forward
prune_zero_rows prune=0,0,1,1,1,1,1,1,1 fx=short_lists+forget_pruned+multi_forward
prune_class_by_entries_left prune_eff=1,0,1,1,1,1,1,1,1 fx=short_lists+forget_pruned+multi_forward
prune_heavy_entries prune_heavy_entries=0,0,1,2,3,64,101,65536,1099511627776 fx=short_lists+forget_pruned+multi_forward
prune_early_entries prune_early_nnz=0,0,1,2,3,64,101,65536,1099511627776 fx=short_lists+multi_forward
prune_giant_rows prune_giant=1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
prune_predict prune_predict=1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
wide_tiles wide=1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
wide_tiles_max_n wide_max_n=0,0,1,2,3,64,101,65536,0 fx=short_lists+multi_forward
wide_tiles_max_n_f16 wide_max_n16=0,0,1,2,3,64,101,65536,0 fx=short_lists+multi_forward
dense_skip_zeros dense_skip=1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
table_tiles t4=1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
table_tiles_solo t4_solo=1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
table_tiles_min_n t4_min_n=0,0,1,2,3,64,101,65536,0 fx=short_lists+multi_forward
table_tiles_max_bytes t4_max_bytes=0,0,1,2,3,64,101,65536,1099511627776 fx=short_lists+multi_forward
prune_predict_min_entries predict_min_nnz=0,0,1,2,3,64,101,65536,1099511627776 fx=short_lists+multi_forward
giant_gather_first giant_gather_first=-1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
long_rows_on_main long_on_main=-1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
filter_zero_rows filter=1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
filter_keep_lists filter_keep=1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
filter_min_entries filter_min_nnz=0,0,1,2,3,64,101,65536,1099511627776 fx=short_lists+multi_forward
filter_min_long_percent filter_min_long_pct=0,0,1,2,3,64,101,101,101 fx=short_lists+multi_forward
filter_min_percent filter_min_pct=0,0,1,2,3,64,101,101,101 fx=short_lists+multi_forward
prune_min_entries prune_min_nnz=0,0,1,2,3,64,101,65536,1099511627776 fx=short_lists+multi_forward
prune_min_drop_percent prune_min_drop=0,0,1,2,3,64,100,100,100 fx=short_lists+multi_forward
lds_table_skewed lds_skewed=1,0,1,1,1,1,1,1,1 fx=short_lists+multi_forward
lds_table_skewed_rows lds_skewed_rows=0,0,1,2,3,64,101,65536,0 fx=short_lists+multi_forward
lds_table lds_table=0,0,1,2,2,2,2,2,2 fx=short_lists+multi_forward
lds_table_min_chunks lt_min_chunks=1,1,1,2,3,64,101,65536,0 fx=short_lists+multi_forward
lds_table_bits lt_bits=0,0,0,0,0,0,0,0,0 fx=short_lists+multi_forward
plans_at_handoff handoff=0,0,1,2,2,2,2,2,2 fx=short_lists+multi_forward
handoff_min_entries handoff_min_nnz=0,0,1,2,3,64,101,65536,1099511627776 fx=short_lists+multi_forward
pilot_rows pilot_rows=0,0,1,2,3,64,101,65536,0 fx=short_lists+multi_forward
sorted_min_nnz sorted_min_nnz=0,0,1,2,3,64,101,65536,1099511627776 fx=short_lists+multi_forward
sorted_long_row_threshold sorted_long_thresh=1,1,1,2,3,64,101,65536,0 long_auto=0,0,0,0,0,0,0,0,0 fx=short_lists+long_explicit+multi_forward
mfma_dense mfma=2,0,1,2,2,2,2,2,2 fx=short_lists+multi_forward
sorted_tiles sorted=-1,0,1,1,1,1,1,1,1 fx=short_lists+sorted_stale+multi_forward
lds_table_bits@8,10,12,16 lt_bits=8,10,0,16 fx=short_lists+multi_forward
"""


@pytest.fixture(scope="module")
def printed():
    if not EXE.exists() or EXE.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-o", str(EXE), str(SRC)], check=True)
    r = subprocess.run([str(EXE)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr     # (a sanitizer report ends the program with a non-zero code)
    return r.stdout


def test_every_key_writes_what_it_wrote_before(printed):
    got = dict(line.split(" ", 1) for line in printed.splitlines())
    want = dict(line.split(" ", 1) for line in EXPECTED.splitlines())
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def test_the_options_header_needs_nothing_of_hip():
    text = HDR.read_text()
    assert "#include <hip" not in text and "#include \"gnnvc_" not in text
