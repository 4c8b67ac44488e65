"""One engine of the trained model, handed graph after graph: after every hand-off it is in the state of a fresh engine.

csrc/gnnvc_engine_state.h keeps what is known about the resident graph in gnnvc_engine::PerGraph, which every hand-off replaces
(reset_graph_state).  tests/flip_harness.py states the property — "a graph handed over afterwards leaves the engine in the state
of a fresh one" — on fifteen read-outs; here it is held on every gnnvc_get_info key that takes neither a stage index nor a part
index (KEYS, written out below), across the graphs of tests/test_modelgen.py::GRAPHS on which each per-graph plan engages:

  hub4096   long and giant rows, pruned adjacency                        (upload)
  er300k    LDS table, compact table                                      (staged: the plans begin while the columns arrive)
  er100k    table tiles                                                   (upload)
  er1933    wide tiles                                                    (staged)
  a graph of no vertices                                                  (upload)
  rmat13    skewed: long rows, sorted and interleaved tiles, pruned adjacency   (staged)
  an empty slice of rmat13 at the front (row_hi == 0), then one in the middle (row_lo == row_hi > 0), gnnvc_attach_graph_slice

The options are the ones tools/optionflips.py engages the plans with on its graph classes (PLANNED and PREDICT together,
"poison_features" 1), the two size bounds at 200 000 vertices instead of 0: with them at 0 the LDS-table and compact-table plans
would take er100k and er1933 as well, and neither table tiles nor wide tiles would be seen; and "sorted_min_nnz" 0, under which the
tile waste alone decides on sorted tiles (rmat13 has them; hub4096's natural tiles waste 1.8 x, below the rule's 2, so it has none
under any one option set that leaves er300k its plans).  ENGAGES holds each graph to the plans it is in the sequence for, so that
the comparison cannot come down to zeros against zeros.

After every hand-off a second engine is opened, given the same gnnvc_set_option calls and handed the same graph the same way
(by gnnvc_upload_graph where the first was staged, as tests/flip_harness.py does): every key of KEYS agrees, and on a graph that
has vertices again after three forwards on both.  Every forward: logits bit for bit the oracle's, scores within 1 ulp
(flip_harness.Run.forward).  Left out, and nothing else:

  plan_build_us, handoff_build_us, handoff_early_us, multi_last_forward_us   wall-clock times
  side_queue_probes       how many streams the runtime made the engine try until one ran beside the main stream: the placement of
                          queues depends on what else the process has open, not on the engine's state
  flip_harness.CARRIED_BY_TABLE_TILES   under that module's own condition: the first engine carries a choice of columns and the
                          graph has table tiles"""
import numpy as np
import pytest

from tools import optionflips as of
from tools import graphgen as gg
from tests import flip_harness as fh
from tests.test_expf_restatement import shim   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)

pytestmark = pytest.mark.gpu

OPTIONS = {**of.PLANNED, **of.PREDICT, "blocked_min_n": 200_000, "compact_min_n": 200_000, "sorted_min_nnz": 0, "poison_features": 1}
MODEL = "trained"
STEPS = ["hub4096", "er300k", "er100k", "er1933", "no_vertices", "rmat13", "rmat13_empty_front", "rmat13_empty_middle"]

# every gnnvc_get_info key without a stage or part index (csrc/gnnvc_engine.cpp: gnnvc_get_info), in its order there
KEYS = [
    "devices", "generic_stages", "plans_at_handoff", "mfma_dense", "generic_stages_model", "generic_stages_active",
    "generic_max_dense_layers", "generic_heavy_from", "generic_heavy_rows", "generic_heavy_entries", "generic_heavy_last_rows",
    "generic_giant_from", "generic_giant_segments", "generic_giant_rows", "generic_giant_entries", "generic_giant_last_rows",
    "generic_giant_last_segmented", "generic_big_lds", "generic_feature_width", "generic_patterns", "generic_live_columns",
    "audit_runs", "audit_failures", "audit_repairs", "audit_nan_pairs", "audit_last_stage", "audit_last_row", "audit_last_col",
    "audit_last_mismatches", "audit_last_fused_bits", "audit_last_plain_bits", "dense_skip_layers",
    "compact_gather_active", "compact_gather_chunks", "compact_gather_block_cols", "compact_gather_rows_per_chunk",
    "compact_gather_steps", "pruned_stage1", "pruned_stage2", "side_queue_runs_beside", "long_entries_percent",
    "filtered_stage1", "filtered_stage2", "short_lists_stage1", "short_lists_stage2", "filter_mass_percent_stage1",
    "filter_mass_percent_stage2", "pruned_vertices_stage1", "pruned_vertices_stage2", "pruned_entries_stage1",
    "pruned_entries_stage2", "pruned_predicted_stage1", "pruned_borrowed_stage2", "pruned_from_previous_stage2",
    "pruned_last_ok_stage1", "pruned_last_ok_stage2", "wide_tiles_used", "table_tiles_active", "table_tiles_fit_stage1",
    "table_tiles_fit_stage2", "lds_table_off", "lds_table_bits", "compact_gather_off_stage1", "compact_gather_off_stage2",
    "compact_gather_blocks", "compact_gather_last_ok", "compact_gather_last_dirty", "compact_gather_last_passes",
    "compact_table_written_by_producer", "plan_memsets_last_forward", "lds_table_active", "lds_table_last_ok", "lds_table_mapped",
    "lds_table_blocks", "lds_table_chunks", "lds_table_steps", "blocked_stage0_active", "blocked_blocks", "block_cols", "long_rows",
    "graph_uses", "slice_rows", "slice_entries", "giant_rows", "giant_segments", "giant_entries", "giant_row_threshold",
    "sorted_tiles_active", "tile_waste_x100", "heavy_tail_x1000", "interleaved_tiles", "long_row_threshold",
]
LEFT_OUT = {
    "plan_build_us": "wall-clock time", "handoff_build_us": "wall-clock time", "handoff_early_us": "wall-clock time",
    "multi_last_forward_us": "wall-clock time",
    "side_queue_probes": "the runtime's placement of queues, which follows what else the process has open",
}
assert not set(KEYS) & set(LEFT_OUT)
# what shows that a graph's plans engaged: {graph: (read-outs at hand-off, read-outs after the forwards)}, 1 or "some" (> 0)
ENGAGES = {
    "hub4096": ({"long_rows": "some", "giant_rows": "some"}, {"pruned_stage1": 1}),
    "er300k": ({"lds_table_active": 1, "compact_gather_active": 1}, {"lds_table_last_ok": 1}),
    "er100k": ({"table_tiles_active": 1}, {"table_tiles_fit_stage1": 1}),
    "er1933": ({}, {"wide_tiles_used": 1}),
    "rmat13": ({"long_rows": "some", "sorted_tiles_active": 1, "interleaved_tiles": 1}, {"pruned_stage1": 1}),
}


def no_vertices():
    z = np.zeros(0, dtype=np.uint32)
    return gg.CsrGraph(n=0, rowptr=np.zeros(1, dtype=np.uint64), col=z, w=z, nw=z)


class Sequence:
    """STEPS on one engine, each run once and in order whichever test asks first."""

    def __init__(self, shim):
        case = of.Case(0, "graph_changes", "random", None, STEPS[0], MODEL, dict(OPTIONS), (), ())
        self.run = fh.Run(case, shim)
        self.done = 0
        self.keep = []

    def close(self):
        self.run.close()

    def hand_over(self, e, step, staged):
        r = self.run
        if step == "no_vertices":
            e.upload_graph(no_vertices())
        elif step.startswith("rmat13_empty"):
            import torch
            n = of.GRAPH_N["rmat13"]
            lo = 0 if step.endswith("front") else n // 2
            rp = torch.zeros(4, dtype=torch.int32, device="cuda:0")     # (no rows: no row pointer, weight or column is read)
            col = torch.zeros(64, dtype=torch.int32, device="cuda:0")
            self.keep += [rp, col]
            e.attach_graph_slice(n, lo, lo, 0, rp.data_ptr(), col.data_ptr(), 0, 0)
        else:
            r.graph = step
            r.hand_over(e, staged=staged)

    def fresh(self, step):
        import gnn_mwvc_amd as G
        e = G.Engine(fh.model_text(MODEL), device=0)
        try:
            for k, v in self.run.history:
                e.set_option(k, v)
            self.hand_over(e, step, staged=False)
        except BaseException:
            e.close()
            raise
        return e

    def compare(self, f, when, left_out=()):
        r = self.run
        a, b = fh.readouts(r.e, KEYS, left_out), fh.readouts(f, KEYS, left_out)
        r.check(a == b, f"{when}: read-outs differ from a fresh engine's with the same options (this engine's, the fresh one's): {fh._diff(a, b)}")
        return a

    def engaged(self, got, expect, when):
        expect = {k: v for k, v in expect.items() if k in got}   # (but what the table tiles carry, where that is left out)
        missing = {k: got[k] for k, v in expect.items() if not (got[k] > 0 if v == "some" else got[k] == v)}
        self.run.check(not missing, f"{when}: the plans this graph is in the sequence for did not engage, read-outs {missing} against {expect}")

    def step(self, i):
        r, step = self.run, STEPS[i]
        r.step = i
        if step in of.GRAPH_N:
            fh.want(MODEL, step)   # (the oracle's logits, once per session: tests/test_gpu_models.py::want_of)
        if i == 0:
            r.open()
        else:
            self.hand_over(r.e, step, staged=i % 2 == 1)
        r.forwards_here = 0
        f = self.fresh(step)
        try:
            a = self.compare(f, f"after the hand-off of {step}")
            if step not in of.GRAPH_N:
                return
            self.engaged(a, ENGAGES[step][0], f"after the hand-off of {step}")
            carried = fh.CARRIED_BY_TABLE_TILES if r.choice_carried and a["table_tiles_active"] == 1 else ()
            for _ in range(fh.FORWARDS_BEFORE_READOUT):
                r.forward("x")
                r.forward("x", e=f)
            a = self.compare(f, f"after {fh.FORWARDS_BEFORE_READOUT} forwards on {step}", carried)
            self.engaged(a, ENGAGES[step][1], f"after {fh.FORWARDS_BEFORE_READOUT} forwards on {step}")
        finally:
            f.close()

    def advance_to(self, i):
        while self.done <= i:
            self.done += 1
            self.step(self.done - 1)


@pytest.fixture(scope="module")
def sequence(shim):
    s = Sequence(shim)
    yield s
    s.close()


@pytest.mark.parametrize("i", range(len(STEPS)), ids=STEPS)
def test_handed_over_graph_leaves_a_fresh_engines_state(sequence, i):
    sequence.advance_to(i)


def test_the_key_list_is_the_engines():
    """KEYS and LEFT_OUT together are exactly the keys gnnvc_get_info spells out: one added there is compared here or left out with a reason."""
    import pathlib
    import re
    src = (pathlib.Path(__file__).resolve().parents[1] / "gnn-mwvc_amd" / "csrc" / "gnnvc_engine.cpp").read_text()
    body = src[src.index("int gnnvc_get_info("):src.index("int gnnvc_num_layers(")]
    assert set(re.findall(r'k == "(\w+)"', body)) == set(KEYS) | set(LEFT_OUT)
