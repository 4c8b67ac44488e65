"""Giant rows of generic stages (gnnvc_set_generic_giant_rows): listed heavy rows of at least the giant threshold are gathered
column-major into a slab (k_any_giant_gather), summed by the exact parallel scan (k_giant_segsum / k_giant_segmap / k_giant_sum)
and their sums placed where the listed rows' k_stage_any launch reads them (k_any_giant_place).

The bars are those of tests/test_gpu_heavy_rows.py and no wider: logits and every stage's output bit for bit against the oracle,
scores through check_scores, rows outside a stage call's ranges and the pad row untouched — for EVERY pair (threshold, segments),
threshold 0 (no giant route) included, and the results of all settings equal to each other.  Models as there: stage inputs
1 .. 32 wide.

The graph and the crafted inputs come from tools/giant_rows_inputs.py (tests/test_giant_rows_inputs.py proves on the CPU that they
are what is needed here): 12 000 vertices, hubs 0 .. 7 of exactly 1023, 1024, 1025, 2049, 4096, 4097, 9000 and 0 entries — around
a window of the scan, around a segment, three segments, an empty row.

The last test is a speed guard: on the power-law graph of the heavy-rows guard (four hubs of 65 536 entries) the default
(16 384, -1) must not be slower than no giant route at all."""
import numpy as np
import pytest

from tools import giant_rows_inputs as gi
from tools import modelgen_depths as md
from tests import generic_harness as gh
from tests.generic_harness import bits, check_scores, crafted_input, degrees, graph_of, ulp
from tests.test_expf_restatement import shim, _run   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)

pytestmark = pytest.mark.gpu

# model -> family (the models of tests/test_gpu_heavy_rows.py)
MODELS = {"narrow": "shapes", "odd": "shapes", "wide": "shapes", "logit": "depths", "two_deep": "depths", "in3_f32": "depths"}
HEAVY_FROM = 512
GIANT_DEFAULT = 16384
GIANT_THRESHOLDS = [0, 1024, 1025, 4097, 16384]
SEGMENT_ADDENDS = 4096       # one segment of the scan: a stream is spread over several waves only when it is longer


def giant_counts(deg, heavy, thr):
    """(rows, entries) of the giant rows: degree >= max(thr, heavy), none when either is 0."""
    if not thr or not heavy:
        return 0, 0
    sel = deg >= max(thr, heavy)
    return int(sel.sum()), int(deg[sel].sum())


def segmented(deg, heavy, thr, seg):
    rows, _ = giant_counts(deg, heavy, thr)
    return int(seg == 1 and rows > 0 and int(deg.max()) > SEGMENT_ADDENDS)


def check_info(e, deg, heavy, thr, seg, label):
    rows, entries = giant_counts(deg, heavy, thr)
    assert e.get_info("generic_giant_from") == thr and e.get_info("generic_giant_segments") == seg, label
    assert e.get_info("generic_giant_last_rows") == rows, label
    assert e.get_info("generic_giant_rows") == rows, label
    assert e.get_info("generic_giant_entries") == entries, label
    assert e.get_info("generic_giant_last_segmented") == segmented(deg, heavy, thr, seg), label
    assert e.get_info("generic_heavy_last_rows") == int((deg >= heavy).sum()), label


def test_the_graph_is_what_the_name_says_and_the_defaults_are_the_trained_paths():
    import gnn_mwvc_amd as G
    deg = degrees(graph_of("giant_hubs"))
    assert deg[:8].tolist() == gi.HUB_DEGREES and deg[8:].max() < 64
    assert [giant_counts(deg, HEAVY_FROM, t)[0] for t in GIANT_THRESHOLDS] == [0, 6, 5, 2, 0]
    assert int((deg >= HEAVY_FROM).sum()) == 7
    e = G.Engine(gh.text_of("shapes", "narrow"), device=0)
    try:
        assert e.get_info("generic_giant_from") == GIANT_DEFAULT and e.get_info("generic_giant_segments") == -1
        for key in ("generic_giant_rows", "generic_giant_entries", "generic_giant_last_rows", "generic_giant_last_segmented"):
            assert e.get_info(key) == 0, key
        e.set_generic_giant_rows(0xFFFFFFFF, 0)
        assert e.get_info("generic_giant_from") == 0xFFFFFFFF and e.get_info("generic_giant_segments") == 0
    finally:
        e.close()


# ---------------------------------------------------------------- the sweep of both values: whole forwards

@pytest.mark.parametrize("name", list(MODELS))
def test_every_setting_gives_the_oracles_bits(shim, name):
    fam = MODELS[name]
    g = graph_of("giant_hubs")
    deg = degrees(g)
    wl = gh.want_of(fam, name, "giant_hubs")[-1][2]
    x = gh.FAMILIES[fam].model_input(name, g)
    e = gh.open_engine(fam, name, g, heavy=HEAVY_FROM)
    try:
        first = None
        for thr in GIANT_THRESHOLDS:
            for seg in (0, 1):
                label = (name, thr, seg)
                e.set_generic_giant_rows(thr, seg)
                sc, lg = e.forward(x)
                mism = int((bits(lg) != bits(wl)).sum())
                assert mism == 0, (label, f"{mism}/{lg.size} logits differ", np.argwhere(bits(lg) != bits(wl))[:6].tolist())
                check_scores(shim, sc.reshape(-1), lg.reshape(-1), gh.flat_logits(fam, name, "giant_hubs"), label)
                if first is None:
                    first = (sc.copy(), lg.copy())
                assert np.array_equal(bits(sc), bits(first[0])) and np.array_equal(bits(lg), bits(first[1])), label
                check_info(e, deg, HEAVY_FROM, thr, seg, label)
                assert e.get_info("generic_heavy_last_rows") == 7 and e.get_info("generic_stages_active") == 1
    finally:
        e.close()


@pytest.mark.parametrize("name", list(MODELS))
def test_thresholds_1_send_every_non_empty_row_the_giant_way(shim, name):
    fam = MODELS[name]
    g = graph_of("giant_er600")
    deg = degrees(g)
    wl = gh.want_of(fam, name, "giant_er600")[-1][2]
    e = gh.open_engine(fam, name, g, giant=(1, -1), heavy=1)
    try:
        sc, lg = e.forward(gh.FAMILIES[fam].model_input(name, g))
        assert e.get_info("generic_giant_last_rows") == int((deg > 0).sum()) <= g.n
        assert e.get_info("generic_giant_rows") == int((deg > 0).sum())
        assert e.get_info("generic_giant_entries") == g.nnz
        assert e.get_info("generic_giant_last_segmented") == 0
        assert np.array_equal(bits(lg), bits(wl)), name
        check_scores(shim, sc.reshape(-1), lg.reshape(-1), gh.flat_logits(fam, name, "giant_er600"), name)
    finally:
        e.close()


# ---------------------------------------------------------------- the order of a row's additions, on both routes of the scan

_stage_want = {}


def crafted(which, stage):
    """(input rows, oracle's stage output, its pre-activation) of stage `stage` of in3_f32: computed once, never changed."""
    if (which, stage) not in _stage_want:
        g = graph_of("giant_hubs")
        f, _ = md.stage_widths("in3_f32")[stage]
        hin = crafted_input(g.n, f, 300 + f) if which == "a" else gi.scan_input(g, f, 200 + f)   # (as tests/test_giant_rows_inputs.py)
        out, pre = gh.oracle_stage("depths", "in3_f32", g, stage, hin)
        _stage_want[which, stage] = (hin, out, pre)
    return _stage_want[which, stage]


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("seg", [0, 1])
@pytest.mark.parametrize("stage", [0, 1])
def test_the_sums_are_added_in_stored_order(stage, seg, which):
    name = "in3_f32"
    g = graph_of("giant_hubs")
    deg = degrees(g)
    assert md.stage_widths(name)[stage][0] == (3, 32)[stage]
    hin, want_out, want_pre = crafted(which, stage)
    e = gh.open_engine("depths", name, g, giant=(1024, seg), heavy=HEAVY_FROM)
    try:
        gh.run_stage_ranges(e, "depths", name, g, stage, hin, [[(0, g.n)]], want_out, want_pre, (name, which, seg))
        check_info(e, deg, HEAVY_FROM, 1024, seg, (name, which, stage, seg))
        assert e.get_info("generic_giant_last_rows") == 6
    finally:
        e.close()


# ---------------------------------------------------------------- the stage entry over split ranges

@pytest.mark.parametrize("name", list(MODELS))
def test_stage_entry_over_split_ranges(name):
    fam = MODELS[name]
    g = graph_of("giant_hubs")
    n = g.n
    want = gh.want_of(fam, name, "giant_hubs")
    # hubs 0 .. 2 and 5 .. 7 in the first two ranges, hubs 3 and 4 in the gap between them: giant rows on both sides of every cut
    first, gap = [(0, 3), (5, n // 2)], [(3, 5), (n // 2, n)]
    for seg in (0, 1):
        e = gh.open_engine(fam, name, g, giant=(1024, seg), heavy=HEAVY_FROM)
        try:
            assert len(want) == e.num_stages
            for s, (hin, hout, pre) in enumerate(want):
                done = gh.run_stage_ranges(e, fam, name, g, s, hin, [first, gap], hout, pre, (name, "giant_hubs", seg))
                assert done[:n].all() and not done[n]
                assert e.get_info("generic_giant_last_rows") == 6 and e.get_info("generic_heavy_last_rows") == 7
                assert e.get_info("generic_giant_last_segmented") == seg
        finally:
            e.close()


# ---------------------------------------------------------------- slices

@pytest.mark.parametrize("name", list(MODELS))
def test_two_slices_compute_the_whole_graph(name):
    import torch
    import gnn_mwvc_amd as G
    from gnn_mwvc_amd import distributed as D
    fam = MODELS[name]
    g = graph_of("giant_hubs")
    n = g.n
    deg = degrees(g)
    want = gh.want_of(fam, name, "giant_hubs")
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(a.astype(np.int64)).to(torch.int32).to(dev)
    rp, col, w, nw = t(g.rowptr), t(g.col), t(g.w), t(g.nw)
    widths = gh.FAMILIES[fam].stage_widths(name)
    outs = [torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev) for _, n_out in widths]
    lgt = torch.full((n + 1, widths[-1][1]), float("nan"), dtype=torch.float32, device=dev)
    for lo, hi in ((0, 4), (4, n)):   # hubs 0 .. 3 in one slice, 4 .. 7 in the other
        sl = D.slice_csr(n, rp, col, w, nw, lo, hi)
        e = G.Engine(gh.text_of(fam, name), device=0)
        try:
            e.set_weight_scale(g.ws)
            e.set_generic_giant_rows(1024, 1)
            torch.cuda.synchronize()
            e.attach_graph_slice(n, lo, hi, sl.nnz, sl.rowptr.data_ptr(), sl.col.data_ptr(), sl.w.data_ptr(), sl.nw.data_ptr(), keepalive=sl)
            mine = int((deg[lo:hi] >= 1024).sum())
            assert mine == 3
            assert e.get_info("generic_giant_rows") == mine, "each engine reports its own slice's giant rows"
            assert e.get_info("generic_giant_entries") == int(deg[lo:hi][deg[lo:hi] >= 1024].sum())
            for s, (hin, _, _) in enumerate(want):
                f = widths[s][0]
                tin = torch.zeros((n + 1, f), dtype=torch.float32, device=dev)
                tin[:n] = torch.from_numpy(np.ascontiguousarray(hin, dtype=np.float32).reshape(n, f)).to(dev)
                torch.cuda.synchronize()
                e.stage_forward_device(s, lo, hi, tin.data_ptr(), outs[s].data_ptr(), lgt.data_ptr() if s + 1 == len(want) else 0)
                e.synchronize()
                assert e.get_info("generic_giant_last_rows") == mine
                assert e.get_info("generic_giant_last_segmented") == int(deg[lo:hi].max() > SEGMENT_ADDENDS)
        finally:
            e.close()
    for s, (_, hout, pre) in enumerate(want):
        got = outs[s].cpu().numpy()
        assert np.isnan(got[n]).all(), (name, s, "the pad row was written")
        if s + 1 == len(want):
            assert np.array_equal(bits(lgt.cpu().numpy()[:n]), bits(pre)), (name, s, "logits")
            assert ulp(got[:n], hout).max(initial=0) <= 1, (name, s, "scores")
        else:
            bad = np.argwhere(bits(got[:n]) != bits(hout))
            assert bad.size == 0, (name, s, f"{len(bad)} values differ, first (row, column)", bad[:6].tolist())


# ---------------------------------------------------------------- the explicit audit

@pytest.mark.parametrize("name", ["odd", "in3_f32"])
def test_the_explicit_audit_is_clean(name):
    fam = MODELS[name]
    g = graph_of("giant_hubs")
    wl = gh.want_of(fam, name, "giant_hubs")[-1][2]
    e = gh.open_engine(fam, name, g, heavy=HEAVY_FROM)
    try:
        runs = 0
        for seg in (0, 1):
            e.set_generic_giant_rows(1024, seg)
            _, lg = e.forward_audited(gh.FAMILIES[fam].model_input(name, g))   # (raises on a mismatch)
            runs += e.num_stages
            assert e.get_info("generic_giant_last_rows") == 6 and e.get_info("generic_giant_last_segmented") == seg
            assert e.get_info("audit_runs") == runs and e.get_info("audit_failures") == 0
            assert np.array_equal(bits(lg), bits(wl)), (name, seg)
    finally:
        e.close()


# ---------------------------------------------------------------- the engine as it was: the trained model, lazy classing, the next graph

def test_the_trained_model_has_no_giant_rows_of_this_kind():
    import gnn_mwvc_amd as G
    g = graph_of("giant_hubs")
    e = G.Engine(G.default_model_text(), device=0)   # no generic stage list in force: stored, does nothing
    try:
        e.set_generic_giant_rows(1, 1)
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
        e.forward(g.x())
        assert e.get_info("generic_giant_from") == 1 and e.get_info("generic_giant_segments") == 1
        for key in ("generic_giant_rows", "generic_giant_entries", "generic_giant_last_rows", "generic_giant_last_segmented"):
            assert e.get_info(key) == 0, key
    finally:
        e.close()


def test_a_graph_attached_before_the_option_is_classed_by_the_first_generic_stage():
    name = "two_deep"
    g = graph_of("giant_hubs")
    x = md.model_input(name, g)
    e = gh.open_engine("depths", name, g, giant=(1024, 1), opts={"generic_stages": 0})
    try:
        assert not e.fused
        sc0, lg0 = e.forward(x)
        assert e.get_info("generic_stages_active") == 0
        assert e.get_info("generic_giant_last_rows") == 0 and e.get_info("generic_giant_rows") == 0
        e.set_option("generic_stages", 1)
        sc1, lg1 = e.forward(x)
        assert e.get_info("generic_stages_active") == 1
        assert e.get_info("generic_giant_last_rows") == 6 and e.get_info("generic_giant_rows") == 6
        assert e.get_info("generic_giant_last_segmented") == 1
        assert np.array_equal(bits(lg0), bits(lg1)) and np.array_equal(bits(sc0), bits(sc1))
        assert np.array_equal(bits(lg1), bits(gh.want_of("depths", name, "giant_hubs")[-1][2]))
        # the next graphs: their own counts
        for gname, rows, heavy in (("er3000", 0, 0), ("giant_hubs", 6, 7)):
            g2 = graph_of(gname)
            e.set_weight_scale(g2.ws)
            e.upload_graph(g2)
            assert e.get_info("generic_giant_rows") == rows, gname   # (classed at the hand-off: the generic list is in force)
            _, lg = e.forward(md.model_input(name, g2))
            assert e.get_info("generic_giant_last_rows") == rows and e.get_info("generic_heavy_last_rows") == heavy, gname
            assert e.get_info("generic_giant_entries") == giant_counts(degrees(g2), HEAVY_FROM, 1024)[1], gname
            assert np.array_equal(bits(lg), bits(gh.want_of("depths", name, gname)[-1][2])), gname
    finally:
        e.close()


# ---------------------------------------------------------------- default <= off

def test_the_giant_route_is_not_slower_than_without_it_on_four_giant_hubs():
    import torch
    import gnn_mwvc_amd as G
    from tools import graphgen_torch as ggt
    dev = torch.device("cuda", 0)
    g = ggt.power_law_hubs(262_144, 8.0, 2.5, 4, 65_536, 3, dev)   # the graph of the heavy-rows guard
    x1 = g.x().contiguous()
    inputs = {"narrow": x1, "in3_f32": torch.stack([x1, x1 * 0.37, 1.0 - x1], dim=1).contiguous()}
    for name, x in inputs.items():
        e = G.Engine(gh.text_of(MODELS[name], name), device=0)
        try:
            e.set_weight_scale(g.ws)
            e.attach_graph_device(g.n, g.nnz, g.rowptr.data_ptr(), g.col.data_ptr(), g.w.data_ptr(), g.nw.data_ptr(), keepalive=g)
            sc = torch.zeros(g.n, device=dev)
            lg = torch.zeros(g.n, device=dev)
            torch.cuda.synchronize()
            assert e.get_info("generic_giant_from") == GIANT_DEFAULT and e.get_info("generic_giant_segments") == -1
            ms_default, lg_on = gh.steady_ms(e, x, sc, lg)   # best of three batches of five
            rows = e.get_info("generic_giant_last_rows")
            e.set_generic_giant_rows(0, -1)
            ms_off, lg_off = gh.steady_ms(e, x, sc, lg)
            assert e.get_info("generic_giant_last_rows") == 0 and e.get_info("generic_heavy_last_rows") >= 4
            print(f"power-law 262144 / four hubs of 65536, {name}: giant rows from 16384 ({rows} rows) {ms_default:.3f} ms, "
                  f"none {ms_off:.3f} ms, {ms_off / ms_default:.2f}x")
            assert rows >= 4, "the default sends the four hubs the giant way"
            assert torch.equal(lg_on.view(torch.int32), lg_off.view(torch.int32)), name
            assert ms_default <= ms_off, f"{name}: giant rows {ms_default:.3f} ms vs none {ms_off:.3f} ms"
        finally:
            e.close()
    del g, x1, inputs
    torch.cuda.empty_cache()
