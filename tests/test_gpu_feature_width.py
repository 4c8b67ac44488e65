"""Feature rows of generic models up to 64 wide (gnnvc_set_generic_feature_width): stages whose feature width f or whose last layer
lies in 33 .. 64 as fused stages, opt-in, under tools/modelgen_feat.py's family (tests/test_modelgen_feat.py shows on the oracle
that every member's logits are alive, and pins the texts and the byte figures used here).

Bars, as in tests/test_gpu_big_stages.py and no wider: logits and every stage's output bit for bit (0 ulp) against the oracle's
stage-by-stage walk, scores within 1 ulp of the oracle's and bit for bit the restated sigmoid's (check_scores), rows outside a
stage call's range and the row behind the end untouched.  Off must be today: not fused, 0 stages, layer by layer, the same bits.

The speed guard at the end: f64 on ER 1 M / 10 M on one engine, fused against layer by layer (which this feature does not touch,
so it is the baseline); the fused forward may not be slower than that by more than the spread of the baseline's own three batches."""
import functools
import time

import numpy as np
import pytest

from tools import giant_rows_inputs as gi
from tools import graphgen as gg
from tools import modelgen_feat as mf
from tests import generic_harness as gh
from tests.generic_harness import bits, check_scores, crafted_input, degrees, graph_of, heavy_counts, ulp
from tests.test_expf_restatement import shim, _run   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)
from tests.test_modelgen_feat import LDS_BYTES

pytestmark = pytest.mark.gpu

gh.FAMILIES["feat"] = mf.family

# rows of exactly these many entries: around every round size the gather of 3 or 4 columns a lane could be built with (8, 16, 32,
# 64 entries a round), an empty row first
ROUND_DEGREES = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65]
ROUND_N = 400


def rounds_graph():
    """400 vertices: vertex i < 14 has exactly ROUND_DEGREES[i] entries, all among the other 386, which carry a sparse background."""
    rng = np.random.default_rng(64)
    nh = len(ROUND_DEGREES)
    others = np.arange(nh, ROUND_N)
    edges = []
    for h, d in enumerate(ROUND_DEGREES):
        for v in rng.choice(others, size=d, replace=False):
            edges.append((h, int(v)))
    a = rng.integers(nh, ROUND_N, size=500)
    b = rng.integers(nh, ROUND_N, size=500)
    edges += list(zip(a.tolist(), b.tolist()))
    return gg.from_edge_list(ROUND_N, edges, rng.integers(20, 121, size=ROUND_N))


gh.GRAPHS["feat_rounds"] = rounds_graph

text_of, want_of, flat_logits = (functools.partial(f, "feat") for f in (gh.text_of, gh.want_of, gh.flat_logits))
ERR_INVALID, ERR_UNSUPPORTED = -1, -5
FULL_LDS = 163840
SMALL_GRAPHS = ["er3000", "er1933", "sparse", "one", "feat_rounds"]
FUSED_ALONE = mf.ADMITTED                  # fused under set_generic_feature_width(64)
FUSED = mf.ADMITTED + mf.NEEDS_BIG         # ... and big_f64 with set_generic_big_stages(163840) as well


def open_engine(name, g, width=None, big=None, **kw):
    """gh.open_engine, then set_generic_feature_width(width) where a width is given — after the graph, as a caller who retrains
    and switches the feature on under a resident graph would."""
    e = gh.open_engine("feat", name, g, big=big, **kw)
    try:
        if width is not None:
            e.set_generic_feature_width(width)
    except BaseException:
        e.close()
        raise
    return e


def open_fused(name, g, **kw):
    return open_engine(name, g, width=64, big=FULL_LDS if name in mf.NEEDS_BIG else None, **kw)


def assert_layer_by_layer(e):
    assert not e.fused and e.num_stages == 0 and e.get_info("generic_stages_model") == 0


def assert_fused_as_specified(e, name, limit=0):
    assert e.fused and e.num_stages == len(mf.SPECS[name][1]) and e.get_info("generic_stages_model") == 1, name
    assert [e.stage_widths(s) for s in range(e.num_stages)] == mf.stage_widths(name), name
    assert [e.get_info(f"generic_stage_layers_{s}") for s in range(e.num_stages)] == mf.stage_depths(name), name
    assert [e.get_info(f"generic_stage_lds_bytes_{s}") for s in range(e.num_stages)] == LDS_BYTES[name], name
    threads = [e.get_info(f"generic_stage_threads_{s}") for s in range(e.num_stages)]
    assert threads == [mf.stage_threads_feat(f, ws, limit) for (f, _), ws in zip(mf.stage_widths(name), mf.SPECS[name][1])], name
    return threads


def assert_oracle_forward(shim, e, name, gname, label):
    g = graph_of(gname)
    sc, lg = e.forward(mf.model_input(name, g))
    wl = want_of(name, gname)[-1][2]
    assert sc.shape == lg.shape == (g.n, mf.out_width(name))
    mism = int((bits(lg) != bits(wl)).sum())
    assert mism == 0, (name, gname, label, f"{mism}/{lg.size} logits differ", np.argwhere(bits(lg) != bits(wl))[:6].tolist())
    check_scores(shim, sc.reshape(-1), lg.reshape(-1), flat_logits(name, gname), (name, gname, label))
    return sc, lg


def test_the_crafted_graph_is_what_it_says():
    g = graph_of("feat_rounds")
    deg = degrees(g)
    assert g.n == ROUND_N and deg[:len(ROUND_DEGREES)].tolist() == ROUND_DEGREES
    assert deg[len(ROUND_DEGREES):].max() < 64


# ---------------------------------------------------------------- 1. off is today

@pytest.mark.parametrize("name", list(mf.SPECS))
def test_off_is_today(shim, name):
    e = open_engine(name, graph_of("er3000"))
    try:
        assert_layer_by_layer(e)
        assert e.get_info("generic_feature_width") == 0
        assert_oracle_forward(shim, e, name, "er3000", "fresh")
        assert e.get_info("generic_stages_active") == 0
        e.set_generic_feature_width(0)
        assert_layer_by_layer(e)
        assert e.get_info("generic_feature_width") == 0
        assert_oracle_forward(shim, e, name, "er3000", "after 0")
        assert e.get_info("generic_stages_active") == 0
    finally:
        e.close()


# ---------------------------------------------------------------- 2. on (64)

@pytest.mark.parametrize("name", FUSED_ALONE)
def test_on_is_fused_and_reports_its_stages(shim, name):
    e = open_engine(name, graph_of("er3000"), width=64)
    try:
        assert e.get_info("generic_feature_width") == 64
        threads = assert_fused_as_specified(e, name)
        assert threads == [256] * e.num_stages   # (within the default LDS bound: the 256-thread form)
        assert_oracle_forward(shim, e, name, "er3000", "on")
        assert e.get_info("generic_stages_active") == 1
    finally:
        e.close()


def test_big_f64_needs_both_calls(shim):
    name = "big_f64"
    e = open_engine(name, graph_of("er3000"), width=64)
    try:
        assert e.get_info("generic_feature_width") == 64
        assert_layer_by_layer(e)
        _, lg0 = assert_oracle_forward(shim, e, name, "er3000", "feature width alone")
        assert e.get_info("generic_stages_active") == 0
        e.set_generic_big_stages(FULL_LDS)
        threads = assert_fused_as_specified(e, name, FULL_LDS)
        assert threads == [256, 512, 256] and e.get_info("generic_stage_threads_1") == 512
        _, lg1 = assert_oracle_forward(shim, e, name, "er3000", "both")
        assert e.get_info("generic_stages_active") == 1
        e.set_generic_feature_width(0)
        assert_layer_by_layer(e)
        assert e.get_info("generic_big_lds") == FULL_LDS
        _, lg2 = assert_oracle_forward(shim, e, name, "er3000", "big stages alone")
        assert e.get_info("generic_stages_active") == 0
        e.set_generic_feature_width(64)   # (the other order: big stages first)
        assert_fused_as_specified(e, name, FULL_LDS)
        _, lg3 = assert_oracle_forward(shim, e, name, "er3000", "both again")
        assert e.get_info("generic_stages_active") == 1
        assert all(np.array_equal(bits(lg0), bits(x)) for x in (lg1, lg2, lg3))
    finally:
        e.close()


@pytest.mark.parametrize("big", [None, FULL_LDS])
def test_f65_stays_layer_by_layer(shim, big):
    e = open_engine("f65", graph_of("er3000"), width=64, big=big)
    try:
        assert_layer_by_layer(e)
        assert e.get_info("generic_feature_width") == 64
        assert_oracle_forward(shim, e, "f65", "er3000", big)
        assert e.get_info("generic_stages_active") == 0
    finally:
        e.close()


# ---------------------------------------------------------------- 3. bounds

def test_the_width_is_a_bound(shim):
    import gnn_mwvc_amd as G
    name = "f48_49"
    e = open_engine(name, graph_of("er3000"), width=48)
    try:
        assert e.get_info("generic_feature_width") == 48
        assert_layer_by_layer(e)
        _, lg0 = assert_oracle_forward(shim, e, name, "er3000", 48)
        assert e.get_info("generic_stages_active") == 0
        e.set_generic_feature_width(49)
        assert e.get_info("generic_feature_width") == 49
        assert_fused_as_specified(e, name)
        _, lg1 = assert_oracle_forward(shim, e, name, "er3000", 49)
        assert e.get_info("generic_stages_active") == 1
        assert np.array_equal(bits(lg0), bits(lg1))
        for bad in (32, 65, 1):
            with pytest.raises(G.engine.GnnvcError) as ei:
                e.set_generic_feature_width(bad)
            assert ei.value.code == ERR_INVALID, bad
            assert e.get_info("generic_feature_width") == 49   # the engine is unchanged
            assert_fused_as_specified(e, name)
        e.set_generic_feature_width(0)
        for bad in (32, 65, 1):
            with pytest.raises(G.engine.GnnvcError) as ei:
                e.set_generic_feature_width(bad)
            assert ei.value.code == ERR_INVALID, bad
            assert e.get_info("generic_feature_width") == 0
            assert_layer_by_layer(e)
        e.set_generic_feature_width(33)   # the least value: admits f33, not this model
        assert_layer_by_layer(e)
    finally:
        e.close()
    e = open_engine("f33", graph_of("er3000"), width=33)
    try:
        assert_fused_as_specified(e, "f33")
        assert_oracle_forward(shim, e, "f33", "er3000", 33)
        assert e.get_info("generic_stages_active") == 1
    finally:
        e.close()


def test_a_multi_device_handle_refuses_the_call(model_text):
    import gnn_mwvc_amd as G
    e = G.Engine(model_text, devices=[0, 0])
    try:
        for value in (0, 64):
            with pytest.raises(G.engine.GnnvcError) as ei:
                e.set_generic_feature_width(value)
            assert ei.value.code == ERR_UNSUPPORTED, value
    finally:
        e.close()


def test_a_model_within_the_default_bounds_keeps_its_kernels():
    """`narrow` (f <= 32 everywhere) is planned and reported the same with the feature on."""
    g = graph_of("er3000")
    e = gh.open_engine("shapes", "narrow", g, expect_fused=True)
    try:
        before = [(e.stage_widths(s), e.get_info(f"generic_stage_threads_{s}"), e.get_info(f"generic_stage_lds_bytes_{s}"))
                  for s in range(e.num_stages)]
        _, lg0 = e.forward(gh.FAMILIES["shapes"].model_input("narrow", g))
        e.set_generic_feature_width(64)
        after = [(e.stage_widths(s), e.get_info(f"generic_stage_threads_{s}"), e.get_info(f"generic_stage_lds_bytes_{s}"))
                 for s in range(e.num_stages)]
        assert before == after
        _, lg1 = e.forward(gh.FAMILIES["shapes"].model_input("narrow", g))
        assert np.array_equal(bits(lg0), bits(lg1)) and e.get_info("generic_stages_active") == 1
    finally:
        e.close()


# ---------------------------------------------------------------- 4. parity on small graphs: forward and stage entry

@pytest.mark.parametrize("gname", SMALL_GRAPHS)
@pytest.mark.parametrize("name", FUSED)
def test_forward_and_stage_entry(shim, name, gname):
    g = graph_of(gname)
    want = want_of(name, gname)
    e = open_fused(name, g)
    try:
        for rep in range(2):   # (twice: nothing may depend on what an earlier forward left)
            assert_oracle_forward(shim, e, name, gname, rep)
            assert e.get_info("generic_stages_active") == 1
        n = g.n
        first, gap = gh.split_ranges(n)
        assert len(want) == e.num_stages
        for s, (hin, hout, pre) in enumerate(want):
            done = gh.run_stage_ranges(e, "feat", name, g, s, hin, [first, gap], hout, pre, (name, gname))
            assert done[:n].all() and not done[n]
    finally:
        e.close()


@pytest.mark.parametrize("name", FUSED)
def test_the_empty_graph(name):
    g = graph_of("empty")
    e = open_fused(name, g)
    try:
        assert e.fused
        sc, lg = e.forward(mf.model_input(name, g))
        assert sc.shape == lg.shape == (0, mf.out_width(name))
    finally:
        e.close()


# ---------------------------------------------------------------- 5. the order of a row's additions

WIDE_STAGES = [("f33", 1), ("f48_49", 1), ("f48_49", 2), ("f64", 1), ("f64", 2)]   # the stages whose f is above 32: 33, 48, 49, 64, 64

_stage_want = {}


def crafted_stage(name, stage, gname, which="a"):
    """(input rows, oracle's stage output, its pre-activation) of the stage under a crafted input: computed once, never changed."""
    key = (name, stage, gname, which)
    if key not in _stage_want:
        g = graph_of(gname)
        f, _ = mf.stage_widths(name)[stage]
        hin = crafted_input(g.n, f, 300 + f) if which == "a" else gi.scan_input(g, f, 200 + f)
        out, pre = gh.oracle_stage("feat", name, g, stage, hin)
        _stage_want[key] = (hin, out, pre)
    return _stage_want[key]


def test_the_crafted_input_tells_the_orders_apart():
    g = graph_of("feat_rounds")
    hin = crafted_input(g.n, 64, 364)
    assert (bits(hin) == 0x80000000).any()
    row = len(ROUND_DEGREES) - 1   # 65 entries
    nb = g.col[int(g.rowptr[row]): int(g.rowptr[row + 1])].astype(np.int64)
    fwd = np.zeros(64, dtype=np.float32)
    for v in nb:
        fwd = (fwd + hin[v]).astype(np.float32)
    rev = np.zeros(64, dtype=np.float32)
    for v in nb[::-1]:
        rev = (rev + hin[v]).astype(np.float32)
    assert (bits(fwd) != bits(rev)).sum() > 32, "the crafted input does not tell the two orders apart in most columns"


@pytest.mark.parametrize("gname", ["feat_rounds", "er1933"])
@pytest.mark.parametrize("name,stage", WIDE_STAGES)
def test_the_sums_are_added_in_stored_order(name, stage, gname):
    g = graph_of(gname)
    n = g.n
    assert mf.stage_widths(name)[stage][0] > 32
    hin, want_out, want_pre = crafted_stage(name, stage, gname)
    e = open_fused(name, g)
    try:
        gh.run_stage_ranges(e, "feat", name, g, stage, hin, [[(0, n)]], want_out, want_pre, (name, gname, "whole"))
        first, gap = gh.split_ranges(n)
        done = gh.run_stage_ranges(e, "feat", name, g, stage, hin, [first, gap], want_out, want_pre, (name, gname, "split"))
        assert done[:n].all() and not done[n]
    finally:
        e.close()


@pytest.mark.parametrize("name,stage", [("f33", 1), ("f48_49", 2), ("f64", 1)])
def test_two_slices_compute_the_whole_stage(name, stage):
    import torch
    import gnn_mwvc_amd as G
    from gnn_mwvc_amd import distributed as D
    gname = "feat_rounds"
    g = graph_of(gname)
    n = g.n
    hin, want_out, want_pre = crafted_stage(name, stage, gname)
    f, n_out = mf.stage_widths(name)[stage]
    last = stage + 1 == len(mf.stage_widths(name))
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(a.astype(np.int64)).to(torch.int32).to(dev)
    rp, col, w, nw = t(g.rowptr), t(g.col), t(g.w), t(g.nw)
    out = torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)
    lgt = torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)
    tin = torch.zeros((n + 1, f), dtype=torch.float32, device=dev)
    tin[:n] = torch.from_numpy(hin).to(dev)
    for lo, hi in ((0, 9), (9, n)):   # the crafted rows on both sides of the cut
        sl = D.slice_csr(n, rp, col, w, nw, lo, hi)
        e = G.Engine(text_of(name), device=0)
        try:
            e.set_weight_scale(g.ws)
            e.set_generic_feature_width(64)
            assert e.fused
            torch.cuda.synchronize()
            e.attach_graph_slice(n, lo, hi, sl.nnz, sl.rowptr.data_ptr(), sl.col.data_ptr(), sl.w.data_ptr(), sl.nw.data_ptr(), keepalive=sl)
            e.stage_forward_device(stage, lo, hi, tin.data_ptr(), out.data_ptr(), lgt.data_ptr() if last else 0)
            e.synchronize()
        finally:
            e.close()
    got = out.cpu().numpy()
    assert np.isnan(got[n]).all(), (name, "the pad row was written")
    if last:
        assert np.array_equal(bits(lgt.cpu().numpy()[:n]), bits(want_pre)), (name, "logits")
        assert ulp(got[:n], want_out).max(initial=0) <= 1, (name, "scores")
    else:
        bad = np.argwhere(bits(got[:n]) != bits(want_out))
        assert bad.size == 0, (name, f"{len(bad)} values differ, first (row, column)", bad[:6].tolist())


# ---------------------------------------------------------------- 6. heavy rows

HEAVY_THRESHOLDS = [0, 1, 512, 513]


@pytest.mark.parametrize("name", ["f33", "f64"])
def test_every_heavy_threshold_gives_the_oracles_bits(shim, name):
    gname = "hubs"
    g = graph_of(gname)
    e = open_fused(name, g)
    try:
        first = None
        for thr in HEAVY_THRESHOLDS:
            e.set_generic_heavy_rows(thr)
            sc, lg = assert_oracle_forward(shim, e, name, gname, ("heavy", thr))
            if first is None:
                first = (sc.copy(), lg.copy())
            assert np.array_equal(bits(sc), bits(first[0])) and np.array_equal(bits(lg), bits(first[1])), (name, thr)
            rows, entries = heavy_counts(g, thr)
            assert e.get_info("generic_heavy_from") == thr
            assert e.get_info("generic_heavy_last_rows") == rows == e.get_info("generic_heavy_rows"), (name, thr)
            assert e.get_info("generic_heavy_entries") == entries, (name, thr)
            assert e.get_info("generic_stages_active") == 1
    finally:
        e.close()


@pytest.mark.parametrize("thr", [512, 1])
@pytest.mark.parametrize("name,stage", [("f33", 1), ("f64", 1)])
def test_heavy_sums_are_added_in_stored_order(name, stage, thr):
    gname = "hubs"
    g = graph_of(gname)
    hin, want_out, want_pre = crafted_stage(name, stage, gname)
    e = open_fused(name, g, heavy=thr)
    try:
        # hubs 0 .. 2 and 6 .. 8 in the first two ranges, hubs 3 .. 5 in the gap between them
        first, gap = [(0, 3), (6, g.n // 2)], [(3, 6), (g.n // 2, g.n)]
        done = gh.run_stage_ranges(e, "feat", name, g, stage, hin, [first, gap], want_out, want_pre, (name, "crafted", thr))
        assert done[:g.n].all()
        assert e.get_info("generic_heavy_last_rows") == heavy_counts(g, thr)[0]
    finally:
        e.close()


# ---------------------------------------------------------------- 7. giant rows

GIANT_THRESHOLDS = [0, 1024, 1025, 4097]   # as tests/test_gpu_giant_rows.py lowers them, and none
HEAVY_FROM = 512


def giant_counts(g, thr):
    return heavy_counts(g, max(thr, HEAVY_FROM)) if thr else (0, 0)


@pytest.mark.parametrize("name", ["f47", "f64"])
def test_every_giant_setting_gives_the_oracles_bits(shim, name):
    gname = "giant_hubs"
    g = graph_of(gname)
    deg = degrees(g)
    e = open_fused(name, g, heavy=HEAVY_FROM)
    try:
        first = None
        for thr in GIANT_THRESHOLDS:
            for seg in (0, 1):
                label = (name, thr, seg)
                e.set_generic_giant_rows(thr, seg)
                sc, lg = assert_oracle_forward(shim, e, name, gname, label)
                if first is None:
                    first = (sc.copy(), lg.copy())
                assert np.array_equal(bits(sc), bits(first[0])) and np.array_equal(bits(lg), bits(first[1])), label
                rows, entries = giant_counts(g, thr)
                assert e.get_info("generic_giant_last_rows") == rows == e.get_info("generic_giant_rows"), label
                assert e.get_info("generic_giant_entries") == entries, label
                assert e.get_info("generic_giant_last_segmented") == int(seg == 1 and rows > 0 and int(deg.max()) > 4096), label
                assert e.get_info("generic_heavy_last_rows") == 7 and e.get_info("generic_stages_active") == 1
    finally:
        e.close()


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("seg", [0, 1])
@pytest.mark.parametrize("stage", [1, 2])
def test_giant_sums_are_added_in_stored_order_at_f64(stage, seg, which):
    name, gname = "f64", "giant_hubs"
    g = graph_of(gname)
    assert mf.stage_widths(name)[stage][0] == 64
    hin, want_out, want_pre = crafted_stage(name, stage, gname, which)
    e = open_fused(name, g, giant=(1024, seg), heavy=HEAVY_FROM)
    try:
        gh.run_stage_ranges(e, "feat", name, g, stage, hin, [[(0, g.n)]], want_out, want_pre, (name, which, seg, "whole"))
        assert e.get_info("generic_giant_last_rows") == 6 and e.get_info("generic_giant_last_segmented") == seg
        # hubs 0 .. 2 and 5 .. 7 in the first two ranges, hubs 3 and 4 in the gap between them
        first, gap = [(0, 3), (5, g.n // 2)], [(3, 5), (g.n // 2, g.n)]
        done = gh.run_stage_ranges(e, "feat", name, g, stage, hin, [first, gap], want_out, want_pre, (name, which, seg, "split"))
        assert done[:g.n].all() and not done[g.n]
    finally:
        e.close()


# ---------------------------------------------------------------- 8. the audit

@pytest.mark.parametrize("gname", ["er3000", "hubs"])
@pytest.mark.parametrize("name", ["f64", "out64"])
def test_forward_audited_is_clean(name, gname):
    g = graph_of(gname)
    e = open_fused(name, g)
    try:
        ns = e.num_stages
        sc, lg = e.forward_audited(mf.model_input(name, g))
        rep = e.audit_report()
        assert rep["audit_runs"] == ns == len(mf.SPECS[name][1]) and rep["audit_failures"] == 0 and rep["audit_repairs"] == 0, rep
        assert np.array_equal(bits(lg), bits(want_of(name, gname)[-1][2])), (name, gname)
    finally:
        e.close()


@pytest.mark.parametrize("name", ["f64", "out64"])
def test_repairing_zeros_writes_the_oracles_stage(shim, name):
    import torch
    gname = "er1933"
    g = graph_of(gname)
    n = g.n
    want = want_of(name, gname)
    restated = _run(shim.sigmoid_restated, flat_logits(name, gname)).reshape(n, -1)   # the device's scores, bit for bit
    e = open_fused(name, g, opts={"audit_repair": 1})
    try:
        for s, (hin, hout, pre) in enumerate(want):
            last = s + 1 == len(want)
            tin, out, lgt, f, n_out = gh.stage_buffers("feat", name, gname, s)
            w_out = restated if last else np.ascontiguousarray(hout, dtype=np.float32).reshape(n, n_out)
            w_pre = np.ascontiguousarray(pre, dtype=np.float32).reshape(n, n_out)
            out[:n] = 0.0
            if last:
                lgt[:n] = 0.0
            torch.cuda.synchronize()
            before = e.audit_report()
            e.audit_stage_device(s, 0, n, tin.data_ptr(), out.data_ptr(), lgt.data_ptr() if last else 0)
            rep = e.audit_report()
            expect = int((bits(w_out) != 0).sum()) + (int((bits(w_pre) != 0).sum()) if last else 0)
            assert expect > 0
            assert rep["audit_repairs"] - before["audit_repairs"] == expect, (name, s, rep, expect)
            assert rep["audit_runs"] == before["audit_runs"] + 1
            got, gotl = out.cpu().numpy(), lgt.cpu().numpy()
            assert np.array_equal(bits(got[:n]), bits(w_out)), (name, s, "stage output")
            if last:
                assert np.array_equal(bits(gotl[:n]), bits(w_pre)), (name, s, "logits")
            assert np.isnan(got[n]).all(), (name, s, "the row behind the end was written")
            assert np.isnan(gotl[n]).all() if last else np.isnan(gotl).all(), (name, s, "logits rows")
    finally:
        e.close()


# ---------------------------------------------------------------- 9. live changes under a resident graph

def test_live_changes_under_a_resident_graph(shim):
    name, gname = "f64", "hubs"
    g = graph_of(gname)
    x = mf.model_input(name, g)

    def readouts(e, heavy, giant, label):
        rows, entries = heavy_counts(g, heavy)
        assert e.get_info("generic_heavy_last_rows") == rows == e.get_info("generic_heavy_rows"), label
        assert e.get_info("generic_heavy_entries") == entries, label
        grows, gentries = heavy_counts(g, max(giant, heavy)) if giant and heavy else (0, 0)
        assert e.get_info("generic_giant_last_rows") == grows == e.get_info("generic_giant_rows"), label
        assert e.get_info("generic_giant_entries") == gentries, label

    e = open_engine(name, g)   # off; heavy rows at their default (512), giant rows at theirs (16 384: none here)
    try:
        assert_layer_by_layer(e)
        _, lg_off = assert_oracle_forward(shim, e, name, gname, "off")
        assert e.get_info("generic_stages_active") == 0
        e.set_generic_feature_width(64)
        assert_fused_as_specified(e, name)
        _, lg = assert_oracle_forward(shim, e, name, gname, "on")
        assert e.get_info("generic_stages_active") == 1 and np.array_equal(bits(lg), bits(lg_off))
        readouts(e, 512, 16384, "on")
        e.set_generic_heavy_rows(513)
        e.set_generic_giant_rows(1024, 1)
        _, lg = assert_oracle_forward(shim, e, name, gname, "heavy 513, giant 1024")
        assert np.array_equal(bits(lg), bits(lg_off))
        readouts(e, 513, 1024, "heavy 513, giant 1024")
        # another weight scale: the oracle at that scale
        ws2 = g.ws * 1.75
        e.set_weight_scale(ws2)
        want2 = gh.logits_at("feat", name, g, ws=ws2)
        _, lg2 = e.forward(x)
        assert np.array_equal(bits(lg2), bits(want2)), "on, another weight scale"
        assert not np.array_equal(bits(lg2), bits(lg_off))
        e.set_generic_feature_width(0)
        assert_layer_by_layer(e)
        _, lg2_off = e.forward(x)
        assert e.get_info("generic_stages_active") == 0 and np.array_equal(bits(lg2_off), bits(want2)), "off, another weight scale"
        e.set_weight_scale(g.ws)
        e.set_generic_heavy_rows(1)
        e.set_generic_giant_rows(0, 0)
        e.set_generic_feature_width(64)
        assert_fused_as_specified(e, name)
        _, lg = assert_oracle_forward(shim, e, name, gname, "on again, heavy 1")
        assert e.get_info("generic_stages_active") == 1 and np.array_equal(bits(lg), bits(lg_off))
        readouts(e, 1, 0, "on again, heavy 1")
        e.set_generic_heavy_rows(0)
        _, lg = assert_oracle_forward(shim, e, name, gname, "heavy 0")
        assert np.array_equal(bits(lg), bits(lg_off))
        readouts(e, 0, 0, "heavy 0")
    finally:
        e.close()


# ---------------------------------------------------------------- 10. speed guard

def batches_ms(e, x, sc, lg):
    """[ms a forward] of three batches of five after two warm-up forwards (the loop of gh.steady_ms, every batch kept), the logits."""
    import torch
    for _ in range(2):
        e.forward_device(x.data_ptr(), sc.data_ptr(), lg.data_ptr())
    e.synchronize()
    ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(5):
            e.forward_device(x.data_ptr(), sc.data_ptr(), lg.data_ptr())
        e.synchronize()
        ms.append((time.perf_counter() - t) * 200.0)
    return ms, lg.clone()


def test_fused_f64_is_not_slower_than_layer_by_layer():
    import torch
    import gnn_mwvc_amd as G
    from tools import graphgen_torch as ggt
    dev = torch.device("cuda", 0)
    g = ggt.erdos_renyi(1_000_000, 10_000_000, 2, dev)
    x = g.x().contiguous()
    name = "f64"
    e = G.Engine(text_of(name), device=0)
    try:
        e.set_weight_scale(g.ws)
        e.attach_graph_device(g.n, g.nnz, g.rowptr.data_ptr(), g.col.data_ptr(), g.w.data_ptr(), g.nw.data_ptr(), keepalive=g)
        sc = torch.zeros(g.n, device=dev)
        lg = torch.zeros(g.n, device=dev)
        torch.cuda.synchronize()
        off, lg0 = batches_ms(e, x, sc, lg)
        assert e.get_info("generic_stages_active") == 0
        e.set_generic_feature_width(64)
        on, lg1 = batches_ms(e, x, sc, lg)
        assert e.get_info("generic_stages_active") == 1
        spread = max(off) - min(off)
        print(f"er1m {name}: fused {min(on):.3f} ms (batches {on}), layer by layer {min(off):.3f} ms (batches {off}), "
              f"spread {spread:.3f} ms, {min(off) / min(on):.2f}x")
        assert torch.equal(lg0.view(torch.int32), lg1.view(torch.int32)), name
        assert min(on) <= min(off) + spread, f"{name}: fused {min(on):.3f} ms vs layer by layer {min(off):.3f} ms (+ {spread:.3f})"
    finally:
        e.close()
    del g, x
    torch.cuda.empty_cache()
