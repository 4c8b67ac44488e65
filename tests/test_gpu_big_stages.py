"""Big stages of generic models (gnnvc_set_generic_big_stages): stages with hidden widths up to 128 and up to 160 KiB of LDS as
fused stages, opt-in, under tools/modelgen_big.py's family (tests/test_modelgen_big.py shows on the oracle that every member's
logits are alive, and pins the byte figures used here).

Bars, as in tests/test_gpu_depths.py and no wider: logits and every stage's output bit for bit against the oracle, scores within
1 ulp of the oracle's and bit for bit the restated sigmoid's (check_scores of tests/test_gpu_models.py), rows outside a stage
call's range and the row behind the end untouched.  The graphs are that file's.

The speed guard at the end is that file's too: big stages on against off (layer by layer) on one engine, ER 1 M / 10 M."""
import functools

import numpy as np
import pytest

from tools import modelgen_big as mb
from tests import generic_harness as gh
from tests.generic_harness import LDS_BYTES, bits, check_scores, graph_of
from tests.test_expf_restatement import shim, _run   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)

pytestmark = pytest.mark.gpu

# the accessors of tests/generic_harness.py, for the family of this file
text_of, want_of, flat_logits, open_engine = (functools.partial(f, "big")
                                              for f in (gh.text_of, gh.want_of, gh.flat_logits, gh.open_engine))
GRAPHS = ["er3000", "sparse", "er1933", "one", "hub6k"]   # tests/test_gpu_depths.py's (tests/generic_harness.py has what each is)
ERR_INVALID, ERR_UNSUPPORTED = -1, -5
FULL = 163840


def assert_layer_by_layer(e):
    assert not e.fused and e.num_stages == 0 and e.get_info("generic_stages_model") == 0


def assert_fused_as_specified(e, name, limit=FULL):
    assert e.fused and e.num_stages == len(mb.SPECS[name][1]), name
    assert [e.stage_widths(s) for s in range(e.num_stages)] == mb.stage_widths(name), name
    assert [e.get_info(f"generic_stage_layers_{s}") for s in range(e.num_stages)] == mb.stage_depths(name), name
    assert [e.get_info(f"generic_stage_lds_bytes_{s}") for s in range(e.num_stages)] == LDS_BYTES[name], name
    threads = [e.get_info(f"generic_stage_threads_{s}") for s in range(e.num_stages)]
    for s, ((f, _), ws) in enumerate(zip(mb.stage_widths(name), mb.SPECS[name][1])):
        assert threads[s] in (256, 512, 1024), (name, s)
        if mb.stage_is_small(f, ws):
            assert threads[s] == 256, (name, s, "a stage within the default bounds runs the kernel it always ran")
        assert mb.stage_lds_bytes(f, ws, threads[s] // 16) <= limit, (name, s, threads[s])
    return threads


def assert_oracle_forward(shim, e, name, gname, label):
    g = graph_of(gname)
    sc, lg = e.forward(mb.model_input(name, g))
    wl = want_of(name, gname)[-1][2]
    assert sc.shape == lg.shape == (g.n, mb.out_width(name))
    mism = int((bits(lg) != bits(wl)).sum())
    assert mism == 0, (name, gname, label, f"{mism}/{lg.size} logits differ", np.argwhere(bits(lg) != bits(wl))[:6].tolist())
    check_scores(shim, sc.reshape(-1), lg.reshape(-1), flat_logits(name, gname), (name, gname, label))
    return sc, lg


# ---------------------------------------------------------------- 1. off is today

@pytest.mark.parametrize("name", list(mb.SPECS))
def test_off_is_today(shim, name):
    import gnn_mwvc_amd as G
    e = open_engine(name, graph_of("er3000"), big=None)
    try:
        assert_layer_by_layer(e)
        assert e.get_info("generic_big_lds") == 0
        for key in ("generic_stage_lds_bytes_0", "generic_stage_threads_0"):
            with pytest.raises(G.engine.GnnvcError) as ei:
                e.get_info(key)
            assert ei.value.code == ERR_INVALID, key
        assert_oracle_forward(shim, e, name, "er3000", "fresh")
        assert e.get_info("generic_stages_active") == 0
        e.set_generic_big_stages(0)
        assert_layer_by_layer(e)
        assert e.get_info("generic_big_lds") == 0
        assert_oracle_forward(shim, e, name, "er3000", "after 0")
        assert e.get_info("generic_stages_active") == 0
    finally:
        e.close()


# ---------------------------------------------------------------- 2. on

@pytest.mark.parametrize("name", mb.ADMITTED)
def test_on_is_fused_and_reports_its_stages(shim, name):
    import gnn_mwvc_amd as G
    e = open_engine(name, graph_of("er3000"), big=FULL)
    try:
        assert e.get_info("generic_big_lds") == FULL and e.get_info("generic_stages_model") == 1
        threads = assert_fused_as_specified(e, name)
        if name == "edge":
            assert threads == [256, 256]   # stage 0 fits the limit at 256 threads only; stage 1 is within the default bounds
        for key in (f"generic_stage_lds_bytes_{e.num_stages}", "generic_stage_lds_bytes_", "generic_stage_threads_-1", "generic_stage_threads_0x"):
            with pytest.raises(G.engine.GnnvcError) as ei:
                e.get_info(key)
            assert ei.value.code == ERR_INVALID, key
        assert_oracle_forward(shim, e, name, "er3000", "on")
        assert e.get_info("generic_stages_active") == 1
    finally:
        e.close()


# ---------------------------------------------------------------- 3. every admitted model on every graph: forward and stage entry

@pytest.mark.parametrize("gname", list(GRAPHS))
@pytest.mark.parametrize("name", mb.ADMITTED)
def test_forward_and_stage_entry(shim, name, gname):
    import torch
    g = graph_of(gname)
    want = want_of(name, gname)
    e = open_engine(name, g, big=FULL)
    try:
        for rep in range(2):   # (twice: nothing may depend on what an earlier forward left)
            assert_oracle_forward(shim, e, name, gname, rep)
            assert e.get_info("generic_stages_active") == 1
        # the stage entry over split row ranges, each stage fed the oracle's input: first two ranges with a gap between them
        # (the gap, the rows behind and the row behind the end stay as they were), then the gap
        n = g.n
        first, gap = gh.split_ranges(n)
        assert len(want) == e.num_stages
        for s, (hin, hout, pre) in enumerate(want):
            done = gh.run_stage_ranges(e, "big", name, g, s, hin, [first, gap], hout, pre, (name, gname))
            assert done[:n].all() and not done[n]
    finally:
        e.close()


# ---------------------------------------------------------------- 4. the limit is a limit

def test_the_limit_is_a_limit(shim):
    import gnn_mwvc_amd as G
    e = open_engine("h128", graph_of("er3000"), big=99647)
    try:
        assert_layer_by_layer(e)
        assert e.get_info("generic_big_lds") == 99647
        _, lg0 = assert_oracle_forward(shim, e, "h128", "er3000", 99647)
        assert e.get_info("generic_stages_active") == 0
        e.set_generic_big_stages(99648)
        assert_fused_as_specified(e, "h128", 99648)
        assert e.get_info("generic_stage_threads_0") == 256   # (the layout at 512 threads does not fit 99 648 bytes)
        _, lg1 = assert_oracle_forward(shim, e, "h128", "er3000", 99648)
        assert e.get_info("generic_stages_active") == 1
        e.set_generic_big_stages(0)
        assert_layer_by_layer(e)
        _, lg2 = assert_oracle_forward(shim, e, "h128", "er3000", 0)
        assert e.get_info("generic_stages_active") == 0
        assert np.array_equal(bits(lg0), bits(lg1)) and np.array_equal(bits(lg0), bits(lg2))
        for bad in (65535, 163841, 1):
            with pytest.raises(G.engine.GnnvcError) as ei:
                e.set_generic_big_stages(bad)
            assert ei.value.code == ERR_INVALID, bad
            assert e.get_info("generic_big_lds") == 0
    finally:
        e.close()
    e = open_engine("edge", graph_of("er3000"), big=161487)
    try:
        assert_layer_by_layer(e)
        e.set_generic_big_stages(161488)
        assert assert_fused_as_specified(e, "edge", 161488) == [256, 256]
        assert_oracle_forward(shim, e, "edge", "er3000", 161488)
        assert e.get_info("generic_stages_active") == 1
    finally:
        e.close()


# ---------------------------------------------------------------- 5. outside every limit

@pytest.mark.parametrize("option", [1, 2])
def test_over_stays_layer_by_layer(shim, option):
    e = open_engine("over", graph_of("er3000"), big=FULL, opts={"generic_stages": option})
    try:
        assert_layer_by_layer(e)
        assert e.get_info("generic_big_lds") == FULL
        assert_oracle_forward(shim, e, "over", "er3000", option)
        assert e.get_info("generic_stages_active") == 0
    finally:
        e.close()


# ---------------------------------------------------------------- 6. heavy and giant rows under a big stage

@pytest.mark.parametrize("name", ["h128", "odd_wide"])
def test_heavy_and_giant_rows_feed_a_big_stage(shim, name):
    gname = "hub6k"
    e = open_engine(name, graph_of(gname), big=FULL)
    try:
        assert_fused_as_specified(e, name)
        ref = None
        for heavy in (0, 512, 1):
            e.set_generic_heavy_rows(heavy)
            _, lg = assert_oracle_forward(shim, e, name, gname, ("heavy", heavy))
            assert (e.get_info("generic_heavy_last_rows") > 0) == (heavy != 0)
            ref = lg if ref is None else ref
            assert np.array_equal(bits(lg), bits(ref)), (name, heavy)
        e.set_generic_heavy_rows(512)
        for seg in (0, 1):
            e.set_generic_giant_rows(1024, seg)
            _, lg = assert_oracle_forward(shim, e, name, gname, ("giant", seg))
            assert e.get_info("generic_giant_last_rows") == 2 and e.get_info("generic_heavy_last_rows") == 2
            assert np.array_equal(bits(lg), bits(ref)), (name, seg)
    finally:
        e.close()


# ---------------------------------------------------------------- 7. the audit

@pytest.mark.parametrize("gname", ["er3000", "hub6k"])
@pytest.mark.parametrize("name", ["too_big", "h128"])
def test_forward_audited_is_clean_on_big_stages(name, gname):
    g = graph_of(gname)
    e = open_engine(name, g, big=FULL)
    try:
        ns = e.num_stages
        sc, lg = e.forward_audited(mb.model_input(name, g))
        rep = e.audit_report()
        assert rep["audit_runs"] == ns == len(mb.SPECS[name][1]) and rep["audit_failures"] == 0 and rep["audit_repairs"] == 0, rep
        assert np.array_equal(bits(lg), bits(want_of(name, gname)[-1][2])), (name, gname)
    finally:
        e.close()


@pytest.mark.parametrize("name", ["too_big", "h128"])
def test_repairing_zeros_writes_the_oracles_stage(shim, name):
    import torch
    gname = "er1933"
    g = graph_of(gname)
    n = g.n
    want = want_of(name, gname)
    restated = _run(shim.sigmoid_restated, flat_logits(name, gname)).reshape(n, -1)   # the device's scores, bit for bit
    e = open_engine(name, g, big=FULL, opts={"audit_repair": 1})
    try:
        cuts = sorted({0, n // 5, n // 3, (2 * n) // 3, n})
        ranges = list(zip(cuts[:-1], cuts[1:]))
        order = ranges[0::2] + ranges[1::2]   # with gaps first, then the gaps
        for s, (hin, hout, pre) in enumerate(want):
            last = s + 1 == len(want)
            tin, out, lgt, f, n_out = gh.stage_buffers("big", name, gname, s)
            w_out = restated if last else np.ascontiguousarray(hout, dtype=np.float32).reshape(n, n_out)
            w_pre = np.ascontiguousarray(pre, dtype=np.float32).reshape(n, n_out)
            done = np.zeros(n + 1, dtype=bool)
            for lo, hi in order:
                out[lo:hi] = 0.0
                if last:
                    lgt[lo:hi] = 0.0
                torch.cuda.synchronize()
                before = e.audit_report()
                e.audit_stage_device(s, lo, hi, tin.data_ptr(), out.data_ptr(), lgt.data_ptr() if last else 0)
                rep = e.audit_report()
                expect = int((bits(w_out[lo:hi]) != 0).sum()) + (int((bits(w_pre[lo:hi]) != 0).sum()) if last else 0)
                assert rep["audit_repairs"] - before["audit_repairs"] == expect, (name, s, lo, hi, rep, expect)
                assert rep["audit_runs"] == before["audit_runs"] + 1
                done[lo:hi] = True
                got, gotl = out.cpu().numpy(), lgt.cpu().numpy()
                assert np.array_equal(bits(got[lo:hi]), bits(w_out[lo:hi])), (name, s, lo, hi, "stage output")
                if last:
                    assert np.array_equal(bits(gotl[lo:hi]), bits(w_pre[lo:hi])), (name, s, lo, hi, "logits")
                assert np.isnan(got[~done]).all(), (name, s, "rows outside the range or the row behind the end were written")
                assert np.isnan(gotl[~done]).all() if last else np.isnan(gotl).all(), (name, s, "logits rows")
            assert done[:n].all() and not done[n]
    finally:
        e.close()


def test_forward_audited_is_still_refused_with_big_stages_off():
    import gnn_mwvc_amd as G
    g = graph_of("er3000")
    e = open_engine("too_big", g, big=None)
    try:
        with pytest.raises(G.GnnvcError) as err:
            e.forward_audited(mb.model_input("too_big", g))
        assert err.value.code == ERR_UNSUPPORTED
    finally:
        e.close()


# ---------------------------------------------------------------- 8. option interplay

def test_generic_stages_option_still_rules(shim):
    name, gname = "h128", "er3000"
    e = open_engine(name, graph_of(gname), big=FULL)
    try:
        _, lg1 = assert_oracle_forward(shim, e, name, gname, "on")
        assert e.get_info("generic_stages_active") == 1
        e.set_option("generic_stages", 0)
        assert_layer_by_layer(e)
        assert e.get_info("generic_big_lds") == FULL
        _, lg0 = assert_oracle_forward(shim, e, name, gname, "generic_stages 0")
        assert e.get_info("generic_stages_active") == 0
        assert np.array_equal(bits(lg0), bits(lg1))
        e.set_option("generic_stages", 1)
        assert_fused_as_specified(e, name)
        assert_oracle_forward(shim, e, name, gname, "generic_stages 1")
        assert e.get_info("generic_stages_active") == 1
    finally:
        e.close()


def test_trained_model_keeps_its_kernels_under_option_2(model_text):
    import gnn_mwvc_amd as G
    e = G.Engine(model_text, device=0)
    try:
        e.set_generic_big_stages(FULL)
        assert e.fused and e.num_stages == 3 and e.get_info("generic_stages_model") == 0
        e.set_option("generic_stages", 2)
        assert [e.get_info(f"generic_stage_threads_{s}") for s in range(3)] == [256, 256, 256]
    finally:
        e.close()


def test_a_multi_device_handle_refuses_the_call(model_text):
    import gnn_mwvc_amd as G
    e = G.Engine(model_text, devices=[0, 0])
    try:
        for value in (0, FULL):
            with pytest.raises(G.engine.GnnvcError) as ei:
                e.set_generic_big_stages(value)
            assert ei.value.code == ERR_UNSUPPORTED, value
    finally:
        e.close()


# ---------------------------------------------------------------- 9. speed guard

GUARDED = ["too_big", "h128"]   # what the measurement left admitted (profiles/generic_stages/README.md, "Big stages")


def test_big_stages_are_not_slower_than_layer_by_layer():
    import torch
    import gnn_mwvc_amd as G
    from tools import graphgen_torch as ggt
    dev = torch.device("cuda", 0)
    g = ggt.erdos_renyi(1_000_000, 10_000_000, 2, dev)
    x = g.x().contiguous()
    for name in GUARDED:
        e = G.Engine(text_of(name), device=0)
        try:
            e.set_weight_scale(g.ws)
            e.attach_graph_device(g.n, g.nnz, g.rowptr.data_ptr(), g.col.data_ptr(), g.w.data_ptr(), g.nw.data_ptr(), keepalive=g)
            sc = torch.zeros(g.n, device=dev)
            lg = torch.zeros(g.n, device=dev)
            torch.cuda.synchronize()
            ms_off, lg0 = gh.steady_ms(e, x, sc, lg)
            assert e.get_info("generic_stages_active") == 0
            e.set_generic_big_stages(FULL)
            ms_on, lg1 = gh.steady_ms(e, x, sc, lg)
            assert e.get_info("generic_stages_active") == 1
            print(f"er1m {name}: big stages on {ms_on:.3f} ms, off {ms_off:.3f} ms, {ms_off / ms_on:.2f}x")
            assert torch.equal(lg0.view(torch.int32), lg1.view(torch.int32)), name
            assert ms_on <= ms_off + 0.025, f"{name}: big stages {ms_on:.3f} ms vs layer by layer {ms_off:.3f} ms"
        finally:
            e.close()
    del g, x
    torch.cuda.empty_cache()
