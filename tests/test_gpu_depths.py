"""Stages of one to six dense layers as fused stages (option "generic_stages", kernel k_stage_any), under
tools/modelgen_depths.py's family (tests/test_modelgen_depths.py shows on the oracle that every member's logits are alive).

Bars, as in tests/test_gpu_shapes.py and no wider: logits and every stage's output bit for bit against the oracle, scores
within 1 ulp of the oracle's and bit for bit the restated sigmoid's (check_scores of tests/test_gpu_models.py), rows outside a
stage call's range and the pad row untouched.  With the option at 0 the same models are not fused, have no stages and run
layer by layer — with the same bits.  `too_big` lies outside the kernel's 64 KiB of LDS and stays layer by layer under every
option value.  Several devices, gnnvc_stage_input_ready and the audit stay refused / idle for these models.

The speed guard at the end is test_generic_stages_are_not_slower_than_layer_by_layer's, for a four-deep and a one-deep model."""
import functools

import numpy as np
import pytest

from tools import modelgen_depths as md
from tests import generic_harness as gh
from tests.generic_harness import bits, check_scores, graph_of
from tests.test_expf_restatement import shim, _run   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)

pytestmark = pytest.mark.gpu

# the accessors of tests/generic_harness.py, for the family of this file
text_of, want_of, flat_logits, open_engine = (functools.partial(f, "depths")
                                              for f in (gh.text_of, gh.want_of, gh.flat_logits, gh.open_engine))
GRAPHS = ["er3000", "sparse", "er1933", "one", "hub6k"]   # (tests/generic_harness.py has what each is)
ERR_UNSUPPORTED = -5
ERR_INVALID = -1


def test_graphs_are_what_the_names_say():
    deg = {k: np.diff(graph_of(k).rowptr.astype(np.int64)) for k in GRAPHS}
    assert (deg["hub6k"] >= 3000).sum() == 2
    assert (deg["sparse"] == 0).mean() > 0.2
    assert graph_of("er1933").n % 16 != 0 and graph_of("one").n == 1


# ---------------------------------------------------------------- 1. fused, and what the interface reports

@pytest.mark.parametrize("name", md.FITTING)
def test_model_is_fused_and_reports_its_stages(name):
    import gnn_mwvc_amd as G
    e = G.Engine(text_of(name), device=0)
    try:
        assert e.fused, name
        assert e.num_stages == len(md.SPECS[name][1]), name
        assert [e.stage_widths(s) for s in range(e.num_stages)] == md.stage_widths(name), name
        assert [e.get_info(f"generic_stage_layers_{s}") for s in range(e.num_stages)] == md.stage_depths(name), name
        assert e.get_info("generic_stages_model") == 1
        assert e.get_info("generic_max_dense_layers") == md.MAX_DENSE_LAYERS == 6
        for key in (f"generic_stage_layers_{e.num_stages}", "generic_stage_layers_", "generic_stage_layers_-1", "generic_stage_layers_0x"):
            with pytest.raises(G.engine.GnnvcError) as ei:
                e.get_info(key)
            assert ei.value.code == ERR_INVALID, key
        e.set_option("generic_stages", 0)   # not generic any more: the key has nothing to report
        with pytest.raises(G.engine.GnnvcError) as ei:
            e.get_info("generic_stage_layers_0")
        assert ei.value.code == ERR_INVALID
        assert e.get_info("generic_max_dense_layers") == 6
    finally:
        e.close()


def test_trained_model_has_no_generic_stage_layers():
    import gnn_mwvc_amd as G
    e = G.Engine(G.default_model_text(), device=0)
    try:
        assert e.fused and e.get_info("generic_stages_model") == 0
        with pytest.raises(G.engine.GnnvcError) as ei:
            e.get_info("generic_stage_layers_0")
        assert ei.value.code == ERR_INVALID
        e.set_option("generic_stages", 2)
        assert [e.get_info(f"generic_stage_layers_{s}") for s in range(3)] == [3, 3, 3]
    finally:
        e.close()


# ---------------------------------------------------------------- 2. + 3. every model on every graph: forward and stage entry

@pytest.mark.parametrize("gname", list(GRAPHS))
@pytest.mark.parametrize("name", md.FITTING)
def test_forward_and_stage_entry(shim, name, gname):
    import torch
    import gnn_mwvc_amd as G
    g = graph_of(gname)
    want = want_of(name, gname)
    wl = want[-1][2]
    x = md.model_input(name, g)
    e = open_engine(name, g, expect_fused=True)
    try:
        # ---- whole forwards (twice: nothing may depend on what an earlier forward left)
        for rep in range(2):
            sc, lg = e.forward(x)
            assert sc.shape == lg.shape == (g.n, md.out_width(name))
            mism = int((bits(lg) != bits(wl)).sum())
            assert mism == 0, (name, gname, rep, f"{mism}/{lg.size} logits differ", np.argwhere(bits(lg) != bits(wl))[:6].tolist())
            assert e.get_info("generic_stages_active") == 1
            check_scores(shim, sc.reshape(-1), lg.reshape(-1), flat_logits(name, gname), (name, gname, rep))
        # ---- the stage entry over split row ranges, each stage fed the oracle's input: first two ranges with a gap between
        # them (the gap, the rows behind and the pad row stay as they were), then the gap
        n = g.n
        first, gap = gh.split_ranges(n)
        assert len(want) == e.num_stages
        for s, (hin, hout, pre) in enumerate(want):
            done = gh.run_stage_ranges(e, "depths", name, g, s, hin, [first, gap], hout, pre, (name, gname))
            assert done[:n].all() and not done[n]
        # a stage index beyond the model
        t = torch.zeros((n + 1, 32), dtype=torch.float32, device="cuda:0")
        with pytest.raises(G.engine.GnnvcError) as ei:
            e.stage_forward_device(len(want), 0, n, t.data_ptr(), t.data_ptr())
        assert ei.value.code == ERR_INVALID
    finally:
        e.close()


# ---------------------------------------------------------------- 4. the option

@pytest.mark.parametrize("name", md.FITTING)
def test_option_0_is_layer_by_layer_with_the_same_bits(name):
    for gname in ("er3000", "hub6k"):
        g = graph_of(gname)
        x = md.model_input(name, g)
        e = open_engine(name, g, expect_fused=True)
        try:
            sc1, lg1 = e.forward(x)
            assert e.get_info("generic_stages_active") == 1
            e.set_option("generic_stages", 0)   # (takes effect at once)
            assert not e.fused and e.num_stages == 0 and e.get_info("generic_stages_model") == 0
            with pytest.raises(Exception) as ei:
                e.stage_widths(0)
            assert ei.value.code == ERR_INVALID
            sc0, lg0 = e.forward(x)
            assert e.get_info("generic_stages_active") == 0
            assert np.array_equal(bits(lg0), bits(lg1)) and np.array_equal(bits(sc0), bits(sc1)), (name, gname)
            assert np.array_equal(bits(lg0), bits(want_of(name, gname)[-1][2])), (name, gname)
            e.set_option("generic_stages", 1)
            assert e.fused and e.num_stages == len(md.SPECS[name][1])
        finally:
            e.close()
        # an engine that has the option at 0 from the start
        e = open_engine(name, g, {"generic_stages": 0})
        try:
            assert not e.fused and e.num_stages == 0
            sc, lg = e.forward(x)
            assert np.array_equal(bits(lg), bits(lg1)) and np.array_equal(bits(sc), bits(sc1)), (name, gname)
        finally:
            e.close()


# ---------------------------------------------------------------- 5. outside the LDS bound

@pytest.mark.parametrize("option", [1, 2])
def test_too_big_stays_layer_by_layer(shim, option):
    g = graph_of("er3000")
    e = open_engine("too_big", g, {"generic_stages": option})
    try:
        assert not e.fused and e.num_stages == 0 and e.get_info("generic_stages_model") == 0
        sc, lg = e.forward(md.model_input("too_big", g))
        assert e.get_info("generic_stages_active") == 0
        wl = want_of("too_big", "er3000")[-1][2]
        assert np.array_equal(bits(lg), bits(wl))
        check_scores(shim, sc.reshape(-1), lg.reshape(-1), flat_logits("too_big", "er3000"), "too_big")
    finally:
        e.close()


# ---------------------------------------------------------------- 6. what stays refused

@pytest.mark.parametrize("name", ["two_deep", "mixed"])
def test_several_devices_refuse_a_generic_model(name):
    import gnn_mwvc_amd as G
    with pytest.raises(G.engine.GnnvcError) as ei:
        G.Engine(text_of(name), devices=[0, 0])
    assert ei.value.code == ERR_UNSUPPORTED, name


@pytest.mark.parametrize("name", ["two_deep", "mixed"])
def test_stage_input_ready_is_refused_and_the_audit_idle(name):
    import torch
    import gnn_mwvc_amd as G
    g = graph_of("er3000")
    e = open_engine(name, g, expect_fused=True)
    try:
        f, _ = md.stage_widths(name)[1]
        t = torch.zeros((g.n + 1, f), dtype=torch.float32, device="cuda:0")
        with pytest.raises(G.engine.GnnvcError) as ei:
            e.stage_input_ready(1, t.data_ptr(), 0, g.n)
        assert ei.value.code == ERR_UNSUPPORTED
        if f != 16:
            with pytest.raises(G.engine.GnnvcError) as ei:
                e.live_columns(t.data_ptr(), g.n, f)
            assert ei.value.code == ERR_UNSUPPORTED
        e.set_option("audit_period", 1)
        _, lg = e.forward(md.model_input(name, g))
        assert e.get_info("audit_runs") == 0 and e.get_info("audit_failures") == 0
        assert np.array_equal(bits(lg), bits(want_of(name, "er3000")[-1][2]))
    finally:
        e.close()


# ---------------------------------------------------------------- 7. speed guard

def test_deeper_and_shallower_stages_are_not_slower_than_layer_by_layer():
    import torch
    import gnn_mwvc_amd as G
    from tools import graphgen_torch as ggt
    dev = torch.device("cuda", 0)
    g = ggt.erdos_renyi(1_000_000, 10_000_000, 2, dev)
    x = g.x().contiguous()
    for name in ("four_deep", "one_each"):
        ms_layers, lg0 = gh.steady_ms_under_option("depths", name, g, x, 0)
        ms_fused, lg1 = gh.steady_ms_under_option("depths", name, g, x, 1)
        print(f"er1m {name}: generic_stages=1 {ms_fused:.3f} ms, =0 {ms_layers:.3f} ms, {ms_layers / ms_fused:.2f}x")
        assert torch.equal(lg0.view(torch.int32), lg1.view(torch.int32)), name
        assert ms_fused <= ms_layers + 0.025, f"{name}: generic stages {ms_fused:.3f} ms vs layer by layer {ms_layers:.3f} ms"
    del g, x
    torch.cuda.empty_cache()
