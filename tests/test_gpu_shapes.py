"""Models of other layer widths than the trained one as fused stages (option "generic_stages", kernel k_stage_any), under
tools/modelgen_shapes.py's family (tests/test_modelgen_shapes.py shows on the oracle that every member's logits are alive).

Bars, as in the rest of the GPU suite and no wider: logits and every stage's output bit for bit against the oracle, scores
within 1 ulp of the oracle's and bit for bit the restated sigmoid's (check_scores of tests/test_gpu_models.py), rows outside a
stage call's range and the pad row untouched.  With the option at 0 the same models are what they were before it existed: not
fused, no stages, layer by layer — and the same bits.  With it at 2 the TRAINED model goes through the generic kernel and
reproduces tests/golden/ and the default engine.

The speed guard at the end is in the style of tests/test_gpu_perf_guard.py: steady forwards with the option at 1 are not slower
than with it at 0 (which stands for the engine before the option: forward_unfused and the layer-by-layer kernels are
untouched by it)."""
import functools
import json

import numpy as np
import pytest

from oracle import oracle_py
from tools import graphgen as gg
from tools import modelgen_shapes as ms
from tests import generic_harness as gh
from tests.generic_harness import bits, check_scores, graph_of, ulp
from tests.test_expf_restatement import shim, _run   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)

pytestmark = pytest.mark.gpu

MODELS = list(ms.SPECS)
# the accessors of tests/generic_harness.py, for the family of this file
text_of, want_of, flat_logits, open_engine = (functools.partial(f, "shapes")
                                              for f in (gh.text_of, gh.want_of, gh.flat_logits, gh.open_engine))
GRAPHS = ["er3000", "er100k", "hub20k", "sparse", "er1933", "one"]   # (tests/generic_harness.py has what each is)
ERR_UNSUPPORTED = -5
ERR_INVALID = -1


def test_graphs_are_what_the_names_say():
    deg = {k: np.diff(graph_of(k).rowptr.astype(np.int64)) for k in GRAPHS}
    assert deg["hub20k"].max() > 16384 and (deg["hub20k"] > 16384).sum() == 2
    assert (deg["sparse"] == 0).mean() > 0.2
    assert graph_of("er1933").n % 64 != 0 and graph_of("er3000").n % 64 != 0
    assert graph_of("one").n == 1 and graph_of("er100k").n == 100000 and graph_of("er100k").n_edges == 1000000


# ---------------------------------------------------------------- every model on every graph: forward and stage entry

@pytest.mark.parametrize("gname", list(GRAPHS))
@pytest.mark.parametrize("name", MODELS)
def test_forward_and_stage_entry(shim, name, gname):
    g = graph_of(gname)
    want = want_of(name, gname)
    wl = want[-1][2]
    x = ms.model_input(name, g)
    e = open_engine(name, g, expect_fused=True)
    try:
        # ---- whole forwards (twice: nothing may depend on what an earlier forward left)
        for rep in range(2):
            sc, lg = e.forward(x)
            assert sc.shape == lg.shape == (g.n, ms.out_width(name))
            mism = int((bits(lg) != bits(wl)).sum())
            assert mism == 0, (name, gname, rep, f"{mism}/{lg.size} logits differ", np.argwhere(bits(lg) != bits(wl))[:6].tolist())
            assert e.get_info("generic_stages_active") == 1
        check_scores(shim, sc.reshape(-1), lg.reshape(-1), flat_logits(name, gname), (name, gname))
        # ---- the stage entry over split row ranges, each stage fed the oracle's input: first two ranges with a gap between
        # them (the gap, the rows behind and the pad row stay as they were), then the gap
        first, gap = gh.split_ranges(g.n)
        for s, (hin, hout, pre) in enumerate(want):
            done = gh.run_stage_ranges(e, "shapes", name, g, s, hin, [first, gap], hout, pre, (name, gname))
            assert done[:g.n].all() and not done[g.n]
    finally:
        e.close()


# ---------------------------------------------------------------- the option

@pytest.mark.parametrize("name", MODELS)
def test_option_0_is_the_engine_before_the_option(name):
    """Not fused, 0 stages, no stage entry, layer by layer — and the generic path's bits, scores included."""
    for gname in ("er3000", "hub20k"):
        g = graph_of(gname)
        x = ms.model_input(name, g)
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
            assert e.fused and e.num_stages == len(ms.SPECS[name][1])
            sc2, lg2 = e.forward(x)
            assert e.get_info("generic_stages_active") == 1 and np.array_equal(bits(lg2), bits(lg1))
        finally:
            e.close()
        # an engine that has the option at 0 from the start
        e = open_engine(name, g, {"generic_stages": 0})
        try:
            assert not e.fused and e.num_stages == 0
            _, lg = e.forward(x)
            assert np.array_equal(bits(lg), bits(lg1)), (name, gname)
        finally:
            e.close()


def _golden_graph(p):
    return (gg.from_edge_list(p["n"], p["edges"], p["weights"]) if p["kind"] == "edge_list" else
            gg.erdos_renyi(p["n"], p["m"], p["seed"]) if p["kind"] == "erdos_renyi" else
            gg.hub_graph(p["n"], p["m"], p["hubs"], p["hub_degree"], seed=p["seed"]))


def _trained_engine(g, opts):
    import gnn_mwvc_amd as G
    e = G.Engine(G.default_model_text(), device=0)
    for k, v in opts.items():
        e.set_option(k, v)
    e.set_weight_scale(g.ws)
    e.upload_graph(g)
    return e


@pytest.mark.parametrize("name", ["ex3", "er4k", "hub2k"])
def test_option_2_trained_model_reproduces_the_layer_fixtures(golden_dir, name):
    """h1, h2 and the logits of tests/golden/manifest_layers.json through the generic kernel's stage entry and forward."""
    import torch
    spec = json.loads((golden_dir / "manifest_layers.json").read_text())["graphs"][name]
    g = _golden_graph(spec["graph"])
    assert gg.metis_md5(g) == spec["metis_md5"]
    gold = {k: np.fromfile(golden_dir / f["file"], dtype=np.float32).reshape(f["shape"]) for k, f in spec["files"].items()}
    e = _trained_engine(g, {"generic_stages": 2})
    try:
        assert e.fused and e.num_stages == 3 and e.get_info("generic_stages_model") == 1
        assert [e.stage_widths(s) for s in range(3)] == [(1, 16), (16, 16), (16, 1)]
        sc, lg = e.forward(g.x())
        assert e.get_info("generic_stages_active") == 1
        assert np.array_equal(bits(lg), bits(gold["logits"])), name
        assert ulp(sc, gold["scores2"]).max() <= 1, name
        dev = torch.device("cuda:0")
        cur = torch.from_numpy(g.x()).to(dev)
        for s, what in enumerate(("h1", "h2", "logits")):
            w = 16 if s < 2 else 1
            out = torch.full((g.n + 1, w), float("nan"), dtype=torch.float32, device=dev)
            lgt = torch.full((g.n + 1, 1), float("nan"), dtype=torch.float32, device=dev)
            e.stage_forward_device(s, 0, g.n, cur.data_ptr(), out.data_ptr(), lgt.data_ptr() if s == 2 else 0)
            e.synchronize()
            got = (lgt if s == 2 else out).cpu().numpy()
            assert np.array_equal(bits(got[: g.n]), bits(gold[what])), (name, what)
            assert np.isnan(got[g.n]).all()
            nxt = torch.zeros((g.n + 1, w), dtype=torch.float32, device=dev)
            nxt[: g.n] = out[: g.n]
            cur = nxt
    finally:
        e.close()


@pytest.mark.parametrize("key", ["ex3", "er100k", "hub200k"])
def test_option_2_trained_model_reproduces_the_golden_scores(golden_dir, key):
    spec = json.loads((golden_dir / "manifest.json").read_text())[key]
    g = _golden_graph(spec["graph"])
    gold = np.fromfile(golden_dir / spec["scores_file"], dtype=np.float32)
    e = _trained_engine(g, {"generic_stages": 2})
    d = _trained_engine(g, {})
    try:
        sc, lg = e.forward(g.x())
        sc_d, lg_d = d.forward(g.x())
        assert e.get_info("generic_stages_active") == 1 and d.get_info("generic_stages_active") == 0
        assert np.array_equal(bits(lg), bits(lg_d)) and np.array_equal(bits(sc), bits(sc_d)), key
        host = oracle_py.sigmoid(lg[:, 0])   # (the host-expf caveat of tests/golden/README.md, as tests/test_gpu_parity.py states it)
        dd = ulp(host, gold)
        assert dd.max() <= 1 and int((dd > 0).sum()) <= 16, key
        assert ulp(sc[:, 0], gold).max() <= 1, key
    finally:
        e.close()
        d.close()


def test_option_2_equals_the_default_engine_on_er300k():
    """The plans at hand-off (LDS table, compact gather) against the kernel that uses none: the same bits, forward after forward;
    and back from 2 to 1 the specialised path is in force again."""
    g = gg.erdos_renyi(300_000, 1_800_000, 11)
    d = _trained_engine(g, {"blocked_min_n": 0, "compact_min_n": 0, "plans_at_handoff": 2})
    e = _trained_engine(g, {"generic_stages": 2})
    try:
        assert d.get_info("generic_stages_model") == 0 and d.fused and d.num_stages == 3
        for rep in range(3):
            sc_d, lg_d = d.forward(g.x())
            sc, lg = e.forward(g.x())
            assert np.array_equal(bits(lg), bits(lg_d)) and np.array_equal(bits(sc), bits(sc_d)), rep
        assert d.get_info("generic_stages_active") == 0 and e.get_info("generic_stages_active") == 1
        e.set_option("generic_stages", 1)
        assert e.get_info("generic_stages_model") == 0
        sc, lg = e.forward(g.x())
        assert e.get_info("generic_stages_active") == 0 and np.array_equal(bits(lg), bits(lg_d))
    finally:
        d.close()
        e.close()


# ---------------------------------------------------------------- what stays refused

@pytest.mark.parametrize("name", ["narrow", "first_trained", "two_stage"])
def test_several_devices_refuse_a_generic_model(name):
    import gnn_mwvc_amd as G
    with pytest.raises(G.engine.GnnvcError) as ei:
        G.Engine(text_of(name), devices=[0, 0])
    assert ei.value.code == ERR_UNSUPPORTED, name


@pytest.mark.parametrize("name", ["narrow", "first_trained"])
def test_stage_input_ready_and_the_codec_keep_their_errors(name):
    import torch
    import gnn_mwvc_amd as G
    g = graph_of("er3000")
    e = open_engine(name, g, expect_fused=True)
    try:
        f, _ = ms.stage_widths(name)[1]
        t = torch.zeros((g.n + 1, f), dtype=torch.float32, device="cuda:0")
        with pytest.raises(G.engine.GnnvcError) as ei:
            e.stage_input_ready(1, t.data_ptr(), 0, g.n)
        assert ei.value.code == ERR_UNSUPPORTED
        if f != 16:
            with pytest.raises(G.engine.GnnvcError) as ei:
                e.live_columns(t.data_ptr(), g.n, f)
            assert ei.value.code == ERR_UNSUPPORTED
        with pytest.raises(G.engine.GnnvcError) as ei:
            e.stage_forward_device(len(ms.SPECS[name][1]), 0, g.n, t.data_ptr(), t.data_ptr())
        assert ei.value.code == ERR_INVALID
        # audit_period on a generic model audits nothing
        e.set_option("audit_period", 1)
        e.forward(ms.model_input(name, g))
        assert e.get_info("audit_runs") == 0 and e.get_info("audit_failures") == 0
    finally:
        e.close()


# ---------------------------------------------------------------- speed guard

@pytest.mark.parametrize("gkind", ["er1m", "rmat20"])
def test_generic_stages_are_not_slower_than_layer_by_layer(gkind):
    import torch
    import gnn_mwvc_amd as G
    from tools import graphgen_torch as ggt
    dev = torch.device("cuda", 0)
    g = ggt.erdos_renyi(1_000_000, 10_000_000, 2, dev) if gkind == "er1m" else ggt.rmat(20, 8, 5, dev)
    x = g.x().contiguous()
    for name in ("wide", "narrow", "first_trained"):
        ms_layers, lg0 = gh.steady_ms_under_option("shapes", name, g, x, 0)
        ms_fused, lg1 = gh.steady_ms_under_option("shapes", name, g, x, 1)
        print(f"{gkind} {name}: generic_stages=1 {ms_fused:.3f} ms, =0 {ms_layers:.3f} ms, {ms_layers / ms_fused:.2f}x")
        assert torch.equal(lg0.view(torch.int32), lg1.view(torch.int32)), (gkind, name)
        assert ms_fused <= ms_layers + 0.025, f"{gkind} {name}: generic stages {ms_fused:.3f} ms vs layer by layer {ms_layers:.3f} ms"
    del g, x
    torch.cuda.empty_cache()
