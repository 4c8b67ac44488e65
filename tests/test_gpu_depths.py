"""Stages of one to six dense layers as fused stages (option "generic_stages", kernel k_stage_any), under
tools/modelgen_depths.py's family (tests/test_modelgen_depths.py shows on the oracle that every member's logits are alive).

Bars, as in tests/test_gpu_shapes.py and no wider: logits and every stage's output bit for bit against the oracle, scores
within 1 ulp of the oracle's and bit for bit the restated sigmoid's (check_scores of tests/test_gpu_models.py), rows outside a
stage call's range and the pad row untouched.  With the option at 0 the same models are not fused, have no stages and run
layer by layer — with the same bits.  `too_big` lies outside the kernel's 64 KiB of LDS and stays layer by layer under every
option value.  Several devices, gnnvc_stage_input_ready and the audit stay refused / idle for these models.

The speed guard at the end is test_generic_stages_are_not_slower_than_layer_by_layer's, for a four-deep and a one-deep model."""
import time

import numpy as np
import pytest

from oracle import oracle_py
from tools import graphgen as gg
from tools import modelgen_depths as md
from tests.test_expf_restatement import shim, _run   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)
from tests.test_gpu_models import bits, check_scores, ulp
from tests.test_modelgen_depths import stage_outputs

pytestmark = pytest.mark.gpu

GRAPHS = {
    "er3000": lambda: gg.erdos_renyi(3000, 15000, 15),
    "sparse": lambda: gg.erdos_renyi(5000, 3000, 23),                     # about three rows in ten are empty
    "er1933": lambda: gg.erdos_renyi(1933, 7000, 61),                     # n is not a multiple of 16
    "one": lambda: gg.from_edge_list(1, [], [57]),                        # n = 1
    "hub6k": lambda: gg.hub_graph(6000, 18000, 2, 3000, seed=9),          # two rows of 3000 entries: many gather rounds a row
}
ERR_UNSUPPORTED = -5
ERR_INVALID = -1

_cache = {}


def text_of(name):
    if ("text", name) not in _cache:
        _cache["text", name] = md.FAMILY[name]()
    return _cache["text", name]


def graph_of(gname):
    if ("graph", gname) not in _cache:
        _cache["graph", gname] = GRAPHS[gname]()
    return _cache["graph", gname]


def want_of(name, gname):
    """[(stage input, stage output, pre-activation of the stage's last linear layer)] from the oracle's layers."""
    if ("want", name, gname) not in _cache:
        g = graph_of(gname)
        om = oracle_py.OracleModel(text_of(name))
        om.set_weight_scale(g.ws)
        _cache["want", name, gname] = stage_outputs(om, name, g)
    return _cache["want", name, gname]


def flat_logits(name, gname):
    key = ("flat", name, gname)
    if key not in _cache:
        _cache[key] = np.ascontiguousarray(want_of(name, gname)[-1][2].reshape(-1))
    return _cache[key]


def open_engine(name, g, opts=(), expect_fused=True):
    import gnn_mwvc_amd as G
    e = G.Engine(text_of(name), device=0)
    try:
        for k, v in dict(opts).items():
            e.set_option(k, v)
        assert e.num_layers == md.num_layers(name) and e.in_width == md.in_width(name) and e.out_width == md.out_width(name), name
        if expect_fused:
            assert e.fused, name
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
    except BaseException:
        e.close()
        raise
    return e


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
    e = open_engine(name, g)
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
        dev = torch.device("cuda:0")
        n = g.n
        cuts = sorted({0, n // 5, n // 3, (2 * n) // 3, n})
        ranges = list(zip(cuts[:-1], cuts[1:]))
        first, gap = (ranges[0::2], ranges[1::2]) if len(ranges) > 1 else (ranges, [])
        assert len(want) == e.num_stages
        for s, (hin, hout, pre) in enumerate(want):
            f, n_out = md.stage_widths(name)[s]
            last = s + 1 == len(want)
            tin = torch.zeros((n + 1, f), dtype=torch.float32, device=dev)
            tin[:n] = torch.from_numpy(np.ascontiguousarray(hin)).to(dev)
            out = torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)
            lgt = torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            for part, todo in enumerate((first, gap)):
                for lo, hi in todo:
                    e.stage_forward_device(s, lo, hi, tin.data_ptr(), out.data_ptr(), lgt.data_ptr() if last else 0)
                e.synchronize()
                got, gotl = out.cpu().numpy(), lgt.cpu().numpy()
                done = np.zeros(n + 1, dtype=bool)
                for lo, hi in (first if part == 0 else first + gap):
                    done[lo:hi] = True
                assert np.isnan(got[~done]).all(), (name, gname, s, part, "rows outside the ranges were written")
                assert np.isnan(gotl[~done]).all() if last else np.isnan(gotl).all(), (name, gname, s, part, "logits rows")
                w_out = hout[done[:n]]
                if last:
                    assert np.array_equal(bits(gotl[:n][done[:n]]), bits(pre[done[:n]])), (name, gname, s, part, "stage logits")
                    assert ulp(got[:n][done[:n]], w_out).max(initial=0) <= 1, (name, gname, s, part, "stage scores")
                else:
                    bad = np.argwhere(bits(got[:n][done[:n]]) != bits(w_out))
                    assert bad.size == 0, (name, gname, s, part, f"{len(bad)} values differ, first (row, column)", bad[:6].tolist())
            assert done[:n].all() and not done[n]
        # a stage index beyond the model
        t = torch.zeros((n + 1, 32), dtype=torch.float32, device=dev)
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
        e = open_engine(name, g)
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
        e = open_engine(name, g, {"generic_stages": 0}, expect_fused=False)
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
    e = open_engine("too_big", g, {"generic_stages": option}, expect_fused=False)
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
    e = open_engine(name, g)
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

def _steady_ms(G, torch, name, g, x, generic, dev):
    e = G.Engine(text_of(name), device=0)
    try:
        e.set_option("generic_stages", generic)
        e.set_weight_scale(g.ws)
        e.attach_graph_device(g.n, g.nnz, g.rowptr.data_ptr(), g.col.data_ptr(), g.w.data_ptr(), g.nw.data_ptr(), keepalive=g)
        sc = torch.zeros(g.n, device=dev)
        lg = torch.zeros(g.n, device=dev)
        torch.cuda.synchronize()
        for _ in range(2):
            e.forward_device(x.data_ptr(), sc.data_ptr(), lg.data_ptr())
        e.synchronize()
        assert e.get_info("generic_stages_active") == (1 if generic else 0)
        best = 1e9
        for _ in range(3):                       # the best of three batches of five, as tests/test_gpu_shapes.py
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(5):
                e.forward_device(x.data_ptr(), sc.data_ptr(), lg.data_ptr())
            e.synchronize()
            best = min(best, (time.perf_counter() - t) * 200.0)
        return best, lg.clone()
    finally:
        e.close()


def test_deeper_and_shallower_stages_are_not_slower_than_layer_by_layer():
    import torch
    import gnn_mwvc_amd as G
    from tools import graphgen_torch as ggt
    dev = torch.device("cuda", 0)
    g = ggt.erdos_renyi(1_000_000, 10_000_000, 2, dev)
    x = g.x().contiguous()
    for name in ("four_deep", "one_each"):
        ms_layers, lg0 = _steady_ms(G, torch, name, g, x, 0, dev)
        ms_fused, lg1 = _steady_ms(G, torch, name, g, x, 1, dev)
        print(f"er1m {name}: generic_stages=1 {ms_fused:.3f} ms, =0 {ms_layers:.3f} ms, {ms_layers / ms_fused:.2f}x")
        assert torch.equal(lg0.view(torch.int32), lg1.view(torch.int32)), name
        assert ms_fused <= ms_layers + 0.025, f"{name}: generic stages {ms_fused:.3f} ms vs layer by layer {ms_layers:.3f} ms"
    del g, x
    torch.cuda.empty_cache()
