"""Generic-stage models (k_stage_any) through every door the trained model is tested through, and through changes made to a live
engine.  The six files beside this one (test_gpu_{shapes,depths,audit_any,heavy_rows,giant_rows,big_stages}.py) hold the
arithmetic to the oracle at every width, depth, row range and threshold, on a fresh engine with an uploaded graph; here the graph
arrives by the staged hand-off, from device arrays, by derivation on the device and through the C++ host mirror, graphs replace
each other on one engine, and thresholds, options, the weight scale and the stream move under a resident graph.  What has to
follow the graph each time is the generic path's per-graph state: the heavy-row list, the giant rows' meta, slab and positions,
the sums buffer sized by the widest stage input, the side queue.

Bars: tests/generic_harness.py's and no other — logits bit for bit the oracle's, scores through check_scores — and the engine's
read-outs of heavy and giant rows equal to numpy's count over the graph that is resident.  The inputs (graphs, the derive chain,
the members) are pinned on the CPU by tests/test_generic_lifecycle_inputs.py."""
import os
import pathlib
import subprocess

import numpy as np
import pytest

from oracle import oracle_py
from tools import graphgen as gg
from tools import modelgen_big as mb
from tests import generic_harness as gh
from tests.generic_harness import bits, check_scores, crafted_input, graph_of, heavy_counts
from tests.test_expf_restatement import shim   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)

pytestmark = pytest.mark.gpu

HEAVY, GIANT = 512, 600
FULL = 163840


def assert_readouts(e, g, heavy, giant, label, ran=True):
    """The engine's classing of the resident graph against numpy: rows of at least `heavy` entries are listed, those among them of
    at least max(heavy, giant) are giant (either threshold 0: none).  ran: a generic stage has run since the last change, so the
    last call's figures are the graph's."""
    rows, entries = heavy_counts(g, heavy)
    grows, gentries = heavy_counts(g, max(heavy, giant)) if heavy and giant else (0, 0)
    got = {k: e.get_info(k) for k in ("generic_heavy_rows", "generic_heavy_entries", "generic_giant_rows", "generic_giant_entries")}
    assert got == {"generic_heavy_rows": rows, "generic_heavy_entries": entries, "generic_giant_rows": grows,
                   "generic_giant_entries": gentries}, label
    if ran:
        assert e.get_info("generic_heavy_last_rows") == rows, label
        assert e.get_info("generic_giant_last_rows") == grows, label


def assert_forward(shim, e, family, name, gname, label):
    """One host forward of the member's model_input on the named graph: logits and scores by the harness's rules."""
    g = graph_of(gname)
    sc, lg = e.forward(gh.FAMILIES[family].model_input(name, g))
    wl = gh.want_of(family, name, gname)[-1][2]
    assert sc.shape == lg.shape == wl.shape, label
    mism = int((bits(lg) != bits(wl)).sum())
    assert mism == 0, (label, f"{mism}/{lg.size} logits differ, first (row, column)", np.argwhere(bits(lg) != bits(wl))[:6].tolist())
    check_scores(shim, sc.reshape(-1), lg.reshape(-1), gh.flat_logits(family, name, gname), label)
    return sc, lg


# ---------------------------------------------------------------- a. every hand-off route, graphs replaced on one live engine

@pytest.mark.parametrize("seg", [0, 1])
@pytest.mark.parametrize("route", gh.ROUTES)
@pytest.mark.parametrize("family,name", gh.LIFECYCLE_MEMBERS)
def test_every_route_replaces_the_graph_on_a_live_engine(shim, family, name, route, seg):
    import gnn_mwvc_amd as G
    fam = gh.FAMILIES[family]
    e = G.Engine(gh.text_of(family, name), device=0)
    try:
        e.set_generic_heavy_rows(HEAVY)
        e.set_generic_giant_rows(GIANT, seg)
        assert e.fused and e.get_info("generic_stages_model") == 1
        heavy_seen = []
        for k, gname in enumerate(gh.LIFECYCLE_SEQUENCE):
            g = graph_of(gname)
            label = (name, route, seg, k, gname)
            gh.hand_over(e, g, route)
            if g.n == 0:
                sc, _ = e.forward(fam.model_input(name, g))
                assert sc.shape == (0, fam.out_width(name)), label
                continue
            assert_forward(shim, e, family, name, gname, label)
            assert e.get_info("generic_stages_active") == 1, label
            assert_readouts(e, g, HEAVY, GIANT, label)
            heavy_seen.append(e.get_info("generic_heavy_last_rows"))
        assert heavy_seen == [7, 0, 7, 0, 0, 7]   # (the empty graph between `one` and `sparse` is not read)
    finally:
        e.close()


# ---------------------------------------------------------------- b. graphs derived on the device

def _chain_wants(family, name):
    """Per step of the derive chain: the oracle's logits on that step's graph at its own weight scale (the last step keeps the
    lists and draws new weights), computed once."""
    key = ("chain wants", family, name)
    if key not in gh._cache:
        gh._cache[key] = [gh.stage_outputs(gh.oracle_of(family, name, g1), family, name, g1)[-1][2] for g1, _ in gh.derive_chain()]
    return gh._cache[key]


def _chain_hashes():
    if "chain hashes" not in gh._cache:
        from tests.test_gpu_parity import _fnv_rows
        first, second = (_fnv_rows(g1) for g1, _ in gh.derive_chain()[:2])
        gh._cache["chain hashes"] = [first, second, second]   # (the last step keeps every list)
    return gh._cache["chain hashes"]


@pytest.mark.parametrize("heavy,seg", [(512, 1), (256, 0)])
@pytest.mark.parametrize("family,name", gh.DERIVE_MEMBERS)
def test_graphs_derived_on_the_device_carry_their_own_heavy_rows(family, name, heavy, seg):
    fam = gh.FAMILIES[family]
    g = graph_of("hubs")
    e = gh.open_engine(family, name, g, heavy=heavy, giant=(GIANT, seg), expect_fused=True)
    try:
        _, lg = e.forward(fam.model_input(name, g))
        assert np.array_equal(bits(lg), bits(gh.want_of(family, name, "hubs")[-1][2]))
        assert_readouts(e, g, heavy, GIANT, (name, heavy, "uploaded"))
        for step, (g1, old_row) in enumerate(gh.derive_chain()):
            label = (name, heavy, step)
            tail = e.derive_graph(g1, old_row)
            ns = int((old_row != 0xFFFFFFFF).sum())
            deg1 = gh.degrees(g1)
            # survivors keep only new-vertex ids in their tails; new vertices' lists are all tail
            want_tail = np.array([int((g1.col[int(g1.rowptr[u]):int(g1.rowptr[u + 1])] >= ns).sum()) if u < ns else deg1[u]
                                  for u in range(g1.n)], dtype=np.uint32)
            assert np.array_equal(tail, want_tail), label
            assert np.array_equal(e.row_hashes(), _chain_hashes()[step]), label
            assert_readouts(e, g1, heavy, GIANT, label, ran=False)   # (classed at the commit: the generic list is in force)
            e.set_weight_scale(g1.ws)
            _, lg = e.forward(fam.model_input(name, g1))
            want = _chain_wants(family, name)[step]
            mism = int((bits(lg) != bits(want)).sum())
            assert mism == 0, (label, f"{mism}/{lg.size} logits differ", np.argwhere(bits(lg) != bits(want))[:6].tolist())
            assert e.get_info("generic_stages_active") == 1, label
            assert_readouts(e, g1, heavy, GIANT, label)
        e.upload_graph(g1)   # ... and the graph an upload would have produced: the same bits again
        _, again = e.forward(fam.model_input(name, g1))
        assert np.array_equal(bits(again), bits(lg)) and np.array_equal(bits(again), bits(_chain_wants(family, name)[2]))
        assert_readouts(e, g1, heavy, GIANT, (name, heavy, "uploaded again"))
    finally:
        e.close()


# ---------------------------------------------------------------- c. live changes on one engine and one graph

@pytest.mark.parametrize("family,name", [("shapes", "odd"), ("depths", "in3_f32")])
def test_live_changes_under_a_resident_graph(shim, family, name):
    import torch
    fam = gh.FAMILIES[family]
    gname = "hubs"
    g = graph_of(gname)
    x = fam.model_input(name, g)
    want = gh.want_of(family, name, gname)[-1][2]
    want77 = gh.logits_at(family, name, g, ws=77.0)     # (once per weight scale)
    assert not np.array_equal(bits(want77), bits(want))
    e = gh.open_engine(family, name, g, heavy=HEAVY, expect_fused=True)
    try:
        e.set_generic_giant_rows(GIANT, 0)

        def step(heavy, giant, label):
            assert_forward(shim, e, family, name, gname, label)
            assert e.get_info("generic_stages_active") == 1, label
            assert_readouts(e, g, heavy, giant, label)

        step(HEAVY, GIANT, "first")
        # the heavy threshold
        for thr in (0, 1, 513, 512):
            e.set_generic_heavy_rows(thr)
            step(thr, GIANT, ("heavy", thr))
        # the giant rows
        e.set_generic_giant_rows(GIANT, 1)
        step(HEAVY, GIANT, "giant rows, segments 1")
        assert e.get_info("generic_giant_segments") == 1
        assert e.get_info("generic_giant_last_segmented") == 0   # (no row of hubs is longer than one segment of the scan, 4096 addends)
        e.set_generic_giant_rows(0, -1)
        step(HEAVY, 0, "no giant rows")
        e.set_generic_giant_rows(GIANT, 1)
        step(HEAVY, GIANT, "giant rows again")
        # option "generic_stages"
        e.set_option("generic_stages", 0)
        assert not e.fused and e.num_stages == 0
        assert_forward(shim, e, family, name, gname, "generic_stages 0")
        assert e.get_info("generic_stages_active") == 0
        e.set_option("generic_stages", 1)
        assert e.fused and e.num_stages == len(fam.specs[name][1])
        step(HEAVY, GIANT, "generic_stages 1")
        # the weight scale
        e.set_weight_scale(77.0)
        _, lg = e.forward(x)
        assert np.array_equal(bits(lg), bits(want77)), "weight scale 77"
        assert_readouts(e, g, HEAVY, GIANT, "weight scale 77")
        e.set_weight_scale(g.ws)
        step(HEAVY, GIANT, "weight scale back")
        # a caller-owned stream, heavy and giant rows in force: the side queue is probed again
        dev = torch.device("cuda:0")
        dx = torch.from_numpy(x).to(dev)
        dsc = torch.full((g.n, 1), float("nan"), dtype=torch.float32, device=dev)
        dlg = torch.full((g.n, 1), float("nan"), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        mine = torch.cuda.Stream(device=dev)
        e.set_stream(mine.cuda_stream)
        try:
            assert e.get_info("side_queue_runs_beside") == 1
            e.forward_device(dx.data_ptr(), dsc.data_ptr(), dlg.data_ptr())
            mine.synchronize()
        finally:
            e.set_stream(None)
        check_scores(shim, dsc.cpu().numpy().reshape(-1), dlg.cpu().numpy().reshape(-1), gh.flat_logits(family, name, gname), "caller's stream")
        assert_readouts(e, g, HEAVY, GIANT, "caller's stream")
        step(HEAVY, GIANT, "the engine's own stream again")
        # the explicit audit, once, at the end
        _, lg = e.forward_audited(x)
        assert np.array_equal(bits(lg), bits(want))
        rep = e.audit_report()
        assert rep["audit_runs"] == e.num_stages and rep["audit_failures"] == 0 and rep["audit_repairs"] == 0, rep
    finally:
        e.close()


def test_big_stages_switched_on_and_off_under_a_resident_graph(shim):
    family, name, gname = "big", "odd_wide", "hubs"
    g = graph_of(gname)
    e = gh.open_engine(family, name, g, heavy=HEAVY)
    try:
        e.set_generic_giant_rows(GIANT, 1)
        assert not e.fused and e.num_stages == 0
        _, lg0 = assert_forward(shim, e, family, name, gname, "layer by layer")
        assert e.get_info("generic_stages_active") == 0
        e.set_generic_big_stages(FULL)
        assert e.fused and e.num_stages == len(mb.SPECS[name][1])
        widths = zip(mb.stage_widths(name), mb.SPECS[name][1])
        assert [e.get_info(f"generic_stage_threads_{s}") for s in range(e.num_stages)] == [mb.stage_threads(f, ws, FULL) for (f, _), ws in widths]
        _, lg1 = assert_forward(shim, e, family, name, gname, "big stages on")
        assert e.get_info("generic_stages_active") == 1
        assert_readouts(e, g, HEAVY, GIANT, "big stages on")
        e.set_generic_big_stages(0)
        assert not e.fused and e.num_stages == 0
        _, lg2 = assert_forward(shim, e, family, name, gname, "big stages off")
        assert e.get_info("generic_stages_active") == 0
        assert np.array_equal(bits(lg0), bits(lg1)) and np.array_equal(bits(lg0), bits(lg2))
        # ... and on again for the explicit audit, which a layer-by-layer model has no stages for
        e.set_generic_big_stages(FULL)
        _, lg3 = e.forward_audited(mb.model_input(name, g))
        assert np.array_equal(bits(lg3), bits(lg0))
        rep = e.audit_report()
        assert rep["audit_runs"] == e.num_stages and rep["audit_failures"] == 0 and rep["audit_repairs"] == 0, rep
        assert_readouts(e, g, HEAVY, GIANT, "big stages on again")
    finally:
        e.close()


# ---------------------------------------------------------------- d. the C++ host mirror

def _predict_tool():
    pkg = pathlib.Path(__file__).resolve().parent.parent / "gnn-mwvc_amd"
    tool = pkg / "gnnvc_predict"
    if not tool.exists():
        r = subprocess.run(["make", "-C", str(pkg / "host")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return tool


def _run_predict(tmp_path, family, name, gname, env=None):
    (tmp_path / "g.metis").write_text(gg.metis_text(graph_of(gname)))
    (tmp_path / "m.txt").write_text(gh.text_of(family, name))
    r = subprocess.run([str(_predict_tool()), str(tmp_path / "m.txt"), str(tmp_path / "g.metis"), str(tmp_path / "s.f32")],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return (tmp_path / "s.f32").read_bytes(), r.stderr


@pytest.mark.parametrize("gname", ["hubs", "er1933"])
@pytest.mark.parametrize("family,name", [("shapes", "odd"), ("depths", "mixed"), ("depths", "too_big")])
def test_host_mirror_predict_with_a_generic_model(tmp_path, family, name, gname):
    """gnn::model::predict hands every graph over staged and scores it once: scores bit for bit the oracle's (too_big stays layer
    by layer through the mirror)."""
    raw, _ = _run_predict(tmp_path, family, name, gname)
    want = gh.want_of(family, name, gname)[-1][1]
    got = np.frombuffer(raw, dtype=np.float32)
    assert got.shape == (graph_of(gname).n,)
    assert np.array_equal(bits(got), bits(want.reshape(-1)))


def test_host_mirror_derives_the_graph_of_a_generic_model(tmp_path):
    """GNNVC_DELTA=1: the second predict of the tool derives its graph on the device; GNNVC_TRACE=1 turns "forward_timing" 2 on
    and reads gnnvc_last_forward_ms, on a model of three generic stages."""
    family, name, gname = "shapes", "odd", "hubs"
    plain, _ = _run_predict(tmp_path, family, name, gname)
    raw, err = _run_predict(tmp_path, family, name, gname, env=dict(os.environ, GNNVC_DELTA="1", GNNVC_TRACE="1"))
    assert raw == plain
    assert np.array_equal(bits(np.frombuffer(raw, dtype=np.float32)), bits(gh.want_of(family, name, gname)[-1][1].reshape(-1)))
    assert err.count("derived on the device") >= 1, err
    assert err.count("gnnvc predict") == 2, err


# ---------------------------------------------------------------- e. the graph-reading entry points beside a generic model

@pytest.mark.parametrize("family,name", [("shapes", "odd"), ("depths", "in3_f32")])
def test_graph_reading_entry_points_on_an_engine_with_a_generic_model(shim, family, name):
    assert gh.FAMILIES[family].out_width(name) == 1
    e = gh.open_engine(family, name, graph_of("er1933"), heavy=HEAVY, giant=(GIANT, 1), expect_fused=True)
    try:
        for gname in ("er1933", "hubs"):
            g = graph_of(gname)
            gh.hand_over(e, g, "upload")
            got = e.reduction_flags(20)
            want = oracle_py.reduction_flags(g, 20)
            assert np.array_equal(got, want), (gname, [int(((got ^ want) >> b & 1).sum()) for b in range(7)])
            sc, _ = assert_forward(shim, e, family, name, gname, (name, gname))
            keys, above = e.score_keys()
            want_k, want_a = oracle_py.score_keys(sc[:, 0])
            assert np.array_equal(bits(keys), bits(want_k)) and np.array_equal(above, want_a), gname
            # the layer-by-layer graph layer, which too_big and every "generic_stages" 0 comparison rest on, at generic widths
            for f in (5, 9, 32):
                h = crafted_input(g.n, f, 300 + f)
                assert np.array_equal(bits(e.graph_layer(h)), bits(oracle_py.graph_layer(g, g.ws, h))), (gname, f)
            assert_forward(shim, e, family, name, gname, (name, gname, "after the entry points"))
            assert_readouts(e, g, HEAVY, GIANT, (name, gname))
    finally:
        e.close()
