"""Heavy rows of generic stages (gnnvc_set_generic_heavy_rows): rows of at least the threshold get a workgroup each for their
neighbour sums (k_any_heavy_sums), k_stage_any runs over the light rows and then over the listed ones with those sums.

The bars are those of tests/test_gpu_depths.py and no wider: logits and every stage's output bit for bit against the oracle,
scores through check_scores (within 1 ulp of the oracle's, bit for bit the restated sigmoid's), rows outside a stage call's
ranges and the pad row untouched — for EVERY threshold, 0 (no heavy path) included, and the results of all thresholds equal to
each other.  Models: narrow, odd, wide (tools/modelgen_shapes.py) and logit, two_deep, in3_f32 (tools/modelgen_depths.py):
stage input widths 1, 3, 4, 5, 9, 12 and 32, one to four dense layers a stage.

The hub graph ("hubs", heavy_hub_graph of tests/generic_harness.py): 6 000 vertices, hubs 0 .. 8 of exactly 511, 512, 513, 767,
768, 769, 1 025, 3 000 and 0 entries (around the default threshold, around the chunk sizes of the sums kernel, several chunks,
and an empty row), neighbours and a sparse background drawn among the other vertices only.

The last test is a speed guard: on a power-law graph with four hubs of 65 536 entries the default threshold must not be slower
than threshold 0, which is the code as it was before the heavy path existed."""
import numpy as np
import pytest

from oracle import oracle_py
from tools import modelgen_depths as md
from tests import generic_harness as gh
from tests.generic_harness import HUB_DEGREES, HUB_N, bits, check_scores, crafted_input, degrees, graph_of, ulp
from tests.test_expf_restatement import shim, _run   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)

pytestmark = pytest.mark.gpu

# model -> family
MODELS = {"narrow": "shapes", "odd": "shapes", "wide": "shapes", "logit": "depths", "two_deep": "depths", "in3_f32": "depths"}
THRESHOLDS = [1, 2, 16, 33, 64, 65, 257, 512, 0]
DEFAULT_FROM = 512
GRAPHS = ["hubs", "er3000", "sparse", "hub6k"]   # (tests/generic_harness.py has what each is)


def test_graphs_are_what_the_names_say():
    deg = degrees(graph_of("hubs"))
    assert graph_of("hubs").n == HUB_N
    assert deg[:len(HUB_DEGREES)].tolist() == HUB_DEGREES
    assert deg[len(HUB_DEGREES):].max() < 64, "only the hubs are heavy at the thresholds from 64 on"
    assert (deg >= DEFAULT_FROM).sum() == 7
    assert (degrees(graph_of("sparse")) == 0).mean() > 0.2
    assert degrees(graph_of("er3000")).max() < DEFAULT_FROM
    assert (degrees(graph_of("hub6k")) >= DEFAULT_FROM).sum() == 2


def test_the_default_threshold_is_512():
    import gnn_mwvc_amd as G
    e = G.Engine(gh.text_of("shapes", "narrow"), device=0)
    try:
        assert e.get_info("generic_heavy_from") == DEFAULT_FROM
        assert e.get_info("generic_heavy_rows") == 0 and e.get_info("generic_heavy_last_rows") == 0
        e.set_generic_heavy_rows(0xFFFFFFFF)
        assert e.get_info("generic_heavy_from") == 0xFFFFFFFF
    finally:
        e.close()
    e = G.Engine(G.default_model_text(), device=0)   # no generic stage list in force: stored, does nothing
    try:
        g = graph_of("hubs")
        e.set_generic_heavy_rows(1)
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
        e.forward(g.x())
        assert e.get_info("generic_heavy_from") == 1
        assert e.get_info("generic_heavy_rows") == 0 and e.get_info("generic_heavy_last_rows") == 0
    finally:
        e.close()


# ---------------------------------------------------------------- the threshold sweep: whole forwards

@pytest.mark.parametrize("name", list(MODELS))
def test_every_threshold_gives_the_oracles_bits(shim, name):
    fam = MODELS[name]
    for gname in ("er3000", "hubs"):
        g = graph_of(gname)
        deg = degrees(g)
        wl = gh.want_of(fam, name, gname)[-1][2]
        x = gh.FAMILIES[fam].model_input(name, g)
        e = gh.open_engine(fam, name, g)
        try:
            first = None
            for thr in THRESHOLDS:
                e.set_generic_heavy_rows(thr)
                sc, lg = e.forward(x)
                mism = int((bits(lg) != bits(wl)).sum())
                assert mism == 0, (name, gname, thr, f"{mism}/{lg.size} logits differ", np.argwhere(bits(lg) != bits(wl))[:6].tolist())
                check_scores(shim, sc.reshape(-1), lg.reshape(-1), gh.flat_logits(fam, name, gname), (name, gname, thr))
                if first is None:
                    first = (sc.copy(), lg.copy())
                assert np.array_equal(bits(sc), bits(first[0])) and np.array_equal(bits(lg), bits(first[1])), (name, gname, thr)
                heavy = int((deg >= thr).sum()) if thr else 0
                assert e.get_info("generic_heavy_from") == thr
                assert e.get_info("generic_heavy_last_rows") == heavy, (name, gname, thr)
                assert e.get_info("generic_heavy_rows") == heavy, (name, gname, thr)
                assert e.get_info("generic_heavy_entries") == (int(deg[deg >= thr].sum()) if thr else 0), (name, gname, thr)
                assert e.get_info("generic_stages_active") == 1
            if gname == "er3000":
                e.set_generic_heavy_rows(DEFAULT_FROM)
                e.forward(x)
                assert e.get_info("generic_heavy_last_rows") == 0
        finally:
            e.close()


@pytest.mark.parametrize("name", list(MODELS))
def test_threshold_1_sends_every_non_empty_row_the_heavy_way(shim, name):
    fam = MODELS[name]
    g = graph_of("sparse")
    deg = degrees(g)
    wl = gh.want_of(fam, name, "sparse")[-1][2]
    e = gh.open_engine(fam, name, g, heavy=1)
    try:
        sc, lg = e.forward(gh.FAMILIES[fam].model_input(name, g))
        assert e.get_info("generic_heavy_last_rows") == int((deg > 0).sum()) < g.n
        assert e.get_info("generic_heavy_entries") == g.nnz
        assert np.array_equal(bits(lg), bits(wl)), name
        check_scores(shim, sc.reshape(-1), lg.reshape(-1), gh.flat_logits(fam, name, "sparse"), name)
    finally:
        e.close()


# ---------------------------------------------------------------- the order of a row's additions

@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("thr", [DEFAULT_FROM, 1])
def test_the_sums_are_added_in_stored_order(stage, thr):
    name = "in3_f32"
    g = graph_of("hubs")
    f, _ = md.stage_widths(name)[stage]
    assert f == (3, 32)[stage]
    hin = crafted_input(g.n, f, 100 + stage)
    assert (bits(hin) == 0x80000000).any()
    # on the CPU: hub 7's row summed in reverse order differs from the stored order in at least one column
    hub = 7
    nb = g.col[int(g.rowptr[hub]): int(g.rowptr[hub + 1])].astype(np.int64)
    assert len(nb) == 3000
    fwd = np.zeros(f, dtype=np.float32)
    for v in nb:
        fwd = (fwd + hin[v]).astype(np.float32)
    rev = np.zeros(f, dtype=np.float32)
    for v in nb[::-1]:
        rev = (rev + hin[v]).astype(np.float32)
    assert (bits(fwd) != bits(rev)).any(), "the crafted input does not tell the two orders apart"
    agg = oracle_py.graph_layer(g, g.ws, hin)
    assert np.array_equal(bits(agg[hub, :f]), bits(fwd)), "the oracle adds a row in stored order"
    want_out, want_pre = gh.oracle_stage("depths", name, g, stage, hin)
    e = gh.open_engine("depths", name, g, heavy=thr)
    try:
        gh.run_stage_ranges(e, "depths", name, g, stage, hin, [[(0, g.n)]], want_out, want_pre, (name, "crafted", thr))
        assert e.get_info("generic_heavy_last_rows") == int((degrees(g) >= thr).sum())
    finally:
        e.close()


# ---------------------------------------------------------------- the stage entry over split ranges

@pytest.mark.parametrize("name", list(MODELS))
def test_stage_entry_over_split_ranges(name):
    fam = MODELS[name]
    g = graph_of("hubs")
    n = g.n
    want = gh.want_of(fam, name, "hubs")
    # hubs 0 .. 2 and 6 .. 8 in the first two ranges, hubs 3 .. 5 in the gap between them: heavy rows on both sides of every cut
    first, gap = [(0, 3), (6, n // 2)], [(3, 6), (n // 2, n)]
    for thr in (DEFAULT_FROM, 1):
        e = gh.open_engine(fam, name, g, heavy=thr)
        try:
            assert len(want) == e.num_stages
            for s, (hin, hout, pre) in enumerate(want):
                done = gh.run_stage_ranges(e, fam, name, g, s, hin, [first, gap], hout, pre, (name, "hubs", thr))
                assert done[:n].all() and not done[n]
                assert e.get_info("generic_heavy_last_rows") == int((degrees(g) >= thr).sum())
        finally:
            e.close()


# ---------------------------------------------------------------- slices (gnnvc_attach_graph_slice accepts a generic model)

@pytest.mark.parametrize("name", list(MODELS))
def test_two_slices_compute_the_whole_graph(name):
    import torch
    import gnn_mwvc_amd as G
    from gnn_mwvc_amd import distributed as D
    fam = MODELS[name]
    g = graph_of("hubs")
    n = g.n
    deg = degrees(g)
    want = gh.want_of(fam, name, "hubs")
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(a.astype(np.int64)).to(torch.int32).to(dev)
    rp, col, w, nw = t(g.rowptr), t(g.col), t(g.w), t(g.nw)
    widths = gh.FAMILIES[fam].stage_widths(name)
    outs = [torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev) for _, n_out in widths]
    lgt = torch.full((n + 1, widths[-1][1]), float("nan"), dtype=torch.float32, device=dev)
    for lo, hi in ((0, 5), (5, n)):   # hubs 0 .. 4 in one slice, 5 .. 8 in the other
        sl = D.slice_csr(n, rp, col, w, nw, lo, hi)
        e = G.Engine(gh.text_of(fam, name), device=0)
        try:
            e.set_weight_scale(g.ws)
            torch.cuda.synchronize()
            e.attach_graph_slice(n, lo, hi, sl.nnz, sl.rowptr.data_ptr(), sl.col.data_ptr(), sl.w.data_ptr(), sl.nw.data_ptr(), keepalive=sl)
            assert e.get_info("generic_heavy_rows") == int((deg[lo:hi] >= DEFAULT_FROM).sum()) > 0
            for s, (hin, _, _) in enumerate(want):
                f = widths[s][0]
                tin = torch.zeros((n + 1, f), dtype=torch.float32, device=dev)
                tin[:n] = torch.from_numpy(np.ascontiguousarray(hin, dtype=np.float32).reshape(n, f)).to(dev)
                torch.cuda.synchronize()
                e.stage_forward_device(s, lo, hi, tin.data_ptr(), outs[s].data_ptr(), lgt.data_ptr() if s + 1 == len(want) else 0)
                e.synchronize()
                assert e.get_info("generic_heavy_last_rows") == int((deg[lo:hi] >= DEFAULT_FROM).sum())
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
    g = graph_of("hubs")
    wl = gh.want_of(fam, name, "hubs")[-1][2]
    e = gh.open_engine(fam, name, g)
    try:
        runs = 0
        for thr in (1, DEFAULT_FROM):
            e.set_generic_heavy_rows(thr)
            _, lg = e.forward_audited(gh.FAMILIES[fam].model_input(name, g))   # (raises on a mismatch)
            runs += e.num_stages
            assert e.get_info("generic_heavy_last_rows") == int((degrees(g) >= thr).sum())
            assert e.get_info("audit_runs") == runs and e.get_info("audit_failures") == 0
            assert np.array_equal(bits(lg), bits(wl)), (name, thr)
    finally:
        e.close()


# ---------------------------------------------------------------- lazy classing, and the next graph

def test_a_graph_attached_before_the_option_is_classed_by_the_first_generic_stage():
    name = "two_deep"
    g = graph_of("hubs")
    x = md.model_input(name, g)
    e = gh.open_engine("depths", name, g, opts={"generic_stages": 0})
    try:
        assert not e.fused
        sc0, lg0 = e.forward(x)
        assert e.get_info("generic_stages_active") == 0
        assert e.get_info("generic_heavy_last_rows") == 0 and e.get_info("generic_heavy_rows") == 0
        e.set_option("generic_stages", 1)
        sc1, lg1 = e.forward(x)
        assert e.get_info("generic_stages_active") == 1
        assert e.get_info("generic_heavy_last_rows") == 7 and e.get_info("generic_heavy_rows") == 7
        assert np.array_equal(bits(lg0), bits(lg1)) and np.array_equal(bits(sc0), bits(sc1))
        assert np.array_equal(bits(lg1), bits(gh.want_of("depths", name, "hubs")[-1][2]))
        # the next graphs: their own counts
        for gname, rows in (("hub6k", 2), ("er3000", 0), ("hubs", 7)):
            g2 = graph_of(gname)
            e.set_weight_scale(g2.ws)
            e.upload_graph(g2)
            assert e.get_info("generic_heavy_rows") == rows, gname   # (classed at the hand-off: the generic list is in force)
            _, lg = e.forward(md.model_input(name, g2))
            assert e.get_info("generic_heavy_last_rows") == rows, gname
            assert e.get_info("generic_heavy_entries") == int(degrees(g2)[degrees(g2) >= DEFAULT_FROM].sum()), gname
            assert np.array_equal(bits(lg), bits(gh.want_of("depths", name, gname)[-1][2])), gname
    finally:
        e.close()


# ---------------------------------------------------------------- on <= off

def test_the_heavy_path_is_not_slower_than_without_it_on_four_giant_hubs():
    import torch
    import gnn_mwvc_amd as G
    from tools import graphgen_torch as ggt
    dev = torch.device("cuda", 0)
    g = ggt.power_law_hubs(262_144, 8.0, 2.5, 4, 65_536, 3, dev)
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
            assert e.get_info("generic_heavy_from") == DEFAULT_FROM
            ms_default, lg_on = gh.steady_ms(e, x, sc, lg)
            assert e.get_info("generic_stages_active") == 1 and e.get_info("generic_heavy_last_rows") >= 4
            e.set_generic_heavy_rows(0)
            ms_off, lg_off = gh.steady_ms(e, x, sc, lg)
            assert e.get_info("generic_heavy_last_rows") == 0
            print(f"power-law 262144 / four hubs of 65536, {name}: heavy rows from 512 {ms_default:.3f} ms, off {ms_off:.3f} ms, "
                  f"{ms_off / ms_default:.2f}x")
            assert torch.equal(lg_on.view(torch.int32), lg_off.view(torch.int32)), name
            assert ms_default <= ms_off, f"{name}: heavy rows {ms_default:.3f} ms vs none {ms_off:.3f} ms"
        finally:
            e.close()
    del g, x1, inputs
    torch.cuda.empty_cache()
