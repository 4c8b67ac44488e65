"""The fused stages under weights other than the one trained model (tools/modelgen.py's family; tests/test_modelgen.py shows
on the oracle what each member lights).  The trained weights leave a third of the dense layers' output lanes, six h1 columns
and eleven h2 columns at zero for every vertex; under these models every lane and column carries values somewhere, rows are
zero for light vertices as well as heavy ones, the zero-row prediction meets rows at the kink, and the logits reach every
branch of the sigmoid.

Bars, as in the rest of the GPU suite and no wider: logits, h1 and h2 bit for bit against the oracle, pad rows untouched,
scores within 1 ulp of the oracle's — and bit for bit against the host build of csrc/expf_glibc.h (sigmoid_restated)."""
import numpy as np
import pytest

from oracle import oracle_py
from tools import graphgen as gg
from tools import modelgen as mg
from tests.test_expf_restatement import shim, _run   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)
from tests.generic_harness import bits, check_scores, ulp   # noqa: F401  (defined there; the trained-shape tests read them here)
from tests.test_gpu_fuzz import _graph, _options
from tests.test_modelgen import GRAPHS, _predicted, layer_outputs

pytestmark = pytest.mark.gpu

MODELS = list(mg.FAMILY)
DENSE = [m for m in MODELS if m.startswith("dense")]
# er300k with the plans at hand-off, as tests/test_gpu_audit.py engages them
PLANNED = {"blocked_min_n": 0, "compact_min_n": 0, "plans_at_handoff": 2}
# the zero-row prediction at hand-off, as test_predicted_pruned_adjacency_is_bit_identical engages it
PREDICT = {"blocked_min_n": 0, "long_row_threshold": 256, "sorted_long_row_threshold": 512, "giant_row_threshold": 4096,
           "prune_min_entries": 0, "prune_predict_min_entries": 0, "filter_min_long_percent": 0, "prune_min_drop_percent": 1}


_cache = {}


def text_of(name):
    if ("text", name) not in _cache:
        _cache["text", name] = mg.FAMILY[name]()
    return _cache["text", name]


def graph_of(gname):
    if ("graph", gname) not in _cache:
        _cache["graph", gname] = dict(GRAPHS, er3000=lambda: gg.erdos_renyi(3000, 15000, 15))[gname]()
    return _cache["graph", gname]


def oracle_of(name):
    if ("oracle", name) not in _cache:
        _cache["oracle", name] = oracle_py.OracleModel(text_of(name))
    return _cache["oracle", name]


def other_input(g):
    return (g.x() * np.float32(0.37)).astype(np.float32)


def want_of(name, gname, what="logits", scale=1):
    """The oracle's logits (for g.x(), or "other": the other input), "h1" or "h2" of a family member on a named graph, computed
    once: one walk through the oracle's layers gives all three (tests/test_modelgen.py checks that walk against predict).
    scale: the weight scale is scale * g.ws instead of the driver's g.ws, the inputs stay the same (tests/flip_harness.py)."""
    at = () if scale == 1 else (scale,)
    if ("want", name, gname, what) + at not in _cache:
        g, om = graph_of(gname), oracle_of(name)
        ws = float(np.float32(g.ws * scale))
        om.set_weight_scale(ws)
        if what == "other":
            _cache[("want", name, gname, what) + at] = om.logits(g, other_input(g))
        else:
            pre = layer_outputs(om, g, ws=ws)
            for k, v in (("h1", oracle_py.relu(pre[2])), ("h2", oracle_py.relu(pre[5])), ("logits", pre[8][:, 0].copy())):
                _cache[("want", name, gname, k) + at] = v
        om.set_weight_scale(g.ws)
    return _cache[("want", name, gname, what) + at]


def open_engine(name, g, opts=(), devices=None):
    import gnn_mwvc_amd as G
    e = G.Engine(text_of(name), devices=devices) if devices else G.Engine(text_of(name), device=0)
    try:
        assert e.fused and e.num_stages == 3 and e.num_layers == 21, name
        for k, v in dict(opts).items():
            e.set_option(k, v)
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
    except BaseException:
        e.close()
        raise
    return e


def forwards(e, shim, name, gname, reps=5, label=()):
    """`reps` forwards (plans settle over forwards), the other input, the first again: logits bit for bit, scores as above."""
    g = graph_of(gname)
    want = want_of(name, gname)
    for rep in range(reps):
        sc, lg = e.forward(g.x())
        mism = int((bits(lg[:, 0]) != bits(want)).sum())
        assert mism == 0, (name, gname, rep, label, f"{mism}/{g.n} logits differ", np.flatnonzero(bits(lg[:, 0]) != bits(want))[:8])
        check_scores(shim, sc[:, 0], lg[:, 0], want, (name, gname, rep, label))
    w2 = want_of(name, gname, "other")
    sc, lg = e.forward(other_input(g))
    assert np.array_equal(bits(lg[:, 0]), bits(w2)), (name, gname, "other input", label)
    check_scores(shim, sc[:, 0], lg[:, 0], w2, (name, gname, "other input", label))
    sc, lg = e.forward(g.x())
    assert np.array_equal(bits(lg[:, 0]), bits(want)), (name, gname, "back", label)


def stages_on_device(e, name, gname, cuts=None, check_masks=True):
    """h1, h2 and the logits through the stage entry point over the row ranges between `cuts`, each stage fed the ORACLE's
    input: bit for bit, pad rows untouched; the exchange codec's live-column masks are the oracle's."""
    import torch
    g = graph_of(gname)
    dev = torch.device("cuda:0")
    cuts = [0, g.n] if cuts is None else cuts
    want = {1: want_of(name, gname, "h1"), 2: want_of(name, gname, "h2")}
    x = torch.from_numpy(g.x()).to(dev)
    ins = {0: x}
    for st in (1, 2):
        t = torch.zeros((g.n + 1, 16), dtype=torch.float32, device=dev)
        t[: g.n] = torch.from_numpy(np.ascontiguousarray(want[st])).to(dev)
        ins[st] = t
    for st in (0, 1, 2):
        out = torch.full((g.n + 1, 16 if st < 2 else 1), 7.0, dtype=torch.float32, device=dev)
        lg = torch.full((g.n + 1,), 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            e.stage_forward_device(st, lo, hi, ins[st].data_ptr(), out.data_ptr(), lg.data_ptr() if st == 2 else 0)
        e.synchronize()
        if st < 2:
            got = out.cpu().numpy()
            bad = np.argwhere(bits(got[: g.n]) != bits(want[st + 1]))
            assert bad.size == 0, (name, gname, f"h{st + 1}", f"{len(bad)} values differ, first (row, column)", bad[:6].tolist())
            assert np.array_equal(bits(got[g.n]), bits(np.full(16, 7.0, dtype=np.float32))), (name, gname, st, "pad row written")
            if check_masks:
                mask = sum(1 << c for c in range(16) if np.any(want[st + 1][:, c] != 0))
                assert e.live_columns(out.data_ptr(), g.n) == mask, (name, gname, st)
        else:
            assert np.array_equal(bits(lg[: g.n].cpu().numpy()), bits(want_of(name, gname))), (name, gname, "stage 2 logits")
            assert float(lg[g.n]) == 7.0
    return ins


# ---------------------------------------------------------------- 3a: whole forwards on graphs that engage each plan

@pytest.mark.parametrize("gname", list(GRAPHS))
@pytest.mark.parametrize("name", MODELS)
def test_whole_forwards(shim, name, gname):
    g = graph_of(gname)
    e = open_engine(name, g, {"poison_features": 1})
    try:
        forwards(e, shim, name, gname)
        stages_on_device(e, name, gname)
        if gname == "er1933":
            assert e.get_info("wide_tiles_used") == 1
        if gname == "hub4096":
            assert e.get_info("long_rows") > 0   # (the hubs; giant rows: test_long_and_giant_rows)
    finally:
        e.close()


# ---------------------------------------------------------------- 3b: every plan takes effect under a non-trained model

@pytest.mark.parametrize("name,fits", [("live_four", True), ("live_pairs", True), ("live_single", True),
                                       ("live_five", False), ("dense_1_0.2", False), ("dense_3_0.35", False)])
def test_table_tiles_fit_by_live_columns(shim, name, fits):
    """ER-100K: the 16-wide stages gather from the four-column table when their inputs have at most four live columns (written
    by the producer for columns the trained model never lights); with five, or all sixteen, the tiles miss and are withdrawn."""
    g = graph_of("er100k")
    e = open_engine(name, g, {"poison_features": 1})
    try:
        assert e.get_info("table_tiles_active") == 1 and e.get_info("compact_gather_active") == 0
        want, seen = want_of(name, "er100k"), []
        for rep in range(8):
            _, lg = e.forward(g.x())
            assert np.array_equal(bits(lg[:, 0]), bits(want)), (name, rep)
            seen.append((e.get_info("table_tiles_fit_stage1"), e.get_info("table_tiles_fit_stage2")))
        if fits:
            assert seen[0] == (0, 0) and seen[3] == (1, 1) and seen[-1] == (1, 1), (name, seen)
        else:
            assert all(f == (0, 0) for f in seen), (name, seen)
            assert e.get_info("table_tiles_active") == 0, name
        forwards(e, shim, name, "er100k", reps=1, label="after the tiles settled")
    finally:
        e.close()


@pytest.mark.parametrize("name,fits", [("live_four", True), ("live_pairs", True), ("live_single", True),
                                       ("live_five", False), ("dense_2_0.2", False)])
def test_lds_table_and_compact_gather_by_live_columns(shim, name, fits):
    """ER-300K with the plans built at hand-off: the LDS table serves stage 0 under every model; the compact gather serves the
    16-wide stages when their inputs have at most four live columns, and steps aside for good otherwise."""
    g = graph_of("er300k")
    e = open_engine(name, g, dict(PLANNED, poison_features=1))
    try:
        assert e.get_info("lds_table_active") == 1 and e.get_info("compact_gather_active") == 1, name
        want, off = want_of(name, "er300k"), []
        for rep in range(10):
            _, lg = e.forward(g.x())
            assert np.array_equal(bits(lg[:, 0]), bits(want)), (name, rep)
            off.append((e.get_info("compact_gather_off_stage1"), e.get_info("compact_gather_off_stage2")))
        assert e.get_info("lds_table_last_ok") == 1, name
        if fits:
            assert e.get_info("compact_gather_last_ok") == 1 and off[-1] == (0, 0), (name, off)
        else:   # (as in test_compact_gather_plan_steps_aside_for_good: not before three verdicts, then at least one stage gives up)
            assert off[2] == (0, 0) and off[-1] != (0, 0) and e.get_info("compact_gather_last_ok") == 0, (name, off)
        forwards(e, shim, name, "er300k", reps=1, label="after the plans settled")
    finally:
        e.close()


@pytest.mark.parametrize("name", ["dense_1_0.2", "dense_3_0.35", "live_four", "zero_rows_light", "saturating_1"])
def test_long_and_giant_rows(shim, name):
    """The hubs as giant rows (streamed, then k_giant_dense) and every row of eight entries or more on the long-row path."""
    g = graph_of("hub4096")
    e = open_engine(name, g, {"long_row_threshold": 8, "giant_row_threshold": 1000, "poison_features": 1})
    try:
        assert e.get_info("giant_rows") == 3 and e.get_info("long_rows") > 0
        forwards(e, shim, name, "hub4096", reps=3, label="giant")
        stages_on_device(e, name, "hub4096")
    finally:
        e.close()


@pytest.mark.parametrize("kind", ["heavy", "light"])
def test_zero_row_prediction_holds(shim, kind):
    """R-MAT at hand-off: the set of zero rows predicted from the graph's own weights — heavy vertices, or light ones at every
    degree — is built, proved on the device for the driver's input and used."""
    name, g = f"zero_rows_{kind}", graph_of("rmat13")
    e = open_engine(name, g, dict(PREDICT, poison_features=1))
    try:
        assert e.get_info("pruned_predicted_stage1") == 1, name
        _, lg = e.forward(g.x())
        assert np.array_equal(bits(lg[:, 0]), bits(want_of(name, "rmat13"))), name
        assert e.get_info("pruned_last_ok_stage1") == 1, name
        # the entries kept are the ones that point outside the predicted set (worked out here on the oracle's layers; a vertex
        # within rounding of the margin may fall on either side: a thousandth of the entries is allowed for those)
        om = oracle_of(name)
        om.set_weight_scale(g.ws)
        ptop, pscale = _predicted(om, g)
        in_set = (np.diff(g.rowptr.astype(np.int64)) > 0) & (ptop <= -1e-3 * (1.0 + pscale))
        zero = ~(want_of(name, "rmat13", "h1") != 0).any(axis=1)
        assert not (in_set & ~zero).any()
        kept, expected = e.get_info("pruned_entries_stage1"), int((~in_set[g.col]).sum())
        print(f"{name}: {kept} of {g.nnz} entries kept, {expected} expected")
        assert expected <= 0.8 * g.nnz and abs(kept - expected) <= g.nnz // 1000, (kept, expected, g.nnz)
        assert kept >= int((~zero[g.col]).sum())                # never without an entry that points to a non-zero row
        forwards(e, shim, name, "rmat13", label="predicted")
        stages_on_device(e, name, "rmat13", check_masks=False)
    finally:
        e.close()


@pytest.mark.parametrize("gname", ["rmat13", "er300k"])
def test_zero_row_prediction_at_the_kink(shim, gname):
    """near_kink: rows the predictor's margin puts in the set are not zero (the rounding of the neighbour sum, which it cannot
    see, lifts them over the kink) and rows outside it are.  A wrong prediction costs time, never a bit: the forward is the
    oracle's whatever the device's check says."""
    name, g = "zero_rows_near_kink", graph_of(gname)
    e = open_engine(name, g, dict(PREDICT, poison_features=1))
    try:
        predicted = e.get_info("pruned_predicted_stage1")
        if gname == "rmat13":   # (tests/test_modelgen.py: 45 % of the entries or more point into the predicted set)
            assert predicted == 1
        _, lg = e.forward(g.x())
        assert np.array_equal(bits(lg[:, 0]), bits(want_of(name, gname))), (gname, predicted)
        if predicted:   # (tests/test_modelgen.py: the set holds rows that are not zero on these graphs) the check must refuse it
            assert e.get_info("pruned_last_ok_stage1") == 0, gname
        forwards(e, shim, name, gname, label=("kink", predicted))
        stages_on_device(e, name, gname, check_masks=False)
    finally:
        e.close()


# ---------------------------------------------------------------- 3c: MFMA against VALU

@pytest.mark.parametrize("mfma", [0, 1, 2])
@pytest.mark.parametrize("name", ["dense_1_0.2", "dense_4_0.35", "live_five", "saturating_1"])
def test_dense_layers_mfma_and_valu_are_bit_identical(shim, name, mfma):
    """Every output lane of every dense layer carries values under these models: the MFMA register layouts, the lane swap
    and the VALU chains against the oracle's fma chains."""
    om = oracle_of(name)
    rng = np.random.default_rng(5)
    graphs = (gg.erdos_renyi(10000, 80000, 51), gg.rmat(11, 16, 6),
              gg.from_edge_list(65, [(i, i + 1) for i in range(64)], list(range(20, 85))))
    e = open_engine(name, graphs[0], {"mfma_dense": mfma, "poison_features": 1})
    try:
        assert e.get_info("mfma_dense") == mfma
        for g in graphs:
            e.set_weight_scale(g.ws)
            om.set_weight_scale(g.ws)
            e.upload_graph(g)
            for x in (g.x(), rng.uniform(0.0, 1.5, g.n).astype(np.float32)):
                want = om.logits(g, x)
                assert np.isfinite(want).all()
                for rep in range(2):
                    sc, lg = e.forward(x)
                    assert np.array_equal(bits(lg[:, 0]), bits(want)), (name, mfma, g.n, rep)
                    check_scores(shim, sc[:, 0], lg[:, 0], want, (name, mfma, g.n))
    finally:
        e.close()


# ---------------------------------------------------------------- 3d: a slice of the plan fuzz under other weights

@pytest.mark.parametrize("block", range(4))
def test_random_graphs_and_plan_options_under_other_weights(block):
    for case in range(block * 6, block * 6 + 6):
        rng = np.random.default_rng(95_000 + case)
        g, opts = _graph(rng), _options(rng)
        name = MODELS[int(rng.integers(len(MODELS)))]
        om = oracle_of(name)
        om.set_weight_scale(g.ws)
        want = om.logits(g)
        e = open_engine(name, g, opts)
        try:
            for rep in range(5):
                _, lg = e.forward(g.x())
                assert np.array_equal(bits(lg[:, 0]), bits(want)), (case, name, rep, g.n, g.nnz, opts)
            x2 = other_input(g)
            _, lg = e.forward(x2)
            assert np.array_equal(bits(lg[:, 0]), bits(om.logits(g, x2))), (case, name, "other input", g.n, g.nnz, opts)
            _, lg = e.forward(g.x())
            assert np.array_equal(bits(lg[:, 0]), bits(want)), (case, name, "back", g.n, g.nnz, opts)
        finally:
            e.close()


# ---------------------------------------------------------------- 3e: sub-ranges, slices, several devices

SPLIT = ["dense_3_0.35", "live_pairs"]


@pytest.mark.parametrize("name", SPLIT)
def test_stage_entry_point_over_row_ranges(name):
    g = graph_of("er3000")
    e = open_engine(name, g)
    try:
        stages_on_device(e, name, "er3000", cuts=[0, 1, 64, 1000, 1777, g.n])
    finally:
        e.close()


@pytest.mark.parametrize("name", SPLIT)
def test_sliced_engines_equal_the_whole_graph(shim, name):
    """Two engines, each holding its rows' CSR slice, driven stage by stage in two pieces on shared buffers (hub4096: long and
    giant rows inside the slices)."""
    import gnn_mwvc_amd as G
    import torch
    from gnn_mwvc_amd import distributed as D
    g = graph_of("hub4096")
    dev = torch.device("cuda:0")
    bounds = D.partition_bounds(g.n, 2, g.rowptr, "nnz")
    t = lambda v: torch.from_numpy(v.astype(np.int64)).to(torch.int32).to(dev)
    rp, col, w, nw = t(g.rowptr), t(g.col), t(g.w), t(g.nw)
    engines = []
    try:
        for lo, hi in bounds:
            e = G.Engine(text_of(name), device=0)
            engines.append(e)
            assert e.fused and e.num_stages == 3 and e.num_layers == 21
            for k, v in (("long_row_threshold", 64), ("giant_row_threshold", 3000), ("prune_min_entries", 0), ("prune_min_drop_percent", 1)):
                e.set_option(k, v)
            e.set_weight_scale(g.ws)
            sl = D.slice_csr(g.n, rp, col, w, nw, lo, hi)
            torch.cuda.synchronize()
            e.attach_graph_slice(g.n, lo, hi, sl.nnz, sl.rowptr.data_ptr(), sl.col.data_ptr(), sl.w.data_ptr(), sl.nw.data_ptr(),
                                 keepalive=sl)
        x = torch.from_numpy(g.x()).to(dev)
        h1 = torch.zeros((g.n + 1, 16), dtype=torch.float32, device=dev)
        h2 = torch.zeros((g.n + 1, 16), dtype=torch.float32, device=dev)
        sc = torch.zeros(g.n, dtype=torch.float32, device=dev)
        lg = torch.zeros(g.n, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for rep in range(3):
            if rep:
                for b in (h1, h2, sc, lg):
                    b.fill_(7.0)
                h1[g.n] = 0.0
                h2[g.n] = 0.0
                torch.cuda.synchronize()
            for st, (src, dst, lgt) in enumerate(((x, h1, None), (h1, h2, None), (h2, sc, lg))):
                for e, (lo, hi) in zip(engines, bounds):
                    mid = lo + ((hi - lo) // 2) // 64 * 64
                    for r0, r1 in ((lo, mid), (mid, hi)):
                        e.stage_forward_device(st, r0, r1, src.data_ptr(), dst.data_ptr(), lgt.data_ptr() if lgt is not None else 0)
                for e in engines:
                    e.synchronize()
            assert np.array_equal(bits(h1[: g.n].cpu().numpy()), bits(want_of(name, "hub4096", "h1"))), (name, rep)
            assert np.array_equal(bits(h2[: g.n].cpu().numpy()), bits(want_of(name, "hub4096", "h2"))), (name, rep)
            assert np.array_equal(bits(lg.cpu().numpy()), bits(want_of(name, "hub4096"))), (name, rep)
            check_scores(shim, sc.cpu().numpy(), lg.cpu().numpy(), want_of(name, "hub4096"), (name, rep))
            assert float(h1[g.n].abs().sum()) == 0.0 and float(h2[g.n].abs().sum()) == 0.0
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("name", SPLIT + ["live_all"])
def test_multi_device_handle_equals_single_engine(shim, name):
    """Three parts behind one handle (all on device 0): rows travel between the parts packed to their live columns — with all
    sixteen live (live_all: ReLU leaves no uniform model all sixteen, tests/test_modelgen.py) the rows travel whole."""
    g = graph_of("hub4096")
    want = want_of(name, "hub4096")
    e = open_engine(name, g, devices=[0, 0, 0])
    try:
        assert e.get_info("devices") == 3
        for rep in range(3):
            sc, lg = e.forward(g.x())
            assert np.array_equal(bits(lg[:, 0]), bits(want)), (name, rep)
            check_scores(shim, sc[:, 0], lg[:, 0], want, (name, rep))
        live = [int((want_of(name, "hub4096", h) != 0).any(axis=0).sum()) for h in ("h1", "h2")]
        cols = [e.get_info("multi_packed_columns_stage0"), e.get_info("multi_packed_columns_stage1")]
        print(f"{name}: live columns {live}, columns shipped {cols}")
        if name == "live_all":
            assert live == [16, 16] and cols == [16, 16], (live, cols)
        _, lg2 = e.forward(other_input(g))
        assert np.array_equal(bits(lg2[:, 0]), bits(want_of(name, "hub4096", "other"))), name
    finally:
        e.close()
    single = open_engine(name, g)
    try:
        sc1, lg1 = single.forward(g.x())
        assert np.array_equal(bits(lg1), bits(lg)) and np.array_equal(bits(sc1), bits(sc)), name
    finally:
        single.close()


# ---------------------------------------------------------------- 3f: the on-device audit agrees

@pytest.mark.parametrize("gname,opts", [("er300k", PLANNED), ("hub4096", {})])
@pytest.mark.parametrize("name", ["dense_2_0.2", "live_four"])
def test_on_device_audit_agrees(name, gname, opts):
    g = graph_of(gname)
    e = open_engine(name, g, dict(opts, audit_period=1))
    try:
        for rep in range(4):
            _, lg = e.forward(g.x())
            assert np.array_equal(bits(lg[:, 0]), bits(want_of(name, gname))), (name, gname, rep)
        r = e.audit_report()
        assert r["audit_runs"] == 4 * e.num_stages and r["audit_failures"] == 0 and r["audit_nan_pairs"] == 0, (name, gname, r)
    finally:
        e.close()


# ---------------------------------------------------------------- 3g: sigmoid bits

@pytest.mark.parametrize("name", ["saturating_1", "dense_3_0.35", "dense_4_0.35"])
def test_fused_sigmoid_bits(shim, name):
    """The last stage's fused sigmoid on logits far outside the trained model's few units: saturated, overflowing,
    underflowing, denormal results — the restated expf's bits."""
    g = graph_of("rmat13")
    want = want_of(name, "rmat13")
    e = open_engine(name, g)
    try:
        sc, lg = e.forward(g.x())
        assert np.array_equal(bits(lg[:, 0]), bits(want))
        assert np.array_equal(bits(sc[:, 0]), bits(_run(shim.sigmoid_restated, np.ascontiguousarray(lg[:, 0]))))
        assert ulp(sc[:, 0], oracle_py.sigmoid(want)).max() <= 1
        if name == "saturating_1":
            s = sc[:, 0]
            assert (s == 0).any() and (s == 1).any() and ((s > 0) & (s < np.float32(1.17549435e-38))).any()
        else:
            assert np.abs(want).max() > 100
    finally:
        e.close()


def test_sigmoid_entry_point_bits(shim):
    import gnn_mwvc_amd as G
    rng = np.random.default_rng(7)
    parts = [rng.uniform(-110, 110, 2_000_000).astype(np.float32)]
    for c in (88.72284, -87.33655, -103.97208):
        base = int(np.float32(c).view(np.uint32))
        parts.append(np.arange(base - 4096, base + 4097, dtype=np.uint32).view(np.float32))
    parts.append(np.arange(0, 4097, dtype=np.uint32).view(np.float32))                            # +0 and the 4096 floats above it
    parts.append((np.arange(0, 4097, dtype=np.uint32) | np.uint32(0x80000000)).view(np.float32))  # -0 and the 4096 below
    parts.append(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3.4e38, -3.4e38], dtype=np.float32))
    x = np.concatenate(parts)
    e = G.Engine(text_of("dense_1_0.2"), device=0)
    try:
        got = e.sigmoid(x)
    finally:
        e.close()
    want = _run(shim.sigmoid_restated, x)
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), f"{int((~same).sum())} of {x.size} differ, e.g. x = {x[~same][:6]}, got {got[~same][:6]}, want {want[~same][:6]}"
    assert np.isnan(got).sum() == 1
