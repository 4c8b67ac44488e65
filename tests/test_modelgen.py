"""tools/modelgen.py: the synthetic models are what their names promise — asserted on ORACLE outputs, over the graphs
tests/test_gpu_models.py runs them on (GRAPHS below), never taken from how the weights were put together: ReLU kills random
units.  The GPU tests under these models are worth what these conditions are worth."""
import numpy as np
import pytest

from oracle import oracle_py
from tools import graphgen as gg
from tools import modelgen as mg

# the graphs of tests/test_gpu_models.py's whole forwards, by the plan they engage
GRAPHS = {
    "er1933": lambda: gg.erdos_renyi(1933, 7000, 61),                 # wide tiles
    "er100k": lambda: gg.erdos_renyi(100000, 1000000, 1),             # table tiles
    "er300k": lambda: gg.erdos_renyi(300_000, 1_800_000, 11),         # LDS table + compact gather
    "rmat13": lambda: gg.rmat(13, 8, 3),                              # skewed
    "hub4096": lambda: gg.hub_graph(20000, 60000, 3, 4096, seed=7),   # long and giant rows
}
LINEAR_AT = (1, 3, 5, 8, 10, 12, 15, 17, 19)   # positions of the linear layers among the 21


@pytest.fixture(scope="module")
def graphs():
    return {k: f() for k, f in GRAPHS.items()}


def layer_outputs(om, g, x=None, ws=None):
    """[pre-activation of linear layer i for i in 0 .. 8] through the oracle's own layer functions (ws = g.ws unless given)."""
    h = np.ascontiguousarray(g.x() if x is None else x, dtype=np.float32).reshape(g.n, 1)
    ws = g.ws if ws is None else ws
    pre = []
    for i, (W, b) in enumerate(om.linear_params()):
        if i % 3 == 0:
            h = oracle_py.graph_layer(g, ws, h)
        h = oracle_py.linear_layer(h, W, b)
        pre.append(h)
        if i < 8:
            h = oracle_py.relu(h)
    return pre


@pytest.fixture(scope="module")
def outputs(graphs):
    """{(model, graph): pre-activations}; the walk above is the oracle's predict (checked here on every pair)."""
    out = {}
    for name, make in mg.FAMILY.items():
        om = oracle_py.OracleModel(make())
        assert om.n_layers == 21 and [k for k in range(21) if om.layer_kinds()[k] == 0] == list(LINEAR_AT)
        assert [W.shape for W, _ in om.linear_params()] == mg.SHAPES
        for gname, g in graphs.items():
            om.set_weight_scale(g.ws)
            pre = layer_outputs(om, g)
            assert np.array_equal(pre[8][:, 0].view(np.uint32), om.logits(g).view(np.uint32)), (name, gname)
            out[name, gname] = pre
    return out


def test_text_round_trips_through_the_oracles_parser():
    rng = np.random.default_rng(0)
    layers = [(rng.normal(size=s).astype(np.float32), rng.normal(size=s[1]).astype(np.float32)) for s in mg.SHAPES]
    layers[0][0][0, :4] = np.array([1e-45, -3.4e38, 1.17549435e-38, -0.0], dtype=np.float32)
    om = oracle_py.OracleModel(mg.model_text(layers))
    for (W, b), (W2, b2) in zip(layers, om.linear_params()):
        assert np.array_equal(W.view(np.uint32), W2.view(np.uint32)) and np.array_equal(b.view(np.uint32), b2.view(np.uint32))
    assert mg.FAMILY["dense_1_0.2"]() == mg.FAMILY["dense_1_0.2"]()   # from the seed alone


def test_all_reference_outputs_are_finite(outputs, graphs):
    for (name, gname), pre in outputs.items():
        assert all(np.isfinite(p).all() for p in pre), (name, gname)
        sc = oracle_py.sigmoid(pre[8][:, 0])
        assert np.isfinite(sc).all() and (sc >= 0).all() and (sc <= 1).all(), (name, gname)


def test_every_lane_is_live_somewhere(outputs):
    """Every output unit of every linear layer is non-zero after its ReLU (the logit: at all) for some vertex under some
    model; every h1 and every h2 column under some model."""
    lit = [np.zeros(s[1], dtype=bool) for s in mg.SHAPES]
    for pre in outputs.values():
        for i, p in enumerate(pre):
            lit[i] |= ((p > 0) if i < 8 else (p != 0)).any(axis=0)
    uncovered = [(i, int(u)) for i, l in enumerate(lit) for u in np.flatnonzero(~l)]
    assert uncovered == [], f"(linear layer, unit) never live: {uncovered}"
    # and not by a hair: a dense model alone lights every h1 and h2 column on some graph
    for i in (2, 5):
        d = np.zeros(16, dtype=bool)
        for (name, _), pre in outputs.items():
            if name.startswith("dense"):
                d |= (pre[i] > 0).any(axis=0)
        assert d.all(), (i, np.flatnonzero(~d))


def test_live_sets_are_as_named(outputs, graphs):
    for name, (cols1, cols2) in mg.LIVE_SETS.items():
        for gname in graphs:
            pre = outputs[name, gname]
            for i, cols in ((2, cols1), (5, cols2)):
                got = set(np.flatnonzero((pre[i] > 0).any(axis=0)).tolist())
                assert got and got <= set(cols), (name, gname, i, got)
                if name in ("live_four", "live_five", "live_all"):
                    assert got == set(cols) and len(got) == {"live_four": 4, "live_five": 5, "live_all": 16}[name], (name, gname, i, got)
    # the columns the trained model never lights are lit by the members made for them, all of them
    for gname in graphs:
        assert set(np.flatnonzero((outputs["live_pairs", gname][2] > 0).any(axis=0)).tolist()) == {13, 15}
        assert set(np.flatnonzero((outputs["live_pairs", gname][5] > 0).any(axis=0)).tolist()) == {3, 13}
        assert set(np.flatnonzero((outputs["live_single", gname][2] > 0).any(axis=0)).tolist()) == {15}


def _zero_row_share(g, pre2):
    zero = ~(pre2 > 0).any(axis=1)
    return float(zero[g.col].mean()), zero


@pytest.mark.parametrize("kind", ["heavy", "light", "near_kink"])
def test_zero_rows_carry_mass(outputs, graphs, kind):
    name = f"zero_rows_{kind}"
    shares = {gname: _zero_row_share(graphs[gname], outputs[name, gname][2])[0] for gname in ("rmat13", "hub4096")}
    assert any(0.20 <= s <= 0.90 for s in shares.values()), shares
    g = graphs["rmat13"]
    share, zero = _zero_row_share(g, outputs[name, "rmat13"][2])
    deg = np.diff(g.rowptr.astype(np.int64))
    has = deg > 0
    if kind == "heavy":      # the zero rows are the high degrees ...
        assert zero[deg >= 40].all() and not zero[has & (deg <= 8)].any()
    elif kind == "light":    # ... or the light vertices, at every degree
        assert zero[has & (g.w <= 55)].mean() > 0.95 and zero[has & (g.w >= 80)].mean() < 0.05
        assert abs(np.median(deg[zero & has]) - np.median(deg[~zero & has])) <= 2


def _predicted(om, g):
    """What the hand-off predictor sees (k_predict_zero_f1): stage 0's dense layers on [NW/ws, W/ws, degree, W/ws, NW/ws] —
    NW/ws, the integer sum, for the neighbours' fp32 sum.  Returns (largest last pre-activation, its scale)."""
    x = g.x()
    nw = (g.nw.astype(np.float32) / np.float32(g.ws)).astype(np.float32)
    h = np.stack([nw, x, np.diff(g.rowptr.astype(np.int64)).astype(np.float32), x, nw], axis=1)
    P = om.linear_params()
    h1 = oracle_py.relu(oracle_py.linear_layer(h, *P[0]))
    h2 = oracle_py.relu(oracle_py.linear_layer(h1, *P[1]))
    h3 = oracle_py.linear_layer(h2, *P[2])
    return h3.max(axis=1), np.maximum(np.abs(h3).max(axis=1), h2.max(axis=1))


def test_near_kink_is_near_the_kink(outputs, graphs):
    om = oracle_py.OracleModel(mg.FAMILY["zero_rows_near_kink"]())
    for gname in ("rmat13", "er300k", "hub4096"):
        g = graphs[gname]
        om.set_weight_scale(g.ws)
        pre = outputs["zero_rows_near_kink", gname]
        top = pre[2].max(axis=1)
        scale = np.maximum(np.abs(pre[2]).max(axis=1), np.maximum(pre[1], 0).max(axis=1))
        near = np.abs(top) <= 2e-3 * (1.0 + scale)
        assert near.mean() >= 0.05, (gname, near.mean())
        # the predictor's margin is wrong in both directions: rows that are zero and not in its set, and rows in its set that
        # are not zero (the engine must find that out per call and take the full adjacency)
        ptop, pscale = _predicted(om, g)
        has = np.diff(g.rowptr.astype(np.int64)) > 0
        in_set = has & (ptop <= -1e-3 * (1.0 + pscale))
        zero = ~(pre[2] > 0).any(axis=1)
        assert (zero & has & ~in_set).sum() >= 0.01 * g.n, (gname, int((zero & has & ~in_set).sum()))
        assert in_set.sum() >= 0.01 * g.n
        if gname == "rmat13":   # enough of the entries point into the set for the engine to build it when the graph is handed over
            assert in_set[g.col].mean() >= 0.45, in_set[g.col].mean()
            assert (in_set & ~zero).sum() >= 5, int((in_set & ~zero).sum())   # (the high degrees: their sums round the most)


def test_saturating_covers_the_sigmoids_branches(outputs, graphs):
    for gname, g in graphs.items():
        lg = outputs["saturating_1", gname][8][:, 0]
        assert np.isfinite(lg).all()
        assert lg.min() <= -110 and lg.max() >= 110, (gname, lg.min(), lg.max())
        assert ((lg >= -104) & (lg <= -87)).mean() >= 0.15, gname
        assert ((lg >= 87) & (lg <= 89)).mean() >= 0.10, gname
        sc = oracle_py.sigmoid(lg)
        tiny = np.float32(1.17549435e-38)
        assert ((sc > 0) & (sc < tiny)).sum() >= 20, gname            # denormal results
        assert (sc == 0).any() and (sc == 1).any(), gname               # underflow, saturation
    # random weights of the same shape, for comparison: logits far outside the trained model's few units
    assert max(np.abs(outputs["dense_3_0.35", "rmat13"][8]).max(), np.abs(outputs["dense_4_0.35", "rmat13"][8]).max()) > 100
