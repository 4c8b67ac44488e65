"""What the tests of gnnvc_set_generic_patterns share (tools/modelgen_patterns.py's family): the oracle's stage-by-stage walk for
models with a dense stage in front and with the three endings, one cache of texts and oracle results, and the engine opener.
A plain module; graphs, the comparison rules and the hand-off helpers are tests/generic_harness.py's.
tests/test_modelgen_patterns.py shows that the walk here equals the oracle's predict over all layers bit for bit, and so
vouches for it in every file that imports it."""
import numpy as np

from oracle import oracle_py
from tools import modelgen_patterns as mp
from tests import generic_harness as gh
from tests.generic_harness import bits, graph_of   # noqa: F401

_cache = {}


def text_of(name):
    if ("text", name) not in _cache:
        _cache["text", name] = mp.FAMILY[name]()
    return _cache["text", name]


def oracle_at(name, ws):
    om = oracle_py.OracleModel(text_of(name))
    om.set_weight_scale(ws)
    return om


def predict(om, g, x, stop_after=-1):
    """OracleModel.predict, which sizes its output buffer by the model's widest layer: the name this family's tests call it by."""
    return om.predict(g, np.ascontiguousarray(x, dtype=np.float32).reshape(g.n, -1), stop_after=stop_after)


def walk(om, name, g, ws=None, x=None, first=0, count=None):
    """An admitted member stage by stage through the oracle's own layer functions (weight scale ws, default g.ws):
    [(input rows, output rows, pre-activation of the stage's last linear layer)].  A dense stage has no graph layer; the last
    stage ends in the ReLU, the sigmoid or nothing (the output rows are then the pre-activation)."""
    h = mp.model_input(name, g) if x is None else np.ascontiguousarray(x, dtype=np.float32).reshape(g.n, -1)
    return walk_stages(om, mp.stages_of(name), g, h, ws=ws, first=first, count=count)


def walk_stages(om, stages, g, h, ws=None, first=0, count=None):
    """walk for any stage list [(dense, f, widths, end code)] (tools/modelgen_patterns.stages_of's form), from the input rows h of
    stage `first`: what tests/fuzz_harness.py walks its drawn models with."""
    P = om.linear_params()
    assert sum(len(s[2]) for s in stages) == len(P)
    i = sum(len(s[2]) for s in stages[:first])
    out = []
    for dense, f, widths, end in stages[first: None if count is None else first + count]:
        hin = h
        assert h.shape[1] == f
        if not dense:
            h = oracle_py.graph_layer(g, g.ws if ws is None else ws, h)
        for l in range(len(widths)):
            pre = oracle_py.linear_layer(h, *P[i])
            i += 1
            how = end if l + 1 == len(widths) else mp.END_RELU
            h = oracle_py.relu(pre) if how == mp.END_RELU else oracle_py.sigmoid(pre) if how == mp.END_SIGMOID else pre
        out.append((hin, h, pre))
    return out


def want_of(name, gname):
    """The walk of an admitted member on a registered graph: computed once, never changed."""
    if ("want", name, gname) not in _cache:
        g = graph_of(gname)
        _cache["want", name, gname] = walk(oracle_at(name, g.ws), name, g)
    return _cache["want", name, gname]


def final_of(name, gname):
    """The oracle's predict over all layers (any member, the not-fitting ones included): computed once, never changed."""
    if ("final", name, gname) not in _cache:
        g = graph_of(gname)
        _cache["final", name, gname] = predict(oracle_at(name, g.ws), g, mp.model_input(name, g))
    return _cache["final", name, gname]


def flat_logits(name, gname):
    if ("flat", name, gname) not in _cache:
        _cache["flat", name, gname] = np.ascontiguousarray(want_of(name, gname)[-1][2].reshape(-1))
    return _cache["flat", name, gname]


GOLDEN_GRAPHS = ["ex3", "er4k", "hub2k"]


def golden_h2(gname):
    """(graph, the reference-generated h2 rows) of tests/golden/manifest_layers.json: what `trunc` computes, n x 16."""
    if ("golden", gname) not in _cache:
        import hashlib
        import json
        import pathlib
        from tools import graphgen as gg
        gdir = pathlib.Path(__file__).resolve().parent / "golden"
        spec = json.loads((gdir / "manifest_layers.json").read_text())["graphs"][gname]
        p = spec["graph"]
        g = (gg.from_edge_list(p["n"], p["edges"], p["weights"]) if p["kind"] == "edge_list" else
             gg.erdos_renyi(p["n"], p["m"], p["seed"]) if p["kind"] == "erdos_renyi" else
             gg.hub_graph(p["n"], p["m"], p["hubs"], p["hub_degree"], seed=p["seed"]))
        assert gg.metis_md5(g) == spec["metis_md5"] and g.ws == spec["ws"]
        f = spec["files"]["h2"]
        raw = (gdir / f["file"]).read_bytes()
        assert hashlib.md5(raw).hexdigest() == f["md5"] and f["after_layer_index"] == 13
        _cache["golden", gname] = (g, np.frombuffer(raw, dtype=np.float32).reshape(f["shape"]).copy())
    return _cache["golden", gname]


def ends_in_sigmoid(name):
    return mp.sequence(name).split()[-1] == "S"


def open_engine(name, g, mask=None, width=None, big=None, heavy=None, giant=None, opts=()):
    """An engine on device 0 with the member's text; options, big stages and the heavy threshold before the graph, then the
    graph at its weight scale, then — as a caller who switches them on under a resident graph — the giant threshold, the
    feature width and the mask, each only where a value is given."""
    import gnn_mwvc_amd as G
    e = G.Engine(text_of(name), device=0)
    try:
        for k, v in dict(opts).items():
            e.set_option(k, v)
        if big is not None:
            e.set_generic_big_stages(big)
        if heavy is not None:
            e.set_generic_heavy_rows(heavy)
        assert e.num_layers == mp.num_layers(name) and e.in_width == mp.in_width(name) and e.out_width == mp.out_width(name), name
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
        if giant is not None:
            e.set_generic_giant_rows(*giant)
        if width is not None:
            e.set_generic_feature_width(width)
        if mask is not None:
            e.set_generic_patterns(mask)
    except BaseException:
        e.close()
        raise
    return e


def open_fused(name, g, **kw):
    """open_engine with the member's own mask and, where the table says so, its other opt-in."""
    return open_engine(name, g, mask=mp.MASK[name], width=64 if name in mp.NEEDS_FEAT else None,
                       big=mp.FULL_LDS if name in mp.NEEDS_BIG else None, **kw)


def assert_layer_by_layer(e):
    assert not e.fused and e.num_stages == 0 and e.get_info("generic_stages_model") == 0


def assert_fused_as_specified(e, name, lds_bytes):
    ns = len(mp.stages_of(name))
    assert e.fused and e.num_stages == ns and e.get_info("generic_stages_model") == 1, name
    rd = lambda key: [e.get_info(f"{key}_{s}") for s in range(ns)]
    assert [e.stage_widths(s) for s in range(ns)] == mp.stage_widths(name), name
    assert rd("generic_stage_layers") == mp.stage_depths(name), name
    assert rd("generic_stage_dense") == mp.stage_dense(name), name
    assert rd("generic_stage_end") == mp.stage_ends(name), name
    assert rd("generic_stage_lds_bytes") == lds_bytes[name], name
    assert rd("generic_stage_threads") == mp.stage_threads(name, mp.FULL_LDS), name


def assert_oracle_forward(shim, e, name, gname, label):
    """gnnvc_forward against the oracle: the outputs bit for bit — a sigmoid member's logits bit for bit and its scores by
    generic_harness.check_scores.  Returns the outputs."""
    g = graph_of(gname)
    x = mp.model_input(name, g)
    if ends_in_sigmoid(name):
        sc, lg = e.forward(x)
        want = want_of(name, gname)[-1][2] if name in mp.SPECS else predict(oracle_at(name, g.ws), g, x, stop_after=mp.num_layers(name) - 2)
        assert sc.shape == lg.shape == (g.n, mp.out_width(name))
        if name not in mp.SPECS:
            _cache.setdefault(("oddlogits", name, gname), np.ascontiguousarray(want.reshape(-1)))
        flat = flat_logits(name, gname) if name in mp.SPECS else _cache["oddlogits", name, gname]
        assert np.array_equal(bits(lg), bits(want)), (name, gname, label, "logits")
        gh.check_scores(shim, sc.reshape(-1), lg.reshape(-1), flat, (name, gname, label))
        return lg
    out, _ = e.forward(x, want_logits=False)
    want = final_of(name, gname)
    assert out.shape == want.shape == (g.n, mp.out_width(name))
    bad = np.argwhere(bits(out) != bits(want))
    assert bad.size == 0, (name, gname, label, f"{len(bad)} values differ, first (row, column)", bad[:6].tolist())
    return out
