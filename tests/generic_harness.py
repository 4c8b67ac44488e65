"""What the tests of the generic fused stage (k_stage_any) share: the comparison rules, the oracle's stage-by-stage walk that every
GPU test takes its expected values from, one cache of texts, graphs and oracle results, the engine opener, the hand-off routes
onto a live engine, the stage-entry loop and the timing loop.  A plain module: tests/test_modelgen_{shapes,depths,big}.py show that the walk here equals the oracle's
predict bit for bit, and so vouch for it in every file that imports it.

A model is named by (family, member): family is "shapes", "depths" or "big" (tools/modelgen_shapes.py, _depths.py, _big.py), and
`too_big` is a member of two of them."""
import time

import numpy as np

from oracle import oracle_py
from tools import giant_rows_inputs as gi
from tools import graphgen as gg
from tools import modelgen_big, modelgen_depths, modelgen_shapes
from tests.test_expf_restatement import _run

FAMILIES = {m.family.prefix: m.family for m in (modelgen_shapes, modelgen_depths, modelgen_big)}

# tools/modelgen_big.py's members -> bytes per stage of stage_any_layout at 16 rows a workgroup (256 threads): the agreed figures that
# tests/test_modelgen_big.py holds the generator's restatement to, and tests/test_gpu_big_stages.py the engine
LDS_BYTES = {
    "too_big": [91008, 97056],
    "h128": [99648, 65568],
    "odd_wide": [50896, 83616],
    "edge": [161488, 4640],
    "over": [176256, 48416],
}

# ---------------------------------------------------------------- comparison rules


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ulp(a, b):
    return np.abs(bits(a).view(np.int32).astype(np.int64) - bits(b).view(np.int32).astype(np.int64))


_cache = {}


def check_scores(shim, scores, logits, want_logits, label):
    """<= 1 ulp from the oracle's scores (the host libm's sigmoid of the oracle's logits), and the restated sigmoid's bits."""
    assert np.array_equal(bits(logits), bits(want_logits)), label
    key = ("sigmoid", id(want_logits))   # (equal logits: one host sigmoid of each kind per reference array, which the entry keeps alive)
    if key not in _cache:
        w = np.ascontiguousarray(want_logits, dtype=np.float32)
        _cache[key] = (want_logits, oracle_py.sigmoid(w), _run(shim.sigmoid_restated, w))
    _, host, restated = _cache[key]
    assert ulp(scores, host).max() <= 1, label
    diff = int((bits(scores) != bits(restated)).sum())
    assert diff == 0, f"{label}: {diff} scores differ from sigmoid_restated(logits)"


# ---------------------------------------------------------------- the oracle's walk

def _walk(om, family, name, g, h, first, count):
    """Stages first .. first + count - 1 from the input rows h, through the oracle's own layer functions (ws = g.ws):
    [(input rows, output rows after the stage's last activation, pre-activation of its last linear layer)]."""
    P = om.linear_params()
    depths = FAMILIES[family].stage_depths(name)
    assert sum(depths) == len(P)
    i = sum(depths[:first])
    out = []
    for d in depths[first: first + count]:
        hin = h
        h = oracle_py.graph_layer(g, g.ws, h)
        for _ in range(d):
            pre = oracle_py.linear_layer(h, *P[i])
            i += 1
            h = oracle_py.sigmoid(pre) if i == len(P) else oracle_py.relu(pre)
        out.append((hin, h, pre))
    return out


def stage_outputs(om, family, name, g, x=None):
    """Per stage: (input rows, output rows after the stage's last activation, pre-activation of its last linear layer).  The last
    stage's output is the scores, its pre-activation the logits."""
    h = FAMILIES[family].model_input(name, g) if x is None else np.ascontiguousarray(x, dtype=np.float32).reshape(g.n, -1)
    return _walk(om, family, name, g, h, 0, len(FAMILIES[family].stage_depths(name)))


def oracle_of(family, name, g):
    om = oracle_py.OracleModel(text_of(family, name))
    om.set_weight_scale(g.ws)
    return om


def oracle_at(family, name, ws):
    """The oracle's model of the member's text at the weight scale ws (oracle_of: at a graph's own)."""
    om = oracle_py.OracleModel(text_of(family, name))
    om.set_weight_scale(ws)
    return om


def logits_at(family, name, g, ws=None, x=None):
    """The oracle's logits (n x out_width) for g from the member's model_input (or x) at the weight scale ws (default: g.ws): the
    oracle's own predict up to the last linear layer — which tests/test_modelgen_{shapes,depths,big}.py show equal to the walk."""
    om = oracle_at(family, name, g.ws if ws is None else ws)
    x = FAMILIES[family].model_input(name, g) if x is None else x
    return om.predict(g, x, stop_after=om.n_layers - 2)


def oracle_stage(family, name, g, s, hin):
    """(output rows, pre-activation of the last linear layer) of stage s alone, from the input rows hin: the walk from stage s."""
    (_, h, pre), = _walk(oracle_of(family, name, g), family, name, g, np.ascontiguousarray(hin, dtype=np.float32), s, 1)
    return h, pre


# ---------------------------------------------------------------- graphs: one registry, a name means one graph in every file

HUB_DEGREES = [511, 512, 513, 767, 768, 769, 1025, 3000, 0]
HUB_N = 6000


def heavy_hub_graph():
    """6 000 vertices, hubs 0 .. 8 of exactly HUB_DEGREES entries, neighbours and a sparse background among the other vertices only."""
    rng = np.random.default_rng(77)
    nh = len(HUB_DEGREES)
    others = np.arange(nh, HUB_N)
    edges = []
    for h, d in enumerate(HUB_DEGREES):
        for v in rng.choice(others, size=d, replace=False):
            edges.append((h, int(v)))
    a = rng.integers(nh, HUB_N, size=9000)
    b = rng.integers(nh, HUB_N, size=9000)
    edges += list(zip(a.tolist(), b.tolist()))
    return gg.from_edge_list(HUB_N, edges, rng.integers(20, 121, size=HUB_N))


GRAPHS = {
    "er3000": lambda: gg.erdos_renyi(3000, 15000, 15),
    "er100k": lambda: gg.erdos_renyi(100000, 1000000, 1),
    "sparse": lambda: gg.erdos_renyi(5000, 3000, 23),                     # about three rows in ten are empty
    "er1933": lambda: gg.erdos_renyi(1933, 7000, 61),                     # n = 30 * 64 + 13: no multiple of 64 or of 16
    "one": lambda: gg.from_edge_list(1, [], [57]),                        # n = 1
    "empty": lambda: gg.from_edge_list(0, [], []),                        # n = 0: what the reference's driver hands over last
    "hub6k": lambda: gg.hub_graph(6000, 18000, 2, 3000, seed=9),          # two rows of 3000 entries: many gather rounds a row
    "hub8k": lambda: gg.hub_graph(8000, 24000, 2, 5000, seed=9),          # rows 0 and 1: about 5000 entries, 78 fetch batches of the audit
    "hub20k": lambda: gg.hub_graph(40000, 120000, 2, 20000, seed=9),      # two rows of 20000 entries (beyond 16384)
    "hubs": heavy_hub_graph,                                              # tests/test_gpu_heavy_rows.py
    "giant_hubs": gi.hub_graph,                                           # tests/test_gpu_giant_rows.py
    "giant_er600": lambda: gg.erdos_renyi(600, 1800, 31),
}


def degrees(g):
    return np.diff(g.rowptr.astype(np.int64))


def heavy_counts(g, thr):
    """(rows, their entries) of g with at least thr entries — what "generic_heavy_rows" / "generic_heavy_entries" read at the
    threshold thr, and "generic_giant_rows" / "generic_giant_entries" at max(heavy, giant) — or (0, 0) for thr = 0 (none)."""
    if not thr or g.n == 0:
        return 0, 0
    deg = degrees(g)
    return int((deg >= thr).sum()), int(deg[deg >= thr].sum())


def crafted_input(n, f, seed):
    """Magnitudes from 2^-20 to 2^20, both signs, some -0.0f: sums whose bits depend on the order of their terms."""
    rng = np.random.default_rng(seed)
    v = np.ldexp(rng.uniform(1.0, 2.0, (n, f)), rng.integers(-20, 21, (n, f))).astype(np.float32)
    v = np.where(rng.random((n, f)) < 0.5, -v, v).astype(np.float32)
    v[rng.random((n, f)) < 0.05] = np.float32(-0.0)
    return np.ascontiguousarray(v, dtype=np.float32)


# ---------------------------------------------------------------- the cache: computed once, never changed

def text_of(family, name):
    if ("text", family, name) not in _cache:
        _cache["text", family, name] = FAMILIES[family].FAMILY[name]()
    return _cache["text", family, name]


def graph_of(gname):
    if ("graph", gname) not in _cache:
        _cache["graph", gname] = GRAPHS[gname]()
    return _cache["graph", gname]


# tests/test_gpu_generic_lifecycle.py's models and graphs, which tests/test_generic_lifecycle_inputs.py pins on the CPU: the members
# handed every route (f = 1, 3, 5, 9 and 32, depths 1 to 5), the graphs one live engine is handed in turn (7 heavy rows, none,
# 7, none ...), and the members whose graph is derived on the device
LIFECYCLE_MEMBERS = [("shapes", "odd"), ("shapes", "in3"), ("depths", "mixed"), ("depths", "in3_f32")]
LIFECYCLE_SEQUENCE = ["hubs", "er1933", "hubs", "one", "empty", "sparse", "hubs"]
DERIVE_MEMBERS = [("shapes", "odd"), ("depths", "mixed")]
DERIVE_STEPS = ((0.7, 50, 40), (0.5, 7, 300), (1.0, 0, 0))   # (share of vertices kept, new fold vertices, their fan)


def derive_chain():
    """[(g1, old_row)] per step of DERIVE_STEPS: "hubs" shrunk three times as the reference's driver shrinks its graph, by
    tests/test_gpu_parity.py's own _shrunk_graph, rng and steps (test_graph_derived_on_the_device_equals_an_upload)."""
    if "chain" not in _cache:
        from tests.test_gpu_parity import _shrunk_graph
        rng = np.random.default_rng(17)
        g, out = graph_of("hubs"), []
        for frac, nv, fan in DERIVE_STEPS:
            g1, old_row = _shrunk_graph(g, rng, frac, nv, fan)
            out.append((g1, old_row))
            g = g1
        _cache["chain"] = out
    return _cache["chain"]


def want_of(family, name, gname):
    """[(stage input, stage output, pre-activation of the stage's last linear layer)] from the oracle's layers."""
    if ("want", family, name, gname) not in _cache:
        g = graph_of(gname)
        _cache["want", family, name, gname] = stage_outputs(oracle_of(family, name, g), family, name, g)
    return _cache["want", family, name, gname]


def flat_logits(family, name, gname):
    key = ("flat", family, name, gname)
    if key not in _cache:
        _cache[key] = np.ascontiguousarray(want_of(family, name, gname)[-1][2].reshape(-1))
    return _cache[key]


# ---------------------------------------------------------------- engines

def open_engine(family, name, g, opts=(), heavy=None, giant=None, big=None, expect_fused=None):
    """An engine on device 0 with the model's text and g uploaded.  The calls come in the order they always came in: the options,
    set_generic_big_stages(big), set_generic_heavy_rows(heavy), the weight scale, the graph, and — after the graph, so that it
    meets rows that are classed already — set_generic_giant_rows(*giant); each setter only where a value is given."""
    import gnn_mwvc_amd as G
    fam = FAMILIES[family]
    e = G.Engine(text_of(family, name), device=0)
    try:
        for k, v in dict(opts).items():
            e.set_option(k, v)
        if big is not None:
            e.set_generic_big_stages(big)
        if heavy is not None:
            e.set_generic_heavy_rows(heavy)
        assert e.num_layers == fam.num_layers(name) and e.in_width == fam.in_width(name) and e.out_width == fam.out_width(name), name
        if expect_fused:
            assert e.fused, name
            assert e.num_stages == len(fam.specs[name][1]), name
            assert [e.stage_widths(s) for s in range(e.num_stages)] == fam.stage_widths(name), name
            assert e.get_info("generic_stages_model") == 1
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
        if giant is not None:
            e.set_generic_giant_rows(*giant)
    except BaseException:
        e.close()
        raise
    return e


ROUTES = ["upload", "staged1", "staged7", "attach"]


def hand_over(e, g, route):
    """Make g the graph of the live engine e, with g's weight scale, by one of ROUTES: gnnvc_upload_graph, the staged hand-off
    with the column array in 1 or 7 pieces, or gnnvc_attach_graph_device on device tensors (which the engine keeps alive).  The
    attached column array carries its GNNVC_COL_PAD tail filled with the valid id n - 1 (0 where the graph has no vertex)."""
    e.set_weight_scale(g.ws)
    if route == "upload":
        e.upload_graph(g)
    elif route in ("staged1", "staged7"):
        e.upload_graph_staged(g, pieces=int(route[len("staged"):]))
    elif route == "attach":
        import torch
        from gnn_mwvc_amd.engine import COL_PAD
        dev = torch.device("cuda:0")
        col = np.full(g.nnz + COL_PAD, max(g.n - 1, 0), dtype=np.int64)
        col[: g.nnz] = g.col
        one = np.zeros(1, dtype=np.int64)   # (no vertex: one word each, never a null pointer)
        arrays = (g.rowptr, col, g.w, g.nw) if g.n else (one, col, one, one)
        t = [torch.from_numpy(np.asarray(a).astype(np.int64)).to(torch.int32).to(dev) for a in arrays]
        torch.cuda.synchronize()
        e.attach_graph_device(g.n, g.nnz, *[x.data_ptr() for x in t], keepalive=t)
    else:
        raise ValueError(route)


def stage_buffers(family, name, gname, s, fill=float("nan")):
    """(device input of stage s from the oracle with a zero pad row, output and logits buffers filled with `fill`, f, n_out)"""
    import torch
    g = graph_of(gname)
    hin = want_of(family, name, gname)[s][0]
    f, n_out = FAMILIES[family].stage_widths(name)[s]
    dev = torch.device("cuda:0")
    tin = torch.zeros((g.n + 1, f), dtype=torch.float32, device=dev)
    tin[: g.n] = torch.from_numpy(np.ascontiguousarray(hin, dtype=np.float32).reshape(g.n, f)).to(dev)
    out = torch.full((g.n + 1, n_out), fill, dtype=torch.float32, device=dev)
    lgt = torch.full((g.n + 1, n_out), fill, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    return tin, out, lgt, f, n_out


def split_ranges(n):
    """(first, gap): row ranges between the cuts 0, n / 5, n / 3, 2 n / 3, n — every other one, and the ones between them."""
    cuts = sorted({0, n // 5, n // 3, (2 * n) // 3, n})
    ranges = list(zip(cuts[:-1], cuts[1:]))
    return (ranges[0::2], ranges[1::2]) if len(ranges) > 1 else (ranges, [])


def run_stage_ranges(e, family, name, g, s, hin, ranges_by_part, want_out, want_pre, label):
    """The stage entry over the ranges of each part in turn, on NaN-filled outputs: after every part the rows done so far are the
    oracle's and every other row (the pad row included) is still NaN."""
    import torch
    dev = torch.device("cuda:0")
    n = g.n
    widths = FAMILIES[family].stage_widths(name)
    f, n_out = widths[s]
    last = s + 1 == len(widths)
    tin = torch.zeros((n + 1, f), dtype=torch.float32, device=dev)
    tin[:n] = torch.from_numpy(np.ascontiguousarray(hin, dtype=np.float32).reshape(n, f)).to(dev)
    out = torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)
    lgt = torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    done = np.zeros(n + 1, dtype=bool)
    for part, todo in enumerate(ranges_by_part):
        for lo, hi in todo:
            e.stage_forward_device(s, lo, hi, tin.data_ptr(), out.data_ptr(), lgt.data_ptr() if last else 0)
            done[lo:hi] = True
        e.synchronize()
        got, gotl = out.cpu().numpy(), lgt.cpu().numpy()
        assert np.isnan(got[~done]).all(), (label, s, part, "rows outside the ranges were written")
        assert np.isnan(gotl[~done]).all() if last else np.isnan(gotl).all(), (label, s, part, "logits rows")
        d = done[:n]
        if last:
            assert np.array_equal(bits(gotl[:n][d]), bits(want_pre[d])), (label, s, part, "stage logits")
            assert ulp(got[:n][d], want_out[d]).max(initial=0) <= 1, (label, s, part, "stage scores")
        else:
            bad = np.argwhere(bits(got[:n][d]) != bits(want_out[d]))
            assert bad.size == 0, (label, s, part, f"{len(bad)} values differ, first (row, column)", bad[:6].tolist())
    return done


# ---------------------------------------------------------------- timing

def steady_ms(e, x, sc, lg):
    """(ms a forward, the logits): two warm-up forwards, then the best of three batches of five, as tests/test_gpu_perf_guard.py."""
    import torch
    for _ in range(2):
        e.forward_device(x.data_ptr(), sc.data_ptr(), lg.data_ptr())
    e.synchronize()
    best = 1e9
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(5):
            e.forward_device(x.data_ptr(), sc.data_ptr(), lg.data_ptr())
        e.synchronize()
        best = min(best, (time.perf_counter() - t) * 200.0)
    return best, lg.clone()


def steady_ms_under_option(family, name, g, x, generic):
    """steady_ms of a fresh engine with "generic_stages" at `generic`, on the device graph g."""
    import torch
    import gnn_mwvc_amd as G
    e = G.Engine(text_of(family, name), device=0)
    try:
        e.set_option("generic_stages", generic)
        e.set_weight_scale(g.ws)
        e.attach_graph_device(g.n, g.nnz, g.rowptr.data_ptr(), g.col.data_ptr(), g.w.data_ptr(), g.nw.data_ptr(), keepalive=g)
        sc = torch.zeros(g.n, device=x.device)
        lg = torch.zeros(g.n, device=x.device)
        torch.cuda.synchronize()
        best, logits = steady_ms(e, x, sc, lg)
        assert e.get_info("generic_stages_active") == (1 if generic else 0)
        return best, logits
    finally:
        e.close()
