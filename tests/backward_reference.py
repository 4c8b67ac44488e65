"""The CPU reference of the backward pass (include/gnnvc.h "backward") and the case table its tests share.

Assembled from the oracle alone: activations from the oracle's layer functions, each layer run from the one before (bit for bit
oracle_py.OracleModel.predict(stop_after=...), which tests/test_backward_reference.py asserts), products from oracle_py.sgemm (one
k-ordered fmaf chain per output; per block of GRAD_BLOCK_ROWS rows for grad_W), neighbour sums from oracle_py.graph_layer on
grad[:, :f], everything else float32 numpy, one rounded operation at a time.  tests/test_backward_reference.py holds it to float64
autograd; tests/test_gpu_backward.py and tests/test_gpu_backward_shapes.py hold the engine to it bit for bit.  A plain module:
nothing here touches a GPU.
"""
import numpy as np

from oracle import oracle_py
from tests import generic_harness as H
from tools import graphgen as gg
from tools import modelgen_big, modelgen_feat, modelgen_patterns

GRAD_BLOCK_ROWS = 4096   # GNNVC_GRAD_BLOCK_ROWS
LINEAR, GRAPH, RELU, SIGMOID = 0, 1, 2, 3   # OracleModel.layer_kinds()
F32 = np.float32

# ---------------------------------------------------------------- the case table

# (n, k, m) of the layer-level linear_backward: one row; one row under, at and over a block; two blocks and a bit with one output
# column; the widest layer the parser's models reach; one input and one output column
LINEAR_SHAPES = [(1, 5, 32), (4095, 35, 32), (4096, 35, 32), (4097, 35, 32), (8209, 32, 1), (4097, 131, 128), (4097, 1, 1)]
GRAPH_LAYER_F = [1, 2, 3, 4, 5, 16, 17, 33, 64]
GRAPH_LAYER_GRAPHS = ["er1933", "sparse", "one", "hub8k"]

GRAPHS = {
    "er4097": lambda: gg.erdos_renyi(4097, 16000, 41),     # one row over a block of the parameter gradients
    "er8209": lambda: gg.erdos_renyi(8209, 33000, 43),     # two blocks and seventeen rows
}
MODEL_GRAPHS = ["one", "empty", "er1933", "hub8k", "er4097", "er8209"]


def _trained_text():
    import pathlib
    return (pathlib.Path(__file__).resolve().parent.parent / "gnn-mwvc_amd" / "data" / "mwvc_model.txt").read_text()


# name -> the model's text.  h128: a 128-wide layer; f64: graph layers of f = 32 and 64 (k = 67, 131); embed: a dense prologue;
# linear_end: a bare linear ending; two_graphs: two graph layers in a row
MODELS = {
    "trained": _trained_text,
    "odd": lambda: H.text_of("shapes", "odd"),
    "in3": lambda: H.text_of("shapes", "in3"),
    "mixed": lambda: H.text_of("depths", "mixed"),
    "h128": lambda: modelgen_big.FAMILY["h128"](),
    "f64": lambda: modelgen_feat.FAMILY["f64"](),
    "embed": lambda: modelgen_patterns.FAMILY["embed"](),
    "linear_end": lambda: modelgen_patterns.FAMILY["linear_end"](),
    "two_graphs": lambda: modelgen_patterns.FAMILY["two_graphs"](),
}

_cache = {}

# ---------------------------------------------------------------- tables that reach every form of the kernels
# (tests/test_backward_reference.py, test_tables_cover_every_kernel_form, restates the dispatch of csrc/gnnvc_backward.hip as
# arithmetic on these shapes: whoever changes one changes the other)

# the parameter gradient's tile of ke = k + 1 rows (k when W is asked for alone, 1 for the bias alone) by m columns is chosen
# per side by tile(v) = 4 if v > 48 else 3 if v > 32 else 2 if v > 16 else 1, sixteen values a tile step
TILE_EDGE_K = [15, 16, 31, 32, 47, 48, 63, 64]    # ke = 16, 17 .. 64, 65: the bias row last of a tile, and alone in the next
TILE_EDGE_M = [16, 17, 32, 33, 48, 49, 64, 65]    # the last tile full, and with one live column
# n = 97: three chunks of 32 rows and one row, one block
TILE_EDGES = [(97, k, m) for k in TILE_EDGE_K for m in TILE_EDGE_M]
# n = 4129: a full block, then a block of one chunk and one row; one (k, m) per class, no multiple of 16
_TILE_K, _TILE_M = [10, 20, 40, 55], [10, 20, 40, 55]
TILE_BLOCKS = [(4129, k, m) for k in _TILE_K for m in _TILE_M]
# eight k-tiles, the bias in the last; k = 482 is also the input gradient's path without LDS
TILE_WIDE = [(97, 482, 17), (4129, 482, 5)]
TILE_SHAPES = TILE_EDGES + TILE_BLOCKS + TILE_WIDE

# the input gradient stages W through LDS while k * 17 * 4 <= 32768 (k <= 481), sixteen columns of m at a time; n * k is no
# multiple of 256 and a workgroup straddles rows
DX_K, DX_M = [1, 16, 17, 481, 482, 500], [1, 15, 16, 17, 33]
DX_SHAPES = [(3 if k > 400 else 97, k, m) for k in DX_K for m in DX_M]

# the graph layer's group of lanes is the power of two from f up to 64; wider rows take their columns 64 at a time
GRAPH_LAYER_F_WIDE = [65, 100, 129]
GRAPH_LAYER_WIDE_GRAPHS = ["er1933", "hub8k"]
LADDER_DEGREES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]
MULTIGRAPH_F = [1, 5, 17]


def ladder():
    """Twenty rung vertices of LADDER_DEGREES entries — GS - 1, GS, GS + 1 and 2 GS + 1 for every group size GS of the graph
    kernel — rung i joined to the first d_i of 129 leaves, and one isolated vertex: 150 vertices, rows ascend."""
    if ("graph", "ladder") not in _cache:
        rungs, leaves = len(LADDER_DEGREES), max(LADDER_DEGREES)
        a = np.concatenate([np.full(d, i) for i, d in enumerate(LADDER_DEGREES)])
        b = np.concatenate([rungs + np.arange(d) for d in LADDER_DEGREES])
        n = rungs + leaves + 1
        _cache["graph", "ladder"] = gg.csr_from_pairs(n, a, b, np.random.default_rng(83).integers(20, 121, size=n))
    return _cache["graph", "ladder"]


def multigraph():
    """erdos_renyi(300, 1200, 7) as a symmetric multigraph: every entry (v, u) with (v + u) % 3 == 0 stored twice (in both rows,
    the rule is symmetric), a self loop once at every fifth vertex and once more at every tenth; rows sorted."""
    if ("graph", "multigraph") not in _cache:
        g = gg.erdos_renyi(300, 1200, 7)
        rows = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(g.rowptr.astype(np.int64)))
        cols = g.col[: g.nnz].astype(np.int64)
        twice = (rows + cols) % 3 == 0
        fifth, tenth = np.arange(0, g.n, 5), np.arange(0, g.n, 10)
        src = np.concatenate([rows, rows[twice], fifth, tenth])
        dst = np.concatenate([cols, cols[twice], fifth, tenth])
        order = np.lexsort((dst, src))
        rowptr = np.zeros(g.n + 1, np.uint64)
        np.cumsum(np.bincount(src, minlength=g.n).astype(np.uint64), out=rowptr[1:])
        col = dst[order].astype(np.uint32)
        _cache["graph", "multigraph"] = gg.CsrGraph(g.n, rowptr, col, g.w, gg.neighbourhood_weights(rowptr, col, g.w))
    return _cache["graph", "multigraph"]


# ---------------------------------------------------------------- graphs that are not symmetric, by one entry

def _without_entry(g, e):
    rp = g.rowptr.astype(np.int64)
    v = int(np.searchsorted(rp, e, side="right") - 1)
    rowptr = rp.copy()
    rowptr[v + 1:] -= 1
    return gg.CsrGraph(g.n, rowptr.astype(np.uint64), np.delete(g.col[: g.nnz], e).astype(np.uint32), g.w, g.nw)


def _entry(g, v, u):
    """The first stored entry (v, u)."""
    rp = g.rowptr.astype(np.int64)
    return int(rp[v] + np.flatnonzero(g.col[rp[v]: rp[v + 1]] == u)[0])


def defects(gname):
    """[(label, graph)]: copies of the graph `gname` (rows ascend) with one stored entry deleted — at the places where the
    symmetry check's searches begin and end — and one with an entry redirected to a vertex that is no neighbour, its row sorted
    again: the row lengths stay and only the multiset is wrong.  Column ids stay in range; nw is left as it was."""
    g = graph_of(gname)
    rp, deg = g.rowptr.astype(np.int64), np.diff(g.rowptr.astype(np.int64))
    v = int(np.flatnonzero((deg >= 3) & (np.arange(g.n) > g.n // 2))[0])    # a row of three entries or more, away from the hubs
    first, last = int(g.col[rp[v]]), int(g.col[rp[v + 1] - 1])
    out = [("entry 0", _without_entry(g, 0)),
           ("entry nnz - 1", _without_entry(g, g.nnz - 1)),
           ("the first entry of a row", _without_entry(g, int(rp[v]))),
           ("the last entry of a row", _without_entry(g, int(rp[v + 1] - 1))),
           ("the partner of a row's first entry", _without_entry(g, _entry(g, first, v))),
           ("the partner of a row's last entry", _without_entry(g, _entry(g, last, v)))]
    if gname == "hub8k":
        e = int(rp[0] + deg[0] // 2)
        out += [("the middle of a hub row", _without_entry(g, e)),
                ("the partner of the middle of a hub row", _without_entry(g, _entry(g, int(g.col[e]), 0)))]
    e = int(rp[v] + 1)
    known = set(g.col[rp[v]: rp[v + 1]].tolist()) | {v}
    stranger = next(w for w in range(g.n // 3, g.n) if w not in known)
    col = g.col[: g.nnz].copy()
    col[e] = stranger
    col[rp[v]: rp[v + 1]] = np.sort(col[rp[v]: rp[v + 1]])
    out.append(("an entry redirected", gg.CsrGraph(g.n, g.rowptr, col, g.w, g.nw)))
    return out


# name -> the model's text: members of tools/modelgen_patterns.py nobody ran backwards.  relu_end ends in a ReLU of width 4;
# linear_end17 has 2 inputs and 17 outputs; mid_sigmoid has a sigmoid inside; mlp, bare_pair have no graph layer; prologue7
# has seven dense layers in front of its only graph layer
MORE_MODELS = {name: (lambda name=name: modelgen_patterns.FAMILY[name]())
               for name in ("relu_end", "linear_end17", "mid_sigmoid", "mlp", "bare_pair", "prologue7")}
MORE_MODEL_GRAPHS = ["one", "empty", "er1933", "er4097"]


def directed3():
    """0 -> 1 -> 2: the smallest graph that is not symmetric."""
    return gg.CsrGraph(3, np.array([0, 1, 2, 2], np.uint64), np.array([1, 2], np.uint32), np.array([30, 40, 50], np.uint32),
                       np.array([40, 50, 0], np.uint32))


def text_of(model):
    if ("text", model) not in _cache:
        _cache["text", model] = (MODELS[model] if model in MODELS else MORE_MODELS[model])()
    return _cache["text", model]


def graph_of(gname):
    if gname in GRAPHS:
        if ("graph", gname) not in _cache:
            _cache["graph", gname] = GRAPHS[gname]()
        return _cache["graph", gname]
    return H.graph_of(gname)


def model_input(g, width):
    """x = W / ws, and for wider inputs the columns x, 0.37 x, 1 - x, 3 x, 4 x ... (tools/modelgen_generic.py's rule)."""
    x = np.ascontiguousarray(g.x(), dtype=F32).reshape(g.n, 1)
    cols = [x, (x * F32(0.37)).astype(F32), (F32(1.0) - x).astype(F32)]
    while len(cols) < width:
        cols.append((x * F32(len(cols))).astype(F32))
    return np.ascontiguousarray(np.concatenate(cols[:width], axis=1), dtype=F32)


def in_width_of(text):
    """The model's input width: the first linear layer's k walked back through the graph layers in front of it."""
    from gnn_mwvc_amd import training
    graphs = 0
    for rec in training._walk(text)[1]:
        if rec[0] == "Graph_Layer":
            graphs += 1
        elif rec[0] == "Linear_Layer":
            k = rec[2]
            for _ in range(graphs):
                k = (k - 3) // 2
            return k
    return 1


def perturbed(params, seed):
    """Every parameter scaled by about 10 % and shifted by about 0.01: other bits everywhere, the same signs mostly."""
    rng = np.random.default_rng([97, seed])
    p = np.ascontiguousarray(params, dtype=F32)
    return (p * (1.0 + 0.1 * rng.standard_normal(p.size)) + 0.01 * rng.standard_normal(p.size)).astype(F32)


def grad_scores_of(n, width, seed):
    """One sign, magnitudes over a factor of four: the sums over the rows then do not cancel in their first step, so float64
    autograd can hold them to a few float32 roundings, and their bits still depend on the order of the terms."""
    rng = np.random.default_rng([53, seed])
    return rng.uniform(0.25, 1.0, (n, width)).astype(F32)


def loss_weighted(gs, scores):
    """gs times 2 min(s, 1 - s): the size of an MSE gradient against the hard label of each score.  The sigmoid's backward takes
    s (1 - s) from the ROUNDED output, whose relative error is eps / (1 - s) — 1 at a score that has rounded
    to 1, where float64 autograd still sees a derivative.  Generated models on the hub graph saturate 85 to 99 % of their scores;
    with every row weighted alike their gradient would be made of those rows alone, and the comparison with float64 would measure
    that stated price of the rule instead of the reference's terms.  A loss gradient shrinks where the score has settled, as
    this one does; the bits of every sum still depend on the order of its terms."""
    s = np.asarray(scores, dtype=F32)
    return (gs * (F32(2.0) * np.minimum(s, (F32(1.0) - s).astype(F32))).astype(F32)).astype(F32)


# (model, graph) -> the seed of the perturbed parameters where the default (len(model) + len(graph)) puts a ReLU input within
# rounding of zero, so that the float32 and the float64 forward switch the unit differently: ("odd", "hub8k") under seed 8 has
# z = +4.7e-6 in float32 and -4.7e-6 in float64 at row 3301, unit 6 of layer 8 — two different functions, 4.6e-4 apart in grad_bias
PERTURB_SEEDS = {("odd", "hub8k"): 108}


def flat_params(om):
    parts = []
    for W, b in om.linear_params():
        parts += [W.reshape(-1), b.reshape(-1)]
    return np.concatenate(parts).astype(F32) if parts else np.zeros(0, F32)


def is_symmetric(g):
    """(v, u) is stored as often as (u, v)."""
    rows = np.repeat(np.arange(g.n, dtype=np.int64), np.diff(g.rowptr.astype(np.int64)))
    cols = g.col[: g.nnz].astype(np.int64)
    a = np.sort(rows * max(g.n, 1) + cols)
    b = np.sort(cols * max(g.n, 1) + rows)
    return bool(np.array_equal(a, b))


# ---------------------------------------------------------------- the layer rules

def relu_backward(z, grad_out):
    z = np.asarray(z, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.where(z >= F32(0.0), np.asarray(grad_out, dtype=F32), F32(0.0)).astype(F32)


def sigmoid_backward(s, grad_out):
    s = np.asarray(s, dtype=F32)
    with np.errstate(all="ignore"):
        d = (s * (F32(1.0) - s).astype(F32)).astype(F32)
        return (d * np.asarray(grad_out, dtype=F32)).astype(F32)


def linear_backward(h, W, grad_out, old=None):
    """(grad_in, grad_W, grad_bias); old = (grad_W, grad_bias) to accumulate into."""
    h = np.ascontiguousarray(h, dtype=F32)
    W = np.ascontiguousarray(W, dtype=F32)
    go = np.ascontiguousarray(grad_out, dtype=F32)
    n, (k, m) = h.shape[0], W.shape
    gw, gb = np.zeros((k, m), F32), np.zeros((1, m), F32)   # +0.0f
    with np.errstate(all="ignore"):
        for lo in range(0, n, GRAD_BLOCK_ROWS):
            hi = min(n, lo + GRAD_BLOCK_ROWS)
            gw = (gw + oracle_py.sgemm(h[lo:hi], go[lo:hi], trans_a=True)).astype(F32)
            gb = (gb + oracle_py.sgemm(np.ones((hi - lo, 1), F32), go[lo:hi], trans_a=True)).astype(F32)
        if old is not None:
            gw = (np.asarray(old[0], dtype=F32).reshape(k, m) + gw).astype(F32)
            gb = (np.asarray(old[1], dtype=F32).reshape(1, m) + gb).astype(F32)
    gi = oracle_py.sgemm(go, W, trans_b=True) if n else np.zeros((0, k), F32)
    return gi, gw, gb.reshape(m)


def graph_layer_backward(g, grad_out):
    go = np.ascontiguousarray(grad_out, dtype=F32).reshape(g.n, -1)
    f = (go.shape[1] - 3) // 2
    nb = oracle_py.graph_layer(g, 1.0, np.ascontiguousarray(go[:, :f]))[:, :f]   # CSR-order sums of the neighbours' rows
    own = go[:, f: 2 * f].copy()
    own[:, 1:4] = F32(0.0)   # columns f + 1 .. f + 3 are overwritten by the forward: no own term for h[1 .. 3]
    with np.errstate(all="ignore"):
        return (nb + own).astype(F32)


# ---------------------------------------------------------------- the model level

def forward_acts(om, g, x, ws, sigmoid=None):
    """[x, the output of layer 0, of layer 1 ...]: every layer run from the previous activation with the oracle's own layer
    functions, so a sigmoid inside the model hands ITS output on — `sigmoid` (below) at every sigmoid layer, not only the last.
    With sigmoid = None this is om.predict(stop_after = i) bit for bit (tests/test_backward_reference.py asserts it)."""
    acts, li, P = [x], 0, om.linear_params()
    for kind in om.layer_kinds():
        h = np.ascontiguousarray(acts[-1], dtype=F32)
        if kind == LINEAR:
            acts.append(oracle_py.linear_layer(h, P[li][0], P[li][1]))
            li += 1
        elif kind == GRAPH:
            acts.append(oracle_py.graph_layer(g, ws, h))
        elif kind == RELU:
            acts.append(oracle_py.relu(h))
        else:
            acts.append(oracle_py.sigmoid(h) if sigmoid is None else sigmoid(h))
    return acts


def forward_acts_by_predict(om, g, x, sigmoid=None):
    """The same list from om.predict(stop_after = i), every layer from the model's input: how this module ran the forward before
    it met a sigmoid inside a model, which this way cannot take `sigmoid`.  Kept so that the test can hold forward_acts to it."""
    acts = [x]
    for i, kind in enumerate(om.layer_kinds()):
        if kind == SIGMOID and sigmoid is not None:
            assert i + 1 == om.n_layers, "a sigmoid inside the model"
            acts.append(sigmoid(np.ascontiguousarray(acts[i], dtype=F32)))
        else:
            acts.append(om.predict(g, x, stop_after=i))
    return acts


def backward(text, g, x, grad_scores, params=None, old=None, ws=None, sigmoid=None, by_predict=False):
    """dict(scores, grad_params, grad_x, layers=[(layer index, grad_W, grad_bias)]) of the model `text` — with `params` (flat) in
    place of its own — on g: the gradient of sum(grad_scores * scores).  old: a flat array to accumulate the parameter gradient into.
    sigmoid: the function that gives a sigmoid layer's output from its input, in place of the oracle's (host libm) — the GPU
    tests pass the restatement of the device's sigmoid (tests/support/libexpf_shim.so), whose scores the engine's are bit for bit.
    by_predict: the forward through forward_acts_by_predict."""
    from gnn_mwvc_amd import training
    om = oracle_py.OracleModel(text if params is None else training.text_with_params(text, params))
    om.set_weight_scale(g.ws if ws is None else ws)
    kinds = om.layer_kinds()
    P = om.linear_params()
    layout, total = training.param_layout(text)
    gp = np.zeros(total, F32) if old is None else np.ascontiguousarray(old, dtype=F32).copy()
    if g.n == 0:   # no row: every sum is empty
        return dict(scores=np.zeros((0, 1), F32), grad_params=gp, grad_x=np.zeros((0, in_width_of(text)), F32), layers=[],
                    relu_passes={}, inner_sigmoids={})
    x = np.ascontiguousarray(x, dtype=F32).reshape(g.n, -1)
    acts = forward_acts_by_predict(om, g, x, sigmoid) if by_predict else forward_acts(om, g, x, g.ws if ws is None else ws, sigmoid)
    grad = np.ascontiguousarray(grad_scores, dtype=F32).reshape(g.n, -1)
    li, layers = len(P), []
    for i in range(len(kinds) - 1, -1, -1):
        if kinds[i] == SIGMOID:
            grad = sigmoid_backward(acts[i + 1], grad)
        elif kinds[i] == RELU:
            grad = relu_backward(acts[i], grad)
        elif kinds[i] == GRAPH:
            grad = graph_layer_backward(g, grad)
        else:
            li -= 1
            k, m, w_off, b_off = layout[li]
            prev = None if old is None else (gp[w_off: w_off + k * m], gp[b_off: b_off + m])
            grad, gw, gb = linear_backward(acts[i], P[li][0], grad, prev)
            gp[w_off: w_off + k * m] = gw.reshape(-1)
            gp[b_off: b_off + m] = gb
            layers.append((i, gw, gb))
    with np.errstate(invalid="ignore"):   # which units every ReLU lets through, packed: what a float64 forward is compared with
        passes = {i: np.packbits(acts[i] >= F32(0.0)) for i, kind in enumerate(kinds) if kind == RELU}
    # the outputs of the sigmoids inside the model: what their backward read
    inner = {i: acts[i + 1] for i, kind in enumerate(kinds) if kind == SIGMOID and i + 1 < len(kinds)}
    return dict(scores=acts[-1], grad_params=gp, grad_x=grad, layers=layers[::-1], relu_passes=passes, inner_sigmoids=inner)


def case(model, gname, variant, sigmoid=None, by_predict=False):
    """The reference of one model-level case, computed once: variant "own" (params = None) or "perturbed"."""
    key = ("case", model, gname, variant, sigmoid is not None, by_predict)
    if key not in _cache:
        text, g = text_of(model), graph_of(gname)
        om = oracle_py.OracleModel(text)
        w_in = in_width_of(text)
        x = model_input(g, w_in)
        params = None if variant == "own" else perturbed(flat_params(om), seed=PERTURB_SEEDS.get((model, gname), len(model) + len(gname)))
        if params is not None:
            from gnn_mwvc_amd import training
            om = oracle_py.OracleModel(training.text_with_params(text, params))
        om.set_weight_scale(g.ws)
        scores = om.predict(g, x) if g.n else np.zeros((0, 1), F32)
        gs = grad_scores_of(g.n, scores.shape[1], seed=len(gname))
        if om.layer_kinds()[-1] == SIGMOID:
            gs = loss_weighted(gs, scores)
        ref = backward(text, g, x, gs, params, sigmoid=sigmoid, by_predict=by_predict)
        _cache[key] = dict(ref, text=text, g=g, x=x, params=params, grad_scores=gs)
    return _cache[key]
