"""The CPU reference of the backward pass (include/gnnvc.h "backward") and the case table its tests share.

Assembled from the oracle alone: activations from oracle_py.OracleModel.predict(stop_after=...), products from oracle_py.sgemm (one
k-ordered fmaf chain per output; per block of GRAD_BLOCK_ROWS rows for grad_W), neighbour sums from oracle_py.graph_layer on
grad[:, :f], everything else float32 numpy, one rounded operation at a time.  tests/test_backward_reference.py holds it to float64
autograd; tests/test_gpu_backward.py holds the engine to it bit for bit.  A plain module: nothing here touches a GPU.
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


def text_of(model):
    if ("text", model) not in _cache:
        _cache["text", model] = MODELS[model]()
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

def backward(text, g, x, grad_scores, params=None, old=None, ws=None, sigmoid=None):
    """dict(scores, grad_params, grad_x, layers=[(layer index, grad_W, grad_bias)]) of the model `text` — with `params` (flat) in
    place of its own — on g: the gradient of sum(grad_scores * scores).  old: a flat array to accumulate the parameter gradient into.
    sigmoid: the function that gives a last sigmoid layer's output from its input, in place of the oracle's (host libm) — the GPU
    tests pass the restatement of the device's sigmoid (tests/support/libexpf_shim.so), whose scores the engine's are bit for bit."""
    from gnn_mwvc_amd import training
    om = oracle_py.OracleModel(text if params is None else training.text_with_params(text, params))
    om.set_weight_scale(g.ws if ws is None else ws)
    kinds = om.layer_kinds()
    P = om.linear_params()
    layout, total = training.param_layout(text)
    gp = np.zeros(total, F32) if old is None else np.ascontiguousarray(old, dtype=F32).copy()
    if g.n == 0:   # no row: every sum is empty
        return dict(scores=np.zeros((0, 1), F32), grad_params=gp, grad_x=np.zeros((0, in_width_of(text)), F32), layers=[],
                    relu_passes={})
    x = np.ascontiguousarray(x, dtype=F32).reshape(g.n, -1)
    acts = [x]
    for i, kind in enumerate(kinds):
        if kind == SIGMOID and sigmoid is not None:
            assert i + 1 == len(kinds), "a sigmoid inside the model"
            acts.append(sigmoid(np.ascontiguousarray(acts[i], dtype=F32)))
        else:
            acts.append(om.predict(g, x, stop_after=i))
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
    return dict(scores=acts[-1], grad_params=gp, grad_x=grad, layers=layers[::-1], relu_passes=passes)


def case(model, gname, variant, sigmoid=None):
    """The reference of one model-level case, computed once: variant "own" (params = None) or "perturbed"."""
    key = ("case", model, gname, variant, sigmoid is not None)
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
        ref = backward(text, g, x, gs, params, sigmoid=sigmoid)
        _cache[key] = dict(ref, text=text, g=g, x=x, params=params, grad_scores=gs)
    return _cache[key]
