"""The fp32 reference of the backward pass (tests/backward_reference.py) against float64 autograd, on the CPU.

The model is rebuilt in torch from its text: aggregation by index_add, ReLU as where(z >= 0, z, 0), the graph layer's columns
f + 1 .. f + 3 overwritten by degree, W / ws and NW / ws as in the forward.  Every tensor the reference returns — grad_x, and grad_W
and grad_bias of every linear layer — is compared as a relative L2 error.

The bound.  The largest relative L2 error measured over the whole table below — every model-level GPU case, and the graph-layer
rule at every f and graph of the GPU table — is 1.34e-5 (1.332e-5 rounded up; grad_W of the first linear layer of the patterns member "embed" on hub8k
with perturbed parameters; next: ("shapes", "odd") on hub8k, 9.6e-6, and ("shapes", "in3") on `one`, 8.6e-6; the graph-layer rule
alone: 8.2e-7, f = 2 on hub8k).  Asserted is 64 x that, 8.6e-4, under the 1e-3 the bound has to stay under; chain lengths in the
table span about that factor, and a wrong term or a missed dead column shows as 1e-2 or more.

Two choices of input keep the comparison one of the reference's terms.  A ReLU whose input lies within rounding of zero is switched
differently by the float32 and the float64 forward, and the two are then gradients of different functions: the test counts such
units in every case and asserts there are none, and one perturbation seed was moved for it (R.PERTURB_SEEDS: ("odd", "hub8k") had
one such unit, worth 4.6e-4 in a grad_bias).  And the score gradients of a model that ends in the sigmoid are weighted like a
loss gradient, by 2 min(s, 1 - s) (R.loss_weighted): the sigmoid's backward takes s (1 - s) from the rounded output, by contract,
with a relative error of eps / (1 - s); generated models saturate 85 to 99 % of their scores on hub8k, and with every row
weighted alike the table's largest error was 3.1e-5, made of those rows.

Each layer's reference grad_W is asserted finite and to have a non-zero entry in every case but those that cannot have one: the
graph `empty` has no row to sum (there every parameter gradient is asserted to be +0.0f bit for bit), and on `one` — a single
vertex without a neighbour — a stage hands gradient to the stage before it through the own columns alone, of which three are
overwritten, so the layers of DEAD_ON_ONE (stage 0 of ("shapes", "odd"), the prologue of "embed") are exact zeros where the ReLUs
switch the remaining own units off for that vertex, with the model's own and with the perturbed parameters alike."""
import numpy as np
import pytest
import torch

from tests import backward_reference as R

MEASURED = 1.34e-5
BOUND = 64 * MEASURED
assert BOUND < 1e-3

# (model, layer index) whose grad_W is exactly zero on the graph `one`, with the model's own and with the perturbed parameters
DEAD_ON_ONE = {("odd", 1), ("odd", 3), ("odd", 5), ("embed", 0)}


def _rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    denom = np.linalg.norm(want)
    err = np.linalg.norm(np.asarray(got, dtype=np.float64) - want)
    return err / denom if denom else err


def _graph_layer64(g, h, ws):
    """graph_layer::forward in float64 torch: neighbour sums by index_add, the own columns, then the three overwritten columns."""
    n, f = h.shape
    deg = np.diff(g.rowptr.astype(np.int64))
    rows = torch.from_numpy(np.repeat(np.arange(n, dtype=np.int64), deg))
    cols = torch.from_numpy(g.col[: g.nnz].astype(np.int64))
    agg = torch.zeros((n, f), dtype=torch.float64).index_add(0, rows, h[cols])
    const = torch.zeros((n, 3), dtype=torch.float64)
    const[:, 0] = torch.from_numpy(deg.astype(np.float64))
    const[:, 1] = torch.from_numpy(g.w.astype(np.float32).astype(np.float64) / np.float64(np.float32(ws)))
    const[:, 2] = torch.from_numpy(g.nw.astype(np.float32).astype(np.float64) / np.float64(np.float32(ws)))
    out = torch.cat([agg, h, torch.zeros((n, 3), dtype=torch.float64)], dim=1)
    keep = torch.ones(2 * f + 3, dtype=torch.bool)
    keep[f + 1: f + 4] = False
    full = torch.zeros((n, 2 * f + 3), dtype=torch.float64)
    full[:, f + 1: f + 4] = const
    return torch.where(keep, out, full)


def _autograd(text, g, x, grad_scores, params):
    """(grad_x, [(grad_W, grad_bias)], {ReLU layer: which units pass, packed}) of sum(grad_scores * scores) in float64."""
    from gnn_mwvc_amd import training
    from oracle import oracle_py
    om = oracle_py.OracleModel(text if params is None else training.text_with_params(text, params))
    kinds, P = om.layer_kinds(), om.linear_params()
    tx = torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(True)
    tp = [(torch.from_numpy(W.astype(np.float64)).requires_grad_(True), torch.from_numpy(b.astype(np.float64)).requires_grad_(True))
          for W, b in P]
    h, li, passes = tx, 0, {}
    for i, kind in enumerate(kinds):
        if kind == R.LINEAR:
            h = h @ tp[li][0] + tp[li][1]
            li += 1
        elif kind == R.GRAPH:
            h = _graph_layer64(g, h, g.ws)
        elif kind == R.RELU:
            passes[i] = np.packbits(h.detach().numpy() >= 0)
            h = torch.where(h >= 0, h, torch.zeros_like(h))
        else:
            h = torch.sigmoid(h)
    (h * torch.from_numpy(np.asarray(grad_scores, dtype=np.float64))).sum().backward()
    return tx.grad.numpy(), [(W.grad.numpy(), b.grad.numpy()) for W, b in tp], passes


CASES = [(m, gname, v) for m in R.MODELS for gname in R.MODEL_GRAPHS for v in ("own", "perturbed")]


@pytest.mark.parametrize("model", list(R.MODELS))
def test_model_gradients_against_float64_autograd(model):
    worst = 0.0
    for gname in R.MODEL_GRAPHS:
        for variant in ("own", "perturbed"):
            c = R.case(model, gname, variant)
            g = c["g"]
            assert R.is_symmetric(g), gname
            if g.n == 0:
                assert not c["grad_params"].view(np.uint32).any(), (model, gname, variant)
                continue
            gx, layers, passes = _autograd(c["text"], g, c["x"], c["grad_scores"], c["params"])
            # the two forwards are the same function only while every ReLU decides alike: a pre-activation within rounding of
            # zero makes the case one about the input, not about the reference (R.PERTURB_SEEDS)
            flips = {i: int(np.unpackbits(passes[i] ^ c["relu_passes"][i]).sum()) for i in passes}
            assert not any(flips.values()), (model, gname, variant, "ReLU decisions differ between float32 and float64", flips)
            errs = {"grad_x": _rel(c["grad_x"], gx)}
            assert len(layers) == len(c["layers"])
            for (i, gw, gb), (W64, b64) in zip(c["layers"], layers):
                assert np.isfinite(gw).all(), (model, gname, variant, "layer", i, "grad_W is not finite")
                assert gw.any() or (gname == "one" and (model, i) in DEAD_ON_ONE), (model, gname, variant, "layer", i, "grad_W is dead")
                errs[f"grad_W[{i}]"] = _rel(gw, W64)
                errs[f"grad_bias[{i}]"] = _rel(gb, b64)
            top = max(errs, key=errs.get)
            print(f"{model:>11} {gname:>7} {variant:>9}: worst {top} {errs[top]:.3e}")
            worst = max(worst, errs[top])
            bad = {k: v for k, v in errs.items() if not v <= BOUND}
            assert not bad, (model, gname, variant, bad)
    print(f"{model}: largest relative L2 error {worst:.3e}")


@pytest.mark.parametrize("f", R.GRAPH_LAYER_F)
def test_graph_layer_rule_against_float64_autograd(f):
    for gname in R.GRAPH_LAYER_GRAPHS:
        g = R.graph_of(gname)
        rng = np.random.default_rng([71, f])
        go = rng.standard_normal((g.n, 2 * f + 3)).astype(np.float32)
        h = torch.from_numpy(rng.standard_normal((g.n, f))).requires_grad_(True)
        (_graph_layer64(g, h, g.ws) * torch.from_numpy(go.astype(np.float64))).sum().backward()
        err = _rel(R.graph_layer_backward(g, go), h.grad.numpy())
        print(f"graph layer f = {f:>2} {gname:>7}: {err:.3e}")
        assert err <= BOUND, (f, gname, err)
        dead = R.graph_layer_backward(g, go)[:, 1:4] - R.oracle_py.graph_layer(g, 1.0, np.ascontiguousarray(go[:, :f]))[:, 1:min(f, 4)]
        assert not dead.any(), "h[1 .. 3] carry no own term"


def test_case_table_covers_the_issue():
    assert set(R.MODEL_GRAPHS) == {"one", "empty", "er1933", "hub8k", "er4097", "er8209"}
    assert R.graph_of("er4097").n == 4097 and R.graph_of("er8209").n == 8209
    shapes = {name: [(k, m) for k, m, _, _ in __import__("gnn_mwvc_amd.training", fromlist=["x"]).param_layout(R.text_of(name))[0]]
              for name in R.MODELS}
    assert any(m == 128 for k, m in shapes["h128"]) and any(k == 131 for k, m in shapes["f64"])
    assert len(CASES) == 9 * 6 * 2
