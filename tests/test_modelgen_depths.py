"""tools/modelgen_depths.py: models whose stages have one to six dense layers (what the generic fused stage, k_stage_any, runs
beyond the trained depth of three).  On the ORACLE, on erdos_renyi(3000, 15000, 15): every text parses with the named layer
count and layer kinds, the stage-by-stage walk that tests/test_gpu_depths.py takes its per-stage references from equals
predict bit for bit, and every member's logits are finite and take more than one value (random ReLU units die; a model whose
output were constant would test nothing)."""
import numpy as np
import pytest

from oracle import oracle_py
from tools import graphgen as gg
from tools import modelgen_depths as md
from tests.generic_harness import bits, stage_outputs

LINEAR, GRAPH, RELU, SIGMOID = 0, 1, 2, 3


@pytest.fixture(scope="module")
def graph():
    return gg.erdos_renyi(3000, 15000, 15)


def test_the_required_members_are_there():
    S = md.SPECS
    assert S["logit"] == (1, [(1,)])
    assert S["one_each"] == (1, [(8,), (4,), (1,)])
    assert S["two_deep"] == (1, [(24, 12), (24, 1)])
    assert S["four_deep"] == (1, [(32, 32, 32, 16), (32, 32, 16, 1)])
    assert S["six_deep"] == (1, [(16, 16, 16, 16, 16, 8), (16, 16, 16, 16, 16, 1)])
    assert S["mixed"] == (1, [(32, 32, 16), (20,), (9, 7, 13, 11, 1)])
    assert S["late_wide"] == (1, [(8, 8, 8, 64, 4), (8, 64, 7, 64, 1)])
    assert S["in3_f32"] == (3, [(40, 32), (61, 3, 50, 1)])
    assert S["too_big"] == (1, [(64, 64, 64, 64, 64, 32), (64, 64, 64, 64, 64, 1)])
    assert md.FITTING == [n for n in S if n != "too_big"] and len(md.FITTING) == 8
    assert md.num_layers("logit") == 3 and md.stage_depths("mixed") == [3, 1, 5]
    assert md.linear_shapes("in3_f32")[2] == (67, 61) and md.stage_widths("in3_f32") == [(3, 32), (32, 1)]
    assert all(1 <= len(ws) <= md.MAX_DENSE_LAYERS for _, st in S.values() for ws in st)


@pytest.mark.parametrize("name", list(md.SPECS))
def test_text_parses_and_has_the_named_shapes(name):
    text = md.FAMILY[name]()
    assert text == md.FAMILY[name]()   # from the seed alone
    om = oracle_py.OracleModel(text)
    assert om.n_layers == md.num_layers(name) == sum(1 + 2 * d for d in md.stage_depths(name))
    want_kinds = []
    for d in md.stage_depths(name):
        want_kinds += [GRAPH] + [LINEAR, RELU] * d
    want_kinds[-1] = SIGMOID
    assert om.layer_kinds() == want_kinds
    assert [tuple(W.shape) for W, _ in om.linear_params()] == md.linear_shapes(name)
    assert md.linear_shapes(name)[0][0] == 2 * md.in_width(name) + 3
    for (W, b), (W2, b2) in zip(md.layers_of(name), om.linear_params()):
        assert np.array_equal(bits(W), bits(W2)) and np.array_equal(bits(b), bits(b2))


@pytest.mark.parametrize("name", list(md.SPECS))
def test_walk_equals_predict_and_logits_are_alive(graph, name):
    g = graph
    om = oracle_py.OracleModel(md.FAMILY[name]())
    om.set_weight_scale(g.ws)
    x = md.model_input(name, g)
    assert x.shape == (g.n, md.in_width(name))
    st = stage_outputs(om, "depths", name, g)
    assert [(a.shape[1], b.shape[1]) for a, b, _ in st] == md.stage_widths(name)
    logits = om.predict(g, x, stop_after=om.n_layers - 2)
    scores = om.predict(g, x)
    assert logits.shape == (g.n, md.out_width(name))
    assert np.array_equal(bits(st[-1][2]), bits(logits)), name
    assert np.array_equal(bits(st[-1][1]), bits(scores)), name
    # alive: finite, and more than one value over the vertices — in every output column
    assert np.isfinite(logits).all() and np.isfinite(scores).all(), name
    for c in range(logits.shape[1]):
        assert np.unique(bits(logits[:, c])).size > 1, (name, c)
    # and every stage hands something on: no stage output is all zero
    for s, (_, h, _) in enumerate(st):
        assert (h != 0).any(), (name, s)
