"""tools/modelgen_big.py: models whose stages lie outside the generic fused stage's default bounds (what
gnnvc_set_generic_big_stages admits, and one member it does not).  The specs and the byte figures of the kernel's LDS layout —
restated in Python by the generator — are pinned here (LDS_BYTES of tests/generic_harness.py, which the GPU test holds the engine
to as well); on the ORACLE, on erdos_renyi(3000, 15000, 15), every text parses with the named shapes, the stage-by-stage walk that
tests/test_gpu_big_stages.py takes its per-stage references from equals predict bit for bit, and every member's logits are finite
and take more than one value."""
import numpy as np
import pytest

from oracle import oracle_py
from tools import graphgen as gg
from tools import modelgen_big as mb
from tools import modelgen_depths as md
from tests.generic_harness import LDS_BYTES, bits, stage_outputs

LINEAR, GRAPH, RELU, SIGMOID = 0, 1, 2, 3


@pytest.fixture(scope="module")
def graph():
    return gg.erdos_renyi(3000, 15000, 15)


def test_the_specs_are_the_agreed_ones():
    S = mb.SPECS
    assert list(S) == ["too_big", "h128", "odd_wide", "edge", "over"]
    assert S["too_big"] == (1, [(64, 64, 64, 64, 64, 32), (64, 64, 64, 64, 64, 1)]) == md.SPECS["too_big"]
    assert S["h128"] == (1, [(128, 128, 16), (128, 64, 1)])
    assert S["odd_wide"] == (3, [(97, 65, 32), (113, 80, 7, 1)])
    assert S["edge"] == (1, [(128, 128, 106, 32), (1,)])
    assert S["over"] == (1, [(128, 128, 128, 32), (128, 1)])
    assert mb.ADMITTED == ["too_big", "h128", "odd_wide", "edge"] and mb.NOT_FITTING == ["over"]
    assert mb.stage_widths("odd_wide") == [(3, 32), (32, 1)] and mb.stage_depths("odd_wide") == [3, 4]
    assert all(1 <= len(ws) <= md.MAX_DENSE_LAYERS for _, st in S.values() for ws in st)


def test_the_layout_restatement_gives_the_agreed_bytes():
    for name, want in LDS_BYTES.items():
        assert mb.lds_bytes(name) == want, name
    # the layout of modelgen_depths' fitting members stays within the default bound (the restatement is not off by a constant)
    for name in md.FITTING:
        f = md.in_width(name)
        for ws in md.SPECS[name][1]:
            assert mb.stage_lds_bytes(f, ws) <= mb.SMALL_LDS and mb.stage_is_small(f, ws), name
            f = ws[-1]
    assert mb.stage_lds_bytes(1, (32, 32, 16)) == 4 * (32 * 12 + 32 * 36 + 16 * 36 + 80 + 16 * (32 + 32))   # by hand: the trained stage 0


def test_which_side_of_the_limits_every_stage_lies_on():
    small = {name: [mb.stage_is_small(f, ws) for (f, _), ws in zip(mb.stage_widths(name), mb.SPECS[name][1])] for name in mb.SPECS}
    assert small == {"too_big": [False, False], "h128": [False, False], "odd_wide": [False, False], "edge": [False, True],
                     "over": [False, False]}   # (over's second stage is within 64 KiB, but 128 wide)
    assert mb.lds_bytes("h128")[1] == mb.SMALL_LDS + 32                       # 32 bytes over
    assert mb.lds_bytes("odd_wide")[0] <= mb.SMALL_LDS                        # fits, and is not small: a 97-wide layer
    for name in mb.ADMITTED:
        assert max(mb.lds_bytes(name)) <= mb.MAX_LDS, name
    assert mb.lds_bytes("over")[0] > mb.MAX_LDS
    assert mb.lds_bytes("edge")[0] <= mb.MAX_LDS < mb.lds_bytes("edge", rows=32)[0]   # fits at 256 threads only
    assert mb.lds_bytes("h128", rows=64)[0] == 148800
    # the launcher's rule at the full limit
    threads = {name: [mb.stage_threads(f, ws, mb.MAX_LDS) for (f, _), ws in zip(mb.stage_widths(name), mb.SPECS[name][1])]
               for name in mb.ADMITTED}
    assert threads == {"too_big": [1024, 1024], "h128": [1024, 1024], "odd_wide": [1024, 1024], "edge": [256, 256]}
    assert mb.stage_threads(1, (128, 128, 16), 99648) == 256


def test_too_big_is_modelgen_depths_text():
    assert mb.FAMILY["too_big"]() == md.FAMILY["too_big"]()


@pytest.mark.parametrize("name", list(mb.SPECS))
def test_text_parses_and_has_the_named_shapes(name):
    text = mb.FAMILY[name]()
    assert text == mb.FAMILY[name]()   # from the seed alone
    om = oracle_py.OracleModel(text)
    assert om.n_layers == mb.num_layers(name) == sum(1 + 2 * d for d in mb.stage_depths(name))
    want_kinds = []
    for d in mb.stage_depths(name):
        want_kinds += [GRAPH] + [LINEAR, RELU] * d
    want_kinds[-1] = SIGMOID
    assert om.layer_kinds() == want_kinds
    assert [tuple(W.shape) for W, _ in om.linear_params()] == mb.linear_shapes(name)
    for (W, b), (W2, b2) in zip(mb.layers_of(name), om.linear_params()):
        assert np.array_equal(bits(W), bits(W2)) and np.array_equal(bits(b), bits(b2))


@pytest.mark.parametrize("name", list(mb.SPECS))
def test_walk_equals_predict_and_logits_are_alive(graph, name):
    g = graph
    om = oracle_py.OracleModel(mb.FAMILY[name]())
    om.set_weight_scale(g.ws)
    x = mb.model_input(name, g)
    assert x.shape == (g.n, mb.in_width(name))
    st = stage_outputs(om, "big", name, g)
    assert [(a.shape[1], b.shape[1]) for a, b, _ in st] == mb.stage_widths(name)
    logits = om.predict(g, x, stop_after=om.n_layers - 2)
    scores = om.predict(g, x)
    assert logits.shape == (g.n, mb.out_width(name))
    assert np.array_equal(bits(st[-1][2]), bits(logits)), name
    assert np.array_equal(bits(st[-1][1]), bits(scores)), name
    assert np.isfinite(logits).all() and np.isfinite(scores).all(), name
    for c in range(logits.shape[1]):
        assert np.unique(bits(logits[:, c])).size > 1, (name, c)
    for s, (_, h, _) in enumerate(st):
        assert (h != 0).any(), (name, s)
