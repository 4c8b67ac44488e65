"""tools/modelgen_patterns.py: models whose layer sequence lies outside the generic fused stage's default pattern (what
gnnvc_set_generic_patterns admits: a dense stage in front of the first graph layer, a model that ends in a ReLU or in its bare
linear layer; two members that need a second opt-in; four that nothing admits).  The table, the text of every member (SHA-256)
and the byte figures of the kernel's LDS layout are pinned here (LDS_BYTES, which tests/test_gpu_patterns.py holds the engine to
as well); on the ORACLE, on erdos_renyi(3000, 15000, 15) and on the heavy-hub graph, every text parses, the stage-by-stage walk
of tests/pattern_harness.py — dense stage, graph stages, the three endings — equals predict over all layers bit for bit, and
the outputs are finite and vary over the vertices; `trunc` equals the reference-generated h2 rows of tests/golden bit for bit.

The bar for "vary": every output column of a member that ends in the sigmoid or in its bare linear layer takes more than one
value; of a drawn member that ends in a ReLU — which switches about half of a random layer's outputs off — at least half of the
columns do; of `trunc`, whose weights are the trained model's and not a seed's, at least one does."""
import hashlib

import numpy as np
import pytest

from oracle import oracle_py
from tools import modelgen_generic as mg
from tools import modelgen_patterns as mp
from tests import generic_harness as gh
from tests import pattern_harness as ph
from tests.generic_harness import bits, graph_of

KIND = {"L": 0, "G": 1, "R": 2, "S": 3}

# member -> SHA-256 of its text
DIGESTS = {
    "embed": "a0082e1f982ce0bd6479412313511d86e52f7b63d2d876d86ec8e0bb38e1d0fc",
    "embed1": "1f8ca35b7bd1abfc2389a730d0fa59d2fac26c41861ee11d540e505d76353630",
    "embed_deep": "d802db944b8da1c3ece118f8a298346e6f1cb20759d17beb56d4044442ab1883",
    "embed32": "9aae0ae7ee48eeba40ba2709d79e7609336b24e310504c678de1be322551430c",
    "mlp": "be6b243800ce85f9dbf94021110bc9146767dfad37e8798e59fa80b21a4a89c7",
    "relu_end": "29ba2a01dc4021f13986b0b8815468d19160f504058a06fa8e434f58ef685bf7",
    "trunc": "a9db98d2aabe3c4f91b2166dea46f8541c3758ba594451ca3c3f936298b59e47",
    "linear_end": "a058c8eedf1083701b3b8f4ca3df23df19fc7611d5b1a342b36a18b42d75c1a4",
    "linear_end17": "3822ce433a6f04aee45c7991183b13e0d1b6d11bf4e86f683a4aa24ca9b07a7c",
    "both": "7a29e1d6d89c30788c9950167c3d2c523b21a3caff40b930c5b333f338d694f7",
    "embed48": "efd2230a0b204d03d6b358ea15bf7a8ec9553f6d7bf27d35f712f2eff528420a",
    "embed_h128": "39b554ee88a30cce196ffc35005e6bca465588d0965d6b165e57fe27f064df8e",
    "mid_sigmoid": "d81e5f1c732b8224f983a4deee1c62eddb8a6c73dfddf37237e7a7e229c9ca52",
    "two_graphs": "955fab4e49df52abc92788d8f162d55a00865f0058188a586381a4074b281131",
    "prologue7": "1f051bd1a5d2ec4ad8e7f0007e53be3b12bed8db7d42935ae6ab326f47edea4a",
    "bare_pair": "d816f041cd8fe168f5027bbf7174bf1228d8f145a6f7e5b35924ef71668877dd",
}

# admitted member -> bytes per stage of stage_any_layout at 16 rows a workgroup (256 threads): "generic_stage_lds_bytes_<s>"
LDS_BYTES = {
    "embed": [416, 4320, 2528],
    "embed1": [672, 1760],
    "embed_deep": [9264, 4768],
    "embed32": [24448, 17600, 5792],
    "mlp": [3104],
    "relu_end": [3712, 6032],
    "trunc": [12864, 16192],
    "linear_end": [3040, 2528],
    "linear_end17": [3808],
    "both": [416, 2880],
    "embed48": [17824, 11936],
    "embed_h128": [28480, 5792],
}


def test_the_table_is_the_agreed_one():
    S = mp.SPECS
    assert list(S) == ["embed", "embed1", "embed_deep", "embed32", "mlp", "relu_end", "trunc", "linear_end", "linear_end17", "both",
                       "embed48", "embed_h128"] == mp.ADMITTED == list(LDS_BYTES)
    assert S["embed"] == (3, (8,), [(16, 8), (8, 1)], "sigmoid")
    assert S["embed1"] == (1, (4, 4), [(8, 1)], "sigmoid")
    assert S["embed_deep"] == (5, (16, 16, 16, 16, 16, 12), [(16, 1)], "sigmoid")
    assert S["embed32"] == (32, (64, 32), [(32, 16), (16, 1)], "sigmoid")
    assert S["mlp"] == (7, (16, 8, 1), [], "sigmoid")
    assert S["relu_end"] == (1, None, [(16, 16), (16, 4)], "relu")
    assert S["linear_end"] == (1, None, [(16, 8), (8, 1)], "none")
    assert S["linear_end17"] == (2, None, [(16, 17)], "none")
    assert S["both"] == (4, (8,), [(8, 8)], "relu")
    assert S["embed48"] == (48, (32, 40), [(16, 1)], "sigmoid")
    assert S["embed_h128"] == (16, (128, 16), [(16, 1)], "sigmoid")
    assert mp.MASK == {"embed": 1, "embed1": 1, "embed_deep": 1, "embed32": 1, "mlp": 1, "relu_end": 2, "trunc": 2, "linear_end": 2,
                       "linear_end17": 2, "both": 3, "embed48": 1, "embed_h128": 1}
    assert mp.NEEDS_FEAT == ["embed48"] and mp.NEEDS_BIG == ["embed_h128"]
    assert mp.NOT_FITTING == ["mid_sigmoid", "two_graphs", "prologue7", "bare_pair"] and mp.sequence("bare_pair") == "L4 L1"
    assert mp.NAMES == list(DIGESTS)
    assert mp.TAG not in {m.tag for m in gh.FAMILIES.values()} and mp.TAG != 23   # (23: tools/modelgen_feat.py)
    assert mp.sequence("embed") == "L8 R G L16 R L8 R G L8 R L1 S" and mp.sequence("linear_end17") == "G L16 R L17"
    assert mp.sequence("both") == "L8 R G L8 R L8 R" and mp.sequence("mlp") == "L16 R L8 R L1 S"
    assert mp.stage_widths("embed") == [(3, 8), (8, 8), (8, 1)] and mp.stage_depths("embed_deep") == [6, 2]
    assert mp.stage_dense("embed") == [1, 0, 0] and mp.stage_dense("trunc") == [0, 0] and mp.stage_dense("mlp") == [1]
    assert mp.stage_ends("embed") == [0, 0, 1] and mp.stage_ends("trunc") == [0, 0] and mp.stage_ends("linear_end") == [0, 2]
    assert mp.linear_shapes("embed") == [(3, 8), (19, 16), (16, 8), (19, 8), (8, 1)]
    assert mp.linear_shapes("two_graphs") == [(13, 8), (8, 1)] and mp.linear_shapes("prologue7")[7] == (19, 8)
    for mask in range(4):
        assert [n for n in mp.NAMES if mp.admitted_by(n, mask)] == [n for n in mp.ADMITTED if mp.MASK[n] & mask == mp.MASK[n]]
    assert [n for n in mp.NAMES if mp.admitted_by(n, 1)] == ["embed", "embed1", "embed_deep", "embed32", "mlp", "embed48", "embed_h128"]
    assert [n for n in mp.NAMES if mp.admitted_by(n, 2)] == ["relu_end", "trunc", "linear_end", "linear_end17"]


@pytest.mark.parametrize("name", mp.NAMES)
def test_the_text_is_the_pinned_one(name):
    text = mp.FAMILY[name]()
    assert text == mp.build(name)
    assert text.splitlines()[0] == ("patterns_trunc" if name == "trunc" else f"patterns_{name}_{mp.SEEDS[name]}")
    assert hashlib.sha256(text.encode()).hexdigest() == DIGESTS[name], name


def test_trunc_is_the_first_14_layers_of_the_trained_model():
    import gnn_mwvc_amd as G
    trained = oracle_py.OracleModel(G.default_model_text())
    om = oracle_py.OracleModel(ph.text_of("trunc"))
    assert om.n_layers == 14 and om.layer_kinds() == trained.layer_kinds()[:14]
    for (W, b), (W2, b2) in zip(om.linear_params(), trained.linear_params()[:6]):
        assert np.array_equal(bits(W), bits(W2)) and np.array_equal(bits(b), bits(b2))


def test_the_layout_restatement_gives_the_agreed_bytes():
    for name, want in LDS_BYTES.items():
        assert mp.lds_bytes(name) == want, name
    # by hand, a dense stage of f = 3 and one layer of 8: K = 3 at a pitch of 4, 8 biases, A = 4 and B = 0 floats a row
    assert mg.stage_lds_bytes(3, (8,), first_k=3) == 4 * (8 * 4 + 8 + 16 * 4) == 416
    # f = 32, widths (64, 32): K = 32 at a pitch of 36, K = 64 at a pitch of 68, 96 biases, A = 32 and B = 64 floats a row
    assert mg.stage_lds_bytes(32, (64, 32), first_k=32) == 4 * (64 * 36 + 32 * 68 + 96 + 16 * (32 + 64)) == 24448
    # the defaulted argument leaves a graph stage's figure where it was: K = 2 f + 3
    assert mg.stage_lds_bytes(3, (8,)) == mg.stage_lds_bytes(3, (8,), first_k=9) == 4 * (8 * 12 + 8 + 16 * 12)
    assert mp.stage_threads("embed_h128", mp.FULL_LDS) == [1024, 256]   # a 128-wide hidden layer: a big stage, whatever its bytes
    assert all(mp.stage_threads(n, mp.FULL_LDS) == [256] * len(mp.stages_of(n)) for n in mp.ADMITTED if n != "embed_h128")


@pytest.mark.parametrize("name", mp.NAMES)
def test_text_parses_and_has_the_named_shapes(name):
    om = oracle_py.OracleModel(ph.text_of(name))
    assert om.n_layers == mp.num_layers(name)
    assert om.layer_kinds() == [KIND[t[0]] for t in mp.sequence(name).split()]
    assert [tuple(W.shape) for W, _ in om.linear_params()] == mp.linear_shapes(name)
    if name != "trunc":
        for (W, b), (W2, b2) in zip(mp.layers_of(name), om.linear_params()):
            assert np.array_equal(bits(W), bits(W2)) and np.array_equal(bits(b), bits(b2))


@pytest.mark.parametrize("gname", ["er3000", "hubs"])
@pytest.mark.parametrize("name", mp.NAMES)
def test_walk_equals_predict_and_outputs_are_alive(name, gname):
    g = graph_of(gname)
    om = ph.oracle_at(name, g.ws)
    x = mp.model_input(name, g)
    assert x.shape == (g.n, mp.in_width(name))
    final = ph.predict(om, g, x)
    assert final.shape == (g.n, mp.out_width(name)) and np.isfinite(final).all(), name
    assert np.array_equal(bits(final), bits(ph.final_of(name, gname)))
    varying = sum(int(np.unique(bits(final[:, c])).size > 1) for c in range(final.shape[1]))
    ending = mp.sequence(name).split()[-1]
    need = 1 if name == "trunc" else (final.shape[1] + 1) // 2 if ending == "R" else final.shape[1]
    assert varying >= need, (name, gname, f"{varying} of {final.shape[1]} output columns vary")
    if ending == "S":
        logits = ph.predict(om, g, x, stop_after=om.n_layers - 2)
        assert np.isfinite(logits).all() and all(np.unique(bits(logits[:, c])).size > 1 for c in range(logits.shape[1])), name
    if name in mp.NOT_FITTING:
        return
    st = ph.walk(om, name, g)
    assert [(a.shape[1], b.shape[1]) for a, b, _ in st] == mp.stage_widths(name)
    assert np.array_equal(bits(st[-1][1]), bits(final)), (name, "the walk's last stage against predict over all layers")
    at = -1
    for (dense, _, widths, end), (_, h, pre) in zip(mp.stages_of(name), st):   # every stage boundary against predict up to it
        at += (0 if dense else 1) + 2 * len(widths) - (1 if end == mp.END_NONE else 0)
        assert np.array_equal(bits(h), bits(ph.predict(om, g, x, stop_after=at))), (name, at)
        if end != mp.END_NONE:
            assert np.array_equal(bits(pre), bits(ph.predict(om, g, x, stop_after=at - 1))), (name, at - 1)
        assert (h != 0).any(), name
    assert at == om.n_layers - 1
    assert ph.want_of(name, gname)[-1][1].shape == final.shape


@pytest.mark.parametrize("gname", ph.GOLDEN_GRAPHS)
def test_trunc_equals_the_reference_generated_h2(gname):
    g, h2 = ph.golden_h2(gname)
    om = ph.oracle_at("trunc", g.ws)
    assert np.array_equal(bits(ph.predict(om, g, g.x())), bits(h2)), gname
    st = ph.walk(om, "trunc", g, x=g.x())
    assert np.array_equal(bits(st[-1][1]), bits(h2)), gname
