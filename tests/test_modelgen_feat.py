"""tools/modelgen_feat.py: models whose feature widths lie outside the generic fused stage's default bounds (what
gnnvc_set_generic_feature_width admits, one member that needs gnnvc_set_generic_big_stages as well, and one that nothing admits).
The specs, the text of every member (SHA-256, as tests/test_modelgen_generic.py pins the other families) and the byte figures of
the kernel's LDS layout are pinned here (LDS_BYTES, which tests/test_gpu_feature_width.py holds the engine to as well); on the
ORACLE, on erdos_renyi(3000, 15000, 15) and on the heavy-hub graph, the stage-by-stage walk that the GPU tests take their
per-stage references from equals predict bit for bit, and every member's logits are finite and take more than one value."""
import hashlib

import numpy as np
import pytest

from oracle import oracle_py
from tools import modelgen_feat as mf
from tests import generic_harness as gh
from tests.generic_harness import bits, graph_of, stage_outputs

gh.FAMILIES["feat"] = mf.family

LINEAR, GRAPH, RELU, SIGMOID = 0, 1, 2, 3


def predict(om, g, x, stop_after=-1):
    """OracleModel.predict: its output buffer is as wide as the model's widest layer (out64's 64 scores a vertex fit)."""
    return om.predict(g, x, stop_after=stop_after)

# member -> SHA-256 of its text
DIGESTS = {
    "f33": "67d62634980a9d6d8f2ee9177757ef0c55e0092d94fec0acbe37c808d2007c5c",
    "f47": "9e1095861fa3b1c3e0046dfdcd5eb53bea984cf2e38c560b860fe9731dc0135a",
    "f48_49": "5e66892db488e2ed07c475b401bd885c5c74244e708898dc4f4f8afa2aed6423",
    "f64": "543660647dbb5492ddf792987a550e1d70f3c5f6515c55da557d9c4be009e0ec",
    "in40": "3d8a7200705d97f7c359ead34131e0304979fc3fa8ace21b78e0fc851b774064",
    "out64": "ef0273288732b8202efea32b637f0843838c9fcffdef38cbdeffe5fad25e07f5",
    "big_f64": "783bf9c3a48af7cb7e5e6892da580cc6dc12ec5bac5646b63659d287b60eae8f",
    "f65": "97cb65ffe40e83e1f0d9dd913be110aaff6e3867bd9db47cb6a4735eb4fcc1b6",
}

# member -> bytes per stage of stage_any_layout at 16 rows a workgroup (256 threads): "generic_stage_lds_bytes_<s>"
LDS_BYTES = {
    "f33": [5152, 10656],
    "f47": [8752, 23088, 10208],
    "f48_49": [11328, 28640, 14752],
    "f64": [13696, 64256, 27680],
    "in40": [20672, 5792],
    "out64": [3712, 18560],
    "big_f64": [25600, 118784, 46880],
    "f65": [13856, 18848],
}


def test_the_specs_are_the_agreed_ones():
    S = mf.SPECS
    assert list(S) == ["f33", "f47", "f48_49", "f64", "in40", "out64", "big_f64", "f65"] == list(DIGESTS) == list(LDS_BYTES)
    assert S["f33"] == (1, [(16, 33), (16, 1)])
    assert S["f47"] == (1, [(24, 47), (24, 47), (8, 1)])
    assert S["f48_49"] == (1, [(32, 48), (32, 49), (16, 1)])
    assert S["f64"] == (1, [(32, 64), (64, 64), (32, 1)])
    assert S["in40"] == (40, [(32, 16), (16, 1)])
    assert S["out64"] == (1, [(16, 16), (32, 64)])
    assert S["big_f64"] == (1, [(64, 64), (128, 64), (64, 1)])
    assert S["f65"] == (1, [(32, 65), (16, 1)])
    assert mf.ADMITTED == ["f33", "f47", "f48_49", "f64", "in40", "out64"] and mf.NEEDS_BIG == ["big_f64"] and mf.NOT_FITTING == ["f65"]
    assert mf.family.prefix == "feat" and mf.family.tag == 23
    assert mf.family.tag not in {m.tag for k, m in gh.FAMILIES.items() if k != "feat"}
    assert mf.stage_widths("f48_49") == [(1, 48), (48, 49), (49, 1)] and mf.stage_depths("f47") == [2, 2, 2]
    assert mf.in_width("in40") == 40 and mf.out_width("out64") == 64
    assert {name: mf.feature_width_needed(name) for name in S} == {"f33": 33, "f47": 47, "f48_49": 49, "f64": 64, "in40": 40,
                                                                     "out64": 64, "big_f64": 64, "f65": 65}


@pytest.mark.parametrize("name", list(mf.SPECS))
def test_the_text_is_the_pinned_one(name):
    text = mf.FAMILY[name]()
    assert text == mf.build(name) == mf.family.build(name, mf.SEEDS[name])
    assert text.splitlines()[0] == f"feat_{name}_{mf.SEEDS[name]}"
    assert hashlib.sha256(text.encode()).hexdigest() == DIGESTS[name], name


def test_the_layout_restatement_gives_the_agreed_bytes():
    for name, want in LDS_BYTES.items():
        assert mf.lds_bytes(name) == want, name
    assert mf.lds_bytes("f64")[1] == 64256 <= mf.SMALL_LDS                                  # the widest small stage: inside 64 KiB
    assert mf.lds_bytes("big_f64")[1] == 118784
    assert mf.lds_bytes("big_f64", rows=32)[1] == 135424 <= mf.MAX_LDS < mf.lds_bytes("big_f64", rows=64)[1] == 168704
    # by hand, f = 64 and widths (64, 64): K = 131 at a pitch of 132, then K = 64 at a pitch of 68, A = 132 and B = 64 floats a row
    assert mf.stage_lds_bytes(64, (64, 64)) == 4 * (64 * 132 + 64 * 68 + 128 + 16 * (132 + 64)) == 64256


def test_which_side_of_the_bounds_every_member_lies_on():
    off = {name: mf.model_fits(name) for name in mf.SPECS}
    assert not any(off.values()), off                                                         # off: none is fused
    on = {name: mf.model_fits(name, 64) for name in mf.SPECS}
    assert on == {name: name in mf.ADMITTED for name in mf.SPECS}
    both = {name: mf.model_fits(name, 64, mf.MAX_LDS) for name in mf.SPECS}
    assert both == {name: name != "f65" for name in mf.SPECS}
    assert not mf.model_fits("big_f64", 0, mf.MAX_LDS)                                        # big stages alone do not admit it
    assert not mf.model_fits("f48_49", 48) and mf.model_fits("f48_49", 49)
    assert not mf.model_fits("f33", 32) and mf.model_fits("f33", 33)                          # (32 is no value of the call: the default)
    assert not mf.model_fits("f65", 65)                                                       # (nor is 65)
    threads = [mf.stage_threads_feat(f, ws, mf.MAX_LDS) for (f, _), ws in zip(mf.stage_widths("big_f64"), mf.SPECS["big_f64"][1])]
    assert threads == [256, 512, 256]
    for name in mf.ADMITTED:
        assert all(mf.stage_threads_feat(f, ws) == 256 for (f, _), ws in zip(mf.stage_widths(name), mf.SPECS[name][1])), name


@pytest.mark.parametrize("name", list(mf.SPECS))
def test_text_parses_and_has_the_named_shapes(name):
    om = oracle_py.OracleModel(gh.text_of("feat", name))
    assert om.n_layers == mf.num_layers(name) == sum(1 + 2 * d for d in mf.stage_depths(name))
    want_kinds = []
    for d in mf.stage_depths(name):
        want_kinds += [GRAPH] + [LINEAR, RELU] * d
    want_kinds[-1] = SIGMOID
    assert om.layer_kinds() == want_kinds
    assert [tuple(W.shape) for W, _ in om.linear_params()] == mf.linear_shapes(name)
    for (W, b), (W2, b2) in zip(mf.layers_of(name), om.linear_params()):
        assert np.array_equal(bits(W), bits(W2)) and np.array_equal(bits(b), bits(b2))


@pytest.mark.parametrize("gname", ["er3000", "hubs"])
@pytest.mark.parametrize("name", list(mf.SPECS))
def test_walk_equals_predict_and_logits_are_alive(name, gname):
    g = graph_of(gname)
    om = gh.oracle_of("feat", name, g)
    x = mf.model_input(name, g)
    assert x.shape == (g.n, mf.in_width(name))
    st = stage_outputs(om, "feat", name, g)
    assert [(a.shape[1], b.shape[1]) for a, b, _ in st] == mf.stage_widths(name)
    logits = predict(om, g, x, stop_after=om.n_layers - 2)
    scores = predict(om, g, x)
    assert logits.shape == (g.n, mf.out_width(name))
    assert np.array_equal(bits(st[-1][2]), bits(logits)), name
    assert np.array_equal(bits(st[-1][1]), bits(scores)), name
    assert np.isfinite(logits).all() and np.isfinite(scores).all(), name
    for c in range(logits.shape[1]):
        assert np.unique(bits(logits[:, c])).size > 1, (name, c)
    for s, (_, h, _) in enumerate(st):
        assert (h != 0).any(), (name, s)
        live = int((h != 0).any(axis=0).sum())
        assert live >= max(1, h.shape[1] // 4), (name, s, f"only {live} of {h.shape[1]} columns of the stage's output are ever non-zero")
