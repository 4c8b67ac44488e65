"""tools/modelgen_generic.py: the text of every member of the three generic-stage families, byte for byte.  The digests were taken
before the three generators were folded into one; an edit of the shared draw, of the rng seed lists or of the text format that
moves any of them changes the weights every generic-stage test runs under, and has to say so here."""
import hashlib

import pytest

from tools import modelgen_big, modelgen_depths, modelgen_shapes

FAMILIES = {"shapes": modelgen_shapes, "depths": modelgen_depths, "big": modelgen_big}

# (family, member) -> SHA-256 of the member's text
DIGESTS = {
    ("shapes", "narrow"): "b5bf54adea8dcbd8c12934c5ba96d7bda42bef7577486032ef5b49715b61b6a0",
    ("shapes", "wide"): "1a1ce1e61aa2c2d943185014777704b3814e131924165538a0636e5fa657203e",
    ("shapes", "odd"): "f07761c998f7d1b1dc8b1fd618f05afa4ae5f0b02780ee738e2599e4c05b2e17",
    ("shapes", "two_stage"): "a40a58bc181c8cbc23e422963c9099e45f92f4cb75994bf97673d9191ffe8889",
    ("shapes", "deep5"): "1272c10ee48f8244251c815075006c94ced8043dcedcb4eeaa5d42974ae48d38",
    ("shapes", "in3"): "5e5ac9ec532aba03b487f2c2e560791710a307ccc86f64893bd38c7701440d57",
    ("shapes", "out4"): "f9bf462d3f018c911acdd5dab2c62bdb28a4ff99b5c6468869b63e73ad01afe0",
    ("shapes", "first_trained"): "7e65106a0d09b1ed054282139f0dfafc512d7628dc0dc272047c800ae0e92711",
    ("depths", "logit"): "0217eb81f2726c96e8fad1a6da63fd39eb299b3c87c58a1ca7b7b075628bd53e",
    ("depths", "one_each"): "c022752dabe61150a86087d39125692aeafc8d2bc610a95744ed11415fa5ea77",
    ("depths", "two_deep"): "77bb8898b500626c749fc2195c144ed2c6568ae9f891ab82187f80daac9e36d2",
    ("depths", "four_deep"): "9118d555ee87403e29ca479e585c671223c98af7974ed7386381546ab929a3f7",
    ("depths", "six_deep"): "53921e5194ed3af470ba828fc21ceb46e8cd910173cc28ae814dadb40ae7ae3e",
    ("depths", "mixed"): "de52dd901a13f2959a702ecd0c1944cd44200f716c398949f24f9c34e4f134a1",
    ("depths", "late_wide"): "dc2efa2306a9ebf0725bd8919cd4bb32fee15292a8ca327a446948d750495430",
    ("depths", "in3_f32"): "5fbf0675b4f7c4fd0fc511fc6086c3657acf51145f3715f8bae9c9165eeb78d2",
    ("depths", "too_big"): "24afb9795c163cde08d6c52f5e8f838957d3956b832328616b84a92f5552af89",
    ("big", "too_big"): "24afb9795c163cde08d6c52f5e8f838957d3956b832328616b84a92f5552af89",
    ("big", "h128"): "d90227a3296e9062776b479166a491ef67e345a3c0f4a90cd773da7ca097025c",
    ("big", "odd_wide"): "bccda7325476e299a28e4b4381ec2b23cb7b79aa1bf30d06cf7ffb0a186223a0",
    ("big", "edge"): "37fb9873e023dd613942dee9a2e0de0ac45b172ac421611fa9d47334cf25b053",
    ("big", "over"): "c894e6c52ae312321314f9f765c2b0a1da3a74b28f7914f33a7af7e960304e35",
}


def test_every_member_is_pinned():
    assert list(DIGESTS) == [(fam, name) for fam, m in FAMILIES.items() for name in m.SPECS] and len(DIGESTS) == 22


@pytest.mark.parametrize("family,name", list(DIGESTS))
def test_the_text_is_the_pinned_one(family, name):
    m = FAMILIES[family]
    text = m.FAMILY[name]()
    assert text == m.build(name) == m.family.build(name, m.family.seeds[name])
    first_line = "depths_too_big_0" if name == "too_big" else f"{family}_{name}_{m.family.seeds[name]}"   # (big's too_big is depths')
    assert text.split("\n", 1)[0] == first_line
    assert hashlib.sha256(text.encode()).hexdigest() == DIGESTS[family, name], (family, name)
