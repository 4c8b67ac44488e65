"""tools/modelgen_live.py's family on the CPU: the members' texts pinned by SHA-256 (the rng seed list and the order of the draws
are part of every test's weights), sparse32's dead units dead on the oracle whatever the graph, the lemma that lets a gather
skip a dead column — a column that is +-0.0 in every row sums to +0.0f, bits 0x00000000, for every vertex, and the other
columns' sums do not notice its absence — shown on the oracle's own graph layer, and the per-stage live masks that
tests/test_gpu_live_columns.py expects of the engine, computed with the oracle's walk and pinned here."""
import hashlib

import numpy as np
import pytest

from oracle import oracle_py
from tools import modelgen_live as ml
from tests import generic_harness as gh
from tests import live_harness as lh
from tests.generic_harness import bits, crafted_input, graph_of

SHA256 = {
    "in2": "c552f21a81352eea41811e1e8d813d44cc95ed4a88c99d762bc798a63d2948c3",
    "in16": "231ce992e93dc93d5b10465c60f19a26c4c7da393664652e7a45c01974934163",
    "in17": "043f5a20eda8400d7d11911e06d5a4409997cfde8d1d3bfbee3ed2d3a1ba0e5a",
    "in32": "9d6465517a8a6dd1cb54fc6b1e58cee915e87429bafadaaec91c2cf9a6a5c6c5",
    "in33": "a9981f389e83ff96e94824270ad173744a32702a1694e7b098bb553dd6d5317a",
    "in48": "027663fbc194368a9383ad3aa0d1e30282bc1a38e8ad568890e02b40772a9a4f",
    "in49": "8e2f207ac5999a8564360524f6dfe452fbc33a48b0bc4afb9de74fe6b26abd8c",
    "in64": "ad41d91c98326532fc3c5188c7079897794add8b1bfd22d03b8fb094c4ec5c25",
    "sparse32": "88b05767761aa6eeb540c2ef84db94af5681736f5cb15a89dd75c3cd38fa95e7",
}

# (family, member, graph) -> [(f, mask of the live columns of the stage's input)] per stage, by the oracle's walk
MASKS = {
    ("shapes", "wide", "er3000"): [(1, 0x1), (32, 0x4e9bf4c2), (32, 0x97fdec0b)],   # kept [1, 17, 20]
    ("shapes", "wide", "er1933"): [(1, 0x1), (32, 0x4e9bf6c7), (32, 0x97fdfd2b)],   # kept [1, 20, 23]
    ("shapes", "wide", "sparse"): [(1, 0x1), (32, 0x4e9bf6c7), (32, 0x97f9bd2b)],   # kept [1, 20, 21]
    ("shapes", "wide", "hubs"): [(1, 0x1), (32, 0x4e9bf6c7), (32, 0x97f9ffab)],   # kept [1, 20, 24]
    ("shapes", "narrow", "er3000"): [(1, 0x1), (4, 0xd), (4, 0x4)],   # kept [1, 3, 1]
    ("shapes", "narrow", "er1933"): [(1, 0x1), (4, 0xd), (4, 0x4)],   # kept [1, 3, 1]
    ("shapes", "narrow", "sparse"): [(1, 0x1), (4, 0xd), (4, 0x4)],   # kept [1, 3, 1]
    ("shapes", "narrow", "hubs"): [(1, 0x1), (4, 0xd), (4, 0x7)],   # kept [1, 3, 3]
    ("shapes", "odd", "er3000"): [(1, 0x1), (5, 0x6), (9, 0xc7)],   # kept [1, 2, 5]
    ("shapes", "odd", "er1933"): [(1, 0x1), (5, 0x6), (9, 0xc7)],   # kept [1, 2, 5]
    ("shapes", "odd", "sparse"): [(1, 0x1), (5, 0x6), (9, 0xc7)],   # kept [1, 2, 5]
    ("shapes", "odd", "hubs"): [(1, 0x1), (5, 0x6), (9, 0xcf)],   # kept [1, 2, 6]
    ("shapes", "in3", "er3000"): [(3, 0x7), (16, 0xfcb7), (16, 0x997f)],   # kept [3, 12, 11]
    ("shapes", "in3", "er1933"): [(3, 0x7), (16, 0xfcff), (16, 0x9b7f)],   # kept [3, 14, 12]
    ("shapes", "in3", "sparse"): [(3, 0x7), (16, 0xfcf7), (16, 0x9b5d)],   # kept [3, 13, 10]
    ("shapes", "in3", "hubs"): [(3, 0x7), (16, 0xfcf7), (16, 0xbb7f)],   # kept [3, 13, 13]
    ("shapes", "first_trained", "er3000"): [(1, 0x1), (16, 0x3ed9), (20, 0xaf7ef)],   # kept [1, 10, 16]
    ("shapes", "first_trained", "er1933"): [(1, 0x1), (16, 0x3ed9), (20, 0xaf7ef)],   # kept [1, 10, 16]
    ("shapes", "first_trained", "sparse"): [(1, 0x1), (16, 0x3ed9), (20, 0xab6af)],   # kept [1, 10, 13]
    ("shapes", "first_trained", "hubs"): [(1, 0x1), (16, 0x3ed9), (20, 0xef7ef)],   # kept [1, 10, 17]
    ("depths", "mixed", "er3000"): [(1, 0x1), (16, 0xf7e0), (20, 0xd4fc9)],   # kept [1, 10, 12]
    ("depths", "mixed", "er1933"): [(1, 0x1), (16, 0xf7e2), (20, 0xd4fc9)],   # kept [1, 11, 12]
    ("depths", "mixed", "sparse"): [(1, 0x1), (16, 0xf7e2), (20, 0xdcfc8)],   # kept [1, 11, 12]
    ("depths", "mixed", "hubs"): [(1, 0x1), (16, 0xf7ea), (20, 0xdcfc9)],   # kept [1, 12, 13]
    ("depths", "in3_f32", "er3000"): [(3, 0x7), (32, 0xb4cfde35)],   # kept [3, 20]
    ("depths", "in3_f32", "er1933"): [(3, 0x7), (32, 0xfccffe3d)],   # kept [3, 24]
    ("depths", "in3_f32", "sparse"): [(3, 0x7), (32, 0xfdcffebd)],   # kept [3, 26]
    ("depths", "in3_f32", "hubs"): [(3, 0x7), (32, 0xfdcffebd)],   # kept [3, 26]
    ("trained", "model", "er3000"): [(1, 0x1), (16, 0x4dab), (16, 0x8603)],   # kept [1, 9, 5]
    ("trained", "model", "er1933"): [(1, 0x1), (16, 0x4deb), (16, 0x8603)],   # kept [1, 10, 5]
    ("trained", "model", "sparse"): [(1, 0x1), (16, 0x4deb), (16, 0x607)],   # kept [1, 10, 5]
    ("trained", "model", "hubs"): [(1, 0x1), (16, 0x4deb), (16, 0x8647)],   # kept [1, 10, 7]
    ("live", "sparse32", "er3000"): [(1, 0x1), (32, 0x42424242), (32, 0x42400202)],   # kept [1, 8, 5]
    ("live", "sparse32", "er1933"): [(1, 0x1), (32, 0x42424242), (32, 0x42404202)],   # kept [1, 8, 6]
    ("live", "sparse32", "sparse"): [(1, 0x1), (32, 0x42424242), (32, 0x42404202)],   # kept [1, 8, 6]
    ("live", "sparse32", "hubs"): [(1, 0x1), (32, 0x42424242), (32, 0x42404202)],   # kept [1, 8, 6]
}

GRAPHS = ["er3000", "er1933", "sparse", "hubs"]


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    oracle_py.build()
    oracle_py.lib()


@pytest.mark.parametrize("name", list(ml.SPECS))
def test_text_is_pinned(name):
    text = ml.build(name)
    assert text.splitlines()[0] == f"live_{name}_0"
    assert hashlib.sha256(text.encode()).hexdigest() == SHA256[name], name
    om = oracle_py.OracleModel(text)
    assert om.n_layers == ml.num_layers(name)
    assert [W.shape for W, _ in om.linear_params()] == ml.linear_shapes(name)


def test_the_table_of_members_is_the_agreed_one():
    assert list(ml.SPECS) == ["in2", "in16", "in17", "in32", "in33", "in48", "in49", "in64", "sparse32"]
    for w in (2, 16, 17, 32, 33, 48, 49, 64):
        assert ml.SPECS[f"in{w}"] == (w, [(16, 8), (8, 1)])
    assert ml.SPECS["sparse32"] == (1, [(64, 32), (64, 32), (32, 1)])
    assert sorted(ml.DEFAULT_BOUNDS + ml.NEEDS_FEAT) == sorted(ml.SPECS)
    assert len(ml.DEAD_UNITS) == 24 and set(ml.MINUS_ZERO_BIAS) < set(ml.DEAD_UNITS) and len(ml.MINUS_ZERO_BIAS) == 8


def test_sparse32_kills_its_units_in_the_text_the_engine_parses():
    P = oracle_py.OracleModel(ml.build("sparse32")).linear_params()
    wide = [P[1], P[3]]   # the last layers of stages 0 and 1; stage 2's 32-wide layer is a hidden one and keeps its draw
    assert [W.shape for W, _ in wide] == [(64, 32), (64, 32)] and P[4][0].shape == (67, 32)
    assert (bits(P[4][0]) & 0x7FFFFFFF).all()
    for W, b in wide:
        assert not (bits(W[:, ml.DEAD_UNITS]) & 0x7FFFFFFF).any()
        assert (b[ml.DEAD_UNITS] <= 0).all()
        assert (bits(b[ml.MINUS_ZERO_BIAS]) == 0x80000000).all()
        live = [u for u in range(32) if u not in ml.DEAD_UNITS]
        assert (bits(W[:, live]) & 0x7FFFFFFF).any(axis=0).all()


@pytest.mark.parametrize("gname", GRAPHS)
def test_sparse32_dead_units_are_dead_on_the_oracle(gname):
    masks = lh.stage_masks("live", "sparse32", gname)
    dead = sum(1 << u for u in ml.DEAD_UNITS)
    for s in (1, 2):
        f, mask = masks[s]
        assert f == 32 and mask & dead == 0 and 0 < bin(mask).count("1") <= 8, (gname, s, hex(mask))


# ---------------------------------------------------------------- the lemma

@pytest.mark.parametrize("gname", ["er3000", "sparse", "hubs", "one"])
@pytest.mark.parametrize("f", [2, 5, 16, 17, 32, 49, 64])
def test_a_dead_column_sums_to_plus_zero_and_the_others_do_not_notice(gname, f):
    g = graph_of(gname)
    rng = np.random.default_rng([101, f])
    x = crafted_input(g.n, f, 7 + f)
    dead = sorted(rng.choice(f, size=max(1, f // 3), replace=False).tolist())
    for i, c in enumerate(dead):   # +0.0 only, -0.0 only, and the two mixed
        x[:, c] = [np.float32(0.0), np.float32(-0.0)][i % 2] if i % 3 else np.where(rng.random(g.n) < 0.5, np.float32(-0.0), np.float32(0.0))
    live = [c for c in range(f) if c not in dead]
    assert ml.live_mask(x) == sum(1 << c for c in live) or g.n == 1   # (one row: crafted_input's own -0.0 may kill a column more)
    row = oracle_py.graph_layer(g, g.ws, x)
    assert row.shape == (g.n, 2 * f + 3)
    assert not bits(row[:, dead]).any(), "a dead column's neighbour sum is not +0.0f"
    if live:
        packed = oracle_py.graph_layer(g, g.ws, np.ascontiguousarray(x[:, live]))
        assert np.array_equal(bits(row[:, live]), bits(packed[:, :len(live)])), "a live column's chain changed with the dead ones gone"


def test_a_chain_value_is_never_minus_zero():
    """The three facts behind the lemma, on fp32 itself (round to nearest)."""
    z, mz = np.float32(0.0), np.float32(-0.0)
    assert bits(np.array([z + mz, mz + z, z + z], dtype=np.float32)).tolist() == [0, 0, 0]
    v = crafted_input(64, 4, 3).reshape(-1)
    v = v[(bits(v) & 0x7FFFFFFF) != 0]
    assert not bits((v + (-v)).astype(np.float32)).any()                    # x + (-x) = +0
    assert np.array_equal(bits((v + z).astype(np.float32)), bits(v))        # adding +-0 to a non-zero value returns its bits
    assert np.array_equal(bits((v + mz).astype(np.float32)), bits(v))


def test_a_denormal_keeps_its_column_alive():
    x = np.zeros((5, 3), dtype=np.float32)
    x[:, 1] = np.float32(-0.0)
    x.view(np.uint32)[3, 2] = 1   # the smallest denormal
    assert ml.live_mask(x) == 0b100
    assert ml.live_mask(np.zeros((0, 4), dtype=np.float32)) == 0


def test_the_rule():
    assert [ml.used_by_rule(k, 16, 50) for k in (0, 8, 9)] == [1, 1, 0]
    assert ml.used_by_rule(9, 16, 57) == 1 and ml.used_by_rule(9, 16, 56) == 0   # 900 <= 912, 900 > 896
    assert all(ml.used_by_rule(f, f, 100) for f in (2, 16, 17, 32, 33, 64))
    assert all(ml.used_by_rule(0, f, 1) for f in (2, 64))
    assert ml.used_by_rule(1, 64, 1) == 0


# ---------------------------------------------------------------- the masks the GPU tests expect

@pytest.mark.parametrize("key", list(MASKS), ids=lambda k: "-".join(k))
def test_stage_masks_are_pinned(key):
    family, name, gname = key
    got = lh.stage_masks(family, name, gname)
    assert got == MASKS[key], [(f, hex(m)) for f, m in got]
    assert [f for f, _ in got] == [f for f, _ in gh.FAMILIES[family].stage_widths(name)]


def test_the_counts_the_issue_was_opened_with():
    kept = lambda key: [bin(m).count("1") for _, m in MASKS[key]][1:]
    assert kept(("shapes", "wide", "er3000")) == [17, 20]
    assert kept(("shapes", "narrow", "er3000")) == [3, 1]
    assert kept(("shapes", "odd", "er3000")) == [2, 5]
    assert kept(("depths", "in3_f32", "er3000")) == [20]
    assert [kept(("trained", "model", g)) for g in ("er3000", "hubs", "sparse")] == [[9, 5], [10, 7], [10, 5]]
