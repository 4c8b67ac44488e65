"""tools/modelgen_units.py on the oracle: the patterns its models promise really occur in groups of 64 consecutive rows (the
rows a wave of k_stage_f1 / k_dense_f16 holds) on the graphs tests/test_gpu_dense_units.py runs them on."""
import numpy as np
import pytest

from oracle import oracle_py
from tools import graphgen as gg
from tools import modelgen as mg
from tools import modelgen_units as mu
from tools.unit_sparsity import group_live
from tests.test_modelgen import GRAPHS, layer_outputs

# graph 1 and graph 2 of tests/test_gpu_dense_units.py
UNIT_GRAPHS = {"er3000": lambda: gg.erdos_renyi(3000, 15000, 15), "er1933": GRAPHS["er1933"]}


@pytest.fixture(scope="module")
def graphs():
    return {k: f() for k, f in UNIT_GRAPHS.items()}


@pytest.fixture(scope="module")
def hidden(graphs):
    """{(model, graph): [ReLU output of linear layer i, i in 0 .. 7] + [logits]}"""
    out = {}
    for name, make in mu.FAMILY.items():
        om = oracle_py.OracleModel(make())
        assert [W.shape for W, _ in om.linear_params()] == mg.SHAPES
        for gname, g in graphs.items():
            om.set_weight_scale(g.ws)
            pre = layer_outputs(om, g)
            out[name, gname] = [oracle_py.relu(p) for p in pre[:8]] + [pre[8]]
    return out


def test_texts_parse_to_what_was_written():
    for name, make in mu.FAMILY.items():
        om = oracle_py.OracleModel(make())
        assert om.n_layers == 21, name
    _, b2 = oracle_py.OracleModel(mu.neg_zero_bias()).linear_params()[2]
    assert b2[3] == 0 and np.signbit(b2[3])
    _, b3 = oracle_py.OracleModel(mu.neg_zero_bias()).linear_params()[3]
    assert b3[11] == 0 and np.signbit(b3[11])
    W7, _ = oracle_py.OracleModel(mu.inf_weight()).linear_params()[7]
    assert np.isposinf(W7[mu.UNIT, 5]) and np.isfinite(np.delete(W7.ravel(), mu.UNIT * 16 + 5)).all()


@pytest.mark.parametrize("gname", list(UNIT_GRAPHS))
def test_one_row_has_groups_with_a_single_live_row(hidden, graphs, gname):
    """(a) in every feeder, unit UNIT is non-zero exactly on the vertices of weight 120; some group of 64 consecutive rows holds
    exactly one of them (with zeros in its other 63 rows) and some group none; the term matters to that row's output."""
    g = graphs[gname]
    heaviest = np.flatnonzero(g.w == 120)
    assert heaviest.size > 0
    for i in mu.FEEDERS:
        col = hidden["one_row", gname][i][:, mu.UNIT]
        assert np.array_equal(np.flatnonzero(col != 0), heaviest), (gname, i)
        pad = np.concatenate([col != 0, np.zeros((-g.n) % 64, dtype=bool)]).reshape(-1, 64)
        per_group = pad.sum(axis=1)
        assert (per_group == 1).any() and (per_group == 0).any(), (gname, i, np.bincount(per_group))
    for i in mu.SKIPPED:   # the next layer's row of that unit is not zero: a skipped term would change the output
        W, _ = oracle_py.OracleModel(mu.one_row()).linear_params()[i]
        assert (W[mu.UNIT] != 0).any(), i


@pytest.mark.parametrize("gname", list(UNIT_GRAPHS))
def test_all_dead_layers_are_zero_everywhere(hidden, gname):
    """(b) layers 0 and 4 are zero for every row, so layers 1 and 5 give relu(bias) — and the model still tells vertices apart."""
    h = hidden["all_dead", gname]
    params = oracle_py.OracleModel(mu.all_dead()).linear_params()
    for i in (0, 4):
        assert not h[i].any(), (gname, i)
        assert not group_live(h[i]).any()
        b = params[i + 1][1]
        assert (b > 0).any() and (b < 0).any()
        want = np.broadcast_to(oracle_py.relu(b.reshape(1, -1).copy()), h[i + 1].shape)
        assert np.array_equal(h[i + 1].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (gname, i)
    assert (params[0][1] == 0).any() and (params[0][1] < 0).any()
    assert np.isfinite(h[8]).all() and np.unique(h[8]).size > 100, gname


@pytest.mark.parametrize("gname", list(UNIT_GRAPHS))
def test_all_live_feeders_are_positive_everywhere(hidden, gname):
    """(c) every unit of every feeder is non-zero in every row: no group of 64 rows can skip a term."""
    h = hidden["all_live", gname]
    for i in mu.FEEDERS:
        assert (h[i] > 0).all(), (gname, i)
        assert group_live(h[i]).all()
    assert np.isfinite(h[8]).all() and np.unique(h[8]).size > 100, gname


@pytest.mark.parametrize("gname", list(UNIT_GRAPHS))
def test_inf_weight_sits_on_a_dead_unit(hidden, gname):
    """(e) unit UNIT of layer 6 is zero for every row, 0 * inf makes unit 5 of layer 7 — and with it every logit — NaN; h1 and
    h2 are finite."""
    h = hidden["inf_weight", gname]
    assert not h[6][:, mu.UNIT].any()
    assert np.isnan(h[7][:, 5]).all() and np.isfinite(np.delete(h[7], 5, axis=1)).all()
    assert np.isnan(h[8]).all()
    assert np.isfinite(h[2]).all() and np.isfinite(h[5]).all()


@pytest.mark.parametrize("gname", list(UNIT_GRAPHS))
def test_neg_zero_bias_model_is_an_ordinary_one(hidden, gname):
    h = hidden["neg_zero_bias", gname]
    assert np.isfinite(h[8]).all() and np.unique(h[8]).size > 100, gname


def strays(h):
    """k_c4_choose's figure for a 16-column input: the non-zeros outside its four fullest columns."""
    return int(np.sort((h != 0).sum(axis=0))[:-4].sum())


@pytest.mark.parametrize("gname", list(UNIT_GRAPHS))
def test_h1_and_h2_fit_one_four_column_table(hidden, graphs, gname):
    """The compact-table plan takes an input whose non-zeros outside its four fullest columns number at most n / 512
    (k_c4_choose); only then does k_dense_f16 run the stage's dense layers.  Every model here keeps h1 and h2 inside the columns
    LIVE — none outside at all — and has values in them, on er1933 (where tests/test_gpu_dense_units.py engages the plan) too."""
    n = graphs[gname].n
    dead = np.setdiff1d(np.arange(16), mu.LIVE)
    for name in mu.FAMILY:
        for i in (2, 5):
            h = hidden[name, gname][i]
            assert not h[:, dead].any(), (name, gname, i)
            assert strays(h) == 0 and n // 512 >= 0, (name, gname, i)
            assert h.any(), (name, gname, i)


def test_the_fitting_members_of_the_modelgen_family_fit_on_er1933(graphs):
    """live_four and live_pairs (tools/modelgen.py), the random models tests/test_gpu_dense_units.py adds so that hidden layers
    with ordinary weights reach k_dense_f16 as well: within the bound on er1933."""
    g = graphs["er1933"]
    for name in ("live_four", "live_pairs"):
        om = oracle_py.OracleModel(mg.FAMILY[name]())
        om.set_weight_scale(g.ws)
        pre = layer_outputs(om, g)
        for i in (2, 5):
            assert strays(oracle_py.relu(pre[i])) <= g.n // 512, (name, i)


def test_skip_layer_masks_name_the_layers():
    assert mu.SKIP_LAYERS["neg_zero_bias"] == 0o777 - (1 << 2) - (1 << 3)
    assert mu.SKIP_LAYERS["inf_weight"] == 0o777 - (1 << 7)
    assert all(mu.SKIP_LAYERS[m] == 0o777 for m in ("one_row", "all_dead", "all_live"))
