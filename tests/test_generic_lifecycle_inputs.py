"""The inputs of tests/test_gpu_generic_lifecycle.py, pinned on the CPU: what those GPU tests need their graphs, their derive
chain and their models to be in order to test anything.  A generator that changes — a hub graph without rows around the
thresholds, a chain that never puts a new vertex on the heavy list, a METIS text that reads back as another graph — fails here,
where no GPU is needed, instead of quietly turning a lifecycle test into a test of nothing."""
import numpy as np
import pytest

from tools import graphgen as gg
from tests import generic_harness as gh
from tests.generic_harness import degrees, graph_of, heavy_counts

ROUTE_MEMBERS, DERIVE_MEMBERS, SEQUENCE = gh.LIFECYCLE_MEMBERS, gh.DERIVE_MEMBERS, gh.LIFECYCLE_SEQUENCE


def test_the_members_cover_the_widths_and_depths():
    f = {w for fam, name in ROUTE_MEMBERS for w, _ in gh.FAMILIES[fam].stage_widths(name)}
    assert f == {1, 3, 5, 9, 16, 20, 32}   # 1, 3, 5, 9 and 32 (and the trained shape's 16, mixed's 20)
    d = {k for fam, name in ROUTE_MEMBERS for k in gh.FAMILIES[fam].stage_depths(name)}
    assert d == {1, 2, 3, 4, 5}
    assert all(gh.FAMILIES[fam].out_width(name) == 1 for fam, name in ROUTE_MEMBERS)


def test_hubs_has_rows_on_both_sides_of_every_threshold():
    g = graph_of("hubs")
    deg = degrees(g)
    assert (g.n, g.nnz) == (6000, 33718)
    assert sorted(deg)[-8:] == [511, 512, 513, 767, 768, 769, 1025, 3000]
    assert heavy_counts(g, 512)[0] == 7 and heavy_counts(g, 256)[0] == 8
    assert heavy_counts(g, 513)[0] == 6 and heavy_counts(g, 1) == (int((deg > 0).sum()), g.nnz) and heavy_counts(g, 0) == (0, 0)
    assert heavy_counts(g, 600) == (5, 767 + 768 + 769 + 1025 + 3000)
    assert heavy_counts(g, 512)[1] == 512 + 513 + 767 + 768 + 769 + 1025 + 3000


def test_only_hubs_is_heavy_in_the_sequence():
    want = {"hubs": 7, "er1933": 0, "one": 0, "empty": 0, "sparse": 0}
    for gname in SEQUENCE:
        assert heavy_counts(graph_of(gname), 512)[0] == want[gname], gname
    assert graph_of("empty").n == 0 and graph_of("empty").nnz == 0 and graph_of("one").n == 1
    assert [want[a] for a in SEQUENCE] == [7, 0, 7, 0, 0, 0, 7]


def test_the_derive_chain_moves_the_heavy_list():
    chain = gh.derive_chain()
    assert [(g.n, g.nnz) for g, _ in chain] == [(4318, 23490), (2162, 11212), (2162, 11212)]
    assert [int(degrees(g).max()) for g, _ in chain] == [2121, 1061, 1061]
    assert [heavy_counts(g, 512)[0] for g, _ in chain] == [5, 1, 1]
    assert [heavy_counts(g, 256)[0] for g, _ in chain] == [7, 10, 10]
    assert [heavy_counts(g, 600)[0] for g, _ in chain] == [2, 1, 1]
    new = [int((old_row == 0xFFFFFFFF).sum()) for _, old_row in chain]
    assert new == [50, 7, 0]
    # the rise to 10 at threshold 256: fold vertices, whose rows are all tail, land on the heavy list
    g1, old_row = chain[1]
    fresh = old_row == 0xFFFFFFFF
    assert (degrees(g1)[fresh] >= 256).sum() >= 3
    # the last step keeps every vertex and adds none: the same lists derived again, under new weights
    g2, old_row2 = chain[2]
    assert np.array_equal(old_row2, np.arange(g1.n, dtype=np.uint32))
    assert np.array_equal(g2.rowptr, g1.rowptr) and np.array_equal(g2.col, g1.col) and not np.array_equal(g2.w, g1.w)


@pytest.mark.parametrize("gname", ["hubs", "er1933"])
def test_the_metis_text_reads_back_as_the_same_graph(gname):
    g = graph_of(gname)
    back = gg.parse_metis(gg.metis_text(g))
    assert back.n == g.n
    for field in ("rowptr", "col", "w", "nw"):
        assert np.array_equal(getattr(back, field), getattr(g, field)), field
    assert float(g.w.max()) == g.ws   # the scale gnnvc_predict sets: the largest weight


def test_every_adjacency_list_is_ascending():
    graphs = [graph_of(gname) for gname in ("hubs", "er1933", "sparse")] + [g for g, _ in gh.derive_chain()]
    for g in graphs:
        rp = g.rowptr.astype(np.int64)
        inner = np.ones(g.nnz, dtype=bool)
        inner[rp[:-1][rp[:-1] < g.nnz]] = False          # the first entry of a row has no predecessor in it
        step = np.diff(g.col.astype(np.int64), prepend=-1)
        assert (step[inner] > 0).all()


@pytest.mark.parametrize("family,name", DERIVE_MEMBERS)
def test_the_oracles_logits_are_finite_along_the_chain(family, name):
    for step, (g, _) in enumerate(gh.derive_chain()):
        lg = gh.stage_outputs(gh.oracle_of(family, name, g), family, name, g)[-1][2]
        assert lg.shape == (g.n, 1) and np.isfinite(lg).all(), step
        assert np.unique(lg).size > g.n // 100, (step, "the logits do not vary over the vertices")


@pytest.mark.parametrize("family,name", ROUTE_MEMBERS + [("depths", "too_big"), ("big", "odd_wide")])
def test_the_oracles_logits_are_finite_on_hubs(family, name):
    lg = gh.want_of(family, name, "hubs")[-1][2]
    assert np.isfinite(lg).all() and np.unique(lg).size > 60
    lg77 = gh.logits_at(family, name, graph_of("hubs"), ws=77.0)
    assert np.isfinite(lg77).all()
    assert not np.array_equal(gh.bits(lg77), gh.bits(lg)), "another weight scale gives other logits"
    assert np.array_equal(gh.bits(gh.logits_at(family, name, graph_of("hubs"))), gh.bits(lg)), "the oracle's predict is the walk"
