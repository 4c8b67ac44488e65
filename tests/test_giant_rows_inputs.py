"""The graph and the crafted inputs of tests/test_gpu_giant_rows.py (tools/giant_rows_inputs.py, and crafted_input of
tests/generic_harness.py) are what that test needs — proven here on the CPU: the hubs' degrees, that the oracle adds a row in
stored order, and that the input made for the integer route of the exact scan really walks it: many binades, exact ties, one
large jump per hub, and a sum that tells the stored order from the reversed one."""
import numpy as np
import pytest

from oracle import oracle_py
from tools import giant_rows_inputs as gi
from tests.generic_harness import bits, crafted_input

WIDTHS = (3, 32)       # stages 0 and 1 of the model in3_f32


@pytest.fixture(scope="module")
def g():
    return gi.hub_graph()


def inputs(g, f):
    return {"a": crafted_input(g.n, f, 300 + f), "b": gi.scan_input(g, f, 200 + f)}


def test_the_degrees_are_exactly_the_listed_ones(g):
    deg = np.diff(g.rowptr.astype(np.int64))
    assert g.n == gi.HUB_N == 12000
    assert deg[:8].tolist() == gi.HUB_DEGREES == [1023, 1024, 1025, 2049, 4096, 4097, 9000, 0]
    assert deg[8:].max() < 64, "only the hubs are heavy at the thresholds from 64 on"
    assert g.col[: int(g.rowptr[8])].min() >= 8, "a hub's neighbours are among the other vertices"
    for thr, rows in ((1024, 6), (1025, 5), (4097, 2), (16384, 0)):
        assert int((deg >= thr).sum()) == rows
    assert int((deg >= 512).sum()) == 7
    for h in range(8):   # without replacement: no neighbour twice, stored ascending
        assert (np.diff(gi.neighbours(g, h)) > 0).all()


@pytest.mark.parametrize("f", WIDTHS)
def test_the_oracle_adds_every_hub_in_stored_order(g, f):
    for which, hin in inputs(g, f).items():
        agg = oracle_py.graph_layer(g, g.ws, hin)
        for h in range(8):
            assert np.array_equal(bits(agg[h, :f]), bits(gi.chain(g, h, hin))), (which, f, h)


@pytest.mark.parametrize("f", WIDTHS)
def test_input_a_has_both_signs_and_minus_zero(g, f):
    hin = inputs(g, f)["a"]
    assert (hin < 0).any() and (hin > 0).any() and (bits(hin) == 0x80000000).any()
    fwd, rev = gi.chain(g, gi.BIG_HUB, hin), gi.chain(g, gi.BIG_HUB, hin, reverse=True)
    assert (bits(fwd) != bits(rev)).any()


@pytest.mark.parametrize("f", WIDTHS)
def test_input_b_walks_the_integer_route(g, f):
    hin = inputs(g, f)["b"]
    assert not (hin < 0).any() and np.isfinite(hin).all()
    assert (bits(hin) == 0x80000000).any() and (bits(hin) == 0).any(), "zeros of both signs"
    den = (bits(hin) & 0x7F800000) == 0
    assert (den & ((bits(hin) & 0x7FFFFF) != 0)).any(), "a few denormals"
    # values m * 2^e, e from -24 to 20 (the spikes and the denormals aside): every value is a multiple of 2^-24 below 2^45
    normal = hin[~den & (hin < np.float32(2.0 ** 44))].astype(np.float64)
    assert (np.ldexp(normal, 24) == np.floor(np.ldexp(normal, 24))).all()
    facts = gi.chain_facts(g, gi.BIG_HUB, hin)
    assert len(gi.neighbours(g, gi.BIG_HUB)) == 9000
    rev = gi.chain(g, gi.BIG_HUB, hin, reverse=True)
    assert (bits(facts["sum"]) != bits(rev)).any(), "the input does not tell the stored order from the reversed one"
    assert (facts["binades"] >= 8).all(), facts["binades"]
    assert (facts["ties"] >= 1).all(), facts["ties"]
    for h in range(7):   # every non-empty hub: one add that lifts its accumulator several binades at once
        assert (gi.chain_facts(g, h, hin)["jump"] >= gi.SPIKE_LIFT - 1).all(), h
