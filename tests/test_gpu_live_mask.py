"""The liveness mask the VALU dense kernels hand from layer to layer, and the compact-table emit taken from compares.

k_stage_f1<.., MFMA = false> and k_dense_f16 decide which terms of a hidden layer's chains run from a wave-uniform mask that the
ReLU of the layer before built out of its own compares (bit set: !(t < 0) in some lane; relu_live / dense_live in
csrc/gnnvc_kernels.hip), and their epilogues count the non-zeros of the output columns and flag stray vertices from sixteen
ballots (c4_emit_regs).  Everything here is bit for bit against the oracle, with "dense_skip_zeros" 1 and 0; where the oracle's
value is NaN the device's must be NaN.

Stage calls: erdos_renyi(20000, 200000, 70) with the options of tests/test_gpu_dense_routes.py (plus "wide_tiles" 0, so that
stage 0 runs k_stage_f1 at every call size).  Models: the trained one, live_four, units_neg_zero_bias (its -0.0 biases keep two
layers' skip off) and tools/modelgen_mask.mask_units, whose feeders each hold a unit that is exactly +0.0 before the ReLU in every
row (live for the mask, dead for a test of the values), one that is negative in every row and one that is exactly 0 in one row
in a hundred and negative in the others — asserted on the oracle's pre-activations below.  Row ranges of 64, 65 and 129 rows and
plan-sized ranges of 64 k + 1 rows (the last wave holds one row, its other lanes are clamped to it); stage 0 with a NaN and an
inf in x, stages 1 and 2 with the inputs of test_gpu_dense_routes (clean, dirty rows, a last wave of one dirty row, NaN / inf in
stray columns, which reach the first layer's pre-activations through the dirty rows' sums and make every hidden unit NaN).

Emit: whole forwards on er1933 with the plans at hand-off, the smallest graph on which the suite runs the compact-table plan (at
most 1933 / 512 = 3 stray values fit), under tools/modelgen_mask.emit_strays with its two degrees picked from the graph: h1 and
h2 have stray non-zeros outside the table's columns and h2 a NaN in one of them.  Every logit against the oracle (a vertex
k_stage_f1 failed to flag would cost its neighbours a term of stage 1), and "compact_gather_last_dirty" of the last stage equal to
the number of rows with a flagged neighbour in the oracle's h2."""
import numpy as np
import pytest

from oracle import oracle_py
from tools import modelgen_mask as mm
from tools import modelgen_units as mu
from tests import test_gpu_dense_routes as dr
from tests import test_gpu_models as tm
from tests.test_gpu_models import PLANNED
from tests.test_gpu_parity import _oracle_stage, bits
from tests.test_gpu_round_counters import fullest_columns
from tests.test_modelgen import layer_outputs

pytestmark = pytest.mark.gpu

GNAME = "er20000"
OPTS = dict(dr.GRAPHS[GNAME][1], wide_tiles=0)
MODELS = dr.MODELS + ["mask_units"]
SMALL = [(0, 64), (0, 65), (0, 129)]
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def texts(model_text):
    tm._cache["text", "trained"] = model_text
    tm._cache["text", "units_neg_zero_bias"] = mu.FAMILY["neg_zero_bias"]()
    tm._cache["text", "mask_units"] = mm.mask_units()


def one_row_ranges(n):
    """Plan-sized calls (at least half of the rows) of 64 k + 1 rows, from the first row and from somewhere inside a wave."""
    a = (n * 3 // 4) // 64 * 64 + 1
    b = (n * 2 // 3) // 64 * 64 + 1
    return [(0, a), (n - 37 - b, n - 37)]


def x_inputs(g):
    """{name: x}: the driver's input, and the same with a NaN in the first wave of the graph and an inf in the second."""
    x = np.ascontiguousarray(g.x(), dtype=np.float32).reshape(g.n)
    odd = x.copy()
    odd[10] = np.nan
    odd[70] = np.inf
    return {"x": x, "nan_inf": odd}


def want_of(name, stage, key, h):
    if ("want", name, stage, key) not in _cache:
        g = dr.graph_of(GNAME)
        with np.errstate(all="ignore"):
            _cache["want", name, stage, key] = _oracle_stage(tm.oracle_of(name), g, stage, h.reshape(g.n, -1))
    return _cache["want", name, stage, key]


def run_stage0(e, g, x, lo, hi):
    import torch
    dev = torch.device("cuda:0")
    xin = torch.zeros(g.n + 1, dtype=torch.float32, device=dev)
    xin[: g.n] = torch.from_numpy(x).to(dev)
    out = torch.full((g.n + 1, 16), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    e.stage_forward_device(0, lo, hi, xin.data_ptr(), out.data_ptr(), 0)
    e.synchronize()
    got = out.cpu().numpy()
    assert (got[:lo] == 7.0).all() and (got[hi:] == 7.0).all(), "rows outside the call were written"
    return got[lo:hi]


def check(got, want, label, need_nan=False):
    nan = np.isnan(want)
    assert nan.any() or not need_nan, (label, "no NaN reaches this range: the case checks nothing")
    assert np.array_equal(np.isnan(got), nan), (label, "NaN positions")
    same = (bits(got) == bits(want)) | nan
    assert same.all(), (label, f"{int((~same).sum())} values differ, first (row, column)", np.argwhere(~same)[:6].tolist())


def test_mask_units_hold_what_they_promise():
    """CPU only (the oracle's layer functions)."""
    g = dr.graph_of(GNAME)
    om = tm.oracle_of("mask_units")
    om.set_weight_scale(g.ws)
    pre = layer_outputs(om, g)
    for i in mu.FEEDERS:
        p = pre[i]
        assert (bits(p[:, mm.ZERO]) == 0).all(), (i, "not +0.0 in every row")
        assert (p[:, mm.NEG] < 0).all(), i
        zero = p[:, mm.MIX] == 0
        assert 0 < int(zero.sum()) <= g.n // 50 and (p[~zero, mm.MIX] < 0).all(), (i, int(zero.sum()))
        groups = zero[: g.n // 64 * 64].reshape(-1, 64).sum(axis=1)
        assert (groups == 1).any() and (groups == 0).any(), i    # a wave with one such row, and waves with none
    for h in (oracle_py.relu(pre[2]), oracle_py.relu(pre[5])):
        assert fullest_columns(h) == list(mu.LIVE) and not (h[:, [c for c in range(16) if c not in mu.LIVE]] != 0).any()


@pytest.mark.parametrize("name", MODELS)
def test_stage_calls_are_bit_identical(name):
    g = dr.graph_of(GNAME)
    om = tm.oracle_of(name)
    om.set_weight_scale(g.ws)
    logits = om.logits(g)
    xs = x_inputs(g)
    cases = dr.inputs_of(GNAME)
    for skip in (1, 0):
        e = tm.open_engine(name, g, dict(OPTS, dense_skip_zeros=skip))
        try:
            may = {"units_neg_zero_bias": mu.SKIP_LAYERS["neg_zero_bias"]}.get(name, mu.ALL_LAYERS)
            assert e.get_info("dense_skip_layers") == may, name
            for rep in range(3):   # (the plans are built in the second forward)
                _, lg = e.forward(g.x())
                assert np.array_equal(bits(lg[:, 0]), bits(logits)), (name, skip, rep)
            assert e.get_info("compact_gather_active") == 1, name
            # stage 0: k_stage_f1
            for key, x in xs.items():
                want = want_of(name, 0, key, x)
                for lo, hi in SMALL + [(g.n - 129, g.n)] + one_row_ranges(g.n) + [(0, g.n)]:
                    check(run_stage0(e, g, x, lo, hi), want[lo:hi], (name, skip, 0, key, lo, hi),
                          need_nan=key == "nan_inf" and lo == 0)
            # stages 1 and 2: k_dense_f16 where the call is plan-sized, the gathering kernel below that
            for case, (h, lo, hi) in cases.items():
                ranges = [(lo, hi)]
                if case in ("clean", "nan_inf"):
                    ranges += SMALL + one_row_ranges(g.n)
                for stage in (1, 2):
                    want = want_of(name, stage, case, h)
                    for a, b in ranges:
                        got = dr.run_stage(e, g, stage, h, a, b)
                        if (b - a) * 2 >= g.n:
                            assert e.get_info("compact_gather_last_passes") == 1, (name, case, stage, a, b, "the plan did not take this call")
                        check(got, want[a:b], (name, skip, stage, case, a, b), need_nan=case == "nan_inf" and (a, b) == (lo, hi))
        finally:
            e.close()


def flagged_rows(h, cols):
    """What the emit flags: a non-zero outside the table's columns, or a table value that is not >= 0 (NaN, negative)."""
    other = [c for c in range(16) if c not in cols]
    with np.errstate(invalid="ignore"):
        return (h[:, other] != 0).any(axis=1) | ~(h[:, cols] >= 0).all(axis=1)


def rows_with_a_flagged_neighbour(g, flagged):
    rp = g.rowptr.astype(np.int64)
    hits = np.concatenate(([0], np.cumsum(flagged[g.col[: rp[-1]]])))
    return hits[rp[1:]] > hits[rp[:-1]]


def test_emit_counts_and_flags_in_whole_forwards():
    g = tm.graph_of("er1933")
    deg = np.diff(g.rowptr.astype(np.int64))
    heavy = np.asarray(g.w) == g.ws
    assert heavy.any()
    d_low = max(d for d in range(int(deg.max()) + 1) if int((heavy & (deg <= d)).sum()) <= g.n // 512)
    d_high = int(deg[heavy].max())
    assert d_high > d_low and (heavy & (deg <= d_low)).any(), (d_low, d_high)
    tm._cache["text", "emit_strays"] = mm.emit_strays(d_low, d_high)
    om = tm.oracle_of("emit_strays")
    om.set_weight_scale(g.ws)
    with np.errstate(all="ignore"):
        pre = layer_outputs(om, g)
        h1, h2 = oracle_py.relu(pre[2]), oracle_py.relu(pre[5])
        logits = om.logits(g)
    live = list(mu.LIVE)
    other = [c for c in range(16) if c not in live]
    for h in (h1, h2):   # what the model promises, on the CPU first
        with np.errstate(invalid="ignore"):
            assert fullest_columns(h) == live and 0 < int((h[:, other] != 0).sum()) <= g.n // 512 and not (h < 0).any()
        assert not np.isnan(h[:, other]).any()
    assert not np.isnan(h1).any() and np.isnan(h2[:, live]).any()
    expect = int(rows_with_a_flagged_neighbour(g, flagged_rows(h2, live)).sum())
    strays_only = (h2[:, other] != 0).any(axis=1)
    assert expect > int(rows_with_a_flagged_neighbour(g, strays_only).sum()) > 0     # (the NaN row's neighbours count too)
    assert np.isnan(logits).any()
    for skip in (1, 0):
        e = tm.open_engine("emit_strays", g, dict(PLANNED, poison_features=1, dense_skip_zeros=skip))
        try:
            for rep in range(3):   # (the third forward gathers from the table the second one's kernels emitted)
                _, lg = e.forward(g.x())
                check(lg[:, 0], logits, ("emit_strays", skip, rep))
            assert e.get_info("compact_gather_active") == 1
            assert e.get_info("compact_gather_last_passes") == 1 and e.get_info("compact_table_written_by_producer") == 1
            got = e.get_info("compact_gather_last_dirty")
            assert got == expect, (skip, got, expect)
        finally:
            e.close()
