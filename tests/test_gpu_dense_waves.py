"""The dense kernels of the metric route after they were slimmed for more waves per SIMD (tests/test_kernel_waves.py holds the
figures): k_stage_f1 with the output tile as its only LDS on the LDS-table route, and k_dense_f16's route C in three groups of
terms over one set of accumulators.  Everything is bit for bit against the oracle, with "dense_skip_zeros" 1 and 0; where the
oracle's value is NaN the device's must be NaN.

Stage 0: er1933 under PLANNED plus "wide_tiles" 0 and "poison_features" 1, the smallest graph on which the suite has the
LDS-table plan; the trained model and tools/modelgen_mask.mask_units; the stage entry point over the whole range and over the
two plan-sized ranges of 64 k + 1 rows (the last wave holds one row, its clamped lanes recompute it).  With the driver's input
the sums arrive complete and the kernel's gather loop runs no trip ("lds_table_last_ok" 1); with an input that is no k / ws
(x * 0.999, and x with a NaN and an inf) the same kernel gathers with its indices straight from the adjacency
("lds_table_last_ok" 0).  Four whole forwards with such an input: the bits hold in each and the plan is off at the end.  With
"mfma_dense" 1 the route keeps the full-region matrix-core instantiation (the kernel trace names the launch) and the bits.

Stages 1 and 2: the inputs of tests/test_gpu_dense_routes.py on both of its graphs and under its three models
(units_neg_zero_bias: every wave takes route C with every term), and one more on er20000, `full_strays`: two vertices that are
neighbours of each other carry non-zeros in all twelve dead columns (24 stray values where the plan admits 20000 / 512 = 39).
Each is a stray vertex AND a dirty row (its neighbour is a stray), so their waves take route C with dirty rows in them, their
own rows have all 32 first-layer inputs non-zero, and the waves of their other neighbours are dirty without a stray.  Such a
vertex is always dirty itself, so this input cannot hold a wave with a stray and no dirty row: that class is asserted on
`one_dirty`, and the three classes (stray only, stray and dirty, dirty only) over the calls of er20000 together."""
import numpy as np
import pytest

from oracle import oracle_py
from tools import modelgen_mask as mm
from tools import modelgen_units as mu
from tests import test_gpu_dense_routes as dr
from tests import test_gpu_live_mask as lm
from tests import test_gpu_models as tm
from tests.test_gpu_models import PLANNED
from tests.test_gpu_parity import _oracle_stage, bits

pytestmark = pytest.mark.gpu

STAGE0_GRAPH = "er1933"
STAGE0_OPTS = dict(PLANNED, wide_tiles=0, poison_features=1)
STAGE0_MODELS = ["trained", "mask_units"]
SLIM_LAUNCH = "k_stage_f1<32, 32, 16, 4, false, GNNVC_STAGE0_SLIM"     # (launch sites as the kernel trace spells them)
MFMA_LAUNCH = "k_stage_f1<32, 32, 16, 4, true>"
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def texts(model_text):
    tm._cache["text", "trained"] = model_text
    tm._cache["text", "units_neg_zero_bias"] = mu.FAMILY["neg_zero_bias"]()
    tm._cache["text", "mask_units"] = mm.mask_units()


# ---------------------------------------------------------------- stage 0: the slim k_stage_f1

def stage0_inputs(g):
    """{name: (x, fits the table)}"""
    xs = lm.x_inputs(g)
    return {"x": (xs["x"], 1), "x0999": ((xs["x"] * np.float32(0.999)).astype(np.float32), 0), "nan_inf": (xs["nan_inf"], 0)}


def stage0_want(name, key, x):
    if ("want0", name, key) not in _cache:
        g = tm.graph_of(STAGE0_GRAPH)
        om = tm.oracle_of(name)
        om.set_weight_scale(g.ws)
        with np.errstate(all="ignore"):
            _cache["want0", name, key] = _oracle_stage(om, g, 0, x.reshape(g.n, 1))
    return _cache["want0", name, key]


def logits_want(name, key, x):
    if ("logits", name, key) not in _cache:
        g = tm.graph_of(STAGE0_GRAPH)
        om = tm.oracle_of(name)
        om.set_weight_scale(g.ws)
        with np.errstate(all="ignore"):
            _cache["logits", name, key] = om.logits(g, x)
    return _cache["logits", name, key]


def stage0_ranges(n):
    return [(0, n)] + lm.one_row_ranges(n)


def stage0_calls(e, g, name, label):
    for key, (x, fits) in stage0_inputs(g).items():
        want = stage0_want(name, key, x)
        for lo, hi in stage0_ranges(g.n):
            got = lm.run_stage0(e, g, x, lo, hi)      # (asserts that rows outside the call are untouched)
            assert e.get_info("lds_table_last_ok") == fits, (label, key, lo, hi)
            lm.check(got, want[lo:hi], (label, key, lo, hi), need_nan=key == "nan_inf" and lo == 0)


@pytest.mark.parametrize("name", STAGE0_MODELS)
def test_stage0_on_the_lds_table_route(name):
    g = tm.graph_of(STAGE0_GRAPH)
    x = stage0_inputs(g)["x"][0]
    x2 = stage0_inputs(g)["x0999"][0]
    for skip in (1, 0):
        e = tm.open_engine(name, g, dict(STAGE0_OPTS, dense_skip_zeros=skip, kernel_trace=1))
        try:
            assert e.get_info("lds_table_active") == 1 and e.get_info("mfma_dense") != 1, (name, skip)   # (1: stage 0 on the matrix cores)
            _, lg = e.forward(x)
            assert np.array_equal(bits(lg[:, 0]), bits(logits_want(name, "x", x))), (name, skip)
            assert e.get_info("lds_table_last_ok") == 1, (name, skip)
            names = [n for n, _ in e.kernel_trace(4096)]
            assert any(SLIM_LAUNCH in n for n in names) and not any(MFMA_LAUNCH in n for n in names), names
            stage0_calls(e, g, name, (name, skip))
            assert e.get_info("lds_table_off") == 0, (name, skip, "stage calls are no verdicts")
            # whole forwards with an input the table does not hold: the slim kernel gathers until the plan steps aside
            want2 = logits_want(name, "x0999", x2)
            for rep in range(4):
                _, lg = e.forward(x2)
                assert np.array_equal(bits(lg[:, 0]), bits(want2)), (name, skip, rep)
            assert e.get_info("lds_table_off") == 1, (name, skip)
        finally:
            e.close()


def test_stage0_on_the_matrix_cores_keeps_the_full_region():
    name = "trained"
    g = tm.graph_of(STAGE0_GRAPH)
    x = stage0_inputs(g)["x"][0]
    e = tm.open_engine(name, g, dict(STAGE0_OPTS, mfma_dense=1, kernel_trace=1))
    try:
        assert e.get_info("lds_table_active") == 1 and e.get_info("mfma_dense") == 1
        _, lg = e.forward(x)
        assert np.array_equal(bits(lg[:, 0]), bits(logits_want(name, "x", x)))
        assert e.get_info("lds_table_last_ok") == 1
        names = [n for n, _ in e.kernel_trace(4096)]
        assert any(MFMA_LAUNCH in n for n in names) and not any(SLIM_LAUNCH in n for n in names), names
        stage0_calls(e, g, name, (name, "mfma"))
    finally:
        e.close()


# ---------------------------------------------------------------- stages 1 and 2: route C in groups

def full_strays(g):
    """(h, lo, hi, u, v): u and v are neighbours, both with non-zeros in every dead column and in every table column."""
    deg = np.diff(g.rowptr.astype(np.int64))
    dead = [c for c in range(16) if c not in dr.LIVE]
    u, v = next((int(a), int(b)) for a in range(g.n // 2, g.n) if 2 <= deg[a] <= 12
                for b in dr.neighbours(g, a) if 2 <= deg[b] <= 12 and b // 64 != a // 64)
    h = dr.base_features(g, 6)
    for i, w in enumerate((u, v)):
        h[w, dead] = np.float32(0.25) * (np.arange(12, dtype=np.float32) + 1 + i)
        h[w, dr.LIVE] = np.float32(0.5) + np.arange(4, dtype=np.float32)
    return h, 0, g.n, u, v


def cases_of(gname):
    """The inputs of test_gpu_dense_routes, and `full_strays` on er20000."""
    if ("cases", gname) not in _cache:
        out = dict(dr.inputs_of(gname))
        if gname == "er20000":
            out["full_strays"] = full_strays(dr.graph_of(gname))[:3]
        _cache["cases", gname] = out
    return _cache["cases", gname]


def check_full_strays():
    """CPU only: the new input holds what the module text says."""
    g = dr.graph_of("er20000")
    h, lo, hi, u, v = full_strays(g)
    dead = [c for c in range(16) if c not in dr.LIVE]
    counts = (h != 0).sum(axis=0)
    assert sorted(sorted(range(16), key=lambda c: (-int(counts[c]), c))[:4]) == dr.LIVE
    assert int((h[:, dead] != 0).sum()) == 24 <= g.n // 512
    assert not (h < 0).any()
    x0 = oracle_py.graph_layer(g, g.ws, np.ascontiguousarray(h))[:, :32]      # the first layer's inputs in k order
    assert (x0[[u, v]] != 0).all(), "a row with all 32 inputs non-zero"
    waves, stray, dirty = dr.wave_classes(g, h, lo, hi)
    assert stray[u] and stray[v] and dirty[u] and dirty[v] and int(stray.sum()) == 2
    assert waves[u // 64][:1] == (True,) and waves[u // 64][1] >= 1 and waves[v // 64][1] >= 1 and u // 64 != v // 64
    assert any(not st and d > 0 for st, d, _ in waves), "no wave of dirty rows without a stray"
    # the three classes over the calls of this graph (a stray with a stray neighbour is dirty itself: see the module text)
    seen = set()
    for case, (hh, a, b) in cases_of("er20000").items():
        for st, d, _ in dr.wave_classes(g, hh, a, b)[0]:
            seen.add((st, d > 0))
    assert {(True, False), (True, True), (False, True)} <= seen, seen
    assert any(st and d == 0 for st, d, _ in dr.wave_classes(g, *dr.inputs_of("er20000")["one_dirty"])[0])


def test_full_strays_holds_the_wave_classes():
    check_full_strays()


def stage_want(name, gname, case, stage):
    key = ("want", name, gname, case, stage)
    if key not in _cache:
        g = dr.graph_of(gname)
        h, lo, hi = cases_of(gname)[case]
        with np.errstate(all="ignore"):
            _cache[key] = _oracle_stage(tm.oracle_of(name), g, stage, h)[lo:hi]
    return _cache[key]


@pytest.mark.parametrize("name", dr.MODELS)
@pytest.mark.parametrize("gname", list(dr.GRAPHS))
def test_route_c_in_groups_is_bit_identical(name, gname):
    g = dr.graph_of(gname)
    if gname == "er20000":
        check_full_strays()
    tm.oracle_of(name).set_weight_scale(g.ws)
    seen = {}
    for skip in (1, 0):
        e = tm.open_engine(name, g, dict(dr.GRAPHS[gname][1], dense_skip_zeros=skip))
        try:
            for rep in range(3):   # (the plans are built at hand-off or in the second forward)
                _, lg = e.forward(g.x())
                assert np.array_equal(bits(lg[:, 0]), bits(dr._logits(name, gname))), (name, gname, rep)
            assert e.get_info("compact_gather_active") == 1, (name, gname)
            for case, (h, lo, hi) in cases_of(gname).items():
                for stage in (1, 2):
                    got = dr.run_stage(e, g, stage, h, lo, hi)
                    assert e.get_info("compact_gather_last_passes") == 1, (name, gname, case, stage, "the plan did not take this input")
                    lm.check(got, stage_want(name, gname, case, stage), (name, gname, case, stage, skip), need_nan=case == "nan_inf")
                    seen[skip, case, stage] = got
        finally:
            e.close()
    for (skip, case, stage), got in seen.items():
        if skip == 1:
            assert np.array_equal(bits(got), bits(seen[0, case, stage])), (name, gname, case, stage, "dense_skip_zeros 1 against 0")
