"""The first layer of k_dense_f16 (the dense layers of a 16-wide stage on the compact-table plan), route by route.

A wave of 64 consecutive rows of a call takes route A (no dirty row, no stray vertex of its own: the table's columns and the
row's own terms), route B (dirty rows, whose sixteen sums come from full rows: each of the sixteen terms only where some lane's
value is non-zero) or route C (a stray vertex of its own, or a first layer whose weights do not allow leaving zero terms out:
the 32-term chain from full rows, term by term behind the same test where the weights allow it).  Inputs are built so that
one call holds the wave classes named in CASES; that each input really does so is checked on the CPU, from the graph and the
oracle's neighbour sums alone, before the device is asked.

Graphs: the two smallest on which the plan runs — er1933 with the plans built at hand-off (at most 1933 / 512 = 3 stray values
fit) and erdos_renyi(20000, 200000, 70).  Models: the trained one, live_four, and units_neg_zero_bias, whose stage 1 may not
skip in its first layer (tools/modelgen_units.SKIP_LAYERS: the kernel is handed no table and every wave takes route C with
every term).  Stages 1 and 2 through the stage entry point with "dense_skip_zeros" 1 and 0: bit for bit against the oracle
and against each other; where the oracle's value is NaN (the NaN / inf case) the device's must be NaN, as in
tests/test_gpu_dense_units.py.

"Only dirty rows" in a 64-row group is realised as a call whose last wave holds ONE row, and that row dirty: the lanes past
the call's end are clamped to it, so all 64 lanes of the wave are dirty.  (A full group of 64 dirty rows would need more stray
values than the plan takes on these graphs: n / 512.)

One class cannot be built: a dirty row whose sums are zero in EVERY column outside the table.  A row is dirty because a
neighbour has a non-zero (or NaN) outside the table's columns, the plan only takes inputs without negative values (anything else
clears its descriptor: the "negative" case of test_compact_gather_plan_is_bit_identical), and a sum of values >= 0 with a
positive or NaN addend is not zero.  `one_dirty` is the nearest there is: one extra term of twelve stays, eleven are skipped —
and the CPU check below asserts that no dirty row of any input has all twelve at zero, so that this remark cannot go stale."""
import numpy as np
import pytest

from oracle import oracle_py
from tools import graphgen as gg
from tools import modelgen_units as mu
from tests import test_gpu_models as tm
from tests.test_gpu_models import PLANNED
from tests.test_gpu_parity import _oracle_stage, _sparse_features, bits

pytestmark = pytest.mark.gpu

GRAPHS = {
    "er1933": (lambda: tm.graph_of("er1933"), dict(PLANNED, poison_features=1)),
    "er20000": (lambda: gg.erdos_renyi(20000, 200000, 70), {"blocked_min_n": 0, "poison_features": 1}),
}
MODELS = ["trained", "live_four", "units_neg_zero_bias"]
LIVE = [2, 4, 9, 12]                 # the table's columns: the four fullest of every input below
BELOW, BETWEEN, ABOVE = 1, 6, 14     # stray columns below, between and above them
CASES = ["clean", "one_dirty", "three_columns", "only_dirty", "nan_inf"]
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def texts(model_text):
    tm._cache["text", "trained"] = model_text
    tm._cache["text", "units_neg_zero_bias"] = mu.FAMILY["neg_zero_bias"]()


def graph_of(gname):
    if ("graph", gname) not in _cache:
        _cache["graph", gname] = GRAPHS[gname][0]()
    return _cache["graph", gname]


def neighbours(g, v):
    return g.col[int(g.rowptr[v]): int(g.rowptr[v + 1])].astype(np.int64)


def base_features(g, seed):
    h = _sparse_features(g.n, np.random.default_rng(seed), LIVE, [1.0, 0.3, 0.6, 1.0])
    h[::3, LIVE[1]] = -0.0            # negative zeros in a table column ...
    h[5, BETWEEN] = -0.0              # ... and in a dead one: no stray
    return h


def inputs_of(gname):
    """{case: (h, lo, hi)}"""
    if ("inputs", gname) in _cache:
        return _cache["inputs", gname]
    g = graph_of(gname)
    deg = np.diff(g.rowptr.astype(np.int64))
    out = {}
    out["clean"] = (base_features(g, 1), 0, g.n)
    # one stray vertex of moderate degree, in the middle of the graph
    s = next(int(v) for v in range(g.n // 2, g.n) if 2 <= deg[v] <= 12)
    h = base_features(g, 2)
    h[s, BETWEEN] = 0.75
    out["one_dirty"] = (h, 0, g.n)
    # the same vertex with stray values below, between and above the table's columns: its neighbours' sums are non-zero there
    h = base_features(g, 3)
    h[s, BELOW], h[s, BETWEEN], h[s, ABOVE] = 0.5, 1.25, 3.0
    out["three_columns"] = (h, 0, g.n)
    # a call whose last wave is one row, and that row dirty: every lane of the wave recomputes it
    last = next(r for r in range((g.n * 2 // 3) // 64 * 64, g.n, 64) if deg[r] > 0 and (neighbours(g, r) // 64 != r // 64).any())
    nb = neighbours(g, last)
    h = base_features(g, 4)
    h[int(nb[nb // 64 != last // 64][0]), ABOVE] = 2.0
    out["only_dirty"] = (h, 0, last + 1)
    # a NaN and an inf in stray columns: their terms stay
    t = next(int(v) for v in range(g.n // 3, g.n) if 2 <= deg[v] <= 12 and v // 64 != s // 64)
    h = base_features(g, 5)
    h[s, BETWEEN] = np.nan
    h[t, ABOVE] = np.inf
    out["nan_inf"] = (h, 0, g.n)
    _cache["inputs", gname] = out
    return out


def wave_classes(g, h, lo, hi):
    """Per 64-row group of the call: has it a stray vertex of its own, how many of its rows are dirty, how many rows."""
    dead = [c for c in range(16) if c not in LIVE]
    stray = (h[:, dead] != 0).any(axis=1)            # (NaN != 0: a NaN is a stray, a negative zero is none)
    rp = g.rowptr.astype(np.int64)
    hits = np.concatenate(([0], np.cumsum(stray[g.col[: rp[-1]]])))
    dirty = hits[rp[1:]] > hits[rp[:-1]]
    waves = []
    for a in range(lo, hi, 64):
        b = min(a + 64, hi)
        waves.append((bool(stray[a:b].any()), int(dirty[a:b].sum()), b - a))
    return waves, stray, dirty


def test_inputs_hold_the_wave_classes():
    """CPU only (the oracle's layer functions): each input produces the classes its name promises."""
    for gname in GRAPHS:
        g = graph_of(gname)
        dead = [c for c in range(16) if c not in LIVE]
        for case, (h, lo, hi) in inputs_of(gname).items():
            counts = (h != 0).sum(axis=0)
            assert sorted(sorted(range(16), key=lambda c: (-int(counts[c]), c))[:4]) == LIVE, (gname, case)
            assert int((h[:, dead] != 0).sum()) <= g.n // 512, (gname, case, "more stray values than the plan takes")
            assert not (h < 0).any(), (gname, case)
            assert (hi - lo) * 2 >= g.n, (gname, case, "too short a call for the plan")
            waves, stray, dirty = wave_classes(g, h, lo, hi)
            agg = oracle_py.graph_layer(g, g.ws, np.ascontiguousarray(h))[:, :16]
            extra = agg[:, dead]
            # (see the module text) a dirty row always has a non-zero sum outside the table's columns
            assert ((extra[dirty] != 0).any(axis=1)).all(), (gname, case)
            if case == "clean":
                assert all(w == (False, 0, w[2]) for w in waves)
                assert (np.signbit(h) & (h == 0)).any()
            else:
                assert any(st for st, _, _ in waves), (gname, case, "no route C wave")
            if case == "one_dirty":
                assert any(not st and d == 1 and n == 64 for st, d, n in waves), (gname, case)
                assert any(not st and d == 0 for st, d, n in waves)
            if case == "three_columns":
                b_rows = [r for r in np.flatnonzero(dirty[lo:hi]) + lo if not waves[(r - lo) // 64][0]]
                assert b_rows and all((agg[r, [BELOW, BETWEEN, ABOVE]] != 0).all() for r in b_rows), (gname, case)
            if case == "only_dirty":
                assert waves[-1] == (False, 1, 1), (gname, case, waves[-1])
            if case == "nan_inf":
                b_rows = [r for r in np.flatnonzero(dirty[lo:hi]) + lo if not waves[(r - lo) // 64][0]]
                assert any(np.isnan(agg[r, BETWEEN]) for r in b_rows) and any(np.isinf(agg[r, ABOVE]) for r in b_rows), (gname, case)


def want_of(name, gname, case, stage):
    key = ("want", name, gname, case, stage)
    if key not in _cache:
        g = graph_of(gname)
        h, lo, hi = inputs_of(gname)[case]
        with np.errstate(all="ignore"):
            _cache[key] = _oracle_stage(tm.oracle_of(name), g, stage, h)[lo:hi]
    return _cache[key]


def run_stage(e, g, stage, h, lo, hi):
    import torch
    dev = torch.device("cuda:0")
    hin = torch.zeros((g.n + 1, 16), dtype=torch.float32, device=dev)
    hin[: g.n] = torch.from_numpy(h).to(dev)
    out = torch.full((g.n + 1, 16 if stage == 1 else 1), 7.0, dtype=torch.float32, device=dev)
    lg = torch.full((g.n + 1, 1), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    e.stage_forward_device(stage, lo, hi, hin.data_ptr(), out.data_ptr(), lg.data_ptr() if stage == 2 else 0)
    e.synchronize()
    got = (out if stage == 1 else lg).cpu().numpy()
    assert (got[hi:] == 7.0).all(), "rows behind the call were written"
    return got[lo:hi]


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_first_layer_routes_are_bit_identical(name, gname):
    g = graph_of(gname)
    seen = {}
    for skip in (1, 0):
        e = tm.open_engine(name, g, dict(GRAPHS[gname][1], dense_skip_zeros=skip))
        try:
            first_layer_may_skip = (e.get_info("dense_skip_layers") >> 3) & 1     # stage 1, dense layer 1
            assert first_layer_may_skip == (0 if name == "units_neg_zero_bias" else 1), name
            for rep in range(3):   # (the plans are built at hand-off or in the second forward)
                _, lg = e.forward(g.x())
                assert np.array_equal(bits(lg[:, 0]), bits(_logits(name, gname))), (name, gname, rep)
            assert e.get_info("compact_gather_active") == 1, (name, gname)
            for case, (h, lo, hi) in inputs_of(gname).items():
                for stage in (1, 2):
                    got = run_stage(e, g, stage, h, lo, hi)
                    assert e.get_info("compact_gather_last_passes") == 1, (name, gname, case, stage, "the plan did not take this input")
                    if case != "clean":
                        assert e.get_info("compact_gather_last_dirty") > 0, (name, gname, case, stage)
                    else:
                        assert e.get_info("compact_gather_last_dirty") == 0, (name, gname, case, stage)
                    want = want_of(name, gname, case, stage)
                    nan = np.isnan(want)
                    if case != "nan_inf":
                        assert not nan.any(), (name, gname, case, stage)
                    assert np.array_equal(np.isnan(got), nan), (name, gname, case, stage, skip, "NaN positions")
                    same = (bits(got) == bits(want)) | nan
                    assert same.all(), (name, gname, case, stage, skip, f"{int((~same).sum())} values differ, first (row, column)",
                                        np.argwhere(~same)[:6].tolist())
                    seen[skip, case, stage] = got
        finally:
            e.close()
    for (skip, case, stage), got in seen.items():
        if skip == 1:
            assert np.array_equal(bits(got), bits(seen[0, case, stage])), (name, gname, case, stage, "dense_skip_zeros 1 against 0")


def _logits(name, gname):
    if ("logits", name, gname) not in _cache:
        g, om = graph_of(gname), tm.oracle_of(name)
        om.set_weight_scale(g.ws)
        _cache["logits", name, gname] = om.logits(g)
    return _cache["logits", name, gname]
