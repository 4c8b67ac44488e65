"""Whole forwards in which the compact-table plan's producers leave out full feature rows (csrc/gnnvc_kernels.hip: kSkipElide,
GNNVC_ELIDE_ROWS; DESIGN.md section 5, "Elided rows").

Inside a whole forward k_stage_f1 and k_dense_f16 store a wave's 64-byte rows only if one of the table rows the wave writes
carries a flag, once the host has seen the consumer take the producer's table as written.  What still reads full rows then
reads a vertex's table row first (k_c4_fix, k_dense_f16's route C), and a forward whose choice of columns does not take the
table has k_c4_compact put every row back before anything gathers.  Every forward here runs with "poison_features" 1, so a
row nobody wrote is NaN when it is read; every logit is compared bit for bit with the oracle's, NaN for NaN, and
gnnvc_get_info "elided_row_stages_last_forward" is asserted at every step, so that no case passes without elision.
(Scores: the NaN positions are the oracle's and every other one is within 1 ulp of it, the suite's rule for the device's exp
against the host's libm — tests/test_gpu_parity.check_forward.  A score is sigmoid(logit) of a logit that is checked bit for
bit, so nothing of the elided path can hide inside that ulp; bit equality of the scores with the host's libm does not hold
for the parent commit either.)

Graphs: the two smallest the plan runs on (tests/test_gpu_dense_routes.py).  Model: tools/modelgen_elide.gated — h1 and h2
keep to four columns, a few vertices carry a stray value, h2 a NaN in a table column, and the INPUT decides h1's live columns.
Inputs (INPUTS) and what each does to the stage inputs is proved on the CPU first, from the oracle's stage outputs
(test_inputs_hold_the_scenarios).  The sequence on one engine (STEPS): steady state with strays; an input that changes stage 1's
four fullest columns (the forward expands and re-compacts, the next one does not elide for that stage, later ones do); an input
with a fifth live column (falls off the plan: the gathering kernel runs on expanded rows); an audited forward in between
(read-out 0, audit clean, elision back afterwards); NaN and inf in x.  The expected read-out of every step comes from a mirror
of the rule (Mirror): a producer elides iff the last forward's k_c4_choose took its table as written.  Two more cases: a model
whose stage 1 may not skip in its first layer (only stage 2's input is elided) and a graph with long rows (none is).

Mutants (local builds, not kept): a k_c4_fix that takes an unflagged neighbour's values from the wrong table column, and a
k_c4_compact that skips the expansion; profiles/elided_rows/README.md records how many cases fail against each."""
import numpy as np
import pytest

from oracle import oracle_py
from tools import modelgen_elide as me
from tools import modelgen_mask as mm
from tools import modelgen_units as mu
from tests import generic_harness as gh
from tests import test_gpu_dense_routes as dr
from tests import test_gpu_models as tm
from tests.test_gpu_models import PLANNED
from tests.test_gpu_parity import bits
from tests.test_gpu_round_counters import fullest_columns
from tests.test_modelgen import layer_outputs

pytestmark = pytest.mark.gpu

GRAPHS = {name: (make, dict(opts, verdict_period=1)) for name, (make, opts) in dr.GRAPHS.items()}
WARM = 6        # forwards after which the plans are built, a table has been taken as written and its verdict has arrived
_cache = {}


def degrees_for(g):
    """emit_strays' two degrees for this graph, as tests/test_gpu_live_mask.py picks them."""
    deg = np.diff(g.rowptr.astype(np.int64))
    heavy = np.asarray(g.w) == g.ws
    d_low = max(d for d in range(int(deg.max()) + 1) if int((heavy & (deg <= d)).sum()) <= g.n // 512)
    d_high = int(deg[heavy].max())
    assert d_high > d_low and (heavy & (deg <= d_low)).any(), (d_low, d_high)
    return d_low, d_high


def model_of(name, gname):
    key = name if name != "gated" else f"gated_{gname}"
    if ("text", key) not in tm._cache:
        if name == "gated":
            tm._cache["text", key] = me.gated(*degrees_for(dr.graph_of(gname)))
        elif name == "units_neg_zero_bias":
            tm._cache["text", key] = mu.FAMILY["neg_zero_bias"]()
    return key


def inputs_of(gname):
    """{name: x}: the driver's input; zeros (column GATED of h1 dies); threes (column EXTRA comes alive in every row); the driver's
    with a NaN and an inf at two vertices of low degree in different 64-row groups."""
    if ("inputs", gname) not in _cache:
        g = dr.graph_of(gname)
        deg = np.diff(g.rowptr.astype(np.int64))
        x = np.ascontiguousarray(g.x(), dtype=np.float32).reshape(g.n)
        odd = x.copy()
        low = int(deg[deg > 0].min())
        a = next(int(v) for v in range(g.n // 2, g.n) if deg[v] == low)
        b = next(int(v) for v in range(g.n // 4, g.n) if 0 < deg[v] <= low + 1 and v // 64 != a // 64 and v != a)
        odd[a], odd[b] = np.nan, np.inf
        _cache["inputs", gname] = {"x": x, "zeros": np.zeros_like(x), "threes": np.full_like(x, 3.0), "nan_inf": odd}
    return _cache["inputs", gname]


def oracle_run(key, gname, xname):
    """(h1, h2, logits, scores) of the oracle for one input, computed once."""
    if ("run", key, gname, xname) not in _cache:
        g, om = dr.graph_of(gname), tm.oracle_of(key)
        om.set_weight_scale(g.ws)
        x = inputs_of(gname)[xname] if xname in inputs_of(gname) else None
        if xname == "other":
            x = tm.other_input(g).reshape(g.n)
        with np.errstate(all="ignore"):
            pre = layer_outputs(om, g, x=x)
            _cache["run", key, gname, xname] = (oracle_py.relu(pre[2]), oracle_py.relu(pre[5]), pre[8][:, 0].copy(), om.scores(g, x))
    return _cache["run", key, gname, xname]


def choice(h, n):
    """k_c4_choose on a stage input: (the four fullest columns, does it fit one table) — a NaN counts as a non-zero."""
    cols = fullest_columns(h)
    other = [c for c in range(16) if c not in cols]
    with np.errstate(invalid="ignore"):
        return tuple(cols), int((h[:, other] != 0).sum()) <= n // 512


def flagged_rows(h, cols):
    """The vertices whose table row carries a flag: a non-zero outside the table's columns, or a value in them that is not >= 0."""
    other = [c for c in range(16) if c not in cols]
    with np.errstate(invalid="ignore"):
        return (h[:, other] != 0).any(axis=1) | ~(h[:, list(cols)] >= 0).all(axis=1)


class Mirror:
    """The host rule, restated: after a forward, stage s's producer may elide in the NEXT one iff k_c4_choose found the producer's
    statistics complete, the input fit for one table, and the table in place written for exactly the columns it chose."""

    def __init__(self, n, allowed):
        self.n, self.allowed = n, allowed
        self.spec = {1: None, 2: None}        # the columns the next forward's producer writes its table for (None: no valid spec)
        self.steady = {1: False, 2: False}

    def expect(self, audited):
        return 0 if audited else sum(1 for s in (1, 2) if self.steady[s] and self.allowed[s])

    def forward(self, h1, h2):
        emitted = True                        # (stage 0's kernel always counts; stage 1's only when the plan ran stage 1)
        for s, h in ((1, h1), (2, h2)):
            cols, fits = choice(h, self.n)
            fits = fits and emitted
            self.steady[s] = fits and self.spec[s] == cols
            self.spec[s] = cols if fits else None
            emitted = fits


# (label, input, audited, the read-out the scenario is about — None: whatever the mirror says, asserted all the same)
STEPS = [("steady", "x", False, 2), ("steady again", "x", False, 2),
         ("choice changes", "zeros", False, 2), ("back: withdrawn for stage 1", "x", False, 1), ("table rewritten", "x", False, 1),
         ("fits again", "x", False, 2),
         ("falls off the plan", "threes", False, 2), ("after the fall", "x", False, 0), ("spec again", "x", False, None),
         ("settling", "x", False, None), ("settled", "x", False, 2),
         ("audited", "x", True, 0), ("after the audit", "x", False, 2),
         ("nan and inf", "nan_inf", False, 2), ("after them", "x", False, None), ("and on", "x", False, None),
         ("and on", "x", False, None), ("steady at the end", "x", False, 2)]


def test_inputs_hold_the_scenarios():
    """CPU only (the oracle's layer functions): each input does to the stage inputs what the sequence needs."""
    for gname in GRAPHS:
        g = dr.graph_of(gname)
        key = model_of("gated", gname)
        rp = g.rowptr.astype(np.int64)
        h1, h2, logits, _ = oracle_run(key, gname, "x")
        assert np.isnan(logits).any() and not np.isnan(logits).all(), gname
        for s, h in ((1, h1), (2, h2)):
            cols, fits = choice(h, g.n)
            assert cols == tuple(mu.LIVE) and fits and not (h < 0).any(), (gname, s, cols)
            flag = flagged_rows(h, cols)
            groups = [flag[a:a + 64] for a in range(0, g.n, 64)]
            assert flag.any() and any(not f.any() for f in groups), (gname, s, "a stray vertex and a group without any")
            # route C with lanes that are not flagged: a group that holds a flagged vertex and others
            assert any(f.any() and not f.all() for f in groups), (gname, s)
            # k_c4_fix reads a rebuilt row: a dirty row (a flagged neighbour) with an unflagged neighbour in a group that stored nothing
            elided_group = np.repeat([not f.any() for f in groups], 64)[: g.n]
            found = False
            for u in _dirty(g, flag):
                nb = g.col[rp[u]: rp[u + 1]]
                if (~flag[nb] & elided_group[nb]).any():
                    found = True
                    break
            assert found, (gname, s)
        assert np.isnan(h2[:, list(mu.LIVE)]).any() and not np.isnan(h1).any(), gname
        # zeros: another four columns for stage 1, and they fit
        z1, z2, _, _ = oracle_run(key, gname, "zeros")
        assert choice(z1, g.n)[0] != tuple(mu.LIVE) and choice(z1, g.n)[1] and (z1[:, me.GATED] == 0).all(), (gname, choice(z1, g.n))
        assert choice(z2, g.n)[1], gname
        # threes: a fifth live column — stage 1's input does not fit
        t1, _, _, _ = oracle_run(key, gname, "threes")
        assert not choice(t1, g.n)[1] and (t1[:, me.EXTRA] != 0).all(), gname
        # NaN and inf reach a table column and a stray column of h1
        o1, _, ologits, _ = oracle_run(key, gname, "nan_inf")
        other = [c for c in range(16) if c not in mu.LIVE]
        assert np.isnan(o1[:, list(mu.LIVE)]).any() and (np.isnan(o1[:, other]).any() or np.isinf(o1[:, other]).any()), gname
        assert np.isinf(o1).any() or np.isnan(o1).sum() > 16, gname
        assert np.isnan(ologits).any(), gname
        # the literal read-outs of STEPS are what the mirror gives for these inputs
        m = Mirror(g.n, {1: True, 2: True})
        for _ in range(WARM):
            m.forward(h1, h2)
        for label, xname, audited, literal in STEPS:
            assert literal is None or m.expect(audited) == literal, (gname, label, m.expect(audited), literal)
            a, b, _, _ = oracle_run(key, gname, xname)
            m.forward(a, b)


def _dirty(g, flag):
    rp = g.rowptr.astype(np.int64)
    hits = np.concatenate(([0], np.cumsum(flag[g.col[: rp[-1]]])))
    return np.flatnonzero(hits[rp[1:]] > hits[rp[:-1]])


class Runner:
    """Whole forwards on device buffers (gnnvc_forward_device), compared with the oracle bit for bit."""

    def __init__(self, e, g):
        import torch
        self.torch, self.e, self.g = torch, e, g
        dev = torch.device("cuda:0")
        self.x = torch.zeros(g.n + 1, dtype=torch.float32, device=dev)
        self.sc = torch.zeros(g.n + 1, dtype=torch.float32, device=dev)
        self.lg = torch.zeros(g.n + 1, dtype=torch.float32, device=dev)

    def forward(self, x, want_logits, want_scores, label):
        torch = self.torch
        self.x[: self.g.n] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32).reshape(self.g.n)).to(self.x.device)
        self.sc.fill_(7.0)
        self.lg.fill_(7.0)
        torch.cuda.synchronize()
        self.e.forward_device(self.x.data_ptr(), self.sc.data_ptr(), self.lg.data_ptr())
        self.e.synchronize()
        lg, sc = self.lg.cpu().numpy()[: self.g.n], self.sc.cpu().numpy()[: self.g.n]
        nan = np.isnan(want_logits)
        assert np.array_equal(np.isnan(lg), nan), (label, "NaN positions of the logits")
        same = (bits(lg) == bits(want_logits)) | nan
        assert same.all(), (label, f"{int((~same).sum())}/{self.g.n} logits differ, first rows", np.flatnonzero(~same)[:6].tolist())
        assert np.array_equal(np.isnan(sc), np.isnan(want_scores)), (label, "NaN positions of the scores")
        d = np.abs(bits(sc).view(np.int32).astype(np.int64) - bits(want_scores).view(np.int32).astype(np.int64))
        assert d[~nan].max(initial=0) <= 1, (label, "scores")   # (device exp against the host's libm: one ulp, as everywhere)
        return self.e.get_info("elided_row_stages_last_forward")


def warm_up(run, key, gname, full):
    h1, h2, logits, scores = oracle_run(key, gname, "x")
    seen = [run.forward(inputs_of(gname)["x"], logits, scores, (gname, "warm-up", rep)) for rep in range(WARM)]
    assert seen[0] == 0, (gname, seen, "a graph's first forward must not elide")
    assert seen[-1] == full and seen == sorted(seen), (gname, seen)
    return seen


@pytest.mark.parametrize("gname", list(GRAPHS))
def test_elided_rows_sequence(gname):
    g = dr.graph_of(gname)
    key = model_of("gated", gname)
    e = tm.open_engine(key, g, GRAPHS[gname][1])
    try:
        run = Runner(e, g)
        warm_up(run, key, gname, 2)
        assert e.get_info("compact_gather_active") == 1 and e.get_info("compact_table_written_by_producer") == 1, gname
        h1, h2, _, _ = oracle_run(key, gname, "x")
        m = Mirror(g.n, {1: True, 2: True})
        for _ in range(WARM):
            m.forward(h1, h2)
        for step, (label, xname, audited, literal) in enumerate(STEPS):
            a, b, logits, scores = oracle_run(key, gname, xname)
            want = m.expect(audited)
            assert literal is None or want == literal
            if audited:
                e.set_option("audit_period", 1)
            got = run.forward(inputs_of(gname)[xname], logits, scores, (gname, step, label))
            if audited:
                e.set_option("audit_period", 0)
                assert e.get_info("audit_failures") == 0 and e.get_info("audit_runs") >= 3, (gname, label, e.audit_report())
            print(gname, step, label, xname, "elided stages:", got, "expected:", want)
            assert got == want, (gname, step, label, got, want)
            m.forward(a, b)
    finally:
        e.close()


@pytest.mark.parametrize("gname", list(GRAPHS))
def test_a_consumer_that_may_not_skip_gets_every_row(gname):
    """units_neg_zero_bias: stage 1's first layer may not leave out zero terms, its dense kernel is handed no table and reads every
    own row — stage 0 never elides; stage 2 may skip, and stage 1's kernel elides for it."""
    g = dr.graph_of(gname)
    key = model_of("units_neg_zero_bias", gname)
    e = tm.open_engine(key, g, GRAPHS[gname][1])
    try:
        assert (e.get_info("dense_skip_layers") >> 3) & 1 == 0 and (e.get_info("dense_skip_layers") >> 6) & 1 == 1
        run = Runner(e, g)
        warm_up(run, key, gname, 1)
        _, _, logits, scores = oracle_run(key, gname, "other")
        assert run.forward(tm.other_input(g), logits, scores, (gname, "other input")) == 1
        _, _, logits, scores = oracle_run(key, gname, "x")
        assert run.forward(inputs_of(gname)["x"], logits, scores, (gname, "back")) == 1
    finally:
        e.close()


def test_a_graph_with_long_rows_never_elides():
    g = gh.graph_of("hubs")
    assert (np.diff(g.rowptr.astype(np.int64)) >= 512).sum() == 7
    om = tm.oracle_of("live_four")
    om.set_weight_scale(g.ws)
    logits, scores = om.logits(g), om.scores(g)
    e = tm.open_engine("live_four", g, dict(PLANNED, poison_features=1, verdict_period=1))
    try:
        run = Runner(e, g)
        for rep in range(WARM):
            assert run.forward(g.x(), logits, scores, ("hubs", rep)) == 0, rep
    finally:
        e.close()
