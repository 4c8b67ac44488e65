"""tools/modelgen_fuzz.py, the case table of the generic path's fuzz (tests/test_gpu_generic_fuzz.py), on the CPU: conditions that
keep the fuzz from hiding a failure, not measurements.

  a. the table is pinned: a SHA-256 over the texts of cases 0 .. N - 1 and the exact count of cases that no setting admits;
  b. the walk is the oracle: for every admitted case the stage-by-stage walk (tests/fuzz_harness.walk_case) ends in the bits of
     predict over all layers on the case's graph — for the other cases predict alone is the expectation;
  c. liveness: every case's output is finite, at least half of its columns (at least one) take more than one value over the
     vertices, every intermediate stage output has a column that varies; at most one case in eight carries a reseed, none above
     7.  A case drawn onto a graph of fewer than 64 vertices (n = 0, 1 and 13, where "varies over the vertices" says nothing or
     next to nothing) is judged on er1933 as well as run on its own graph;
  d. coverage: from the records' predicted routes, every specialisation of k_stage_any and its launchers named below (AT_LEAST_THREE) is
     reached by at least three admitted cases, every listed pair by at least one, and every edge value of the width sets occurs;
  e. the route restatement reproduces the figures the big, feat and patterns families' own tests pin;
  f. sensitivity: the oracle's walk of a stage on the crafted input changes bits when two neighbours of the hub rows swap places,
     for every gather variant — so the crafted-input comparison on the GPU is not satisfied by any summation order."""
import dataclasses
import hashlib

import numpy as np
import pytest

from tools import modelgen_big as mb
from tools import modelgen_feat as mf
from tools import modelgen_fuzz as mz
from tools import modelgen_generic as mg
from tools import modelgen_patterns as mp
from tests import fuzz_harness as fh
from tests import generic_harness as gh
from tests.generic_harness import bits, graph_of
from tests.test_modelgen_feat import LDS_BYTES as FEAT_LDS_BYTES
from tests.test_modelgen_patterns import LDS_BYTES as PATTERNS_LDS_BYTES

# ---------------------------------------------------------------- a. the pinned table

TABLE_SHA256 = "4ecc0d3e34081419da13126df04c54535a27d8a940efcfdbcf8e594b0c9cea26"
NOT_ADMITTED = 37
LAST = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
HIDDEN = LAST + [65, 66, 96, 97, 113, 127, 128]

CASES = list(range(mz.N)) + list(mz.REGRESSIONS)
ADMITTED = [i for i in CASES if mz.case(i).admitted]


def test_the_table_is_the_pinned_one():
    assert mz.N == 240 and mz.LAST == LAST and mz.HIDDEN == HIDDEN
    assert mz.TAG not in {m.tag for m in gh.FAMILIES.values()} | {mf.family.tag, mp.TAG} and mz.TAG > 9   # (1 .. 9: tools/modelgen.py, _units)
    assert mz.HEAVY == [0, 1, 17, 64, 512] and mz.GIANT == [None, 1024, 2048] and mz.SEGMENTS == [-1, 0, 1]
    assert mz.GRAPH_NAMES == ["er1933", "sparse", "hubs", "one", "empty", "tiny13", "rounds"]
    assert all(i >= mz.N for i in mz.REGRESSIONS)
    h = hashlib.sha256()
    for i in range(mz.N):
        t = mz.text(i)
        assert t.splitlines()[0] == f"fuzz_{i}_{mz.SEEDS.get(i, 0)}"
        h.update(t.encode())
    assert h.hexdigest() == TABLE_SHA256
    odd = [i for i in range(mz.N) if not mz.case(i).admitted]
    assert len(odd) == NOT_ADMITTED and 0.10 * mz.N <= len(odd) <= 0.20 * mz.N
    assert {mz.case(i).kind for i in odd} == set(mz.KINDS[1:]), "a kind of not-admitted case that no case is"


def test_the_graphs_are_the_named_ones():
    d = lambda name: gh.degrees(graph_of(name))
    assert graph_of("er1933").n == 30 * 64 + 13 and graph_of("one").n == 1 and graph_of("empty").n == 0
    assert (d("sparse") == 0).sum() > 500
    assert d("hubs")[:9].tolist() == gh.HUB_DEGREES
    assert graph_of("tiny13").n == 13 and d("tiny13")[12] == 0 and d("tiny13").max() == 5
    assert graph_of("rounds").n == mz.ROUNDS_N == 777 and d("rounds")[:9].tolist() == mz.ROUND_DEGREES == [15, 16, 17, 31, 32, 33, 63, 64, 65]
    assert d("rounds")[9:].max() < 15
    assert max(graph_of(name).n for name in mz.GRAPH_NAMES) <= 6000


def test_no_setting_admits_the_not_admitted_cases_and_the_least_setting_is_the_least():
    for i in CASES:
        c = mz.case(i)
        if not c.admitted:
            continue
        least = mz.least_config(c.in_width, c.prologue, c.stages, c.ending)
        model = (c.in_width, c.prologue, c.stages, c.ending)
        assert mz.expect(*model, *least) is not None, i
        mask, feat, big = least
        assert c.mask & mask == mask and c.feature_width >= feat and c.big_lds >= big, i
        for bit in (1, 2):   # every part of the least setting is needed
            if mask & bit:
                assert mz.expect(*model, mask & ~bit, feat, big) is None, i
        if feat:
            assert feat >= 33 and mz.expect(*model, mask, feat - 1 if feat > 33 else 0, big) is None, i
        if big:
            assert mz.expect(*model, mask, feat, big - 1 if big > mz.SMALL_LDS else 0) is None, i
        # no drawn model is the trained shape, which keeps its own plans
        assert not (c.in_width == 1 and c.prologue is None and [tuple(s) for s in c.stages] == [(32, 32, 16), (32, 32, 16), (32, 16, 1)])


# ---------------------------------------------------------------- b. the walk is the oracle, c. liveness

def _alive(i, gname):
    dead = fh.dead(i, gname)
    assert dead is None, (mz.describe(i), gname, dead)


@pytest.mark.parametrize("block", range(8))
def test_walk_equals_predict_and_every_case_is_alive(block):
    for i in CASES[block::8]:
        c = mz.case(i)
        g = graph_of(c.graph)
        final = fh.final_of(i, c.graph)
        assert final.shape == (g.n, c.out_width) and np.isfinite(final).all(), mz.describe(i)
        if c.admitted:
            st = fh.want_of(i, c.graph)
            assert [(a.shape[1], b.shape[1]) for a, b, _ in st] == [(r.f, r.widths[-1]) for r in c.expect], mz.describe(i)
            assert np.array_equal(bits(st[-1][1]), bits(final)), (mz.describe(i), "the walk's last stage against predict over all layers")
            if c.sigmoid_end:
                assert np.array_equal(bits(st[-1][2]), bits(fh.logits_of(i, c.graph))), (mz.describe(i), "the walk's logits")
        _alive(i, fh.live_graph_of(c))


def test_reseeds_stay_rare():
    assert all(0 <= i < mz.N or i in mz.REGRESSIONS for i in mz.SEEDS) and all(1 <= s <= 7 for s in mz.SEEDS.values())
    assert len(mz.SEEDS) <= len(CASES) // 8


# ---------------------------------------------------------------- d. coverage

def _fclass(f):
    return "f=1" if f == 1 else "f=2..16" if f <= 16 else "f=17..32" if f <= 32 else "f=33..48" if f <= 48 else "f=49..64"


def classes_of(i):
    """(classes, pairs) that the admitted case i reaches, from its record's predicted route."""
    c = mz.case(i)
    g = graph_of(c.graph)
    (heavy, _), (giant, _) = fh.rows_present(c)
    rows = (["light rows only"] if not heavy else []) + (["heavy rows"] if heavy > giant else []) + (["giant rows"] if giant else [])
    out, pairs = set(), set()
    ns = len(c.expect)
    for s, r in enumerate(c.expect):
        d = len(r.widths)
        form = "default" if not (r.big or r.feat) else f"BIG {r.threads}" if not r.feat else "FEAT default bounds" if not r.big else "FEAT with BIG"
        if r.dense:
            pairs.add("dense stage x " + ("FEAT" if r.feat else "BIG" if r.big else "default"))
            if r.feat and r.big:
                pairs.add("dense stage x BIG")
            if d == 6:
                out.add("a prologue of 6")
        else:
            out.add("form " + form)
            if g.n:
                out.add("gather " + _fclass(r.f))
                pairs |= {f"gather {_fclass(r.f)} x {w}" for w in rows}
        out.add(f"depth {d} in stage 0" if s == 0 else f"depth {d} in a later stage")
        k = r.f if r.dense else 2 * r.f + 3
        for l, n in enumerate(r.widths):
            out.add("K < 4" if k < 4 else f"K mod 4 = {k % 4}, K >= 4")
            if k == 131:
                out.add("K = 131")
            if l + 1 < d:
                out.add(f"hidden {n}")
                out.add(f"hidden T = {(n + 15) // 16}" if n <= 64 else "hidden 65..128, a multiple of 16" if n % 16 == 0 else "hidden 65..128, no multiple of 16")
                if n == 1:
                    out.add("a hidden layer of width 1")
            else:
                out.add(f"last or input width {n}")
            k = n
    out.add(f"last or input width {c.in_width}")
    last = c.expect[-1]
    if last.end == mz.END_NONE:
        out.add(f"ending none, last-layer T = {(last.widths[-1] + 15) // 16}")
    elif last.end == mz.END_RELU:
        out.add("ending relu")
    elif c.out_width > 32:
        out.add("ending sigmoid, out_width > 32")
    out.add(f"{ns} stages" if ns < 4 else "4 stages or more")
    if all(r.dense for r in c.expect):
        out.add("no graph stage")
    if ns >= 2:
        if g.n == 0:
            out.add("n = 0 with a multi-stage model")
        elif g.n == 1:
            out.add("n = 1 with a multi-stage model")
        elif g.n < 16:
            out.add("n < 16 with a multi-stage model")
        if g.n > 16 and g.n % 64:
            out.add("n no multiple of 64 with a multi-stage model")
    return out, pairs


F_CLASSES = ["f=1", "f=2..16", "f=17..32", "f=33..48", "f=49..64"]
AT_LEAST_THREE = (
    [f"gather {f}" for f in F_CLASSES]
    + ["form default", "form BIG 1024", "form BIG 512", "form BIG 256", "form FEAT default bounds", "form FEAT with BIG"]
    + [f"ending none, last-layer T = {t}" for t in (1, 2, 3, 4)] + ["ending relu", "ending sigmoid, out_width > 32"]
    + [f"hidden T = {t}" for t in (1, 2, 3, 4)] + ["hidden 65..128, a multiple of 16", "hidden 65..128, no multiple of 16", "a hidden layer of width 1"]
    + ["K < 4", "K = 131"] + [f"K mod 4 = {r}, K >= 4" for r in range(4)]
    + [f"depth {d} in stage 0" for d in range(1, 7)] + [f"depth {d} in a later stage" for d in range(1, 7)]
    + ["1 stages", "2 stages", "3 stages", "4 stages or more", "no graph stage", "a prologue of 6"]
    + ["n = 0 with a multi-stage model", "n = 1 with a multi-stage model", "n < 16 with a multi-stage model", "n no multiple of 64 with a multi-stage model"])
AT_LEAST_ONE = ([f"gather {f} x {w}" for f in F_CLASSES for w in ("light rows only", "heavy rows", "giant rows")]
                + [f"dense stage x {w}" for w in ("default", "BIG", "FEAT")])
EVERY_VALUE = [f"last or input width {v}" for v in LAST] + [f"hidden {v}" for v in HIDDEN]


def test_the_cases_reach_every_specialisation():
    count, pairs = {}, set()
    for i in ADMITTED:
        got, p = classes_of(i)
        pairs |= p
        for k in got:
            count[k] = count.get(k, 0) + 1
    missing = [f"{k}: {count.get(k, 0)} cases, 3 needed" for k in AT_LEAST_THREE if count.get(k, 0) < 3]
    missing += [f"{k}: no case" for k in AT_LEAST_ONE if k not in pairs]
    missing += [f"{k}: no case" for k in EVERY_VALUE if k not in count]
    assert not missing, "classes that the fuzz does not reach:\n  " + "\n  ".join(missing)


def test_the_cases_run_under_guard_bands_reach_what_they_are_pinned_for():
    """tests/test_gpu_guard_bands.py runs a short list of these cases, and of tests/test_gpu_fuzz.py's, with guard bands around
    every engine buffer: the lists are chosen for the kernels and list sizes they reach, which their records show here."""
    from tests import test_gpu_guard_bands as gb
    assert len(gb.GENERIC_CASES) <= 24 and len(set(gb.GENERIC_CASES)) == len(gb.GENERIC_CASES)
    assert all(0 <= i < mz.N for i in gb.GENERIC_CASES)
    reached = set().union(*(gb.generic_case_covers(i) for i in gb.GENERIC_CASES))
    want = ({"BIG 256", "BIG 512", "BIG 1024", "FEAT", "OPEN", "dense prologue", "heavy 1", "heavy 17", "heavy 512",
             "giant 1024 with segments 1", "not admitted"} | {f"graph {name}" for name in mz.GRAPH_NAMES})
    assert not want - reached, sorted(want - reached)
    assert len(gb.GENERIC_MULTI) == 6 and set(gb.GENERIC_MULTI) <= set(gb.GENERIC_CASES) & set(ADMITTED)
    assert len(gb.PLAN_CASES) == 8 and len(gb.PLAN_STAGE_CASES) == 4 and set(gb.PLAN_STAGE_CASES) <= set(gb.PLAN_CASES)
    assert {case: gb.plan_case_covers(case) for case in gb.PLAN_CASES} == gb.PLAN_COVERS   # what the list says of each case
    reached = set().union(*gb.PLAN_COVERS.values())
    want = {"plan_chunk_rows 16", "plan_chunk_rows 48", "giant_segments 1", "lds_table_skewed_rows > 0", "compact_gather 1",
            "table_tiles 1 at table_tiles_min_n 0", "mfma_dense 0", "mfma_dense 1", "mfma_dense 2"}
    assert not want - reached, sorted(want - reached)


# ---------------------------------------------------------------- e. the restatement of the route

def test_the_route_restatement_gives_the_agreed_figures():
    full = mz.FULL_LDS
    for name, want in gh.LDS_BYTES.items():   # tools/modelgen_big.py
        f, stages = mb.SPECS[name]
        ex = mz.expect(f, None, stages, "sigmoid", 0, 0, full)
        assert (ex is not None) == (name in mb.ADMITTED), name
        assert mz.expect(f, None, stages, "sigmoid") is None, name
        got = [mz.route(0, sf, ws, 1 if s + 1 == len(stages) else 0, s + 1 == len(stages), 0, 0, full)
               for s, ((sf, _), ws) in enumerate(zip(mb.stage_widths(name), stages))]
        assert [r.lds_bytes for r in got if r is not None] == [b for b in want if b <= full], name
        if ex is not None:
            assert [r.threads for r in ex] == [mg.stage_threads(sf, ws, full) for (sf, _), ws in zip(mb.stage_widths(name), stages)], name
            assert [r.big for r in ex] == [not mg.stage_is_small(sf, ws) for (sf, _), ws in zip(mb.stage_widths(name), stages)], name
    for name, want in FEAT_LDS_BYTES.items():   # tools/modelgen_feat.py
        f, stages = mf.SPECS[name]
        ex = mz.expect(f, None, stages, "sigmoid", 0, 64, full)
        assert (ex is not None) == (name != "f65"), name
        assert mz.expect(f, None, stages, "sigmoid", 0, 0, full) is None, name
        assert (mz.expect(f, None, stages, "sigmoid", 0, 64, 0) is not None) == (name in mf.ADMITTED), name
        if ex is not None:
            assert [r.lds_bytes for r in ex] == want, name
            assert [r.threads for r in ex] == [mf.stage_threads_feat(sf, ws, full) for (sf, _), ws in zip(mf.stage_widths(name), stages)], name
            assert any(r.feat for r in ex), name
    assert [r.threads for r in mz.expect(1, None, mf.SPECS["big_f64"][1], "sigmoid", 0, 64, full)] == [256, 512, 256]
    for name in mp.ADMITTED:   # tools/modelgen_patterns.py
        f, pro, stages, ending = mp.SPECS[name]
        ex = mz.expect(f, pro, stages, ending, 3, 64, full)
        assert [r.lds_bytes for r in ex] == PATTERNS_LDS_BYTES[name] == mp.lds_bytes(name), name
        assert [r.threads for r in ex] == mp.stage_threads(name, full), name
        assert [(r.dense, r.f, r.widths, r.end) for r in ex] == mp.stages_of(name), name
        feat, big = (64 if name in mp.NEEDS_FEAT else 0), (full if name in mp.NEEDS_BIG else 0)
        for mask in range(4):
            assert (mz.expect(f, pro, stages, ending, mask, feat, big) is not None) == mp.admitted_by(name, mask), (name, mask)
        assert mz.least_config(f, pro, stages, ending)[0] == mp.MASK[name], name
        assert mz.sequence_of(pro, stages, ending) == mp.sequence(name).split(), name


# ---------------------------------------------------------------- f. sensitivity

@pytest.mark.parametrize("fclass", F_CLASSES)
def test_the_walk_on_the_crafted_input_sees_a_swapped_pair_of_addends(fclass):
    """The oracle's walk of a graph stage on generic_harness.crafted_input, on `rounds` and on `rounds` with the first and the last
    neighbour of every hub row exchanged: the hub rows' outputs differ in bits for at least one of the first cases of the class."""
    g = graph_of("rounds")
    col = np.array(g.col, copy=True)
    rp = g.rowptr.astype(np.int64)
    for hub in range(len(mz.ROUND_DEGREES)):
        a, b = rp[hub], rp[hub + 1] - 1
        col[a], col[b] = col[b], col[a]
    swapped = dataclasses.replace(g, col=col)
    tried = 0
    for i in ADMITTED:
        c = mz.case(i)
        stages = [s for s in fh.graph_stage_indices(c) if _fclass(c.expect[s].f) == fclass]
        if not stages:
            continue
        s = stages[0]
        hin = gh.crafted_input(g.n, c.expect[s].f, [mz.TAG, i, s])
        (_, out, _), = fh.walk_case(i, g, x=hin, first=s, count=1)
        (_, out2, _), = fh.walk_case(i, swapped, x=hin, first=s, count=1)
        assert np.array_equal(bits(out[9:]), bits(out2[9:])), "rows whose lists were not touched"
        if not np.array_equal(bits(out[:9]), bits(out2[:9])):
            return
        tried += 1
        if tried == 5:
            break
    raise AssertionError(f"{fclass}: the walk of {tried} cases did not notice the swapped addends")
