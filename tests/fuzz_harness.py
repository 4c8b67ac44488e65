"""What the generic path's fuzz shares (tools/modelgen_fuzz.py's cases): the oracle's values for a case — predict over all layers,
and for an admitted case the stage-by-stage walk of tests/pattern_harness.py — cached per (case, graph, input); the engine
opener that makes a case's opt-ins in its order, before the graph or under it; and the three runs the GPU tests make of a case:
one_case (a single engine), one_case_off (option "generic_stages" 0) and one_case_multi (gnnvc_create_multi_generic, all parts
on device 0).  A plain module.  The comparison rules are tests/generic_harness.py's and no others: logits bit for bit, scores
within 1 ulp of the oracle's and bit for bit the restated sigmoid's (check_scores); a model that does not end in the sigmoid has
its outputs compared bit for bit and its logits buffer left as it was.

python -m tests.fuzz_harness --from A --to B runs one_case over cases A .. B - 1 — beyond the pinned ones — once each, and stops
at the first mismatch or error with the case's record on stderr."""
import ctypes as C
import subprocess

import numpy as np

from oracle import oracle_py
from tools import modelgen_fuzz as mz
from tests import generic_harness as gh
from tests import pattern_harness as ph
from tests.generic_harness import bits, graph_of, heavy_counts, ulp

for _name, _fn in mz.NEW_GRAPHS.items():
    gh.GRAPHS.setdefault(_name, _fn)

_cache = {}
SENTINEL = np.float32(-3.0)
SCALE2 = np.float32(0.37)     # the second input: the first one scaled
DEFAULT_GIANT = 16384
LIVE_GRAPH = "er1933"         # where the liveness of a case drawn onto a graph of fewer than 64 vertices is judged


def load_shim():
    """tests/test_expf_restatement.py's fixture for a caller that is not pytest."""
    from tests.test_expf_restatement import HERE, SO, SRC
    hdr = HERE.parent / "gnn-mwvc_amd" / "csrc" / "expf_glibc.h"
    if not SO.exists() or SO.stat().st_mtime < max(SRC.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run(["g++", "-O2", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-builtin-expf", "-std=c++17", "-fPIC", "-shared",
                        "-o", str(SO), str(SRC), "-lm"], check=True)
    L = C.CDLL(str(SO))
    for f in ("expf_restated", "expf_libm", "sigmoid_restated", "sigmoid_libm"):
        getattr(L, f).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    return L


# ---------------------------------------------------------------- the oracle's values: computed once, never changed

def text_of(i):
    if ("text", i) not in _cache:
        _cache["text", i] = mz.text(i)
    return _cache["text", i]


def oracle_at(i, ws):
    om = oracle_py.OracleModel(text_of(i))
    om.set_weight_scale(ws)
    return om


def stages_of(c):
    """An admitted case's stage list in tools/modelgen_patterns.stages_of's form: the walk's."""
    return [(r.dense, r.f, r.widths, r.end) for r in c.expect]


def input_of(i, gname, scaled=False):
    x = mz.model_input(i, graph_of(gname))
    return np.ascontiguousarray((x * SCALE2).astype(np.float32)) if scaled else x


def _no_rows(width):
    """What the oracle gives for the graph of no vertices (its entry point is not asked: it has no row to size its buffers by)."""
    return np.zeros((0, width), dtype=np.float32)


def final_of(i, gname, scaled=False):
    """The oracle's predict over all layers."""
    key = ("final", i, gname, scaled)
    if key not in _cache:
        g = graph_of(gname)
        _cache[key] = ph.predict(oracle_at(i, g.ws), g, input_of(i, gname, scaled)) if g.n else _no_rows(mz.case(i).out_width)
    return _cache[key]


def logits_of(i, gname, scaled=False):
    """A model that ends in the sigmoid: the oracle's predict up to its last linear layer, n x out_width."""
    key = ("logits", i, gname, scaled)
    if key not in _cache:
        g = graph_of(gname)
        om = oracle_at(i, g.ws)
        _cache[key] = ph.predict(om, g, input_of(i, gname, scaled), stop_after=om.n_layers - 2) if g.n else _no_rows(mz.case(i).out_width)
        _cache["flat", i, gname, scaled] = np.ascontiguousarray(_cache[key].reshape(-1))
    return _cache[key]


def flat_logits(i, gname, scaled=False):
    logits_of(i, gname, scaled)
    return _cache["flat", i, gname, scaled]


def walk_case(i, g, x=None, first=0, count=None):
    """The walk adapter: tests/pattern_harness.walk_stages over an admitted case's stage list, from the input rows x of stage `first`."""
    c = mz.case(i)
    if g.n == 0:
        return [(_no_rows(r.f), _no_rows(r.widths[-1]), _no_rows(r.widths[-1])) for r in c.expect[first: None if count is None else first + count]]
    h = mz.model_input(i, g) if x is None else np.ascontiguousarray(x, dtype=np.float32).reshape(g.n, -1)
    return ph.walk_stages(oracle_at(i, g.ws), stages_of(c), g, h, first=first, count=count)


def want_of(i, gname):
    if ("want", i, gname) not in _cache:
        _cache["want", i, gname] = walk_case(i, graph_of(gname))
    return _cache["want", i, gname]


def live_graph_of(c):
    return c.graph if graph_of(c.graph).n >= 64 else LIVE_GRAPH


def _varying(a):
    return sum(int(np.unique(bits(a[:, col])).size > 1) for col in range(a.shape[1]))


def dead(i, gname):
    """None if case i is alive on the graph — its output finite, at least half of its columns (at least one) taking more than one
    value over the vertices, every intermediate stage output with a column that varies — else what is wrong with it."""
    c = mz.case(i)
    final = final_of(i, gname)
    if not np.isfinite(final).all():
        return "an output that is not finite"
    if _varying(final) < max(1, (c.out_width + 1) // 2):
        return f"{_varying(final)} of {c.out_width} output columns vary"
    if c.admitted:
        for s, (_, h, _) in enumerate(want_of(i, gname)[:-1]):
            if not np.isfinite(h).all() or _varying(h) < 1:
                return f"stage {s}'s output does not vary"
    return None


def graph_stage_indices(c):
    return [s for s, r in enumerate(c.expect) if not r.dense]


def rows_present(c, gname=None):
    """(heavy rows, giant rows) the engine lists on the case's graph at its thresholds (generic_harness.heavy_counts)."""
    g = graph_of(c.graph if gname is None else gname)
    heavy = heavy_counts(g, c.heavy)
    gt = DEFAULT_GIANT if c.giant is None else c.giant
    giant = heavy_counts(g, max(c.heavy, gt)) if c.heavy and gt else (0, 0)
    return heavy, giant


# ---------------------------------------------------------------- engines

def open_case(i, g, opts=()):
    """A single engine on device 0 with the case's text, "poison_features" 1 and the case's opt-ins in the case's order: before the
    graph, or — a late case — under the resident graph."""
    import gnn_mwvc_amd as G
    c = mz.case(i)
    e = G.Engine(text_of(i), device=0)

    def opt_in(which):
        if which == "big" and c.big_lds:
            e.set_generic_big_stages(c.big_lds)
        elif which == "feat" and c.feature_width:
            e.set_generic_feature_width(c.feature_width)
        elif which == "mask" and c.mask:
            e.set_generic_patterns(c.mask)
        elif which == "heavy":
            e.set_generic_heavy_rows(c.heavy)
        elif which == "giant" and (c.giant is not None or c.segments != -1):
            e.set_generic_giant_rows(DEFAULT_GIANT if c.giant is None else c.giant, c.segments)
    try:
        e.set_option("poison_features", 1)
        for k, v in dict(opts).items():
            e.set_option(k, v)
        assert (e.num_layers, e.in_width, e.out_width) == (len(c.seq), c.in_width, c.out_width), mz.describe(i)
        if not c.late:
            for which in c.order:
                opt_in(which)
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
        if c.late:
            for which in c.order:
                opt_in(which)
    except BaseException:
        e.close()
        raise
    return e


def assert_read_outs(e, i):
    c = mz.case(i)
    what = mz.describe(i)
    if not c.admitted:
        assert not e.fused and e.num_stages == 0 and e.get_info("generic_stages_model") == 0, what
        return
    ns = len(c.expect)
    assert e.fused and e.num_stages == ns and e.get_info("generic_stages_model") == 1, what
    rd = lambda key: [e.get_info(f"{key}_{s}") for s in range(ns)]
    assert [e.stage_widths(s) for s in range(ns)] == [(r.f, r.widths[-1]) for r in c.expect], what
    assert rd("generic_stage_layers") == [len(r.widths) for r in c.expect], what
    assert rd("generic_stage_dense") == [r.dense for r in c.expect], what
    assert rd("generic_stage_end") == [r.end for r in c.expect], what
    assert rd("generic_stage_lds_bytes") == [r.lds_bytes for r in c.expect], what
    assert rd("generic_stage_threads") == [r.threads for r in c.expect], what
    assert (e.get_info("generic_patterns"), e.get_info("generic_feature_width"), e.get_info("generic_big_lds")) == \
        (c.mask, c.feature_width, c.big_lds), what


def assert_row_counts(e, i, gname=None):
    """After a forward: the rows the engine classed (a model with no graph stage classes none, and is not asked)."""
    c = mz.case(i)
    if not graph_stage_indices(c):
        return
    heavy, giant = rows_present(c, gname)
    got = tuple(e.get_info(k) for k in ("generic_heavy_rows", "generic_heavy_entries", "generic_giant_rows", "generic_giant_entries"))
    assert got == heavy + giant, (mz.describe(i), gname, got, heavy + giant)


def check_outputs(shim, i, gname, sc, lg, label, scaled=False, untouched=None):
    """(sc, lg) n x out_width against the oracle's values for (case, graph, input).  untouched: what the logits of a model that
    does not end in the sigmoid must still hold (a value, or "nan")."""
    c = mz.case(i)
    g = graph_of(gname)
    what = (mz.describe(i), gname, label)
    assert sc.shape == (g.n, c.out_width), what
    if g.n == 0:
        return
    if c.sigmoid_end:
        want = logits_of(i, gname, scaled)
        bad = np.argwhere(bits(lg) != bits(want))
        assert bad.size == 0, (what, f"{len(bad)}/{want.size} logits differ, first (row, column)", bad[:6].tolist())
        gh.check_scores(shim, sc.reshape(-1), lg.reshape(-1), flat_logits(i, gname, scaled), what)
        return
    want = final_of(i, gname, scaled)
    bad = np.argwhere(bits(sc) != bits(want))
    assert bad.size == 0, (what, f"{len(bad)}/{want.size} outputs differ, first (row, column)", bad[:6].tolist())
    if untouched is not None:
        assert (np.isnan(lg).all() if untouched == "nan" else (lg == untouched).all()), (what, "logits written by a model that does not end in the sigmoid")


def host_forward(shim, e, i, gname, label, scaled=False, audited=False):
    c = mz.case(i)
    g = graph_of(gname)
    sc = np.full((g.n, c.out_width), SENTINEL, dtype=np.float32)
    lg = np.full((g.n, c.out_width), SENTINEL, dtype=np.float32)
    (e.forward_audited if audited else e.forward)(input_of(i, gname, scaled), out=(sc, lg))
    check_outputs(shim, i, gname, sc, lg, label, scaled, untouched=SENTINEL)


def device_forward(shim, e, i, gname, label):
    import torch
    c = mz.case(i)
    g = graph_of(gname)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(input_of(i, gname)).to(dev)
    sc = torch.full((g.n, c.out_width), float("nan"), dtype=torch.float32, device=dev)
    lg = torch.full((g.n, c.out_width), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    e.forward_device(x.data_ptr(), sc.data_ptr(), lg.data_ptr())
    e.synchronize()
    check_outputs(shim, i, gname, sc.cpu().numpy(), lg.cpu().numpy(), label, untouched="nan")


def crafted_stage(e, i, gname, s):
    """Stage s through gnnvc_stage_forward_device on generic_harness.crafted_input — sums whose bits depend on the order of their
    terms — over split_ranges, on NaN-filled outputs: after each part the rows done are the oracle's walk from that stage and every
    other row, the pad row included, is still NaN; then gnnvc_audit_stage_device over the whole range is clean."""
    import torch
    c = mz.case(i)
    g = graph_of(gname)
    n = g.n
    r = c.expect[s]
    f, n_out, sig = r.f, r.widths[-1], r.end == mz.END_SIGMOID
    what = (mz.describe(i), gname, "crafted stage", s)
    hin = gh.crafted_input(n, f, [mz.TAG, i, s])
    (_, want_out, want_pre), = walk_case(i, g, x=hin, first=s, count=1)
    dev = torch.device("cuda:0")
    tin = torch.zeros((n + 1, f), dtype=torch.float32, device=dev)
    tin[:n] = torch.from_numpy(hin).to(dev)
    out = torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)
    lgt = torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    done = np.zeros(n + 1, dtype=bool)
    for part, todo in enumerate(gh.split_ranges(n)):
        for lo, hi in todo:
            e.stage_forward_device(s, lo, hi, tin.data_ptr(), out.data_ptr(), lgt.data_ptr())
            done[lo:hi] = True
        e.synchronize()
        got, gotl = out.cpu().numpy(), lgt.cpu().numpy()
        assert np.isnan(got[~done]).all(), (what, part, "rows outside the ranges were written")
        assert np.isnan(gotl[~done]).all() if sig else np.isnan(gotl).all(), (what, part, "logits rows")
        d = done[:n]
        if sig:
            bad = np.argwhere(bits(gotl[:n][d]) != bits(want_pre[d]))
            assert bad.size == 0, (what, part, f"{len(bad)} stage logits differ, first (row of the part, column)", bad[:6].tolist())
            assert ulp(got[:n][d], want_out[d]).max(initial=0) <= 1, (what, part, "stage scores")
        else:
            bad = np.argwhere(bits(got[:n][d]) != bits(want_out[d]))
            assert bad.size == 0, (what, part, f"{len(bad)} values differ, first (row of the part, column)", bad[:6].tolist())
    assert done[:n].all() and not done[n], what
    runs = e.get_info("audit_runs")
    e.audit_stage_device(s, 0, n, tin.data_ptr(), out.data_ptr(), lgt.data_ptr() if sig else 0)   # (raises on a mismatch)
    assert e.get_info("audit_failures") == 0 and e.get_info("audit_runs") == runs + (1 if n else 0), what


# ---------------------------------------------------------------- the runs

def one_case(i, shim):
    """A case on a single engine: see tests/test_gpu_generic_fuzz.py::test_random_models_single_engine."""
    c = mz.case(i)
    g = graph_of(c.graph)
    e = open_case(i, g)
    try:
        assert_read_outs(e, i)
        for rep in range(3):
            host_forward(shim, e, i, c.graph, ("forward", rep))
            if g.n:
                assert e.get_info("generic_stages_active") == int(c.admitted), mz.describe(i)
        host_forward(shim, e, i, c.graph, "scaled input", scaled=True)
        host_forward(shim, e, i, c.graph, "the first input again")
        if not c.admitted:
            assert_read_outs(e, i)
            return
        assert_row_counts(e, i)
        runs = e.get_info("audit_runs")
        host_forward(shim, e, i, c.graph, "audited", audited=True)
        assert e.get_info("audit_failures") == 0, mz.describe(i)
        assert e.get_info("audit_runs") == runs + (len(c.expect) if g.n else 0), mz.describe(i)
        if g.n:
            device_forward(shim, e, i, c.graph, "device pointers")
        gs = graph_stage_indices(c)
        todo = ([gs[c.stage_pick % len(gs)]] if gs else []) + ([0] if c.expect[0].dense else [])
        for s in todo:
            crafted_stage(e, i, c.graph, s)
        assert_read_outs(e, i)
    finally:
        e.close()


def one_case_off(i, shim):
    """An admitted case with option "generic_stages" 0: layer by layer, the same values."""
    c = mz.case(i)
    g = graph_of(c.graph)
    e = open_case(i, g, opts={"generic_stages": 0})
    try:
        assert not e.fused and e.num_stages == 0 and e.get_info("generic_stages_model") == 0, mz.describe(i)
        for rep in range(2):
            host_forward(shim, e, i, c.graph, ("generic_stages 0", rep))
        host_forward(shim, e, i, c.graph, "generic_stages 0, scaled input", scaled=True)
        assert e.get_info("generic_stages_active") == 0, mz.describe(i)
    finally:
        e.close()


def piece_rows(lo, hi, K):
    """The rows of a part's K pieces: nearly equal ranges cut at multiples of 64 rows, as the handle cuts them
    (tests/test_gpu_multi_generic.py's _pieces)."""
    cut = [hi if k == K else min(hi, max(lo, (lo + (hi - lo) * k // K) // 64 * 64)) for k in range(K + 1)]
    for k in range(1, K):
        cut[k] = max(cut[k], cut[k - 1])
    return [b - a for a, b in zip(cut[:-1], cut[1:])]


def one_case_multi(i, shim):
    """An admitted case behind gnnvc_create_multi_generic, c.parts parts on device 0: two graphs handed to the one handle in turn
    (upload, then staged in 7 pieces), three forwards each, and an audited one on the second."""
    import gnn_mwvc_amd as G
    c = mz.case(i)
    what = mz.describe(i)
    cfg = {"heavy_rows": c.heavy, "giant_segments": c.segments, "big_stages_lds": c.big_lds, "feature_width": c.feature_width,
           "patterns": c.mask}
    if c.giant is not None:
        cfg["giant_rows"] = c.giant
    e = G.Engine(text_of(i), devices=[0] * c.parts, generic=cfg)
    try:
        e.set_option("poison_features", 1)
        e.set_option("multi_pieces", c.pieces)
        e.set_option("multi_push", c.push)
        ns = len(c.expect)
        assert e.get_info("multi_generic") == 1 and e.fused and e.num_stages == ns, what
        assert [e.stage_widths(s) for s in range(ns)] == [(r.f, r.widths[-1]) for r in c.expect], what
        assert [e.get_info(f"generic_stage_dense_{s}") for s in range(ns)] == [r.dense for r in c.expect], what
        for gname, route in ((c.graph, "upload"), (c.graph2, "staged7")):
            g = graph_of(gname)
            gh.hand_over(e, g, route)
            rows = [e.get_info(f"part_rows_{r}") for r in range(c.parts)]
            assert sum(rows) == g.n, (what, gname, rows)
            for rep in range(3):
                host_forward(shim, e, i, gname, (c.parts, c.pieces, c.push, route, rep))
            assert_row_counts(e, i, gname)
        K = e.get_info("multi_pieces")
        los = np.concatenate([[0], np.cumsum(rows)]).tolist()
        nonempty = sum(1 for r in range(c.parts) for size in piece_rows(los[r], los[r + 1], K) if size > 0)
        runs = e.get_info("audit_runs")
        host_forward(shim, e, i, c.graph2, "audited", audited=True)
        assert e.get_info("audit_failures") == 0, what
        assert e.get_info("audit_runs") == runs + nonempty * ns, (what, c.graph2, rows, K)
    finally:
        e.close()


# ---------------------------------------------------------------- the long form

def main(argv=None):
    import argparse
    import sys
    import time
    import traceback
    ap = argparse.ArgumentParser(description="one_case over fuzz cases --from .. --to - 1; stops at the first mismatch or error")
    ap.add_argument("--from", dest="lo", type=int, required=True)
    ap.add_argument("--to", dest="hi", type=int, required=True)
    a = ap.parse_args(argv)
    shim = load_shim()
    t0 = time.time()
    for i in range(a.lo, a.hi):
        try:
            one_case(i, shim)
        except BaseException:
            traceback.print_exc()
            print(f"STOPPED at {mz.describe(i)}: {i - a.lo} cases clean before it, 1 mismatch or error", file=sys.stderr, flush=True)
            return 1
        for key in [k for k in _cache if k[0] != "graph"]:   # (a long run keeps no case's values)
            del _cache[key]
        for key in [k for k in gh._cache if k[0] == "sigmoid"]:
            del gh._cache[key]
        mz._cases.pop(i, None)
        if (i - a.lo + 1) % 50 == 0:
            print(f"{i - a.lo + 1} cases, 0 mismatches, {time.time() - t0:.0f} s", flush=True)
    print(f"{a.hi - a.lo} cases ({a.lo} .. {a.hi - 1}), 0 mismatches, {time.time() - t0:.0f} s", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
