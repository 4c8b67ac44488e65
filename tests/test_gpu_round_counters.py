"""The bookkeeping of the compact-table plan without its small launches: the rounds of the dense-only stage count their dirty
rows in a word each and own a slot range each (no k_c4_mark between the rounds), k_c4_choose clears what its stage counts into
(no memset between the compact-table plan's kernels).  The LDS-table plan's "this input does not fit" flag keeps its one memset a
forward (clearing it a forward ahead from k_lt_bytes_x was built, showed no gain and is not in: profiles/compact_bookkeeping).

Graphs and chunk sizes as in test_plans_with_many_small_chunks: erdos_renyi(20000, 200000, 72) at 16 rows a chunk (five rounds
of the grid) and erdos_renyi(20011, 150000, 73) at 48 (two rounds, a ragged last chunk), with the dense layers of the last stage
under the sums (overlap_dense 1: round by round) and after them (0: one launch).

Stage 2 is driven through the stage entry point with inputs whose stray vertices put dirty rows into every round, into the
first round only, into the last round only and nowhere (a round = 256 chunks of the call; a call's chunks that straddle its ends
are done whole).  Whether an input does so is worked out here, on the CPU, from the graph alone, and asserted before the device
is asked; where no vertex of the graph dirties rows of one round only over the whole graph, the call is cut to a row range — `lo`
and `hi` inside chunks — over which one does.  Logits bit for bit against the oracle, and "compact_gather_last_dirty" equal to
the number of rows with a stray neighbour among the rows of the call's chunks."""
import numpy as np
import pytest

from oracle import oracle_py
from tools import graphgen as gg
from tests.test_gpu_parity import _oracle_stage, _sparse_features, bits
from tests.test_modelgen import layer_outputs

pytestmark = pytest.mark.gpu

GRAPHS = {
    "er20000": (lambda: gg.erdos_renyi(20000, 200000, 72), 16),
    "er20011": (lambda: gg.erdos_renyi(20011, 150000, 73), 48),
}
LIVE = [1, 6, 10, 15]
_cache = {}


def graph_of(gname):
    if gname not in _cache:
        _cache[gname] = GRAPHS[gname][0]()
    return _cache[gname]


def open_engine(model_text, g, chunk_rows, overlap, extra=()):
    import gnn_mwvc_amd as G
    e = G.Engine(model_text, device=0)
    try:
        for k, v in dict({"blocked_min_n": 0, "plan_chunk_rows": chunk_rows, "overlap_dense": overlap, "poison_features": 1}, **dict(extra)).items():
            e.set_option(k, v)
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
    except BaseException:
        e.close()
        raise
    return e


def dirty_rows(g, h, cols):
    """Rows with a neighbour that has a non-zero outside the table's columns `cols`."""
    stray = (h[:, [c for c in range(16) if c not in cols]] != 0).any(axis=1)
    rp = g.rowptr.astype(np.int64)
    hits = np.concatenate(([0], np.cumsum(stray[g.col[: rp[-1]]])))
    return hits[rp[1:]] > hits[rp[:-1]]


def fullest_columns(h, passes=1):
    """k_c4_choose's pick: the 4 * passes fullest columns, ties to the lowest index."""
    counts = (h != 0).sum(axis=0)
    return sorted(sorted(range(16), key=lambda c: (-int(counts[c]), c))[: 4 * passes])


def chunk_span(g, rows, lo, hi):
    """The rows of the chunks that hold [lo, hi): what a call's sums cover."""
    return lo // rows * rows, min((hi - 1) // rows * rows + rows, g.n)


def rounds_of(g, rows, lo, hi):
    a, b = chunk_span(g, rows, lo, hi)
    return [(r, min(r + 256 * rows, b)) for r in range(a, b, 256 * rows)]


def neighbours(g, v):
    return g.col[int(g.rowptr[v]): int(g.rowptr[v + 1])].astype(np.int64)


def vertex_dirtying_only(g, rows, lo, hi, which):
    """A vertex all of whose neighbours within the call's chunks lie in round `which` (0 or -1) of the call, and some do."""
    a, b = chunk_span(g, rows, lo, hi)
    ra, rb = rounds_of(g, rows, lo, hi)[which]
    for v in range(g.n):
        nb = neighbours(g, v)
        nb = nb[(nb >= a) & (nb < b)]
        if nb.size and ((nb >= ra) & (nb < rb)).all():
            return v
    return None


def placements(g, rows):
    """{name: (lo, hi, stray vertices)}: where the strays go and over which rows the stage is called."""
    n = g.n
    out = {"nowhere": (0, n, []), "every": None, "first": None, "last": None}
    rng = np.random.default_rng(3)
    picks = [int(v) for v in rng.choice(n, 12, replace=False)]
    out["every"] = (0, n, picks)
    # ranges with `lo` and `hi` inside chunks: the whole graph first, then calls that cover a little more than half of it
    cuts = [(0, n), (0, n // 2 + rows // 2 + 7), (n - n // 2 - rows // 2 - 5, n)]
    for name, which in (("first", 0), ("last", -1)):
        for lo, hi in cuts:
            if len(rounds_of(g, rows, lo, hi)) < 2:
                continue
            v = vertex_dirtying_only(g, rows, lo, hi, which)
            if v is not None:
                out[name] = (lo, hi, [v])
                break
        assert out[name] is not None, (name, "no vertex of this graph dirties rows of that round alone")
    return out


def stage2(e, g, h, lo, hi):
    import torch
    dev = torch.device("cuda:0")
    hin = torch.zeros((g.n + 1, 16), dtype=torch.float32, device=dev)
    hin[: g.n] = torch.from_numpy(h).to(dev)
    out = torch.full((g.n + 1,), 7.0, dtype=torch.float32, device=dev)
    lg = torch.full((g.n + 1,), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    e.stage_forward_device(2, lo, hi, hin.data_ptr(), out.data_ptr(), lg.data_ptr())
    e.synchronize()
    got = lg.cpu().numpy()
    assert (got[:lo] == 7.0).all() and (got[hi:] == 7.0).all(), "rows outside the call were written"
    return got[lo:hi]


def features(g, strays, seed=5):
    h = _sparse_features(g.n, np.random.default_rng(seed), LIVE, [1.0, 0.4, 0.2, 1.0])
    for i, v in enumerate(strays):
        h[v, (3, 8, 12)[i % 3]] = 1.5 + i
    return h


def check_stage2(e, om, g, rows, h, lo, hi, fits=True, label=()):
    want = _oracle_stage(om, g, 2, h)[lo:hi, 0]
    got = stage2(e, g, h, lo, hi)
    assert np.array_equal(bits(got), bits(want)), (label, lo, hi, int((bits(got) != bits(want)).sum()))
    assert e.get_info("compact_gather_last_ok") == (1 if fits else 0), label
    if fits:
        assert e.get_info("compact_gather_last_passes") == 1, label
        a, b = chunk_span(g, rows, lo, hi)
        expect = int(dirty_rows(g, h, fullest_columns(h))[a:b].sum())
        assert e.get_info("compact_gather_last_dirty") == expect, (label, lo, hi, e.get_info("compact_gather_last_dirty"), expect)
        return expect
    return 0


def check_forward(e, om, g, x=None, want=None, label=()):
    """A whole forward: logits bit for bit; the dirty rows of its last stage as the oracle's h2 has them."""
    x = g.x() if x is None else x
    want = om.logits(g, x) if want is None else want
    _, lg = e.forward(x)
    assert np.array_equal(bits(lg[:, 0]), bits(want)), (label, int((bits(lg[:, 0]) != bits(want)).sum()))
    if e.get_info("compact_gather_last_ok") == 1:
        h2 = oracle_py.relu(layer_outputs(om, g, x)[5])
        cols = fullest_columns(h2, e.get_info("compact_gather_last_passes"))
        assert e.get_info("compact_gather_last_dirty") == int(dirty_rows(g, h2, cols).sum()), label


@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_rounds_count_their_own_dirty_rows(model_text, oracle_model, gname, overlap):
    g, chunk_rows = graph_of(gname), GRAPHS[gname][1]
    om = oracle_model
    om.set_weight_scale(g.ws)
    want = om.logits(g)
    e = open_engine(model_text, g, chunk_rows, overlap)
    try:
        for rep in range(3):
            check_forward(e, om, g, want=want, label=("settling", rep))
        assert e.get_info("lds_table_active") == 1 and e.get_info("compact_gather_active") == 1
        rows = e.get_info("compact_gather_rows_per_chunk")
        assert len(rounds_of(g, rows, 0, g.n)) == 5 if gname == "er20000" else len(rounds_of(g, rows, 0, g.n)) >= 2, rows
        place = placements(g, rows)
        # on the CPU first: does each input put its dirty rows where its name says?
        per_round = {}
        for name, (lo, hi, strays) in place.items():
            h = features(g, strays)
            assert fullest_columns(h) == LIVE and (h[:, [c for c in range(16) if c not in LIVE]] != 0).sum() <= g.n // 512
            d = dirty_rows(g, h, LIVE)
            per_round[name] = [int(d[a:b].sum()) for a, b in rounds_of(g, rows, lo, hi)]
        assert all(c > 0 for c in per_round["every"]), per_round
        assert per_round["first"][0] > 0 and not any(per_round["first"][1:]), per_round
        assert per_round["last"][-1] > 0 and not any(per_round["last"][:-1]), per_round
        assert not any(per_round["nowhere"]), per_round
        # strays -> clean -> strays, first round only, last round only, and the sub-ranges with their ends inside chunks
        for name in ("every", "nowhere", "every", "first", "last", "nowhere"):
            lo, hi, strays = place[name]
            dirty = check_stage2(e, om, g, rows, features(g, strays), lo, hi, label=(gname, overlap, name))
            assert dirty == sum(per_round[name])
        h = features(g, place["every"][2])
        for lo, hi in ((rows // 2 + 1, g.n), (0, g.n - rows // 2 - 1), (g.n // 3 + 5, g.n - 3)):
            check_stage2(e, om, g, rows, h, lo, hi, label=(gname, overlap, "range", lo, hi))
        # fit -> too many strays -> fit
        many = features(g, [int(v) for v in np.random.default_rng(9).choice(g.n, 400, replace=False)])
        check_stage2(e, om, g, rows, h, 0, g.n, label="fit")
        check_stage2(e, om, g, rows, many, 0, g.n, fits=False, label="too many strays")
        check_stage2(e, om, g, rows, h, 0, g.n, label="fit again")
        # forward -> a stage entry call -> forward
        check_forward(e, om, g, want=want, label="forward after stage calls")
        check_stage2(e, om, g, rows, h, 0, g.n, label="stage call between forwards")
        check_forward(e, om, g, want=want, label="forward after a stage call")
        # x -> an x that is no k / ws -> x -> 2 x: the LDS-table plan's flag from forward to forward
        x2 = (g.x() * np.float32(0.37)).astype(np.float32)
        x3 = (g.x() * np.float32(2.0)).astype(np.float32)
        for x, fit in ((g.x(), 1), (x2, 0), (g.x(), 1), (x3, 1), (x2, 0), (x2, 0), (g.x(), 1)):
            check_forward(e, om, g, x=x, label=("input", fit))
            assert e.get_info("lds_table_last_ok") == fit, fit
        # forward -> a plan option changes -> forward
        e.set_option("overlap_dense", 1 - overlap)
        check_forward(e, om, g, want=want, label="after overlap_dense changed")
        check_stage2(e, om, g, rows, h, 0, g.n, label="stage call after overlap_dense changed")
        e.set_option("overlap_dense", overlap)
        e.set_option("dense_skip_zeros", 0)
        check_forward(e, om, g, want=want, label="after dense_skip_zeros changed")
        check_forward(e, om, g, want=want, label="steady again")
    finally:
        e.close()


def test_no_mark_launches_in_a_steady_forward(model_text, oracle_model):
    g, chunk_rows = graph_of("er20000"), GRAPHS["er20000"][1]
    oracle_model.set_weight_scale(g.ws)
    want = oracle_model.logits(g)
    e = open_engine(model_text, g, chunk_rows, 1, {"kernel_trace": 1})
    try:
        for rep in range(5):
            _, lg = e.forward(g.x())
            assert np.array_equal(bits(lg[:, 0]), bits(want)), rep
        names = [n for n, _ in e.kernel_trace(4096)]   # (the records of every forward so far)
        steady = names[len(names) - names[::-1].index(next(n for n in names[::-1] if "k_lt_bytes_x" in n)) - 1:]   # the last forward's
        assert sum("k_c4_agg" in n for n in steady) == 5 + 1, steady   # (stage 2's five rounds, stage 1's one launch)
        assert sum("k_c4_choose" in n for n in steady) == 2 and sum("k_c4_fix" in n for n in steady) >= 2, steady
        assert not any("k_c4_mark" in n for n in names), names
        # ... and no memset between the compact-table plan's kernels: the one left is the LDS table's flag (the graph's first
        # forwards, with the pilot and without the plans, had more)
        assert e.get_info("plan_memsets_last_forward") == 1
        e.forward((g.x() * np.float32(0.37)).astype(np.float32))   # (an input the LDS table steps aside for: the same)
        assert e.get_info("plan_memsets_last_forward") == 1
    finally:
        e.close()
