"""No kernel writes past the ends of the engine's own buffers.  With the guard bands on (csrc/gnnvc_device_mem.h; kinds 1001 .. 1007
of gnnvc_debug_probe, which is no part of include/gnnvc.h) every device and page-locked buffer the library allocates carries 4096
bytes of a byte pattern on either side; a check, and every free, reads them back.  The registry's own logic is
tests/test_guard_bands_host.py's; here the project's case tables and harnesses run under the switch, at the smallest sizes at
which a buffer's size can go wrong: n around the 64-row tile, graphs of one vertex and of none, every plan forced onto small
graphs, lists filled to their last entry, graphs that replace each other in ascending size so that every buffer is regrown to an
exact fit.

Every test keeps the bar of the test it borrows from — logits bit for bit the oracle's — and adds: at least 10 guarded buffers
alive while an engine holds a graph (test_gpu_lifetime.py's floor, so that a test cannot pass by guarding nothing), no damaged
band after the forwards, and none after close() (the frees check the bands they give back).

Out of the bands' sight: over-reads, strays further than 4096 bytes, and buffers the caller owns."""
import contextlib
import ctypes as C
import gc
import re

import numpy as np
import pytest

from tools import graphgen as gg
from tools import modelgen_fuzz as mz
from tests import fuzz_harness as fh
from tests import generic_harness as gh
from tests.generic_harness import bits, graph_of
from tests.test_expf_restatement import shim   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)
from tests.test_gpu_lifetime import HUB_OPTIONS, _two_hubs

pytestmark = pytest.mark.gpu

LIVE, ON, OFF, CHECK, ALIVE, HIT_AFTER, HIT_BEFORE, HIT_BAND_END = 1000, 1001, 1002, 1003, 1004, 1005, 1006, 1007
FLOOR = 10   # guarded buffers an engine with a graph holds at the least (test_destroy_frees_everything: peak > start + 10)

# tools/modelgen_fuzz.py's cases run under the bands; tests/test_modelgen_fuzz.py pins on the CPU what they reach: the BIG forms at
# 256, 512 and 1024 threads, FEAT, OPEN, a dense prologue, heavy rows from 1, 17 and 512 entries, giant rows from 1024 on one
# wave (segments 1), every graph of GRAPH_NAMES, and cases no setting admits (5, 30), which run layer by layer
GENERIC_CASES = [0, 1, 5, 6, 8, 10, 12, 19, 22, 30, 43, 47, 60, 75, 96, 117, 124]
GENERIC_MULTI = [1, 6, 12, 19, 75, 96]   # on 3, 3, 8, 2, 3 and 5 parts

# cases of tests/test_gpu_fuzz.py (seed 90 000 + case), the small ones among those that cover the values below: case -> what of
# them it reaches, in plan_case_covers' words (tests/test_modelgen_fuzz.py asserts each entry, not only the union)
SKEWED, TILES = "lds_table_skewed_rows > 0", "table_tiles 1 at table_tiles_min_n 0"
PLAN_COVERS = {
    1: {"compact_gather 1", SKEWED, "giant_segments 1", "mfma_dense 0"},
    18: {TILES, SKEWED, "giant_segments 1", "mfma_dense 1"},
    39: {"plan_chunk_rows 48", "compact_gather 1", SKEWED, "mfma_dense 0"},
    44: {SKEWED, "giant_segments 1", "mfma_dense 0"},
    46: {TILES, SKEWED, "mfma_dense 2"},
    49: {"compact_gather 1", SKEWED, "mfma_dense 1"},
    50: {TILES, "compact_gather 1", SKEWED, "giant_segments 1", "mfma_dense 1"},
    54: {"plan_chunk_rows 16", "compact_gather 1", SKEWED, "mfma_dense 2"},
}
PLAN_CASES = sorted(PLAN_COVERS)
PLAN_STAGE_CASES = [1, 44, 49, 50]   # ... and the stage entry point over sub-ranges


def plan_case_covers(case):
    """What of the values PLAN_COVERS is about a case of tests/test_gpu_fuzz.py reaches, from its drawn options."""
    from tests.test_gpu_fuzz import _graph, _options
    rng = np.random.default_rng(90_000 + case)
    _graph(rng)
    o = _options(rng)
    out = {f"mfma_dense {o['mfma_dense']}"}
    if o.get("plan_chunk_rows") in (16, 48):
        out.add(f"plan_chunk_rows {o['plan_chunk_rows']}")
    for key, hit in (("giant_segments 1", o["giant_segments"] == 1), (SKEWED, o["lds_table_skewed_rows"] > 0),
                     ("compact_gather 1", o["compact_gather"] == 1),
                     (TILES, o["table_tiles"] == 1 and o["table_tiles_min_n"] == 0)):
        if hit:
            out.add(key)
    return out


def generic_case_covers(i):
    """What of GENERIC_CASES' comment case i reaches, from its record."""
    c = mz.case(i)
    out = {f"graph {c.graph}"}
    if not c.admitted:
        return out | {"not admitted"}
    for r in c.expect:
        out |= {k for k, hit in ((f"BIG {r.threads}", r.big and not r.dense), ("FEAT", r.feat), ("OPEN", r.open),
                                 ("dense prologue", r.dense)) if hit}
    (heavy, _), (giant, _) = fh.rows_present(c)
    if fh.graph_stage_indices(c) and heavy:
        out.add(f"heavy {c.heavy}")
        if giant and c.giant == 1024 and c.segments == 1:
            out.add("giant 1024 with segments 1")
    return out


# ---------------------------------------------------------------- the switch and the watch

@pytest.fixture(scope="module")
def probe():
    import gnn_mwvc_amd as G
    L = G.load_library()
    L.gnnvc_debug_probe.argtypes = [C.c_void_p, C.c_int]
    L.gnnvc_debug_probe.restype = C.c_int
    return lambda kind: L.gnnvc_debug_probe(None, kind)


@pytest.fixture(autouse=True)
def guards(probe):
    gc.collect()   # (an engine an earlier test left to the collector goes now, and plain)
    assert probe(ON) == 0
    # (nothing is discarded: damage that frees found since the last check — an engine of an earlier test that only the collector
    # closed — fails the test that meets it)
    assert probe(CHECK) == 0, "bands found damaged at frees before this test began: see the stderr lines"
    yield
    assert probe(OFF) == 0


def held(probe, label=""):
    """While an engine holds a graph: enough buffers are guarded, and no band is damaged."""
    alive, damaged = probe(ALIVE), probe(CHECK)
    print(f"guard bands: {alive} buffers alive, {damaged} damaged bands {label}")
    assert alive >= FLOOR, (label, alive)
    assert damaged == 0, (label, damaged, "see the stderr lines")
    return alive


@contextlib.contextmanager
def watched(probe, label=""):
    """Every engine closed inside — by the test or by a harness that opens and closes its own — is asked `held` just before it
    goes; after the block, the bands the frees gave back are clean too.  Yields the list of buffers alive at each close."""
    import gnn_mwvc_amd as G
    plain_close = G.Engine.close
    seen = []

    def close(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                seen.append(held(probe, (label, "at close")))
        finally:
            plain_close(self)   # (the engine goes whatever the check said: nothing guarded leaks into the next test)

    G.Engine.close = close
    try:
        yield seen
    finally:
        G.Engine.close = plain_close
    assert seen, (label, "no engine was closed under the watch")
    assert probe(CHECK) == 0, (label, "bands found damaged when their buffers were freed: see the stderr lines")


_want = {}


def trained_logits(oracle_model, g, scale=None):
    """The oracle's logits for the trained model on g, the input g.x() or g.x() * scale: computed once."""
    key = (id(g), scale)
    if key not in _want:
        oracle_model.set_weight_scale(g.ws)
        _want[key] = (g, oracle_model.logits(g, None if scale is None else scaled(g, scale)))
    return _want[key][1]


def scaled(g, scale):
    return (g.x() * np.float32(scale)).astype(np.float32)


def trained_forward(e, oracle_model, g, label, scale=None):
    sc, lg = e.forward(g.x() if scale is None else scaled(g, scale))
    if g.n == 0:
        assert sc.shape == (0, 1), label
        return
    want = trained_logits(oracle_model, g, scale)
    bad = np.flatnonzero(bits(lg[:, 0]) != bits(want))
    assert bad.size == 0, (label, f"{bad.size}/{g.n} logits differ from the oracle, first rows", bad[:6].tolist())


def three_forwards(e, oracle_model, g, label):
    """The input, the input scaled by 0.37, the first input again (a row no kernel writes shows when the input changes)."""
    trained_forward(e, oracle_model, g, (label, 0))
    trained_forward(e, oracle_model, g, (label, "scaled"), scale=0.37)
    trained_forward(e, oracle_model, g, (label, "again"))


# ---------------------------------------------------------------- a. the detector detects

LINE = re.compile(r"gnnvc guard \(check\): buffer #(\d+), (\d+) bytes, element size (\d+), device 0: (leading|trailing) band damaged, "
                  r"first at offset (\d+), value 0x5a")


def test_the_detector_detects(model_text, oracle_model, probe, capfd):
    import gnn_mwvc_amd as G
    g = gg.erdos_renyi(3000, 12000, 3)
    start, none_yet = probe(LIVE), probe(ALIVE)
    e = G.Engine(model_text, device=0)
    try:
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
        trained_forward(e, oracle_model, g, "before the hooks")
        held(probe, "one forward")
        capfd.readouterr()
        named = []
        for hook, side, offset in ((HIT_AFTER, "trailing", 0), (HIT_BEFORE, "leading", 4095), (HIT_BAND_END, "trailing", 4095)):
            assert probe(hook) == 0
            assert probe(CHECK) == 1, (hook, "the planted byte was not found, or not once")
            assert probe(CHECK) == 0, (hook, "the damaged band was not refilled")
            lines = [line for line in capfd.readouterr().err.splitlines() if line.startswith("gnnvc guard")]
            assert len(lines) == 1, lines
            m = LINE.fullmatch(lines[0])
            assert m and (m[4], int(m[5])) == (side, offset), lines[0]
            named.append((m[1], m[2], m[3]))
        assert len(set(named)) == 1 and int(named[0][1]) > 0, named   # the same buffer each time, named by its byte count
        trained_forward(e, oracle_model, g, "after the hooks")
        # with the switch off a new engine registers nothing ...
        assert probe(OFF) == 0
        alive = probe(ALIVE)
        plain = G.Engine(model_text, device=0)
        try:
            plain.set_weight_scale(g.ws)
            plain.upload_graph(g)
            trained_forward(plain, oracle_model, g, "switch off")
            assert probe(ALIVE) == alive
        finally:
            plain.close()
        assert probe(ALIVE) == alive and probe(CHECK) == 0
    finally:
        e.close()   # ... and one created while it was on is still looked up, checked and forgotten when it goes
    assert probe(CHECK) == 0
    assert probe(ALIVE) == none_yet
    assert probe(LIVE) == start


# ---------------------------------------------------------------- b. the trained model: every plan at the edge sizes

EDGE_GRAPHS = {
    "empty": lambda: gg.from_edge_list(0, [], []),
    "n1": lambda: gg.from_edge_list(1, [], [57]),
    "n13": mz.tiny13,
    "n63": lambda: gg.erdos_renyi(63, 250, 63),
    "n64": lambda: gg.erdos_renyi(64, 256, 64),
    "n65": lambda: gg.erdos_renyi(65, 260, 65),
    "n127": lambda: gg.erdos_renyi(127, 500, 127),
    "n129": lambda: gg.erdos_renyi(129, 520, 129),
    "n777_rounds": mz.rounds,
    "er3000": lambda: gg.erdos_renyi(3000, 12000, 3),
    "two_hubs": lambda: _two_hubs(600, (300, 500), 1500, 5),
}


def edge_graph(name):
    if ("edge", name) not in _want:
        _want["edge", name] = EDGE_GRAPHS[name]()
    return _want["edge", name]


@pytest.mark.parametrize("name", list(EDGE_GRAPHS))
def test_trained_model_every_plan_at_the_edge_sizes(model_text, oracle_model, probe, name):
    import gnn_mwvc_amd as G
    g = edge_graph(name)
    for options in ({}, HUB_OPTIONS):
        label = (name, "every plan" if options else "defaults")
        with watched(probe, label):
            e = G.Engine(model_text, device=0)
            try:
                for k, v in options.items():
                    e.set_option(k, v)
                e.set_weight_scale(g.ws)
                e.upload_graph(g)
                three_forwards(e, oracle_model, g, label)
                if options and name == "two_hubs":   # (the plans of the hub rows are really in force)
                    assert e.get_info("long_rows") > 0 and e.get_info("giant_rows") > 0
                held(probe, label)
            finally:
                e.close()


# ---------------------------------------------------------------- c. the trained model: a slice of the plan fuzz

@pytest.mark.parametrize("case", PLAN_CASES)
def test_trained_model_plan_fuzz_slice(model_text, oracle_model, probe, case):
    import torch
    import gnn_mwvc_amd as G
    from tests.test_gpu_fuzz import _graph, _options, _oracle_stage
    rng = np.random.default_rng(90_000 + case)
    g, opts = _graph(rng), _options(rng)
    label = (case, g.n, g.nnz, opts)
    with watched(probe, label):
        e = G.Engine(model_text, device=0)
        try:
            for k, v in opts.items():
                e.set_option(k, v)
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            three_forwards(e, oracle_model, g, label)
            held(probe, label)
            if case in PLAN_STAGE_CASES:
                # the 16-wide stages through the stage entry point, on the inputs the plans were built for, over the sub-ranges of
                # tests/test_gpu_fuzz.py::test_random_stage_inputs
                dev = torch.device("cuda:0")
                oracle_model.set_weight_scale(g.ws)
                h = _oracle_stage(oracle_model, g, 0, g.x().reshape(g.n, 1))
                lo = int(np.random.default_rng(70_000 + case).integers(0, g.n // 2)) // 64 * 64
                for st in (1, 2):
                    want = _oracle_stage(oracle_model, g, st, h)
                    hin = torch.zeros((g.n + 1, 16), dtype=torch.float32, device=dev)
                    hin[: g.n] = torch.from_numpy(h).to(dev)
                    for a, b in ((0, g.n), (lo, g.n), (0, max(64, lo))):
                        out = torch.full((g.n + 1, 16 if st == 1 else 1), 7.0, dtype=torch.float32, device=dev)
                        lg = torch.full((g.n + 1,), 7.0, dtype=torch.float32, device=dev)
                        torch.cuda.synchronize()
                        e.stage_forward_device(st, a, b, hin.data_ptr(), out.data_ptr(), lg.data_ptr() if st == 2 else 0)
                        e.synchronize()
                        got = out[a:b].cpu().numpy() if st == 1 else lg[a:b].cpu().numpy().reshape(-1, 1)
                        assert np.array_equal(bits(got), bits(want[a:b])), (label, "stage", st, a, b)
                    h = want
                held(probe, (label, "stage entry"))
        finally:
            e.close()


# ---------------------------------------------------------------- d. generic stages

@pytest.mark.parametrize("i", GENERIC_CASES)
def test_generic_fuzz_cases_single_engine(shim, probe, i):
    """tests/fuzz_harness.one_case: host forwards, the scaled input, an audited forward (gnnvc_forward_audited), device pointers and
    the crafted stage inputs of an admitted case; the layer-by-layer path of one that is not admitted."""
    with watched(probe, mz.describe(i)):
        fh.one_case(i, shim)


@pytest.mark.parametrize("i", GENERIC_MULTI)
def test_generic_fuzz_cases_on_several_parts(shim, probe, i):
    with watched(probe, mz.describe(i)):
        fh.one_case_multi(i, shim)


@pytest.mark.parametrize("gname", ["er1933", "hubs"])
@pytest.mark.parametrize("name", ["sparse32", "in64"])
def test_generic_live_column_gather(shim, probe, name, gname):
    """The live-column table and the packed rows at 100 %: every stage that may gather live columns does."""
    from tests import test_gpu_live_columns as lc
    label = ("live", name, gname)
    with watched(probe, label):
        e = lc.open_live("live", name, graph_of(gname), percent=100)
        try:
            for rep in range(3):
                lc.host_forward(shim, e, "live", name, gname, (label, rep))
            lc.host_forward(shim, e, "live", name, gname, (label, "audited"), audited=True)
            assert e.get_info("audit_failures") == 0, label
            assert any(kept > 0 for kept, _, _ in lc.read_outs(e)), (label, "no stage gathered live columns")
            held(probe, label)
        finally:
            e.close()


# ---------------------------------------------------------------- e. hand-off, growth and reuse

def generic_forward(shim, e, family, name, gname, label):
    from tests.test_gpu_generic_lifecycle import assert_forward
    g = graph_of(gname)
    if g.n == 0:
        sc, _ = e.forward(gh.FAMILIES[family].model_input(name, g))
        assert sc.shape == (0, gh.FAMILIES[family].out_width(name)), label
        return
    assert_forward(shim, e, family, name, gname, label)


def open_model(model_text, model):
    """The trained model, or the generic member ("shapes", "odd") with heavy and giant rows on `hubs`."""
    import gnn_mwvc_amd as G
    if model == "trained":
        return G.Engine(model_text, device=0)
    e = G.Engine(gh.text_of("shapes", "odd"), device=0)
    e.set_generic_heavy_rows(512)
    e.set_generic_giant_rows(600, 1)
    return e


def forward_on(shim, oracle_model, e, model, gname, label):
    if model == "trained":
        three_forwards(e, oracle_model, graph_of(gname), label)
    else:
        for rep in range(2):
            generic_forward(shim, e, "shapes", "odd", gname, (label, rep))


@pytest.mark.parametrize("route", gh.ROUTES)
@pytest.mark.parametrize("model", ["trained", "odd"])
def test_every_hand_off_route(shim, model_text, oracle_model, probe, model, route):
    g = graph_of("er1933")
    label = (model, route)
    with watched(probe, label):
        e = open_model(model_text, model)
        try:
            gh.hand_over(e, g, route)
            forward_on(shim, oracle_model, e, model, "er1933", label)
            held(probe, label)
            gh.hand_over(e, g, route)   # the same graph again, into buffers that fit it exactly
            forward_on(shim, oracle_model, e, model, "er1933", (label, "again"))
            held(probe, (label, "again"))
        finally:
            e.close()


@pytest.mark.parametrize("model", ["trained", "odd"])
def test_graphs_that_grow_on_one_engine(shim, model_text, oracle_model, probe, model):
    """gh.LIFECYCLE_SEQUENCE's graphs in ascending size first: every buffer sized by the graph is regrown to an exact fit each time
    (reserve() never shrinks, so in the listed order the later, smaller graphs run inside the larger one's buffers); then as listed."""
    ascending = sorted(set(gh.LIFECYCLE_SEQUENCE), key=lambda name: (graph_of(name).nnz, graph_of(name).n))
    assert ascending == ["empty", "one", "sparse", "er1933", "hubs"]   # 0, 0, 6 000, 14 000 and 33 718 entries
    with watched(probe, model):
        e = open_model(model_text, model)
        try:
            for k, gname in enumerate(ascending + gh.LIFECYCLE_SEQUENCE):
                label = (model, k, gname)
                gh.hand_over(e, graph_of(gname), ("upload", "staged7")[k % 2])
                forward_on(shim, oracle_model, e, model, gname, label)
                held(probe, label)
        finally:
            e.close()


@pytest.mark.parametrize("family,name", gh.DERIVE_MEMBERS)
def test_graphs_derived_on_the_device(probe, family, name):
    from tests.test_gpu_generic_lifecycle import _chain_wants
    fam = gh.FAMILIES[family]
    g = graph_of("hubs")
    with watched(probe, (family, name)):
        e = gh.open_engine(family, name, g, heavy=512, giant=(600, 1), expect_fused=True)
        try:
            _, lg = e.forward(fam.model_input(name, g))
            assert np.array_equal(bits(lg), bits(gh.want_of(family, name, "hubs")[-1][2]))
            held(probe, (name, "uploaded"))
            for step, (g1, old_row) in enumerate(gh.derive_chain()):
                e.derive_graph(g1, old_row)
                e.set_weight_scale(g1.ws)
                _, lg = e.forward(fam.model_input(name, g1))
                want = _chain_wants(family, name)[step]
                bad = np.argwhere(bits(lg) != bits(want))
                assert bad.size == 0, (name, step, f"{len(bad)}/{lg.size} logits differ", bad[:6].tolist())
                held(probe, (name, "derived", step))
        finally:
            e.close()


def test_trained_model_audited_and_repaired(model_text, oracle_model, probe):
    import gnn_mwvc_amd as G
    g = edge_graph("er3000")
    with watched(probe, "audit"):
        e = G.Engine(model_text, device=0)
        try:
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            trained_forward(e, oracle_model, g, "plain")
            for k, v in (("audit_period", 1), ("audit_repair", 1), ("audit_flip_stage", 1), ("audit_flip_row", g.n // 3 + 7)):
                e.set_option(k, v)
            repairs = e.get_info("audit_repairs")
            trained_forward(e, oracle_model, g, "flipped and repaired")
            assert e.get_info("audit_repairs") == repairs + 1
            e.set_option("audit_flip_stage", -1)
            trained_forward(e, oracle_model, g, "audited, clean")
            assert e.get_info("audit_repairs") == repairs + 1
            held(probe, "audit")
        finally:
            e.close()


# ---------------------------------------------------------------- f. several devices behind one handle

def _fuzz_multi():
    import importlib.util
    import pathlib
    if "fuzz_multi" not in _want:
        path = pathlib.Path(__file__).resolve().parents[1] / "scratch" / "experiments" / "fuzz_multi.py"
        spec = importlib.util.spec_from_file_location("fuzz_multi", path)
        _want["fuzz_multi"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_want["fuzz_multi"])
    return _want["fuzz_multi"]


@contextlib.contextmanager
def packing_traced():
    """Per forward of a multi-device handle inside the block: which of the two exchanged stages went out packed (None at a new
    graph).  A stage that is packed after one forward and not after the next on the same graph overflowed its exception list."""
    import gnn_mwvc_amd as G
    plain = G.Engine.forward, G.Engine.upload_graph, G.Engine.upload_graph_staged
    trace = []

    def forward(self, *a, **kw):
        out = plain[0](self, *a, **kw)
        trace.append((self.get_info("multi_packed_stage0"), self.get_info("multi_packed_stage1")))
        return out

    def upload(self, *a, **kw):
        trace.append(None)
        return plain[1](self, *a, **kw)

    def staged(self, *a, **kw):
        trace.append(None)
        return plain[2](self, *a, **kw)

    G.Engine.forward, G.Engine.upload_graph, G.Engine.upload_graph_staged = forward, upload, staged
    try:
        yield trace
    finally:
        G.Engine.forward, G.Engine.upload_graph, G.Engine.upload_graph_staged = plain


def overflows(trace):
    return sum(1 for a, b in zip(trace[:-1], trace[1:]) if a and b and any(x == 1 and y == 0 for x, y in zip(a, b)))


@pytest.mark.parametrize("pack", [0, 1])
@pytest.mark.parametrize("parts", [2, 3])
def test_trained_model_on_several_parts(probe, parts, pack):
    """Case 232 of scratch/experiments/fuzz_multi.py on two and three parts (two hub graphs on one handle, eight forwards each, one of
    them on an input of arbitrary values): with "multi_pack" 1 that input overflows the packed exchange's exception lists — they are
    filled to their last entry, the flag rises and the stage goes out in full rows from then on."""
    fm = _fuzz_multi()
    for push in (0, 1):
        label = ("fuzz_multi 232", parts, pack, push)
        with watched(probe, label), packing_traced() as trace:
            assert fm.one_case(232, override={"multi_pack": pack, "multi_push": push}, parts_override=parts) == 0, label
        print(f"guard bands: {label}: packed stages per forward {trace}")
        if pack:
            assert overflows(trace) >= 1, (label, "no exception list overflowed", trace)
        else:
            assert not any(t and any(t) for t in trace), (label, trace)


@pytest.mark.parametrize("parts", [2, 3, 5])
def test_generic_model_on_several_parts(shim, probe, parts):
    import gnn_mwvc_amd as G
    with watched(probe, ("odd", parts)):
        e = G.Engine(gh.text_of("shapes", "odd"), devices=[0] * parts, generic=True)
        try:
            for k, gname in enumerate(["er1933", "hubs", "one"]):
                gh.hand_over(e, graph_of(gname), ("upload", "staged7")[k % 2])
                for rep in range(2):
                    generic_forward(shim, e, "shapes", "odd", gname, (parts, gname, rep))
                held(probe, ("odd", parts, gname))
        finally:
            e.close()


# ---------------------------------------------------------------- g. host entry points

def test_host_entry_points(model_text, oracle_model, probe):
    """gnnvc_linear_forward, gnnvc_sgemm, gnnvc_stream_sum and the element-wise calls allocate for the call: their buffers are
    checked when they are freed, on the way out."""
    import gnn_mwvc_amd as G
    from oracle import oracle_py
    rng = np.random.default_rng(11)
    g = edge_graph("er3000")
    with watched(probe, "host entry points"):
        e = G.Engine(model_text, device=0)
        try:
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            trained_forward(e, oracle_model, g, "forward")
            h, W, b = (rng.standard_normal(s).astype(np.float32) for s in ((4, 5), (5, 3), (3,)))
            # (five products of magnitude < 10: a few fp32 roundings of 6e-7 each — tests/test_gpu_lifetime.py's bound)
            np.testing.assert_allclose(e.linear(h, W, b), h @ W + b, rtol=0, atol=1e-5)
            assert probe(CHECK) == 0, "linear"
            np.testing.assert_allclose(e.sgemm(h, W), h @ W, rtol=0, atol=1e-5)
            assert probe(CHECK) == 0, "sgemm"
            v = rng.uniform(0, 2, (3, 70)).astype(np.float32)
            assert np.array_equal(e.stream_sum(v), np.cumsum(v, axis=1, dtype=np.float32)[:, -1])   # (the sequential fp32 chain)
            assert probe(CHECK) == 0, "stream_sum"
            for rows in (1, 63, 65):
                r = rng.standard_normal((rows, 3)).astype(np.float32)
                assert np.array_equal(bits(e.relu(r)), bits(oracle_py.relu(r)))
            held(probe, "host entry points")
        finally:
            e.close()


class Piece(C.Structure):
    _fields_ = [("d_region", C.c_void_p), ("row_lo", C.c_uint32), ("row_hi", C.c_uint32)]


def test_pack_push_unpack_at_the_list_capacity(model_text, oracle_model, probe):
    """gnnvc_pack_rows / gnnvc_push_piece / gnnvc_unpack_pieces with an exception list of no entry, of exactly the entries the rows
    need and of one fewer (tests/test_gpu_parity.py::test_push_and_unpack_pieces_entry_points' input at n = 320).  The regions are
    the caller's: they end in eight words of a sentinel that must stay, since the bands do not see them."""
    import torch
    import gnn_mwvc_amd as G
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    n, kp, tail = 320, 8, 8
    feat = (rng.uniform(0.1, 2.0, (n + 1, 16)) * (rng.random((n + 1, 16)) < 0.3)).astype(np.float32)
    live = [1, 3, 4, 8, 9, 15]
    feat[:, [c for c in range(16) if c not in live]] = 0.0
    feat[rng.integers(0, n, 40), 2] = 0.75          # strays outside the mask: the exception list's
    feat[17, 3] = -0.0
    feat[n] = 0.0
    mask = sum(1 << c for c in live)
    strays = int((feat[:n, 2] != 0).sum())
    assert 20 < strays <= 40
    g = edge_graph("er3000")
    with watched(probe, "pack, push, unpack"):
        e = G.Engine(model_text, device=0)
        L = e._L
        L.gnnvc_push_piece.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.gnnvc_unpack_pieces.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        try:
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            trained_forward(e, oracle_model, g, "forward")
            src = torch.from_numpy(feat).to(dev)
            for cap, fits in ((0, False), (strays, True), (strays - 1, False)):
                words = n * kp + 4 + 4 * cap
                send = torch.zeros(words + tail, dtype=torch.float32, device=dev)
                send[words:] = 9.0
                flag = torch.zeros(1, dtype=torch.int32, device=dev)
                peers = [torch.full((words + tail,), 9.0, dtype=torch.float32, device=dev) for _ in range(3)]
                dst = (C.c_void_p * 3)(*[p.data_ptr() for p in peers])
                torch.cuda.synchronize()
                e._check(L.gnnvc_pack_rows(e._h, src.data_ptr(), 16, 0, n, mask, kp, send.data_ptr(), send.data_ptr() + n * kp * 4, cap,
                                           flag.data_ptr()))
                e._check(L.gnnvc_push_piece(e._h, send.data_ptr(), n, kp, cap, 3, dst, None))
                e.synchronize()
                assert int(flag.item()) == (0 if fits else 2), (cap, strays)
                assert int(send[n * kp:].view(torch.int32)[0].item()) == strays, cap   # (the count goes on past a full list)
                for q, region in enumerate([send] + peers):
                    assert bool((region[words:] == 9.0).all()), (cap, q, "words past the region were written")
                for q in range(3):
                    out = torch.full((n + 1, 16), 5.0, dtype=torch.float32, device=dev)
                    arr = (Piece * 1)(Piece(peers[q].data_ptr(), 0, n))
                    torch.cuda.synchronize()
                    e._check(L.gnnvc_unpack_pieces(e._h, arr, 1, cap, 16, mask, kp, out.data_ptr()))
                    e.synchronize()
                    got = out.cpu().numpy()
                    assert np.all(got[n] == 5.0), (cap, q)             # nothing outside the piece's rows is written
                    inside = np.ones(16, dtype=bool) if fits else np.isin(np.arange(16), live)   # (a short list loses strays only)
                    assert np.array_equal(bits(np.where(got[:n] == 0, np.float32(0), got[:n]))[:, inside],
                                          bits(np.where(feat[:n] == 0, np.float32(0), feat[:n]))[:, inside]), (cap, q)
            held(probe, "pack, push, unpack")
        finally:
            e.close()
