"""Link-level drop-in checks (build container only: needs /root/reference).

oracle/Makefile `make ref` compiles the reference's OWN translation units where
they lie and links them with this repo's host mirror:

  ref_layers.so       reference layers/predict  + our matrix TU  -> the oracle must agree
                      bit for bit with the reference's own code (quirk, sequencing, parser)
  GNN_VC_reflayers    reference driver + reference layers + our matrix TU
  GNN_VC_dropin       reference driver + OUR gnn_inference.cpp + OUR matrix.cpp

with the C ABI served by the oracle-backed test double (no GPU here).  The CLI
known answers (tests/golden/manifest.json) come from the unmodified reference
linked to real OpenBLAS, so matching them also confirms dot() == cblas_sgemm at
every shape the run exercised.

In ref_layers.so the products that the reference's dot() asks for come from the
oracle's chain.  For the trained shapes the chain is what OpenBLAS computes
(tests/test_openblas_seam.py).  For the generic-stage models of the second half
of this module it is the documented contract instead (DESIGN.md §3,
tests/golden/README.md): a stock OpenBLAS does not reproduce most of those
shapes.  So the comparisons of the reference's predict with the oracle's pin the
sequencing and buffer swapping, the graph layer's column layout, the parser,
the bias add, the activations and the widths — not the GEMM.
"""
import ctypes as C
import hashlib
import json
import pathlib
import subprocess

import numpy as np
import pytest

from oracle import oracle_py
from tools import graphgen as gg
from tools import make_golden_generic as mk
from tools import modelgen_fuzz as mz

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUT = ROOT / "oracle" / "_ref"
# what __graft_entry__.build() makes under oracle/_ref where the reference's sources can be read (`make -C oracle ref`)
BUILT = ("ref_layers.so", "GNN_VC_reflayers", "GNN_VC_dropin", "GNN_VC_dropin_fastio")

pytestmark = pytest.mark.skipif(not all((OUT / b).is_file() for b in BUILT),
                                reason="oracle/_ref not built (build() builds it only where the reference sources can be read)")


@pytest.fixture(scope="module")
def built():
    """oracle/_ref, with ref_layers.so brought up to this tree's oracle/ref_harness.cpp first where a build left behind by another
    revision lacks an entry point (tools/make_golden_generic.ensure_ref_layers says why make alone may not notice) — before any
    fixture below loads the library, since a loaded library is not loaded again from a rewritten file."""
    mk.ensure_ref_layers()
    return OUT


@pytest.fixture(scope="module")
def manifest(golden_dir):
    return json.loads((golden_dir / "manifest.json").read_text())


@pytest.fixture(scope="module")
def ref_layers(built):
    L = C.CDLL(str(built / "ref_layers.so"))
    L.ref_predict.argtypes = [C.c_char_p, C.c_int, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    L.ref_graph_layer.argtypes = [C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _ref_predict(L, text, keep, g, x):
    out = np.zeros(g.n * 35 + 8, dtype=np.float32)
    wd = C.c_uint32(0)
    rowptr = np.ascontiguousarray(g.rowptr, dtype=np.uint64)
    L.ref_predict(text.encode(), keep, C.c_float(g.ws), g.n, rowptr.ctypes.data, g.col.ctypes.data,
                  g.w.ctypes.data, x.ctypes.data, out.ctypes.data, C.byref(wd))
    return out[: g.n * wd.value].reshape(g.n, wd.value)


@pytest.mark.parametrize("maker", [
    lambda: gg.from_edge_list(3, [(0, 2), (1, 2)], [15, 15, 20]),
    lambda: gg.erdos_renyi(1000, 5000, 5),
    lambda: gg.rmat(10, 16, 10),
    lambda: gg.hub_graph(20000, 60000, 3, 4096, seed=7),
    lambda: gg.from_edge_list(130, [(0, i) for i in range(1, 40)], list(range(20, 150))),
])
def test_oracle_equals_reference_layer_code(ref_layers, oracle_model, model_text, maker):
    g = maker()
    oracle_model.set_weight_scale(g.ws)
    x = g.x()
    # every prefix that ends a fused stage, the logits, and the scores
    for keep, stop in ((7, 6), (14, 13), (20, 19), (-1, -1)):
        got = _ref_predict(ref_layers, model_text, keep, g, x)
        want = oracle_model.predict(g, x, stop_after=stop)
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (keep, stop)


QUIRK_WIDTHS = (1, 2, 3, 4, 5, 15, 16, 17, 32, 33, 47, 64)


def test_reference_graph_layer_quirk(ref_layers):
    """The reference copies `in` to columns f .. 2 f - 1, then overwrites columns f + 1 .. f + 3 with D, W / ws and NW / ws and
    leaves the rest zero: at every width below, which land those three elsewhere than f = 1 and f = 16 do."""
    g = gg.erdos_renyi(300, 1500, 3)
    rng = np.random.default_rng(0)
    rowptr = np.ascontiguousarray(g.rowptr, dtype=np.uint64)
    for f in QUIRK_WIDTHS:
        h = rng.normal(size=(g.n, f)).astype(np.float32)
        out = np.zeros((g.n, 2 * f + 3), dtype=np.float32)
        wd = ref_layers.ref_graph_layer(C.c_float(77.0), g.n, f, rowptr.ctypes.data, g.col.ctypes.data,
                                        g.w.ctypes.data, h.ctypes.data, out.ctypes.data)
        assert wd == 2 * f + 3
        want = oracle_py.graph_layer(g, 77.0, h)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), f
        # the layout, said once more without either implementation: what of the own row survives, and where the three land
        keep = [j for j in range(f) if not 1 <= j <= 3]
        assert np.array_equal(out[:, [f + j for j in keep]].view(np.uint32), h[:, keep].view(np.uint32)), f
        assert np.array_equal(out[:, f + 1], np.diff(g.rowptr.astype(np.int64)).astype(np.float32)), f
        assert np.array_equal(out[:, f + 2], g.w.astype(np.float32) / np.float32(77.0)), f
        assert np.array_equal(out[:, f + 3], g.nw.astype(np.float32) / np.float32(77.0)), f
        assert not out[:, [j for j in range(2 * f, 2 * f + 3) if j > f + 3]].any(), f


# ---------------------------------------------------------------- every generator's models, not the trained text alone
#
# The reference's parser, set_weight_scale and predict (ref_predict_wide: an n x in_width input, any layer sequence) against the
# oracle's, bit for bit and NaN with NaN, after every layer that ends a stage or a dense block, at the logits and after the last
# layer.  dot()'s products come from the oracle's chain in this build (see the module text): for these shapes that is the
# documented contract (tests/golden/README.md) — a stock OpenBLAS does not reproduce most of them — so what is pinned
# here is predict's sequencing and buffer swapping, the graph layer's column layout, the parser, the bias add, the activations
# (std::max(x, 0.0f) and 1 / (1 + expf(-x)), also on -0.0, NaN and +-inf) and the widths: not the GEMM.

DIFF_GRAPHS = ["ex3", "tiny13", "rounds", "iso5", "empty"]   # and hub2k: every member but the fuzz cases, of which every third
_FUZZ_BLOCKS = 8
_MEMBERS = mk.every_member()
_FAMILY_NAMES = ["shapes", "depths", "big", "feat", "live", "patterns", "trained"]


@pytest.fixture(scope="module")
def ref_wide(built):
    if not mk.ref_layers_current(built / "ref_layers.so"):
        pytest.skip("oracle/_ref/ref_layers.so predates ref_predict_wide and the reference's sources cannot be read to rebuild it")
    return mk.Reference(built / "ref_layers.so")


def _differential(ref, member, gnames):
    """-> number of comparisons made"""
    family, name = member
    text = mk.text_of(family, name)
    raw = text.encode()
    om = oracle_py.OracleModel(text)
    kinds = om.layer_kinds()
    assert kinds == mk.layer_kinds(text), member
    w_in = mk.in_width(family, name)
    wd = mk.widths_after(kinds, [W.shape for W, _ in om.linear_params()], w_in)
    done = 0
    for gname in gnames:
        g = mk.graph_of(gname)
        om.set_weight_scale(g.ws)
        x0 = mk.model_input(family, name, g)
        assert x0.shape == (g.n, w_in), member
        for label, x in (("model_input", x0), ("planted", mk.planted(x0, [ord(c) for c in gname]))):
            for cut in mk.cut_points(kinds):
                got = ref.predict(raw, cut + 1, g, x, wd[cut])
                want = om.predict(g, x, stop_after=cut)
                diff = mk.first_difference(got, want)
                assert diff is None, f"{member} on {gname}, {label}, after layer {cut} of {len(kinds)}: reference against oracle: {diff}"
                done += 1
            # keep = -1 is every layer
            assert mk.same(ref.predict(raw, -1, g, x, wd[-1]), got), (member, gname, label)
    return done


@pytest.mark.parametrize("family", _FAMILY_NAMES)
def test_oracle_equals_reference_layer_code_on_every_family_member(ref_wide, family):
    members = [m for m in _MEMBERS if m[0] == family]
    assert members
    for member in members:
        assert _differential(ref_wide, member, DIFF_GRAPHS + ["hub2k"]) >= 2 * 6


@pytest.mark.parametrize("block", range(_FUZZ_BLOCKS))
def test_oracle_equals_reference_layer_code_on_every_fuzz_case(ref_wide, block):
    cases = [m for m in _MEMBERS if m[0] == "fuzz"]
    assert len(cases) == mz.N + len(mz.REGRESSIONS)
    for member in cases[block::_FUZZ_BLOCKS]:
        hub = ["hub2k"] if int(member[1]) % 3 == 0 else []
        assert _differential(ref_wide, member, DIFF_GRAPHS + hub) >= 2 * 5


def test_the_differential_covers_what_it_is_for():
    """From the members' own layer kinds: an opening Linear_Layer, no Graph_Layer, endings in a ReLU and in a bare linear layer,
    two graph layers in a row, a sigmoid inside, inputs and outputs more than one column wide, and graph layers at widths other
    than 1 and 16."""
    seen, graph_widths = set(), set()
    for family, name in _MEMBERS:
        text = mk.text_of(family, name)
        kinds = mk.layer_kinds(text)
        shapes = [tuple(int(v) for v in line.split()[1:]) for line in text.splitlines() if line.startswith("Weights:")]
        w_in = mk.in_width(family, name)
        wd = mk.widths_after(kinds, shapes, w_in)
        graph_widths |= {([w_in] + wd)[i] for i, k in enumerate(kinds) if k == mk.GRAPH}
        seen |= {"opens linear"} if kinds[0] == mk.LINEAR else set()
        seen |= {"no graph layer"} if mk.GRAPH not in kinds else set()
        seen |= {("ends", kinds[-1])}
        seen |= {"two graphs"} if any(a == b == mk.GRAPH for a, b in zip(kinds, kinds[1:])) else set()
        seen |= {"mid sigmoid"} if mk.SIGMOID in kinds[:-1] else set()
        seen |= {"wide input"} if w_in > 1 else set()
        seen |= {"wide output"} if wd[-1] > 1 else set()
    assert seen >= {"opens linear", "no graph layer", ("ends", mk.RELU), ("ends", mk.LINEAR), ("ends", mk.SIGMOID), "two graphs",
                    "mid sigmoid", "wide input", "wide output"}
    assert graph_widths >= {1, 2, 3, 4, 5, 16, 17, 33, 64}, sorted(graph_widths)


def test_ref_predict_wide_refuses_a_short_buffer(ref_wide, ref_layers):
    g = mk.graph_of("tiny13")
    text = mk.text_of("feat", "out64")
    x = mk.model_input("feat", "out64", g)
    rc, wd, out = ref_wide.call(text, -1, g, x, g.n * 64 - 1)
    assert rc != 0 and wd == 64 and (out == np.float32(-7.0)).all()      # refused, the width reported, nothing written
    rc, wd, out = ref_wide.call(text, -1, g, x, g.n * 64)
    assert rc == 0 and wd == 64 and not (out == np.float32(-7.0)).any()
    # ref_predict, the entry point of tools/make_golden_layers.py, is the n x 1 case of it
    t1 = mk.text_of("shapes", "odd")
    x1 = mk.model_input("shapes", "odd", g)
    assert np.array_equal(_ref_predict(ref_layers, t1, 7, g, x1.reshape(-1)).view(np.uint32), ref_wide.predict(t1, 7, g, x1, 5).view(np.uint32))


@pytest.mark.parametrize("maker", [
    lambda: gg.erdos_renyi(3000, 6000, 5),                 # sparse: many degree-1/2 vertices, twins, dominations
    lambda: gg.erdos_renyi(2000, 12000, 6),
    lambda: gg.rmat(11, 4, 10),
    lambda: gg.from_edge_list(9, [(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5), (5, 6), (7, 8)],
                              [20, 30, 40, 25, 25, 60, 10, 5, 5]),
    lambda: gg.from_edge_list(6, [(0, 2), (0, 3), (1, 2), (1, 3), (4, 5)], [10, 10, 20, 20, 7, 7]),  # twins 0 and 1
    lambda: gg.erdos_renyi(1500, 2200, 8, lo=1, hi=9),     # small weights: the meta rules fire often
    lambda: gg.erdos_renyi(800, 3000, 9, lo=1, hi=40),
    # u larger than all of its own neighbours: neighborhood_difference's unfiltered tail copies u itself
    lambda: gg.from_edge_list(8, [(0, 7), (1, 7), (7, 6), (6, 2), (6, 3), (2, 3), (4, 5)], [3, 4, 9, 2, 6, 6, 12, 5]),
])
def test_reduction_predicates_match_reference_methods(ref_layers, maker):
    """oracle_reduction_flags against the reference's own is_twin / is_dominating / is_isolated."""
    g = maker()
    ref_layers.ref_reduction_flags.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                               C.c_void_p]
    want = np.zeros(g.n, dtype=np.uint8)
    rowptr = np.ascontiguousarray(g.rowptr, dtype=np.uint64)
    ref_layers.ref_reduction_flags(g.n, rowptr.ctypes.data, g.col.ctypes.data, g.w.ctypes.data, 20,
                                   want.ctypes.data)
    got = oracle_py.reduction_flags(g, 20)
    assert np.array_equal(got & 0x1F, want & 0x1F)
    # the two small-solver rules: the oracle's restatement against the reference's own rule functions, each
    # called on a fresh copy of the graph (they apply the reduction when they fire)
    ref_layers.ref_meta_flags.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    meta = np.zeros(g.n, dtype=np.uint8)
    ref_layers.ref_meta_flags(g.n, rowptr.ctypes.data, g.col.ctypes.data, g.w.ctypes.data, 20, meta.ctypes.data)
    assert np.array_equal(got & 0x60, meta), np.flatnonzero((got & 0x60) != meta)[:10]


@pytest.mark.parametrize("maker", [
    lambda: gg.erdos_renyi(3000, 6000, 5),
    lambda: gg.erdos_renyi(20000, 30000, 6),
    lambda: gg.erdos_renyi(30000, 90000, 7),
    lambda: gg.rmat(13, 4, 3),                             # hubs: the marks budget drops the flags
    lambda: gg.erdos_renyi(1500, 2200, 8, lo=1, hi=9),
    lambda: gg.from_edge_list(6, [(0, 2), (0, 3), (1, 2), (1, 3), (4, 5)], [10, 10, 20, 20, 7, 7]),
])
def test_flagged_reduce_is_the_reference_reduce(ref_layers, maker):
    """host/flagged_reduce.hpp (the consumer of the device flags: skips a first test of a vertex whose flags
    say no rule applies and whose 2-hop neighbourhood is untouched) against the reference's own reduce_graph on
    copies of the same graph: identical reduced graph, cover marks and offset (rc 0)."""
    g = maker()
    L = ref_layers
    L.ref_flagged_reduce_check.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    flags = oracle_py.reduction_flags(g, 20)
    rowptr = np.ascontiguousarray(g.rowptr, dtype=np.uint64)
    stats = np.zeros(4)
    rc = L.ref_flagged_reduce_check(g.n, rowptr.ctypes.data, g.col.ctypes.data, g.w.ctypes.data,
                                    flags.ctypes.data, stats.ctypes.data)
    assert rc == 0, (rc, stats)
    assert stats[3] > 0


def _run_cli(binary, graph_path, out_path):
    r = subprocess.run([str(binary), str(graph_path), str(out_path), "0", "-1", "0"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip()


@pytest.mark.parametrize("binary", ["GNN_VC_reflayers", "GNN_VC_dropin"])
def test_cli_readme_graph(built, manifest, tmp_path, binary):
    (tmp_path / "ex3.graph").write_text("3 2 10\n15 3\n15 3\n20 1 2\n")
    out = _run_cli(built / binary, tmp_path / "ex3.graph", tmp_path / "ex3.out")
    spec = manifest["ex3"]["cli"]
    assert out.startswith(spec["stdout_prefix"])
    assert out.split(",")[6] == str(spec["final_cost"])
    assert [int(v) for v in (tmp_path / "ex3.out").read_text().split()] == spec["cover"]


@pytest.mark.slow
@pytest.mark.parametrize("binary", ["GNN_VC_reflayers", "GNN_VC_dropin"])
def test_cli_er100k_identical_cover(built, manifest, golden_dir, tmp_path, binary):
    spec = manifest["er100k"]
    p = spec["graph"]
    g = gg.erdos_renyi(p["n"], p["m"], p["seed"])
    text = gg.metis_text(g)
    assert hashlib.md5(text.encode()).hexdigest() == spec["metis_md5"]
    (tmp_path / "er100k.graph").write_text(text)
    out = _run_cli(built / binary, tmp_path / "er100k.graph", tmp_path / "er100k.out")
    fields = out.split(",")
    assert fields[0] == "er100k" and int(fields[1]) == spec["cli"]["final_cost"]
    raw = (tmp_path / "er100k.out").read_bytes()
    assert hashlib.md5(raw).hexdigest() == spec["cli"]["result_md5"]
    cover = np.array(raw.split(), dtype=np.uint8)
    gold = np.unpackbits(np.fromfile(golden_dir / spec["cli"]["cover_bits_file"], dtype=np.uint8))[: p["n"]]
    assert np.array_equal(cover, gold)
    # identical final vertex-cover weight on this integer-weighted graph
    assert int(g.w[cover == 1].astype(np.int64).sum()) == spec["cli"]["final_cost"]


def test_fast_io_driver_is_the_same_program(built, tmp_path):
    """oracle/ref_driver_fastio.cpp: the reference's driver with this repo's METIS reader behind parse_graph and
    unflushed result writes, against the plain drop-in: same stdout cost fields, byte-identical
    result files."""
    (tmp_path / "ex3.graph").write_text("3 2 10\n15 3\n15 3\n20 1 2\n")
    g = gg.erdos_renyi(30000, 150000, 13)
    (tmp_path / "g.graph").write_text(gg.metis_text(g))
    for name in ("ex3", "g"):
        res = []
        for binary in ("GNN_VC_dropin", "GNN_VC_dropin_fastio"):
            out = tmp_path / f"{name}.{binary}.out"
            r = subprocess.run([str(built / binary), str(tmp_path / f"{name}.graph"), str(out), "0", "-1", "0"],
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
            f = r.stdout.strip().split(",")
            res.append((f[0], f[1], f[2], out.read_bytes()))     # name, cost, best seen; (the last field is a time)
        assert res[0] == res[1], name
    assert len(res[0][3]) == 2 * g.n
