#!/usr/bin/env python3
"""The generic-stage fixtures of tests/golden (tests/golden/generic/*.f32, tests/golden/manifest_generic.json), and the one table of
(family, member) models that the tests of the oracle's pin share: tests/test_dropin_link.py (reference's layer code == oracle, every
member), tests/test_refgold.py (oracle == fixtures, no reference needed) and tests/test_gpu_refgold.py (engine == fixtures, no
oracle and no reference).

Run as a script — build container only, it needs the reference's sources — it writes the fixtures:

Who computes them: the reference's OWN layer code — src/gnn_inference.cpp compiled where it lies into oracle/_ref/ref_layers.so
(`make -C oracle ref`) — through ref_predict_wide (oracle/ref_harness.cpp): gnn::model's parser, set_weight_scale and predict
on the member's text, truncated after the layer asked for.  The products its dot() asks for come from the CHAIN, the fmaf chain
of the oracle that is the engine's documented contract for these shapes — NOT from OpenBLAS, unlike the trained
model's fixtures (tools/make_golden_layers.py): a stock OpenBLAS does not reproduce the chain at most of these shapes.  So
the fixtures pin predict's sequencing and buffer swapping, the graph layer's column layout, the parser, the bias add, the
activations and the widths — not the GEMM.  The script asserts that the oracle agrees bit for bit (NaN with NaN) before it writes
anything.  Then, with the genuine OpenBLAS that SciPy bundles behind dot(), it counts how many of the arrays come out the same,
and records the count in the manifest (data only; nothing asserts it).

Per (member, graph): the rows after every layer that ends a stage or a dense block, the logits (a model that ends in the sigmoid)
and the output of the last layer, little-endian fp32, row-major, packed into files of less than 256 KiB.  Inputs are not stored:
the graphs are regenerated from the parameters in the manifest and the input is the member's own model_input.
"""
import ctypes as C
import hashlib
import json
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
from tools import graphgen as gg  # noqa: E402
from tools import modelgen, modelgen_big, modelgen_depths, modelgen_feat, modelgen_live, modelgen_shapes  # noqa: E402
from tools import modelgen_fuzz as mz  # noqa: E402
from tools import modelgen_patterns as mp  # noqa: E402

GOLD = ROOT / "tests" / "golden"
SUBDIR = "generic"
MANIFEST = GOLD / "manifest_generic.json"
MAX_FILE_BYTES = 256 * 1024 - 1
MAX_SET_BYTES = 3 * 1024 * 1024 - 1

LINEAR, GRAPH, RELU, SIGMOID = 0, 1, 2, 3
TABLE_FAMILIES = {"shapes": modelgen_shapes, "depths": modelgen_depths, "big": modelgen_big, "feat": modelgen_feat,
                  "live": modelgen_live}
FULL_LDS = mz.FULL_LDS

# ---------------------------------------------------------------- graphs

GRAPH_PARAMS = {
    "ex3": {"kind": "edge_list", "n": 3, "edges": [[0, 2], [1, 2]], "weights": [15, 15, 20]},          # the README's graph
    "tiny13": {"kind": "modelgen_fuzz", "name": "tiny13"},
    "rounds": {"kind": "modelgen_fuzz", "name": "rounds"},
    "iso5": {"kind": "edge_list", "n": 5, "edges": [[0, 1]], "weights": [20, 30, 40, 50, 120]},         # test_isolated_vertices'
    "empty": {"kind": "edge_list", "n": 0, "edges": [], "weights": []},
    "hub2k": {"kind": "hub_graph", "n": 2000, "m": 6000, "hubs": 2, "hub_degree": 1500, "seed": 78},    # manifest_layers.json's
}
FIXTURE_GRAPHS = ["ex3", "tiny13", "rounds"]
_graphs = {}


def make_graph(p):
    if p["kind"] == "edge_list":
        return gg.from_edge_list(p["n"], [tuple(e) for e in p["edges"]], p["weights"])
    if p["kind"] == "modelgen_fuzz":
        return mz.NEW_GRAPHS[p["name"]]()
    return gg.hub_graph(p["n"], p["m"], p["hubs"], p["hub_degree"], seed=p["seed"])


def graph_of(gname):
    if gname not in _graphs:
        _graphs[gname] = make_graph(GRAPH_PARAMS[gname])
    return _graphs[gname]


# ---------------------------------------------------------------- members: (family, name), name a string (a fuzz case: its number)

def every_member():
    """Every model of the generators: the five table families, the patterns family (the odd ones included), tools/modelgen.py's
    trained-shape models, and fuzz cases 0 .. N - 1 plus REGRESSIONS."""
    out = [(fam, name) for fam, m in TABLE_FAMILIES.items() for name in m.SPECS]
    out += [("patterns", name) for name in mp.NAMES] + [("trained", name) for name in modelgen.FAMILY]
    return out + [("fuzz", str(i)) for i in list(range(mz.N)) + list(mz.REGRESSIONS)]


def text_of(family, name):
    if family in TABLE_FAMILIES:
        return TABLE_FAMILIES[family].FAMILY[name]()
    return mp.FAMILY[name]() if family == "patterns" else modelgen.FAMILY[name]() if family == "trained" else mz.text(int(name))


def model_input(family, name, g):
    """The member's own input for graph g, n x in_width."""
    if family in TABLE_FAMILIES:
        x = TABLE_FAMILIES[family].model_input(name, g)
    else:
        x = mp.model_input(name, g) if family == "patterns" else g.x() if family == "trained" else mz.model_input(int(name), g)
    return np.ascontiguousarray(x, dtype=np.float32).reshape(g.n, -1 if g.n else in_width(family, name))


def model_of(family, name):
    """(in_width, prologue or None, stages, ending) of a member that is a stage list; None for the others (patterns' odd ones,
    fuzz cases that no setting admits)."""
    if family in TABLE_FAMILIES:
        f, stages = TABLE_FAMILIES[family].SPECS[name]
        return f, None, [tuple(ws) for ws in stages], "sigmoid"
    if family == "trained":
        return 1, None, [(32, 32, 16), (32, 32, 16), (32, 16, 1)], "sigmoid"
    if family == "patterns":
        return None if name in mp.ODD else mp.SPECS[name]
    c = mz.case(int(name))
    return (c.in_width, c.prologue, c.stages, c.ending) if c.admitted else None


def in_width(family, name):
    m = model_of(family, name)
    return m[0] if m else mp.in_width(name) if family == "patterns" else mz.case(int(name)).in_width


def config_of(family, name):
    """(patterns mask, feature width, big-stage LDS limit): the least opt-ins under which the engine fuses the member — for a
    fuzz case tools/modelgen_fuzz.least_config, otherwise what the member's family says in its own tables — or None for a
    member that stays layer by layer under every setting."""
    m = model_of(family, name)
    if m is None or mz.least_config(*m) is None:
        return None
    if family == "fuzz":
        return mz.least_config(*m)
    if family == "patterns":
        return mp.MASK[name], 64 if name in mp.NEEDS_FEAT else 0, FULL_LDS if name in mp.NEEDS_BIG else 0
    if family == "feat":
        return 0, 64, FULL_LDS if name in modelgen_feat.NEEDS_BIG else 0
    if family == "live":
        return 0, 64 if name in modelgen_live.NEEDS_FEAT else 0, 0
    return 0, 0, FULL_LDS if family == "big" else 0


def stages_of(family, name):
    """[(dense, f, widths, end code)] as the engine lists the member's stages under config_of; None where it lists none."""
    cfg = config_of(family, name)
    if cfg is None:
        return None
    ex = mz.expect(*model_of(family, name), *cfg)
    return None if ex is None else [(int(r.dense), int(r.f), [int(n) for n in r.widths], int(r.end)) for r in ex]


def layer_kinds(seq_or_text):
    """Layer kinds from a model text: LINEAR, GRAPH, RELU, SIGMOID per record, by the record's first word."""
    names = {"Linear_Layer": LINEAR, "Graph_Layer": GRAPH, "ReLU_Activation": RELU, "Sigmoid_Activation": SIGMOID}
    return [names[w] for w in seq_or_text.split() if w in names]


def cut_points(kinds):
    """The layer indices a comparison is made after: every layer in front of a Graph_Layer (the end of a stage or of a dense
    block), the input of a closing sigmoid (the logits), and the last layer."""
    n = len(kinds)
    cuts = {i for i in range(n - 1) if kinds[i + 1] == GRAPH} | {n - 1}
    if kinds[-1] == SIGMOID and n >= 2:
        cuts.add(n - 2)
    return sorted(cuts)


def widths_after(kinds, shapes, w):
    """Row width after every layer: shapes = (k, n) of the linear layers in order, w the input width."""
    it, out = iter(shapes), []
    for k in kinds:
        w = next(it)[1] if k == LINEAR else 2 * w + 3 if k == GRAPH else w
        out.append(w)
    return out


SPECIALS = [np.nan, np.inf, -np.inf, -0.0, 1e-45, -1e-40, 3e38, -3e38]


def planted(x, seed):
    """x with NaN, +-inf, -0.0, two denormals and +-3e38 written over some of its values: 8 per 200 values, at least one, at
    most half of them, at positions and in an order drawn from [41, *seed]."""
    x = np.array(x, dtype=np.float32, copy=True)
    k = min(8 * max(1, x.size // 200), x.size // 2) if x.size > 1 else x.size
    rng = np.random.default_rng([41] + list(seed))
    at = rng.choice(x.size, size=k, replace=False) if k else np.zeros(0, dtype=np.int64)
    first = int(rng.integers(len(SPECIALS)))
    flat = x.reshape(-1)
    for j, p in enumerate(at.tolist()):
        flat[p] = np.float32(SPECIALS[(first + j) % len(SPECIALS)])
    return x


def same(a, b):
    """Bit for bit, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def first_difference(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return f"shapes {a.shape} and {b.shape}"
    bad = np.argwhere(~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
    if not len(bad):
        return None
    r, c = bad[0].tolist()
    return f"{len(bad)} of {a.size} values differ, first at (row {r}, column {c}): {a[r, c]!r} against {b[r, c]!r}"


# ---------------------------------------------------------------- the reference's entry point

REF_LAYERS = ROOT / "oracle" / "_ref" / "ref_layers.so"


def ref_layers_current(path=REF_LAYERS) -> bool:
    """Does the built ref_layers.so hold ref_predict_wide?  Asked of the file's bytes, before anything loads it."""
    return path.is_file() and b"ref_predict_wide" in path.read_bytes()


def ensure_ref_layers() -> bool:
    """oracle/_ref/ref_layers.so with ref_predict_wide in it, rebuilt where an earlier build lacks it.  make goes by the files'
    times, and a tree whose sources were written out with times older than a build left behind by another revision looks
    up to date to it — so this asks the library itself and then tells make that oracle/ref_harness.cpp is new.  False where
    the library lacks the entry point and cannot be rebuilt (no reference sources)."""
    if ref_layers_current():
        return True
    if subprocess.run(["make", "-s", "-C", str(ROOT / "oracle"), "ref-available"], capture_output=True).returncode != 0:
        return False
    r = subprocess.run(["make", "-C", str(ROOT / "oracle"), "-W", "ref_harness.cpp", "_ref/ref_layers.so"],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("oracle/_ref/ref_layers.so could not be rebuilt:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    return ref_layers_current()


class Reference:
    """oracle/_ref/ref_layers.so's ref_predict_wide."""

    def __init__(self, path=None):
        self.L = C.CDLL(str(path or REF_LAYERS))
        self.L.ref_predict_wide.restype = C.c_int
        self.L.ref_predict_wide.argtypes = [C.c_char_p, C.c_int, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]
        self.L.gnnvc_test_cblas_calls.restype = C.c_ulong
        self.L.gnnvc_test_set_cblas_sgemm.argtypes = [C.c_void_p]

    def call(self, text, keep, g, x, capacity):
        """(return code, width, the output buffer of `capacity` floats filled with a sentinel first)"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        rowptr = np.ascontiguousarray(g.rowptr, dtype=np.uint64)
        col = np.ascontiguousarray(g.col, dtype=np.uint32)
        w = np.ascontiguousarray(g.w, dtype=np.uint32)
        out = np.full(max(capacity, 1), -7.0, dtype=np.float32)
        wd = C.c_uint32(0)
        rc = self.L.ref_predict_wide(text if isinstance(text, bytes) else text.encode(), keep, C.c_float(g.ws), g.n,
                                     rowptr.ctypes.data, col.ctypes.data, w.ctypes.data, x.shape[1], x.ctypes.data,
                                     out.ctypes.data, capacity, C.byref(wd))
        return rc, wd.value, out

    def predict(self, text, keep, g, x, width):
        """The rows after layer keep - 1 (keep = -1: after the last), n x width: width is what the caller expects, and the
        entry point must report the same."""
        rc, wd, out = self.call(text, keep, g, x, g.n * width)
        assert rc == 0 and wd == width, (rc, wd, width)
        return out[: g.n * width].reshape(g.n, width).copy()


# ---------------------------------------------------------------- the fixtures' members

HUB2K_MEMBERS = [("shapes", "narrow"), ("depths", "one_each"), ("patterns", "embed")]   # every stage output at most 16 wide
MULTI_MEMBERS = [("shapes", "odd"), ("depths", "six_deep"), ("patterns", "embed"), ("feat", "f33")]
TABLE_MEMBERS = [
    ("shapes", "narrow"),            # f = 1, 4, 4
    ("shapes", "odd"),               # f = 1, 5, 9
    ("shapes", "in3"),               # f = 3, 16, 16
    ("depths", "one_each"),          # one dense layer a stage
    ("depths", "six_deep"),          # six
    ("big", "h128"),                 # 128-wide hidden layers
    ("feat", "f33"),                 # f = 33
    ("feat", "in40"),                # a 40-wide input
    ("feat", "out64"),               # 64 outputs
    ("live", "in2"),                 # a 2-wide input, f = 2
    ("live", "in17"),                # f = 17
    ("live", "in64"),                # f = 64
    ("patterns", "embed"),           # a dense prologue
    ("patterns", "mlp"),             # no graph layer
    ("patterns", "relu_end"),        # ends in a ReLU
    ("patterns", "linear_end"),      # ends in its bare linear layer
    ("patterns", "linear_end17"),    # 2-wide input, 17 bare outputs
    ("patterns", "two_graphs"),      # stays layer by layer: two graph layers in a row
    ("patterns", "mid_sigmoid"),     # stays layer by layer: a sigmoid inside
    ("trained", "saturating_1"),     # tools/modelgen.py's saturating
]
# 24 admitted fuzz cases: chosen once, greedily, so that together they reach every model-side route kind of
# tests/test_modelgen_fuzz.py's AT_LEAST_THREE list with the fewest output columns (tests/test_refgold.py recomputes what they reach)
FUZZ_CASES = [15, 19, 23, 24, 37, 53, 58, 66, 68, 84, 93, 96, 108, 117, 138, 145, 150, 171, 182, 189, 193, 218, 219, 226]
LAYER_BY_LAYER = [("patterns", "two_graphs"), ("patterns", "mid_sigmoid")]


def fixture_members():
    return TABLE_MEMBERS + [("fuzz", str(i)) for i in FUZZ_CASES]


def fixture_graphs(member):
    return FIXTURE_GRAPHS + (["hub2k"] if member in HUB2K_MEMBERS else [])


def key_of(member):
    return f"{member[0]}.{member[1]}"


def read_arrays(entry, gname, gold=GOLD):
    """{layer index: array} of a manifest entry's graph, md5 checked."""
    out, raw = {}, {}
    for a in entry["graphs"][gname]["arrays"]:
        if a["file"] not in raw:
            raw[a["file"]] = (gold / a["file"]).read_bytes()
        rows, cols = a["shape"]
        blob = raw[a["file"]][a["offset"]: a["offset"] + 4 * rows * cols]
        assert len(blob) == 4 * rows * cols and hashlib.md5(blob).hexdigest() == a["md5"], (a["file"], a["after_layer_index"])
        out[a["after_layer_index"]] = np.frombuffer(blob, dtype="<f4").reshape(rows, cols).astype(np.float32)
    return out


# ---------------------------------------------------------------- the recipe

def _openblas():
    from oracle import oracle_py
    hit = oracle_py.find_openblas()
    if hit is None:
        return None, None
    blas = C.CDLL(hit[0])
    cfg = ""
    for name in ("scipy_openblas_get_config", "openblas_get_config"):
        if hasattr(blas, name):
            f = getattr(blas, name)
            f.restype = C.c_char_p
            cfg = f().decode()
            break
    for name in ("scipy_openblas_set_num_threads", "openblas_set_num_threads"):   # (one thread: the count below does not depend on the host's CPUs)
        if hasattr(blas, name):
            getattr(blas, name)(1)
            break
    return (blas, getattr(blas, hit[1])), f"{pathlib.Path(hit[0]).name}:{hit[1]} [{cfg.strip()}]"


def main():
    from oracle import oracle_py
    r = subprocess.run(["make", "-C", str(ROOT / "oracle"), "ref"], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("oracle/_ref build failed (needs the reference's sources):\n" + r.stderr[-2000:])
    if not ensure_ref_layers():
        sys.exit("oracle/_ref/ref_layers.so lacks ref_predict_wide and cannot be rebuilt")
    ref = Reference()
    ref.L.gnnvc_test_set_cblas_sgemm(None)
    manifest = {"_generated_by": "tools/make_golden_generic.py",
                "_chain": "reference src/gnn_inference.cpp (compiled where it lies): parser, set_weight_scale, predict -> dot() -> "
                          "the oracle's fmaf chain (NOT OpenBLAS: the contract for these shapes is the chain)",
                "_input_rules": {"model_input": "the member's own model_input(g): x = W / ws, and for a wider input the columns "
                                                "x, 0.37 x, 1 - x, 3 x, 4 x, ... (tools/modelgen_generic.Family.model_input)"},
                "graphs": {}, "members": {}}
    for gname in FIXTURE_GRAPHS + ["hub2k"]:
        g = graph_of(gname)
        manifest["graphs"][gname] = {"graph": GRAPH_PARAMS[gname], "n": int(g.n), "ws": float(g.ws), "metis_md5": gg.metis_md5(g)}
    (GOLD / SUBDIR).mkdir(exist_ok=True)
    written, total, computed = set(), 0, []
    for member in fixture_members():
        family, name = member
        text = text_of(family, name)
        om = oracle_py.OracleModel(text)
        kinds = om.layer_kinds()
        assert kinds == layer_kinds(text)
        wd = widths_after(kinds, [W.shape for W, _ in om.linear_params()], in_width(family, name))
        cuts = cut_points(kinds)
        st, cfg = stages_of(family, name), config_of(family, name)
        assert (st is None) == (member in LAYER_BY_LAYER), member
        entry = {"family": family, "member": name, "text_sha256": hashlib.sha256(text.encode()).hexdigest(),
                 "first_line": text.split("\n", 1)[0], "num_layers": len(kinds), "in_width": in_width(family, name),
                 "out_width": wd[-1], "ends_in_sigmoid": kinds[-1] == SIGMOID, "input": "model_input",
                 "config": None if cfg is None else {"patterns": cfg[0], "feature_width": cfg[1], "big_stages_lds": cfg[2]},
                 "stages": None if st is None else [{"dense": d, "f": f, "widths": ws, "end": e} for d, f, ws, e in st],
                 "graphs": {}}
        if st is not None:   # a fused member's stage ends are the cuts in front of a graph layer and the last layer
            ends = [c for c in cuts if not (kinds[-1] == SIGMOID and c == len(kinds) - 2)]
            assert [wd[c] for c in ends] == [ws[-1] for _, _, ws, _ in st], member
        for gname in fixture_graphs(member):
            g = graph_of(gname)
            om.set_weight_scale(g.ws)
            x = model_input(family, name, g)
            arrays, part, blob = [], 0, b""
            fname = lambda p: f"{SUBDIR}/{key_of(member)}.{gname}.p{p}.f32"
            for c in cuts:
                res = ref.predict(text, c + 1, g, x, wd[c])
                diff = first_difference(res, om.predict(g, x, stop_after=c))
                assert diff is None, f"the oracle differs from the reference at {member} on {gname} after layer {c}: {diff}"
                raw = res.astype("<f4").tobytes()
                assert len(raw) <= MAX_FILE_BYTES, (member, gname, c, len(raw))
                if blob and len(blob) + len(raw) > MAX_FILE_BYTES:
                    (GOLD / fname(part)).write_bytes(blob)
                    written.add(fname(part))
                    total += len(blob)
                    part, blob = part + 1, b""
                what = "output" if c == len(kinds) - 1 else "logits" if kinds[-1] == SIGMOID and c == len(kinds) - 2 else "block"
                arrays.append({"after_layer_index": c, "what": what, "file": fname(part), "offset": len(blob),
                               "shape": list(res.shape), "md5": hashlib.md5(raw).hexdigest()})
                blob += raw
                computed.append((text, c, gname, x, wd[c], res))
            (GOLD / fname(part)).write_bytes(blob)
            written.add(fname(part))
            total += len(blob)
            entry["graphs"][gname] = {"arrays": arrays}
        manifest["members"][key_of(member)] = entry
        print(key_of(member), {gname: len(v["arrays"]) for gname, v in entry["graphs"].items()})
    assert total <= MAX_SET_BYTES, total
    for old in sorted((GOLD / SUBDIR).glob("*.f32")):
        if f"{SUBDIR}/{old.name}" not in written:
            old.unlink()
    # data only: how many of the arrays a stock OpenBLAS behind dot() reproduces
    blas, desc = _openblas()
    if blas is not None:
        ref.L.gnnvc_test_set_cblas_sgemm(C.cast(blas[1], C.c_void_p))
        equal, members = 0, {}
        for text, c, gname, x, width, res in computed:
            got = ref.predict(text, c + 1, graph_of(gname), x, width)
            ok = same(got, res)
            equal += ok
            first = text.split("\n", 1)[0]
            members[first] = members.get(first, True) and ok
        assert ref.L.gnnvc_test_cblas_calls() > 0, "the products did not go through OpenBLAS"
        # ... and of the whole fuzz table (every case's last layer on `rounds`), of which the fixtures hold 24 cases
        g, table_equal, worst = graph_of("rounds"), 0, 0
        for i in range(mz.N):
            text, x = mz.text(i), model_input("fuzz", str(i), g)
            ref.L.gnnvc_test_set_cblas_sgemm(None)
            chain = ref.predict(text, -1, g, x, mz.case(i).out_width)
            ref.L.gnnvc_test_set_cblas_sgemm(C.cast(blas[1], C.c_void_p))
            stock = ref.predict(text, -1, g, x, mz.case(i).out_width)
            table_equal += same(stock, chain)
            both = np.isfinite(stock) & np.isfinite(chain)
            d = np.abs(stock[both].view(np.int32).astype(np.int64) - chain[both].view(np.int32).astype(np.int64))
            worst = max(worst, int(d.max(initial=0)))
        ref.L.gnnvc_test_set_cblas_sgemm(None)
        manifest["_stock_openblas"] = {"openblas": desc, "threads": 1, "arrays": len(computed), "arrays_reproduced": int(equal),
                                       "members": len(members), "members_reproduced_in_every_array": sum(members.values()),
                                       "fuzz_members": sum(1 for k in members if k.startswith("fuzz_")),
                                       "fuzz_members_reproduced_in_every_array": sum(v for k, v in members.items() if k.startswith("fuzz_")),
                                       "fuzz_table_cases": mz.N, "fuzz_table_graph": "rounds",
                                       "fuzz_table_cases_reproduced_in_the_last_layer": int(table_equal),
                                       "fuzz_table_worst_ulp_in_the_last_layer": worst,
                                       "_note": "data only, asserted nowhere: the contract for these shapes is the chain"}
        print("stock OpenBLAS:", manifest["_stock_openblas"])
    manifest["_total_bytes"] = total
    MANIFEST.write_text(json.dumps(manifest, indent=1) + "\n")
    print(f"{len(written)} files, {total} bytes")


if __name__ == "__main__":
    main()
