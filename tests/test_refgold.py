"""tests/golden/manifest_generic.json and tests/golden/generic/*.f32 — what the REFERENCE's own layer code computes for generic-stage
models (tools/make_golden_generic.py wrote them where the reference's sources can be read) — on the CPU, without the reference:

  a. the files are intact (md5 of every array against the manifest, every file under 256 KiB, the set under 3 MiB, no stray file);
  b. the model texts and the graphs regenerate to the pinned digests (the texts' SHA-256 are the ones tests/test_modelgen_*.py pin);
  c. the oracle reproduces every array bit for bit — the scores of a model that ends in the sigmoid within 1 ulp, by
     tests/golden/README.md's rule for the host's expf, and NaN where the fixture is NaN;
  d. the member table reaches every item it was chosen for, computed from the members' specs.

With (c), an engine result that tests/test_gpu_*.py hold to the oracle is held to the reference's layer code for these models too;
tests/test_gpu_refgold.py compares the engine with the same files directly.  The products in these arrays are the chain's (the
engine's documented contract for these shapes), not a stock OpenBLAS's: see tests/golden/README.md."""
import hashlib
import json

import numpy as np
import pytest

from oracle import oracle_py
from tools import graphgen as gg
from tools import make_golden_generic as mk
from tools import modelgen_fuzz as mz
from tools import modelgen_patterns as mp
from tests.generic_harness import ulp

MANIFEST = json.loads(mk.MANIFEST.read_text())
MEMBERS = mk.fixture_members()
KEYS = [mk.key_of(m) for m in MEMBERS]


def test_the_manifest_lists_the_members_and_graphs_of_the_table():
    assert list(MANIFEST["members"]) == KEYS and len(KEYS) == len(set(KEYS)) == 20 + 24
    assert len(mk.FUZZ_CASES) == 24 == len(set(mk.FUZZ_CASES)) and all(0 <= i < mz.N and mz.case(i).admitted for i in mk.FUZZ_CASES)
    for member in MEMBERS:
        e = MANIFEST["members"][mk.key_of(member)]
        assert (e["family"], e["member"]) == member and e["input"] == "model_input" in MANIFEST["_input_rules"]
        assert list(e["graphs"]) == mk.fixture_graphs(member)
    assert len(mk.HUB2K_MEMBERS) == 3 and set(mk.HUB2K_MEMBERS) <= set(MEMBERS)
    assert len(mk.MULTI_MEMBERS) == 4 and set(mk.MULTI_MEMBERS) <= set(MEMBERS)


def test_the_files_are_intact():
    files, total = {}, 0
    for key, e in MANIFEST["members"].items():
        for gname, ge in e["graphs"].items():
            arrays = mk.read_arrays(e, gname)      # (checks every md5)
            assert list(arrays) == [a["after_layer_index"] for a in ge["arrays"]] == sorted(arrays), (key, gname)
            for a in ge["arrays"]:
                files[a["file"]] = max(files.get(a["file"], 0), a["offset"] + 4 * a["shape"][0] * a["shape"][1])
    on_disk = sorted(f"{mk.SUBDIR}/{p.name}" for p in (mk.GOLD / mk.SUBDIR).iterdir())
    assert on_disk == sorted(files), "files under tests/golden/generic that the manifest does not list, or the other way round"
    for name, size in files.items():
        assert (mk.GOLD / name).stat().st_size == size <= mk.MAX_FILE_BYTES, name
        total += size
    assert total == MANIFEST["_total_bytes"] <= mk.MAX_SET_BYTES


def test_the_graphs_regenerate_to_the_pinned_texts():
    assert list(MANIFEST["graphs"]) == mk.FIXTURE_GRAPHS + ["hub2k"]
    for gname, spec in MANIFEST["graphs"].items():
        assert spec["graph"] == mk.GRAPH_PARAMS[gname]
        g = mk.make_graph(spec["graph"])
        assert (g.n, float(g.ws), gg.metis_md5(g)) == (spec["n"], spec["ws"], spec["metis_md5"]), gname
    layers = json.loads((mk.GOLD / "manifest_layers.json").read_text())["graphs"]
    assert MANIFEST["graphs"]["hub2k"]["metis_md5"] == layers["hub2k"]["metis_md5"]     # the same hub2k
    assert MANIFEST["graphs"]["ex3"]["metis_md5"] == layers["ex3"]["metis_md5"]
    assert [int(d) for d in np.diff(mk.graph_of("hub2k").rowptr.astype(np.int64))[:2]] >= [1024, 1024]   # two giant rows at 1024


def _pinned_digest(family, name):
    """The SHA-256 that the family's own test pins for the member's text (None: a fuzz case, pinned as a table, or tools/modelgen.py's)."""
    from tests import test_modelgen_feat, test_modelgen_generic, test_modelgen_live, test_modelgen_patterns
    if family in ("shapes", "depths", "big"):
        return test_modelgen_generic.DIGESTS[family, name]
    return {"feat": test_modelgen_feat.DIGESTS, "live": test_modelgen_live.SHA256, "patterns": test_modelgen_patterns.DIGESTS}.get(family, {}).get(name)


@pytest.mark.parametrize("key", KEYS)
def test_the_text_regenerates_to_the_pinned_digest(key):
    e = MANIFEST["members"][key]
    family, name = e["family"], e["member"]
    text = mk.text_of(family, name)
    sha = hashlib.sha256(text.encode()).hexdigest()
    assert sha == e["text_sha256"] and text.split("\n", 1)[0] == e["first_line"], key
    pinned = _pinned_digest(family, name)
    assert pinned is None or pinned == sha, key
    kinds = mk.layer_kinds(text)
    assert len(kinds) == e["num_layers"] and e["ends_in_sigmoid"] == (kinds[-1] == mk.SIGMOID)
    assert e["in_width"] == mk.in_width(family, name)
    # the stage list and the opt-ins are what the generators' rules give today
    st, cfg = mk.stages_of(family, name), mk.config_of(family, name)
    assert e["stages"] == (None if st is None else [{"dense": d, "f": f, "widths": ws, "end": end} for d, f, ws, end in st]), key
    assert e["config"] == (None if cfg is None else {"patterns": cfg[0], "feature_width": cfg[1], "big_stages_lds": cfg[2]}), key
    assert (e["stages"] is None) == ((family, name) in mk.LAYER_BY_LAYER), key
    for gname, ge in e["graphs"].items():
        assert [a["after_layer_index"] for a in ge["arrays"]] == mk.cut_points(kinds), (key, gname)


@pytest.mark.parametrize("key", KEYS)
def test_the_oracle_reproduces_every_array(key):
    e = MANIFEST["members"][key]
    family, name = e["family"], e["member"]
    om = oracle_py.OracleModel(mk.text_of(family, name))
    last = om.n_layers - 1
    for gname in e["graphs"]:
        g = mk.graph_of(gname)
        om.set_weight_scale(g.ws)
        x = mk.model_input(family, name, g)
        for cut, want in mk.read_arrays(e, gname).items():
            got = om.predict(g, x, stop_after=cut)
            assert got.shape == want.shape, (key, gname, cut)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (key, gname, cut, "NaN positions")
            if cut == last and e["ends_in_sigmoid"]:     # scores: the host's expf may differ in the last place (tests/golden/README.md)
                ok = ~np.isnan(want)
                worst = int(ulp(got[ok], want[ok]).max(initial=0))
                assert worst <= 1, (key, gname, cut, f"scores {worst} ulp from the fixture")
            else:
                diff = mk.first_difference(got, want)
                assert diff is None, f"{key} on {gname} after layer {cut}: oracle against fixture: {diff}"


# ---------------------------------------------------------------- d. what the table reaches

def _reached():
    """What the members reach, from their specs (the stage lists of tools/modelgen_fuzz.expect under each member's own opt-ins,
    and the layer kinds of the texts' generators)."""
    out = set()
    for family, name in MEMBERS:
        st = mk.stages_of(family, name)
        w_in = mk.in_width(family, name)
        out.add(("input width", w_in))
        if st is None:
            seq = mp.sequence(name).split()
            out.add("layer by layer: two graph layers in a row" if any(a == b == "G" for a, b in zip(seq, seq[1:])) else
                    "layer by layer: a sigmoid inside" if "S" in seq[:-1] else "layer by layer: other")
            continue
        out.add(("output width", st[-1][2][-1]))
        out.add(("ending", st[-1][3]))
        if all(dense for dense, _, _, _ in st):
            out.add("no graph layer")
        for dense, f, widths, _ in st:
            out.add("dense prologue" if dense else ("f", f))
            out.add(("depth", len(widths)))
            if 128 in widths[:-1]:
                out.add("hidden 128")
        if (family, name) == ("trained", "saturating_1"):
            out.add("saturating")
    return out


def test_the_members_reach_what_they_were_chosen_for():
    got = _reached()
    want = ({("f", f) for f in (1, 2, 3, 4, 5, 16, 17, 33, 64)} | {("input width", w) for w in (1, 2, 40)}
            | {("output width", w) for w in (1, 3, 64)} | {("depth", 1), ("depth", 6), "hidden 128", "dense prologue", "no graph layer",
                                                            ("ending", mp.END_RELU), ("ending", mp.END_NONE), ("ending", mp.END_SIGMOID),
                                                            "layer by layer: two graph layers in a row", "layer by layer: a sigmoid inside",
                                                            "saturating"})
    assert not want - got, sorted(map(str, want - got))
    for member in mk.HUB2K_MEMBERS:
        assert max(ws[-1] for _, _, ws, _ in mk.stages_of(*member)) <= 16, member


def test_the_fuzz_cases_are_spread_over_the_route_kinds():
    """The model-side classes of tests/test_modelgen_fuzz.py's AT_LEAST_THREE list (the kernel forms, endings, depths, K classes,
    hidden-width classes, stage counts) and its dense-stage pairs: each reached by one of the 24 cases at least.  (The graph-side
    classes — gather x row kinds, n = 0 / 1 — belong to the cases' own graphs, which are not the fixtures'.)"""
    from tests import test_modelgen_fuzz as tf
    model_side = lambda k: not (k.startswith("gather") or k.startswith("n "))
    got = set()
    for i in mk.FUZZ_CASES:
        classes, pairs = tf.classes_of(i)
        got |= {k for k in classes if model_side(k)} | {p for p in pairs if p.startswith("dense stage")}
    want = [k for k in tf.AT_LEAST_THREE if model_side(k)] + [f"dense stage x {w}" for w in ("default", "BIG", "FEAT")]
    assert len(want) >= 40 and not [k for k in want if k not in got], [k for k in want if k not in got]


def test_the_saturating_member_saturates():
    """Its fixture logits reach past +-103 and its scores hold 0.0, 1.0 and denormals: the sigmoid's far branches are in the files."""
    e = MANIFEST["members"]["trained.saturating_1"]
    a = mk.read_arrays(e, "rounds")
    logits, scores = a[e["num_layers"] - 2], a[e["num_layers"] - 1]
    assert logits.min() < -104 and logits.max() > 89
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert (scores == 1.0).any() and ((scores > 0) & (scores < tiny)).any()
    assert (scores == 0.0).any()
