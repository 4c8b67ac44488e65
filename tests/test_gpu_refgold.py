"""The engine against what the REFERENCE's own layer code computes for generic-stage models: tests/golden/manifest_generic.json
and tests/golden/generic/*.f32 (tools/make_golden_generic.py wrote them; tests/test_refgold.py holds the files intact, the texts
and graphs pinned and the member table complete).  The fixtures are the only expected values here: no oracle is read.

Per member, on each of its graphs (the README's 3 vertices, tiny13, rounds; hub2k for three members), under the least opt-ins
that fuse it and with "poison_features" 1:
  * the stage list reads as the manifest says;
  * a whole forward: the logits bit for bit, the scores within 1 ulp (tests/golden/README.md's rule) and NaN where the fixture's
    are; a model that does not end in the sigmoid: its output bit for bit;
  * every stage through gnnvc_stage_forward_device, the fixture of the stage before as input and the stage's own as expectation:
    over the whole range, and over two ranges that meet at a row that is no multiple of 64, with every row outside a range
    (the row behind the end included) untouched;
  * the same forward with option "generic_stages" 0;
  * on hub2k also under set_generic_heavy_rows(17) and set_generic_giant_rows(1024, segments) with segments 0 and 1.
The two members that no setting fuses run as they are.  Four members also run behind gnnvc_create_multi_generic, 2 and 3 parts
on device 0.  Every comparison but the scores' is on bits; a failure names member, graph, stage or layer, and the first element."""
import json

import numpy as np
import pytest

from tools import make_golden_generic as mk

pytestmark = pytest.mark.gpu


def ulp(a, b):
    i = lambda v: np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(i(a) - i(b))


def heavy_counts(g, thr):
    """(rows, their entries) of g with at least thr entries: what "generic_heavy_rows" / "generic_giant_rows" count."""
    deg = np.diff(g.rowptr.astype(np.int64))
    return int((deg >= thr).sum()), int(deg[deg >= thr].sum())

MANIFEST = json.loads(mk.MANIFEST.read_text())
KEYS = list(MANIFEST["members"])
_gold = {}


def gold_of(key, gname):
    if (key, gname) not in _gold:
        _gold[key, gname] = mk.read_arrays(MANIFEST["members"][key], gname)
    return _gold[key, gname]


def graph_of(gname):
    g = mk.graph_of(gname)
    assert g.n == MANIFEST["graphs"][gname]["n"] and float(g.ws) == MANIFEST["graphs"][gname]["ws"]
    return g


def open_engine(entry, opts=()):
    """A single engine on device 0 with the member's text, "poison_features" 1 and the manifest's opt-ins."""
    import gnn_mwvc_amd as G
    e = G.Engine(mk.text_of(entry["family"], entry["member"]), device=0)
    try:
        e.set_option("poison_features", 1)
        for k, v in dict(opts).items():
            e.set_option(k, v)
        cfg = entry["config"] or {}
        if cfg.get("big_stages_lds"):
            e.set_generic_big_stages(cfg["big_stages_lds"])
        if cfg.get("feature_width"):
            e.set_generic_feature_width(cfg["feature_width"])
        if cfg.get("patterns"):
            e.set_generic_patterns(cfg["patterns"])
        assert (e.num_layers, e.in_width, e.out_width) == (entry["num_layers"], entry["in_width"], entry["out_width"])
    except BaseException:
        e.close()
        raise
    return e


def assert_stage_list(e, entry):
    st = entry["stages"]
    if st is None:
        assert not e.fused and e.num_stages == 0 and e.get_info("generic_stages_model") == 0
        return
    ns = len(st)
    assert e.fused and e.num_stages == ns
    assert [e.stage_widths(s) for s in range(ns)] == [(r["f"], r["widths"][-1]) for r in st]
    if entry["family"] != "trained":   # (the trained shape keeps its own plans unless "generic_stages" is 2)
        assert e.get_info("generic_stages_model") == 1
    if e.get_info("generic_stages_model") == 1:
        rd = lambda name: [e.get_info(f"{name}_{s}") for s in range(ns)]
        assert rd("generic_stage_layers") == [len(r["widths"]) for r in st]
        assert rd("generic_stage_dense") == [r["dense"] for r in st]
        assert rd("generic_stage_end") == [r["end"] for r in st]


def first_bad(got, want):
    return mk.first_difference(np.asarray(got), np.asarray(want))


def assert_scores(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "scores: NaN positions")
    ok = ~np.isnan(want)
    d = ulp(got[ok], want[ok])
    worst = int(d.max(initial=0))
    assert worst <= 1, (what, f"scores {worst} ulp from the fixture, first at flat index {int(np.flatnonzero(d > 1)[0])}")


def assert_forward(e, entry, gname, label):
    key = mk.key_of((entry["family"], entry["member"]))
    g = graph_of(gname)
    gold = gold_of(key, gname)
    last = entry["num_layers"] - 1
    x = mk.model_input(entry["family"], entry["member"], g)
    what = (key, gname, label)
    if entry["ends_in_sigmoid"]:
        sc, lg = e.forward(x)
        assert sc.shape == lg.shape == gold[last].shape, what
        diff = first_bad(lg, gold[last - 1])
        assert diff is None, (what, "logits (layer %d)" % (last - 1), diff)
        assert_scores(sc, gold[last], what)
    else:
        out, _ = e.forward(x, want_logits=False)
        diff = first_bad(out, gold[last])
        assert diff is None, (what, "output (layer %d)" % last, diff)


def stage_ends(entry):
    """The layer index each stage ends at: the manifest's arrays but the logits."""
    arrays = next(iter(entry["graphs"].values()))["arrays"]
    ends = [a["after_layer_index"] for a in arrays if a["what"] != "logits"]
    assert len(ends) == len(entry["stages"])
    return ends


def split_row(n):
    """A row in the middle that is no multiple of 64 (n >= 2)."""
    cut = n // 2
    return cut + 1 if cut % 64 == 0 else cut


def assert_stages(e, entry, gname, label, split=True):
    import torch
    key = mk.key_of((entry["family"], entry["member"]))
    g = graph_of(gname)
    n = g.n
    gold = gold_of(key, gname)
    dev = torch.device("cuda:0")
    ends = stage_ends(entry)
    hin = mk.model_input(entry["family"], entry["member"], g)
    cut = split_row(n)
    assert 0 < cut < n and cut % 64
    generic = e.get_info("generic_stages_model") == 1
    for s, (r, end) in enumerate(zip(entry["stages"], ends)):
        f, n_out, sig = r["f"], r["widths"][-1], r["end"] == 1
        want = gold[end]
        want_pre = gold[end - 1] if sig else None
        assert hin.shape == (n, f) and want.shape == (n, n_out)
        tin = torch.zeros((n + 1, f), dtype=torch.float32, device=dev)
        tin[:n] = torch.from_numpy(np.ascontiguousarray(hin)).to(dev)
        for ranges in ([(0, n)], [(0, cut), (cut, n)])[: 2 if split else 1]:
            out = torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)
            lgt = torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            done = np.zeros(n + 1, dtype=bool)
            for lo, hi in ranges:
                # (the logits buffer goes to every generic stage, which must leave it alone unless it ends in the sigmoid; the
                # trained shape's own plans take it for their last stage only)
                e.stage_forward_device(s, lo, hi, tin.data_ptr(), out.data_ptr(), lgt.data_ptr() if sig or generic else 0)
                e.synchronize()
                done[lo:hi] = True
                got, gotl = out.cpu().numpy(), lgt.cpu().numpy()
                what = (key, gname, label, f"stage {s} (layer {end})", f"rows {lo}..{hi} of {ranges}")
                assert np.isnan(got[~done]).all(), (what, "rows outside the range were written")
                assert np.isnan(gotl[~done]).all() if sig else np.isnan(gotl).all(), (what, "logits rows")
                d = done[:n]
                if sig:
                    diff = first_bad(gotl[:n][d], want_pre[d])
                    assert diff is None, (what, "stage logits", diff)
                    assert_scores(got[:n][d], want[d], what)
                else:
                    diff = first_bad(got[:n][d], want[d])
                    assert diff is None, (what, diff)
        hin = want


@pytest.mark.parametrize("key", KEYS)
def test_member_against_the_reference_fixtures(key):
    entry = MANIFEST["members"][key]
    e = open_engine(entry)
    try:
        for gname in entry["graphs"]:
            g = graph_of(gname)
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            assert_stage_list(e, entry)
            assert_forward(e, entry, gname, "fused")
            if entry["stages"] is None:
                assert e.get_info("generic_stages_active") == 0
                continue
            if entry["family"] != "trained":
                assert e.get_info("generic_stages_active") == 1
            assert_stages(e, entry, gname, "fused")
            assert_forward(e, entry, gname, "fused, after the stage calls")
            if gname == "hub2k":
                for segments in (0, 1):
                    e.set_generic_heavy_rows(17)
                    e.set_generic_giant_rows(1024, segments)
                    assert_forward(e, entry, gname, f"heavy 17, giant 1024, segments {segments}")
                    if any(not r["dense"] for r in entry["stages"]):   # the rows the engine classed: both kinds are really there
                        assert (e.get_info("generic_heavy_rows"), e.get_info("generic_giant_rows")) == (heavy_counts(g, 17)[0], 2)
                        assert heavy_counts(g, 17)[0] > 2 == heavy_counts(g, 1024)[0]
                    assert_stages(e, entry, gname, f"heavy 17, giant 1024, segments {segments}")
    finally:
        e.close()


@pytest.mark.parametrize("key", KEYS)
def test_member_with_generic_stages_off(key):
    entry = MANIFEST["members"][key]
    e = open_engine(entry, opts={"generic_stages": 0})
    try:
        for gname in entry["graphs"]:
            g = graph_of(gname)
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            assert_forward(e, entry, gname, "generic_stages 0")
            assert e.get_info("generic_stages_active") == 0
            if entry["family"] != "trained":
                assert not e.fused and e.num_stages == 0
    finally:
        e.close()


def test_the_trained_shape_through_the_generic_kernel():
    """`saturating` with "generic_stages" 2: the trained shape as a generic stage list, against the same fixtures."""
    entry = MANIFEST["members"]["trained.saturating_1"]
    e = open_engine(entry, opts={"generic_stages": 2})
    try:
        for gname in entry["graphs"]:
            g = graph_of(gname)
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            assert e.get_info("generic_stages_model") == 1
            assert_stage_list(e, entry)
            assert_forward(e, entry, gname, "generic_stages 2")
            assert e.get_info("generic_stages_active") == 1
            assert_stages(e, entry, gname, "generic_stages 2")
    finally:
        e.close()


@pytest.mark.parametrize("key", [k for k in KEYS if MANIFEST["members"][k]["stages"] is None])
def test_the_layer_by_layer_members_are_not_fused(key):
    import gnn_mwvc_amd as G
    entry = MANIFEST["members"][key]
    assert (entry["family"], entry["member"]) in mk.LAYER_BY_LAYER
    e = G.Engine(mk.text_of(entry["family"], entry["member"]), device=0)
    try:
        e.set_option("poison_features", 1)
        assert not e.fused and e.num_stages == 0   # (gnnvc_is_fused)
        for gname in entry["graphs"]:
            g = graph_of(gname)
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            assert_forward(e, entry, gname, "as it is")
            assert not e.fused
    finally:
        e.close()


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("member", mk.MULTI_MEMBERS, ids=mk.key_of)
def test_member_behind_the_multi_device_handle(member, parts):
    import gnn_mwvc_amd as G
    entry = MANIFEST["members"][mk.key_of(member)]
    cfg = {k: v for k, v in entry["config"].items() if v}
    e = G.Engine(mk.text_of(*member), devices=[0] * parts, generic=cfg or True)
    try:
        e.set_option("poison_features", 1)
        st = entry["stages"]
        assert e.get_info("multi_generic") == 1 and e.fused and e.num_stages == len(st)
        assert [e.stage_widths(s) for s in range(len(st))] == [(r["f"], r["widths"][-1]) for r in st]
        for gname in entry["graphs"]:
            g = graph_of(gname)
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            assert sum(e.get_info(f"part_rows_{r}") for r in range(parts)) == g.n
            for rep in range(2):
                assert_forward(e, entry, gname, (f"{parts} parts", rep))
    finally:
        e.close()
