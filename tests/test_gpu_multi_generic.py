"""Generic-stage models on several devices behind one handle (gnnvc_create_multi_generic) and the kernel their rows travel by
(gnnvc_push_rows, k_push_rows).  All parts share device 0: parts that share a device always have peer access to themselves, which
is how one GPU reaches the push kernel, the events and the ordering of the exchange — it says nothing about a link.

Bars, tests/generic_harness.py's and no other: logits bit for bit the oracle's (want_of / the pattern harness's walk), scores
within 1 ulp of the oracle's and bit for bit the restated sigmoid's (check_scores); a member that does not end in the sigmoid has
its outputs compared bit for bit.  "poison_features" is 1 on every handle here, so a row that no exchange delivers shows as NaN."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle_py
from tools import graphgen as gg
from tools import modelgen_feat as mf
from tools import modelgen_patterns as mp
from tests import generic_harness as gh
from tests import pattern_harness as ph
from tests.generic_harness import bits, check_scores, graph_of, heavy_counts
from tests.test_expf_restatement import shim   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)

pytestmark = pytest.mark.gpu

gh.FAMILIES.setdefault("feat", mf.family)

ERR_INVALID, ERR_UNSUPPORTED = -1, -5
BIG = max(gh.LDS_BYTES["h128"])   # 99 648 bytes: what the big family's h128 needs, and more than embed_h128's 128-wide layer does

# key -> (family or "patterns", member, the creation config)
MEMBERS = {
    "odd": ("shapes", "odd", True),              # widths 5 and 9: runs neither start nor end on 16 bytes
    "in3": ("shapes", "in3", True),              # in_width 3
    "out4": ("shapes", "out4", True),            # out_width 4
    "two_stage": ("shapes", "two_stage", True),  # one exchange
    "deep5": ("shapes", "deep5", True),          # four exchanges, the ping-pong reused twice
    "mixed": ("depths", "mixed", True),
    "f33": ("feat", "f33", {"feature_width": 64}),                                   # rows of 33 floats: r0 * 33 cycles through every phase
    "h128": ("big", "h128", {"big_stages_lds": BIG}),
    "embed_h128": ("patterns", "embed_h128", {"big_stages_lds": BIG, "patterns": 3}),
    "embed": ("patterns", "embed", {"patterns": 3}),                                 # a dense stage 0 that waits for nobody
    "mlp": ("patterns", "mlp", {"patterns": 3}),                                     # no graph stage: no exchange
    "both": ("patterns", "both", {"patterns": 3}),                                   # prologue and a ReLU end, out_width 8
    "linear_end17": ("patterns", "linear_end17", {"patterns": 3}),                   # one stage, 17 outputs, logits not written
}
DEVICE_LISTS = [[0, 0], [0, 0, 0], [0] * 8]


def text_of(key):
    family, name, _ = MEMBERS[key]
    return ph.text_of(name) if family == "patterns" else gh.text_of(family, name)


def model_input(key, g):
    family, name, _ = MEMBERS[key]
    return mp.model_input(name, g) if family == "patterns" else gh.FAMILIES[family].model_input(name, g)


def widths_of(key):
    """(in_width, out_width, [(f, last width)] per stage) from the generators' tables."""
    family, name, _ = MEMBERS[key]
    fam = mp if family == "patterns" else gh.FAMILIES[family]
    return fam.in_width(name), fam.out_width(name), fam.stage_widths(name)


def sigmoid_end(key):
    family, name, _ = MEMBERS[key]
    return ph.ends_in_sigmoid(name) if family == "patterns" else True


def open_handle(key, devices, generic=None, opts=()):
    import gnn_mwvc_amd as G
    e = G.Engine(text_of(key), devices=devices, generic=MEMBERS[key][2] if generic is None else generic)
    try:
        e.set_option("poison_features", 1)
        for k, v in dict(opts).items():
            e.set_option(k, v)
    except BaseException:
        e.close()
        raise
    return e


def check_outputs(shim, key, gname, sc, lg, label):
    """The oracle's values for (member, graph): logits bit for bit and scores by check_scores, or — a member that does not end in
    the sigmoid — the outputs bit for bit."""
    family, name, _ = MEMBERS[key]
    g = graph_of(gname)
    _, ow, _ = widths_of(key)
    assert sc.shape == (g.n, ow), label
    if not sigmoid_end(key):
        want = ph.final_of(name, gname)
        bad = np.argwhere(bits(sc) != bits(want))
        assert bad.size == 0, (label, f"{len(bad)} values differ, first (row, column)", bad[:6].tolist())
        return
    if family == "patterns":
        wl, flat = ph.want_of(name, gname)[-1][2], ph.flat_logits(name, gname)
    else:
        wl, flat = gh.want_of(family, name, gname)[-1][2], gh.flat_logits(family, name, gname)
    assert lg.shape == wl.shape, label
    bad = np.argwhere(bits(lg) != bits(wl))
    assert bad.size == 0, (label, f"{len(bad)}/{lg.size} logits differ, first (row, column)", bad[:6].tolist())
    check_scores(shim, sc.reshape(-1), lg.reshape(-1), flat, label)


def host_forward(shim, e, key, gname, label, audited=False):
    """One host forward into arrays that hold a sentinel: the logits of a member without a last sigmoid stay untouched."""
    g = graph_of(gname)
    _, ow, _ = widths_of(key)
    sc = np.full((g.n, ow), -3.0, dtype=np.float32)
    lg = np.full((g.n, ow), -3.0, dtype=np.float32)
    (e.forward_audited if audited else e.forward)(model_input(key, g), out=(sc, lg))
    if g.n == 0:
        return sc, lg
    check_outputs(shim, key, gname, sc, lg, label)
    if not sigmoid_end(key):
        assert (lg == -3.0).all(), (label, "logits written by a model that does not end in the sigmoid")
    return sc, lg


def device_forward(shim, e, key, gname, label):
    import torch
    g = graph_of(gname)
    _, ow, _ = widths_of(key)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(np.ascontiguousarray(model_input(key, g), dtype=np.float32)).to(dev)
    sc = torch.full((g.n, ow), float("nan"), dtype=torch.float32, device=dev)
    lg = torch.full((g.n, ow), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    e.forward_device(x.data_ptr(), sc.data_ptr(), lg.data_ptr())   # (complete when it returns: every part is drained)
    check_outputs(shim, key, gname, sc.cpu().numpy(), lg.cpu().numpy(), label)
    if not sigmoid_end(key):
        assert torch.isnan(lg).all(), (label, "logits written by a model that does not end in the sigmoid")


def assert_front_answers(e, key, devices):
    iw, ow, stages = widths_of(key)
    assert e.get_info("multi_generic") == 1 and e.get_info("devices") == len(devices), key
    assert e.fused and e.get_info("generic_stages_model") == 1, key
    assert (e.in_width, e.out_width, e.num_stages) == (iw, ow, len(stages)), key
    assert [e.stage_widths(s) for s in range(e.num_stages)] == stages, key
    assert e.get_info("multi_exchanges") == len(stages) - 1, key
    cfg = MEMBERS[key][2]
    if isinstance(cfg, dict):
        assert e.get_info("generic_patterns") == cfg.get("patterns", 0), key
        assert e.get_info("generic_feature_width") == cfg.get("feature_width", 0), key
        assert e.get_info("generic_big_lds") == cfg.get("big_stages_lds", 0), key
    family, name, _ = MEMBERS[key]
    if family == "patterns":
        assert [e.get_info(f"generic_stage_dense_{s}") for s in range(e.num_stages)] == mp.stage_dense(name), key
        assert [e.get_info(f"generic_stage_layers_{s}") for s in range(e.num_stages)] == mp.stage_depths(name), key


# ---------------------------------------------------------------- 1. equality with the oracle

@pytest.mark.parametrize("key", list(MEMBERS))
def test_equal_to_the_oracle_on_every_part_count(shim, key):
    """er1933 (n = 30 * 64 + 13: eight parts cut at multiples of 64 leave empty parts and empty pieces), hubs (all heavy rows in part
    0), sparse (empty rows), then one vertex and none — each graph handed to the live handle, by upload and staged in turn, three
    forwards in a row each, and a device-pointer forward."""
    for devices in DEVICE_LISTS:
        e = open_handle(key, devices)
        try:
            assert_front_answers(e, key, devices)
            for i, gname in enumerate(["er1933", "hubs", "sparse", "one", "empty"]):
                g = graph_of(gname)
                route = ("upload", "staged7")[i % 2]
                gh.hand_over(e, g, route)
                rows = [e.get_info(f"part_rows_{r}") for r in range(len(devices))]
                assert sum(rows) == g.n and all(r % 64 == 0 for r in rows[:-1]), (key, devices, gname, rows)
                for rep in range(3):
                    host_forward(shim, e, key, gname, (key, len(devices), gname, route, rep))
                if g.n and gname in ("er1933", "one"):
                    device_forward(shim, e, key, gname, (key, len(devices), gname, route, "device pointers"))
            assert e.get_info("audit_runs") == 0
        finally:
            e.close()


# ---------------------------------------------------------------- 2. the exchange's options

def test_exchange_options_change_no_bit(shim):
    key, gname, P = "odd", "er3000", 5
    g = graph_of(gname)
    e = open_handle(key, [0] * P)
    try:
        gh.hand_over(e, g, "upload")
        rows = [e.get_info(f"part_rows_{r}") for r in range(P)]
        assert sum(rows) == g.n
        for pieces in (0, 1, 3, 8):
            for push in (0, 1):
                e.set_option("multi_pieces", pieces)
                e.set_option("multi_push", push)
                label = (key, gname, "pieces", pieces, "push", push)
                assert e.get_info("multi_pieces") == (pieces or 4), label   # (0: by the number of parts — four beyond four parts)
                host_forward(shim, e, key, gname, label)
                assert e.get_info("multi_generic") == 1 and e.get_info("multi_exchanges") == 2, label
                assert e.get_info("multi_exchange_bytes_per_peer_stage0") == max(rows) * 5 * 4, label
                assert e.get_info("multi_exchange_bytes_per_peer_stage1") == max(rows) * 9 * 4, label
        with pytest.raises(Exception) as ei:
            e.get_info("multi_exchange_bytes_per_peer_stage2")   # (the last stage's rows do not travel)
        assert ei.value.code == ERR_INVALID
        # accepted, without effect
        e.set_option("multi_pack", 0)
        e.set_option("multi_announce", 1)
        host_forward(shim, e, key, gname, "multi_pack 0, multi_announce 1")
        # one part's share alone needs no earlier forward of any kind on this graph: nothing is packed, nothing to know
        gh.hand_over(e, g, "upload")
        e.set_option("multi_only_part", 2)
        e.forward(model_input(key, g))
        assert e.get_info("multi_part_span_us_2") >= 0
        e.set_option("multi_only_part", -1)
        host_forward(shim, e, key, gname, "after multi_only_part")
    finally:
        e.close()


# ---------------------------------------------------------------- 3. heavy and giant rows through the config

@pytest.mark.parametrize("heavy", [512, 0])
@pytest.mark.parametrize("key", ["odd", "in3"])
def test_heavy_and_giant_rows_through_the_config(shim, key, heavy):
    gname, giant = "hubs", 1024
    g = graph_of(gname)
    e = open_handle(key, [0, 0, 0], generic={"heavy_rows": heavy, "giant_rows": giant})
    try:
        gh.hand_over(e, g, "upload")
        for rep in range(2):
            host_forward(shim, e, key, gname, (key, heavy, giant, rep))
        assert e.get_info("generic_heavy_rows") == heavy_counts(g, heavy)[0] == (7 if heavy else 0)
        assert e.get_info("generic_heavy_entries") == heavy_counts(g, heavy)[1]
        want_giant = heavy_counts(g, max(heavy, giant)) if heavy else (0, 0)
        assert (e.get_info("generic_giant_rows"), e.get_info("generic_giant_entries")) == want_giant
    finally:
        e.close()


# ---------------------------------------------------------------- 4. refusals, and what stays pinned

def _raises(code, fn, *args, **kw):
    import gnn_mwvc_amd as G
    with pytest.raises(G.GnnvcError) as ei:
        fn(*args, **kw)
    assert ei.value.code == code, ei.value


def test_refusals_stay_and_layer_by_layer_models_are_refused():
    import gnn_mwvc_amd as G
    _raises(ERR_UNSUPPORTED, G.Engine, gh.text_of("shapes", "narrow"), devices=[0, 0])             # the existing call: as ever
    _raises(ERR_UNSUPPORTED, G.Engine, gh.text_of("depths", "too_big"), devices=[0, 0], generic=True)   # too big without big stages
    _raises(ERR_UNSUPPORTED, G.Engine, ph.text_of("mid_sigmoid"), devices=[0, 0], generic=True)
    _raises(ERR_UNSUPPORTED, G.Engine, ph.text_of("mid_sigmoid"), devices=[0, 0], generic={"patterns": 3})
    _raises(ERR_UNSUPPORTED, G.Engine, ph.text_of("embed"), devices=[0, 0], generic=True)          # a prologue without its bit
    _raises(ERR_INVALID, G.Engine, gh.text_of("shapes", "odd"), devices=[0, 0], generic={"patterns": 4})
    e = open_handle("odd", [0, 0])
    try:
        g = graph_of("er1933")
        gh.hand_over(e, g, "upload")
        _raises(ERR_UNSUPPORTED, e.set_generic_patterns, 1)
        _raises(ERR_UNSUPPORTED, e.set_generic_heavy_rows, 1)
        _raises(ERR_UNSUPPORTED, e.set_generic_giant_rows, 1024)
        _raises(ERR_UNSUPPORTED, e.set_generic_big_stages, 0)
        _raises(ERR_UNSUPPORTED, e.set_generic_feature_width, 0)
        _raises(ERR_UNSUPPORTED, e.stage_forward_device, 0, 0, 64, 1, 1)
        _raises(ERR_UNSUPPORTED, e.reduction_flags)
        assert e.get_info("generic_patterns") == 0 and e.get_info("generic_heavy_from") == 512
    finally:
        e.close()


def test_the_trained_model_through_the_new_call_is_the_trained_handle():
    import gnn_mwvc_amd as G
    text = G.engine.default_model_text()
    g = graph_of("er3000")
    x = (g.w.astype(np.float32) / np.float32(g.ws)).reshape(-1, 1)
    om = oracle_py.OracleModel(text)
    om.set_weight_scale(g.ws)
    want = om.predict(g, x, stop_after=om.n_layers - 2).reshape(-1)
    got = []
    for generic in (None, {"heavy_rows": 1, "patterns": 3, "feature_width": 64}):   # (the config has no effect on this model)
        e = G.Engine(text, devices=[0, 0, 0], generic=generic)
        try:
            assert e.get_info("multi_generic") == 0 and e.get_info("generic_stages_model") == 0
            assert e.get_info("generic_patterns") == 0 and e.get_info("generic_feature_width") == 0
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            for _ in range(2):   # (the second one runs on the packing the first one chose)
                _, lg = e.forward(x)
            got.append(lg.reshape(-1))
            assert e.get_info("multi_packed_stage0") in (0, 1)
        finally:
            e.close()
    assert np.array_equal(bits(got[0]), bits(want)) and np.array_equal(bits(got[1]), bits(want))


# ---------------------------------------------------------------- 5. audited forwards

def _pieces(lo, hi, K):
    """The rows of a part's K pieces: nearly equal ranges cut at multiples of 64 rows, as the handle cuts them."""
    cut = [hi if k == K else min(hi, max(lo, (lo + (hi - lo) * k // K) // 64 * 64)) for k in range(K + 1)]
    for k in range(1, K):
        cut[k] = max(cut[k], cut[k - 1])
    return [b - a for a, b in zip(cut[:-1], cut[1:])]


def test_audited_forward_audits_every_piece_of_every_part(shim):
    key, gname, P, K = "odd", "er1933", 3, 3
    g = graph_of(gname)
    e = open_handle(key, [0] * P, opts={"multi_pieces": K})
    try:
        gh.hand_over(e, g, "upload")
        rows = [e.get_info(f"part_rows_{r}") for r in range(P)]
        los = np.concatenate([[0], np.cumsum(rows)]).tolist()
        nonempty = sum(1 for r in range(P) for size in _pieces(los[r], los[r + 1], K) if size > 0)
        assert 0 < nonempty <= P * K
        host_forward(shim, e, key, gname, "audited", audited=True)
        rep = e.audit_report()
        assert rep["audit_runs"] == nonempty * e.num_stages and rep["audit_failures"] == 0 and rep["audit_repairs"] == 0, rep
        host_forward(shim, e, key, gname, "unaudited")
        assert e.get_info("audit_runs") == rep["audit_runs"]
        e.set_option("audit_period", 1)   # audits nothing on such a handle, as on a single generic engine
        host_forward(shim, e, key, gname, "audit_period 1")
        assert e.get_info("audit_runs") == rep["audit_runs"]
        e.set_option("audit_period", 0)
        e.set_option("audit_repair", 1)   # handed on to the parts: a clean audit repairs nothing
        host_forward(shim, e, key, gname, "audited, repair on", audited=True)
        rep2 = e.audit_report()
        assert rep2["audit_runs"] == 2 * rep["audit_runs"] and rep2["audit_failures"] == 0 and rep2["audit_repairs"] == 0, rep2
    finally:
        e.close()


# ---------------------------------------------------------------- 6. gnnvc_push_rows alone

GUARD = 8   # words of guard pattern on both sides of a destination run (32 bytes: the run keeps its 16-byte phase)
LENGTHS = [0, 1, 3, 4, 5, 7, 255, 256, 257, 1933 * 5]


def test_push_rows_copies_exactly_the_run():
    import torch
    import gnn_mwvc_amd as G
    dev = torch.device("cuda:0")
    e = G.Engine("ops 0 Layers\n", device=0)
    try:
        longest = max(LENGTHS)
        src = (torch.arange(longest + 8, dtype=torch.float32, device=dev) + 0.5)
        assert src.data_ptr() % 16 == 0
        host_src = src.cpu().numpy()
        for words in LENGTHS:
            for off in range(4):   # the source starts 0 .. 3 words behind a 16-byte boundary
                for n_dst in (1, 3, 64):
                    room = GUARD + off + 1 + words + GUARD
                    dst = torch.full((n_dst, (room + 3) // 4 * 4), -7.0, dtype=torch.float32, device=dev)
                    assert dst.data_ptr() % 16 == 0
                    # destination i starts GUARD + off words into its row: the source's phase — but the last one of three, which is
                    # one word further on and so out of phase with the source
                    skew = [1 if (n_dst == 3 and i == 2) else 0 for i in range(n_dst)]
                    ptrs = [dst[i].data_ptr() + 4 * (GUARD + off + skew[i]) for i in range(n_dst)]
                    torch.cuda.synchronize()
                    e.push_rows(src.data_ptr() + 4 * off, words, ptrs)
                    e.synchronize()
                    got = dst.cpu().numpy()
                    for i in range(n_dst):
                        at = GUARD + off + skew[i]
                        label = (words, off, n_dst, i)
                        assert np.array_equal(bits(got[i, at: at + words]), bits(host_src[off: off + words])), label
                        assert (got[i, :at] == -7.0).all() and (got[i, at + words:] == -7.0).all(), (label, "a guard word was written")
        # refusals launch nothing
        dst = torch.full((65, 64), -7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        _raises(ERR_INVALID, e.push_rows, src.data_ptr(), 16, [dst[i].data_ptr() for i in range(65)])
        _raises(ERR_INVALID, e.push_rows, src.data_ptr(), 16, [dst[0].data_ptr(), 0, dst[2].data_ptr()])
        _raises(ERR_INVALID, e.push_rows, src.data_ptr() + 2, 16, [dst[0].data_ptr()])
        e.push_rows(src.data_ptr(), 16, [])
        e.synchronize()
        assert (dst.cpu().numpy() == -7.0).all()
    finally:
        e.close()


# ---------------------------------------------------------------- 7. the C++ host mirror

def _predict(tmp_path, family, name, gname, env):
    from tests.test_gpu_generic_lifecycle import _predict_tool
    (tmp_path / "g.metis").write_text(gg.metis_text(graph_of(gname)))
    (tmp_path / "m.txt").write_text(gh.text_of(family, name))
    return subprocess.run([str(_predict_tool()), str(tmp_path / "m.txt"), str(tmp_path / "g.metis"), str(tmp_path / "s.f32")],
                          capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))


def test_host_mirror_runs_a_generic_model_on_several_devices(tmp_path):
    """GNNVC_DEVICES=0,0,0 with GNNVC_GENERIC=1: the tool's scores are bit for bit the oracle's; without GNNVC_GENERIC the same
    run ends as it always did, refused by gnnvc_create_multi."""
    family, name, gname = "shapes", "odd", "hubs"
    r = _predict(tmp_path, family, name, gname, {"GNNVC_DEVICES": "0,0,0", "GNNVC_GENERIC": "1"})
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.frombuffer((tmp_path / "s.f32").read_bytes(), dtype=np.float32)
    want = gh.want_of(family, name, gname)[-1][1]
    assert got.shape == (graph_of(gname).n,)
    assert np.array_equal(bits(got), bits(want.reshape(-1)))
    r = _predict(tmp_path, family, name, gname, {"GNNVC_DEVICES": "0,0,0", "GNNVC_GENERIC": "heavy_rows=0,giant_rows=0"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "s.f32").read_bytes() == got.tobytes()
    r = _predict(tmp_path, family, name, gname, {"GNNVC_DEVICES": "0,0,0"})
    assert r.returncode != 0 and "gnnvc_create_multi" in r.stderr, r.stdout + r.stderr
