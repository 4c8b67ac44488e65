"""Generic graph stages that gather only the live columns of their input (gnnvc_set_generic_live_columns; k_any_live_mask,
k_any_live_pack and the LIVE instantiations of k_stage_any), opt-in and bit-identical.

Bars, the harness's and no wider: logits and every output bit for bit (0 ulp) against the oracle, scores within 1 ulp of the
oracle's and bit for bit the restated sigmoid's (check_scores), host outputs prefilled with a sentinel and device outputs with
NaN, "poison_features" 1 on every engine (the table is poisoned with the feature buffers).  The read-outs of the last forward —
"generic_live_kept_<s>", "_used_<s>", "_mask_lo|hi_<s>" — must equal the oracle's answer for that stage's input
(tests/live_harness.py; tests/test_modelgen_live.py pins it on the CPU) and include/gnnvc.h's rule for `used`.

The speed guard at the end: live/sparse32 (8 live columns of 32 by construction) on ER 1 M / 10 M on one engine, off then on
(100); on may not be slower than off by more than the spread of off's own three batches."""
import time

import numpy as np
import pytest

from tools import modelgen_fuzz as mz
from tools import modelgen_live as ml
from tests import fuzz_harness as fh
from tests import generic_harness as gh
from tests import live_harness as lh
from tests.generic_harness import bits, check_scores, crafted_input, degrees, graph_of
from tests.test_expf_restatement import shim, _run   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)
from tests.test_gpu_feature_width import rounds_graph
from tests.test_modelgen_live import MASKS

pytestmark = pytest.mark.gpu

gh.FAMILIES["live"] = ml.family
gh.GRAPHS.setdefault("feat_rounds", rounds_graph)

ERR_INVALID, ERR_UNSUPPORTED = -1, -5
FULL_LDS = 163840
SENTINEL = np.float32(-3.0)
POISON = {"poison_features": 1}

PINNED_MEMBERS = [("shapes", "wide"), ("shapes", "narrow"), ("shapes", "odd"), ("shapes", "in3"), ("shapes", "first_trained"),
                  ("depths", "mixed"), ("depths", "in3_f32")]
BIG_MEMBERS = [("big", "h128"), ("big", "odd_wide")]
FEAT_MEMBERS = [("feat", "f64"), ("feat", "f48_49"), ("feat", "in40")]
ON_MEMBERS = PINNED_MEMBERS + BIG_MEMBERS + FEAT_MEMBERS + [("live", "sparse32")]
SMALL_GRAPHS = ["er3000", "er1933", "sparse", "one", "feat_rounds"]
HEAVY_FROM, GIANT_FROM = 512, 1024


def open_live(family, name, g, percent=None, opts=(), **kw):
    """gh.open_engine with "poison_features" 1 and the opt-ins the member needs (big stages, feature width), then
    set_generic_live_columns(percent) where one is given — after the graph, under which it takes effect at the next forward."""
    big = FULL_LDS if family == "big" else None
    e = gh.open_engine(family, name, g, opts={**POISON, **dict(opts)}, big=big, **kw)
    try:
        if family == "feat" or (family == "live" and name in ml.NEEDS_FEAT):
            e.set_generic_feature_width(64)
        assert e.fused and e.get_info("generic_stages_model") == 1, (family, name)
        if percent is not None:
            e.set_generic_live_columns(percent)
    except BaseException:
        e.close()
        raise
    return e


def read_outs(e):
    out = []
    for s in range(e.num_stages):
        mask = e.get_info(f"generic_live_mask_lo_{s}") | (e.get_info(f"generic_live_mask_hi_{s}") << 32)
        out.append((e.get_info(f"generic_live_kept_{s}"), e.get_info(f"generic_live_used_{s}"), mask))
    return out


def host_forward(shim, e, family, name, gname, label, audited=False, x=None, want=None):
    """One host forward into sentinel-filled arrays against the oracle's logits (want; default: the member's own input's)."""
    g = graph_of(gname)
    fam = gh.FAMILIES[family]
    x = fam.model_input(name, g) if x is None else x
    wl = gh.want_of(family, name, gname)[-1][2] if want is None else want
    sc = np.full((g.n, fam.out_width(name)), SENTINEL, dtype=np.float32)
    lg = np.full((g.n, fam.out_width(name)), SENTINEL, dtype=np.float32)
    (e.forward_audited if audited else e.forward)(x, out=(sc, lg))
    mism = int((bits(lg) != bits(wl)).sum())
    assert mism == 0, (label, f"{mism}/{lg.size} logits differ", np.argwhere(bits(lg) != bits(wl))[:6].tolist())
    assert not (sc == SENTINEL).any(), label
    flat = gh.flat_logits(family, name, gname) if want is None else np.ascontiguousarray(wl.reshape(-1))
    check_scores(shim, sc.reshape(-1), lg.reshape(-1), flat, label)
    assert e.get_info("generic_stages_active") == 1, label


def device_forward(shim, e, family, name, gname, label):
    import torch
    g = graph_of(gname)
    fam = gh.FAMILIES[family]
    dev = torch.device("cuda:0")
    x = torch.from_numpy(np.ascontiguousarray(fam.model_input(name, g))).to(dev)
    sc = torch.full((g.n, fam.out_width(name)), float("nan"), dtype=torch.float32, device=dev)
    lg = torch.full((g.n, fam.out_width(name)), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    e.forward_device(x.data_ptr(), sc.data_ptr(), lg.data_ptr())
    e.synchronize()
    wl = gh.want_of(family, name, gname)[-1][2]
    assert np.array_equal(bits(lg.cpu().numpy()), bits(wl)), label
    check_scores(shim, sc.cpu().numpy().reshape(-1), lg.cpu().numpy().reshape(-1), gh.flat_logits(family, name, gname), label)


def assert_read_outs(e, family, name, gname, percent, label):
    want = lh.expected_readouts(family, name, gname, percent)
    assert read_outs(e) == want, (label, [(k, u, hex(m)) for k, u, m in read_outs(e)], [(k, u, hex(m)) for k, u, m in want])
    if (family, name, gname) in MASKS and percent:
        for (f, mask), (kept, used, got), ok in zip(MASKS[family, name, gname], want, lh.eligible(family, name)):
            assert not ok or (got == mask and kept == bin(mask).count("1")), (label, "the pinned mask")


NOT_EXAMINED = (-1, 0, 0)


# ---------------------------------------------------------------- 1. off is today

@pytest.mark.parametrize("family,name", [("shapes", "wide"), ("live", "sparse32")])
def test_off_is_the_default_and_reads_nothing(shim, family, name):
    import gnn_mwvc_amd as G
    e = open_live(family, name, graph_of("er3000"))
    try:
        assert e.get_info("generic_live_columns") == 0
        assert read_outs(e) == [NOT_EXAMINED] * e.num_stages            # no forward yet
        host_forward(shim, e, family, name, "er3000", "default")
        assert read_outs(e) == [NOT_EXAMINED] * e.num_stages
        e.set_generic_live_columns(0)                                    # a no-op
        assert e.get_info("generic_live_columns") == 0
        host_forward(shim, e, family, name, "er3000", "after 0")
        assert read_outs(e) == [NOT_EXAMINED] * e.num_stages
        for bad in (101, 1000, 0xFFFFFFFF):
            with pytest.raises(G.engine.GnnvcError) as ei:
                e.set_generic_live_columns(bad)
            assert ei.value.code == ERR_INVALID and e.get_info("generic_live_columns") == 0, bad
        e.set_generic_live_columns(37)
        with pytest.raises(G.engine.GnnvcError) as ei:
            e.set_generic_live_columns(101)
        assert ei.value.code == ERR_INVALID and e.get_info("generic_live_columns") == 37   # the value is kept
        for key in ("generic_live_kept_", "generic_live_used_", "generic_live_mask_lo_", "generic_live_mask_hi_"):
            for tail in (str(e.num_stages), "x_1", "0_1", "", "1x", "-1"):   # no such stage, or no number behind the prefix
                with pytest.raises(G.engine.GnnvcError) as ei:
                    e.get_info(key + tail)
                assert ei.value.code == ERR_INVALID, (key, tail)
        host_forward(shim, e, family, name, "er3000", "37")
        assert_read_outs(e, family, name, "er3000", 37, "37")
        e.set_generic_live_columns(0)                                    # ... and off again: the next forward examines nothing
        host_forward(shim, e, family, name, "er3000", "off again")
        assert read_outs(e) == [NOT_EXAMINED] * e.num_stages
    finally:
        e.close()


def test_multi_device_handles_refuse_the_call(model_text):
    import gnn_mwvc_amd as G
    for kw, text in (({"devices": [0, 0]}, model_text), ({"devices": [0, 0], "generic": True}, gh.text_of("shapes", "odd"))):
        e = G.Engine(text, **kw)
        try:
            for value in (0, 100):
                with pytest.raises(G.engine.GnnvcError) as ei:
                    e.set_generic_live_columns(value)
                assert ei.value.code == ERR_UNSUPPORTED, (kw, value)
        finally:
            e.close()


def test_the_trained_model_on_its_own_plans_keeps_the_value(shim, model_text):
    """Option "generic_stages" 1 (the default): the trained model keeps its specialised kernels; the value is stored and does nothing.

    This departs from one sentence of the issue, which asks that this model report kept -1 after a forward.  The issue also says
    that the per-stage keys follow "generic_stage_layers_<s>" — GNNVC_ERR_INVALID while the model is not generic — and the two
    cannot both hold under option 1.  The header documents the second: the key is refused here, and reads -1 once option 2 has
    made the model generic, before any forward."""
    import gnn_mwvc_amd as G
    g = graph_of("er3000")
    e = G.Engine(model_text, device=0)
    try:
        e.set_option("poison_features", 1)
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
        e.set_generic_live_columns(100)
        assert e.get_info("generic_live_columns") == 100 and e.get_info("generic_stages_model") == 0
        sc, lg = e.forward(g.x())
        assert e.get_info("generic_stages_active") == 0
        assert np.array_equal(bits(lg), bits(gh.want_of("trained", "model", "er3000")[-1][2]))
        with pytest.raises(G.engine.GnnvcError) as ei:                  # (the per-stage keys speak of a generic model only)
            e.get_info("generic_live_kept_1")
        assert ei.value.code == ERR_INVALID
        e.set_option("generic_stages", 2)                               # ... and now it runs as generic stages: no forward yet
        assert read_outs(e) == [NOT_EXAMINED] * 3
    finally:
        e.close()


# ---------------------------------------------------------------- 2. on, existing members

@pytest.mark.parametrize("percent", [100, 50])
@pytest.mark.parametrize("family,name", ON_MEMBERS, ids=lambda v: v if isinstance(v, str) else None)
def test_on_gives_the_oracles_bits_and_masks(shim, family, name, percent):
    e = open_live(family, name, graph_of(SMALL_GRAPHS[0]), percent)
    try:
        assert e.get_info("generic_live_columns") == percent
        for k, gname in enumerate(SMALL_GRAPHS):
            label = (family, name, gname, percent)
            if k:
                gh.hand_over(e, graph_of(gname), "upload")
            host_forward(shim, e, family, name, gname, label)
            assert_read_outs(e, family, name, gname, percent, label)
            before = e.get_info("audit_runs")
            host_forward(shim, e, family, name, gname, label + ("audited",), audited=True)
            assert e.get_info("audit_failures") == 0 and e.get_info("audit_runs") == before + e.num_stages, label
            assert_read_outs(e, family, name, gname, percent, label + ("audited",))
        device_forward(shim, e, family, name, SMALL_GRAPHS[-1], (family, name, "device pointers"))
        assert_read_outs(e, family, name, SMALL_GRAPHS[-1], percent, "device pointers")
    finally:
        e.close()


@pytest.mark.parametrize("percent", [100, 50])
@pytest.mark.parametrize("gname,giant", [("hubs", None), ("giant_hubs", (GIANT_FROM, -1))])
@pytest.mark.parametrize("family,name", ON_MEMBERS, ids=lambda v: v if isinstance(v, str) else None)
def test_on_with_heavy_and_giant_rows(shim, family, name, gname, giant, percent):
    """Every member again on the graphs with heavy (`hubs`) and giant (`giant_hubs`) rows: the light-rows launch reads the table —
    in the default, BIG and FEAT forms, as the member's stages route — while k_any_heavy_sums, the giant chain and the listed-rows
    launch read full rows."""
    g = graph_of(gname)
    e = open_live(family, name, g, percent, heavy=HEAVY_FROM, giant=giant)
    try:
        label = (family, name, gname, percent)
        host_forward(shim, e, family, name, gname, label)
        assert e.get_info("generic_heavy_last_rows") == gh.heavy_counts(g, HEAVY_FROM)[0] > 0
        assert (e.get_info("generic_giant_last_rows") > 0) == (giant is not None)
        assert_read_outs(e, family, name, gname, percent, label)
        before = e.get_info("audit_runs")
        host_forward(shim, e, family, name, gname, label + ("audited",), audited=True)
        assert e.get_info("audit_failures") == 0 and e.get_info("audit_runs") == before + e.num_stages, label
        device_forward(shim, e, family, name, gname, label + ("device pointers",))
    finally:
        e.close()


def _limit_for(family, name, threads):
    """A big-stage limit under which every stage of the member is admitted and an EXAMINED stage (f >= 2) runs at `threads`: that
    stage's layout at that size, raised to what the other stages need at 256 threads (the test asserts the size it got)."""
    fam = gh.FAMILIES[family]
    at = [b for b, ok in zip(fam.lds_bytes(name, threads // 16), lh.eligible(family, name)) if ok]
    return max(65536, max(fam.lds_bytes(name, 16)), max(at))


# (member, workgroup size) pairs the named members can reach within 160 KiB: h128's examined stage never drops to 256 (its stage 0,
# f = 1, needs 99 648 bytes, under which stage 1 already fits 512), and big_f64's 64-wide stage does not fit 1024
BIG_SIZES = [("big", "odd_wide", 256), ("big", "odd_wide", 512), ("big", "odd_wide", 1024), ("big", "h128", 512), ("big", "h128", 1024),
             ("feat", "big_f64", 256), ("feat", "big_f64", 512)]


@pytest.mark.parametrize("gname", ["er1933", "hubs"])
@pytest.mark.parametrize("family,name,threads", BIG_SIZES, ids=lambda v: str(v))
def test_every_workgroup_size_of_the_big_forms(shim, family, name, gname, threads):
    """The BIG (and, big_f64, FEAT) LIVE instantiations at 256, 512 and 1024 threads, all rows (er1933) and light rows (hubs): the
    limit is set so that the member's largest stage, which is an examined one, gets exactly that size."""
    g = graph_of(gname)
    limit = _limit_for(family, name, threads)
    e = gh.open_engine(family, name, g, opts=POISON, big=limit, heavy=HEAVY_FROM)
    try:
        if family == "feat":
            e.set_generic_feature_width(64)
        assert e.fused and e.get_info("generic_stages_model") == 1, (name, limit)
        e.set_generic_live_columns(100)
        sizes = [e.get_info(f"generic_stage_threads_{s}") for s in range(e.num_stages)]
        assert any(t == threads and ok for t, ok in zip(sizes, lh.eligible(family, name))), (name, limit, sizes)
        label = (family, name, gname, threads)
        host_forward(shim, e, family, name, gname, label)
        assert (e.get_info("generic_heavy_last_rows") > 0) == (gname == "hubs")
        assert_read_outs(e, family, name, gname, 100, label)
        host_forward(shim, e, family, name, gname, label + ("audited",), audited=True)
        assert e.get_info("audit_failures") == 0, label
    finally:
        e.close()


# ---------------------------------------------------------------- 3. the trained model as generic stages

@pytest.mark.parametrize("gname", ["er3000", "hubs", "sparse"])
def test_the_trained_model_under_option_2(shim, model_text, gname):
    import gnn_mwvc_amd as G
    g = graph_of(gname)
    e = G.Engine(model_text, device=0)
    try:
        e.set_option("poison_features", 1)
        e.set_option("generic_stages", 2)
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
        e.set_generic_live_columns(100)
        host_forward(shim, e, "trained", "model", gname, ("trained", gname))
        got = read_outs(e)
        assert got[0] == NOT_EXAMINED                                    # f == 1
        for s in (1, 2):
            f, mask = MASKS["trained", "model", gname][s]
            assert got[s] == (bin(mask).count("1"), 1, mask), (gname, s, got[s])
        host_forward(shim, e, "trained", "model", gname, ("trained", gname, "audited"), audited=True)
        assert e.get_info("audit_failures") == 0
    finally:
        e.close()


# ---------------------------------------------------------------- 4. crafted stage-0 inputs

def isolated_vertex(g):
    deg = degrees(g)
    referenced = np.zeros(g.n, dtype=bool)
    referenced[g.col[: g.nnz]] = True
    lone = np.flatnonzero((deg == 0) & ~referenced)
    assert lone.size, "the graph has no isolated vertex"
    return int(lone[len(lone) // 2])


def zeros_mixed(rng, n):
    return np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)


def crafted_cases(w, g):
    """[(label, x)]: crafted_input with columns overwritten so that exactly the chosen ones are live."""
    rng = np.random.default_rng([404, w])
    n = g.n
    base = crafted_input(n, w, 900 + w)
    base[0, :] = np.float32(1.5)   # (every column of the base is live whatever crafted_input's own -0.0 draws)

    def only(live):
        x = base.copy()
        for c in range(w):
            if c not in live:
                x[:, c] = zeros_mixed(rng, n)
        return x

    def lone_value(c, row, value=np.float32(0.75)):
        x = only(set(range(w)) - {c, (c + 1) % w})   # (a second dead column beside it)
        x[:, c] = zeros_mixed(rng, n)
        x[row, c] = value
        return x

    out = [("all dead", only(set())), ("one live", only({w - 1})), ("kept == f", base.copy())]
    c = w // 2
    out.append(("live in row 0 only", lone_value(c, 0)))
    out.append(("live in row n - 1 only", lone_value(c, n - 1)))
    out.append(("live in an isolated vertex only", lone_value(c, isolated_vertex(g))))
    x = base.copy()
    x[:, c] = np.float32(-0.0)
    out.append(("a column of -0.0f", x))
    x = only(set(range(w)) - {c})
    x.view(np.uint32)[n // 3, c] = 0x80000001   # a single (negative) denormal: live
    out.append(("a single denormal", x))
    for kept in (15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64):
        if kept <= w:
            out.append((f"kept {kept}", only(set(rng.choice(w, size=kept, replace=False).tolist()))))
    return out


def crafted_forward(shim, e, name, gname, x, percent, label):
    g = graph_of(gname)
    want = gh.logits_at("live", name, g, x=x)
    host_forward(shim, e, "live", name, gname, label, x=x, want=want)
    stages = gh.stage_outputs(gh.oracle_of("live", name, g), "live", name, g, x=x)
    assert np.array_equal(bits(stages[-1][2]), bits(want)), label       # (the walk is the predict)
    got = read_outs(e)
    for s, (hin, _, _) in enumerate(stages):
        f, mask = hin.shape[1], ml.live_mask(hin)
        kept = bin(mask).count("1")
        assert got[s] == (kept, ml.used_by_rule(kept, f, percent), mask), (label, s, got[s], kept, hex(mask))
    return got


@pytest.mark.parametrize("w", [2, 16, 17, 32, 33, 48, 49, 64])
def test_crafted_stage_0_inputs(shim, w):
    name, gname = f"in{w}", "sparse"
    g = graph_of(gname)
    e = open_live("live", name, g, 100)
    try:
        seen = set()
        for what, x in crafted_cases(w, g):
            got = crafted_forward(shim, e, name, gname, x, 100, (name, what))
            assert got[0][1] == 1                                       # 100: the table at every kept, kept == f included
            seen.add(got[0][0])
        assert {0, 1, w - 1, w} <= seen, seen
        e.set_generic_live_columns(50)
        for what, x in crafted_cases(w, g)[:4]:
            crafted_forward(shim, e, name, gname, x, 50, (name, what, 50))
        what, x = crafted_cases(w, g)[0]
        e.forward_audited(x)
        assert e.get_info("audit_failures") == 0
    finally:
        e.close()


def test_the_edge_of_the_threshold(shim):
    name, gname = "in16", "er1933"
    g = graph_of(gname)
    rng = np.random.default_rng(16)
    base = crafted_input(g.n, 16, 916)
    base[0, :] = np.float32(1.5)

    def with_kept(kept):
        x = base.copy()
        for c in rng.choice(16, size=16 - kept, replace=False).tolist():
            x[:, c] = zeros_mixed(rng, g.n)
        return x

    e = open_live("live", name, g, 50)
    try:
        for percent, kept, used in ((50, 8, 1), (50, 9, 0), (57, 9, 1), (56, 9, 0), (1, 0, 1), (1, 1, 0), (100, 16, 1), (99, 16, 0)):
            e.set_generic_live_columns(percent)
            got = crafted_forward(shim, e, name, gname, with_kept(kept), percent, (percent, kept))
            assert got[0][:2] == (kept, used), (percent, kept, got[0])
    finally:
        e.close()


# ---------------------------------------------------------------- 5. lifecycle

@pytest.mark.parametrize("family,name", [("depths", "in3_f32"), ("shapes", "odd"), ("live", "sparse32")])
def test_lifecycle_on_one_engine(shim, family, name):
    e = open_live(family, name, graph_of("er3000"), heavy=HEAVY_FROM)
    try:
        for percent in (100, 0, 100, 50):                               # under a resident graph
            e.set_generic_live_columns(percent)
            host_forward(shim, e, family, name, "er3000", (name, "resident", percent))
            assert_read_outs(e, family, name, "er3000", percent, (name, "resident", percent))
        e.set_generic_live_columns(100)
        for k, gname in enumerate(gh.LIFECYCLE_SEQUENCE):                # the table grows and shrinks with the graph
            g = graph_of(gname)
            gh.hand_over(e, g, gh.ROUTES[k % len(gh.ROUTES)])
            if g.n == 0:
                sc, _ = e.forward(gh.FAMILIES[family].model_input(name, g))
                assert sc.shape == (0, gh.FAMILIES[family].out_width(name))
                assert read_outs(e) == [NOT_EXAMINED] * e.num_stages     # n == 0: nothing is launched, nothing examined
                continue
            host_forward(shim, e, family, name, gname, (name, k, gname))
            assert_read_outs(e, family, name, gname, 100, (name, k, gname))
    finally:
        e.close()


@pytest.mark.parametrize("family,name", [("shapes", "wide"), ("depths", "in3_f32")])
def test_the_stage_entry_is_as_without_the_call(shim, family, name):
    """gnnvc_stage_forward_device over split ranges with the feature on: today's bits, and the read-outs of the last FORWARD stay."""
    gname = "hubs"
    g = graph_of(gname)
    e = open_live(family, name, g, 100, heavy=HEAVY_FROM)
    try:
        host_forward(shim, e, family, name, gname, (name, "forward"))
        after_forward = read_outs(e)
        assert after_forward == lh.expected_readouts(family, name, gname, 100)
        want = gh.want_of(family, name, gname)
        for s, (hin, hout, pre) in enumerate(want):
            gh.run_stage_ranges(e, family, name, g, s, hin, gh.split_ranges(g.n), hout, pre, (name, "stage entry"))
            assert read_outs(e) == after_forward, (name, s)
    finally:
        e.close()


# ---------------------------------------------------------------- 6. a slice of the fuzz

FUZZ = [i for i in range(mz.N) if mz.case(i).admitted][2::3]


def _blocks(cases, size):
    return [cases[at: at + size] for at in range(0, len(cases), size)]


@pytest.mark.parametrize("block", _blocks(FUZZ, 14), ids=lambda b: f"{b[0]}-{b[-1]}")
def test_random_models_with_live_columns(shim, block):
    for i in block:
        c = mz.case(i)
        g = graph_of(c.graph)
        e = fh.open_case(i, g)
        try:
            e.set_generic_live_columns(100)
            label = f"live {mz.describe(i)}"
            fh.host_forward(shim, e, i, c.graph, label)
            fh.host_forward(shim, e, i, c.graph, label)
            fh.host_forward(shim, e, i, c.graph, label + " (scaled)", scaled=True)
            fh.host_forward(shim, e, i, c.graph, label + " (audited)", audited=True)
            assert e.get_info("audit_failures") == 0, label
            fh.device_forward(shim, e, i, c.graph, label)
            stages = fh.walk_case(i, g)                                  # (the device forward took the unscaled input)
            for s, r in enumerate(c.expect):
                kept = e.get_info(f"generic_live_kept_{s}")
                examined = g.n > 0 and not r.dense and r.f >= 2 and r.end != mz.END_NONE
                if not examined:
                    assert kept == -1, (label, s)
                    continue
                mask = ml.live_mask(stages[s][0])
                assert kept == bin(mask).count("1") and e.get_info(f"generic_live_used_{s}") == 1, (label, s, kept, hex(mask))
                assert e.get_info(f"generic_live_mask_lo_{s}") | (e.get_info(f"generic_live_mask_hi_{s}") << 32) == mask, (label, s)
        finally:
            e.close()


# ---------------------------------------------------------------- 7. speed guard

def batches_ms(e, x, sc, lg):
    """[ms a forward] of three batches of five after two forwards to settle, and the logits."""
    import torch
    for _ in range(2):
        e.forward_device(x.data_ptr(), sc.data_ptr(), lg.data_ptr())
    e.synchronize()
    ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(5):
            e.forward_device(x.data_ptr(), sc.data_ptr(), lg.data_ptr())
        e.synchronize()
        ms.append((time.perf_counter() - t) * 200.0)
    return ms, lg.clone()


def test_sparse32_with_the_table_is_not_slower_than_without():
    """Measured on one MI355X (profiles/generic_stages/README.md, "Live columns"): on 1.482 ms (batches 1.482 / 1.486 / 1.486)
    against off 1.468 ms (1.601 / 1.516 / 1.468, spread 0.133 ms).  The bar holds by off's own early batches: in the steady state
    of that file's table on is 0.03 - 0.04 ms SLOWER than off on this graph (1.485 against 1.443, off / on 0.97), and 5 % faster
    on ER 10 M / 100 M (15.34 against 16.10), where the stage input no longer fits the Infinity Cache."""
    import torch
    import gnn_mwvc_amd as G
    from tools import graphgen_torch as ggt
    dev = torch.device("cuda", 0)
    g = ggt.erdos_renyi(1_000_000, 10_000_000, 2, dev)
    x = g.x().contiguous()
    e = G.Engine(gh.text_of("live", "sparse32"), device=0)
    try:
        e.set_weight_scale(g.ws)
        e.attach_graph_device(g.n, g.nnz, g.rowptr.data_ptr(), g.col.data_ptr(), g.w.data_ptr(), g.nw.data_ptr(), keepalive=g)
        sc = torch.zeros(g.n, device=dev)
        lg = torch.zeros(g.n, device=dev)
        torch.cuda.synchronize()
        off, lg0 = batches_ms(e, x, sc, lg)
        assert e.get_info("generic_stages_active") == 1 and e.get_info("generic_live_kept_1") == -1
        e.set_generic_live_columns(100)
        on, lg1 = batches_ms(e, x, sc, lg)
        kept = [e.get_info(f"generic_live_kept_{s}") for s in range(3)]
        assert kept[0] == -1 and 0 < kept[1] <= 8 and 0 < kept[2] <= 8, kept
        assert [e.get_info(f"generic_live_used_{s}") for s in range(3)] == [0, 1, 1]
        spread = max(off) - min(off)
        print(f"er1m sparse32: on {min(on):.3f} ms (batches {on}), off {min(off):.3f} ms (batches {off}), spread {spread:.3f} ms, "
              f"{min(off) / min(on):.2f}x, kept {kept}")
        assert torch.equal(lg0.view(torch.int32), lg1.view(torch.int32))
        assert min(on) <= min(off) + spread, f"on {min(on):.3f} ms vs off {min(off):.3f} ms (+ {spread:.3f})"
    finally:
        e.close()
    del g, x
    torch.cuda.empty_cache()
