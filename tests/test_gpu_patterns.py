"""Generic models with a dense prologue or an open ending as fused stages (gnnvc_set_generic_patterns), opt-in, under
tools/modelgen_patterns.py's family (tests/test_modelgen_patterns.py shows on the oracle that the stage-by-stage walk used here
equals predict, that every member's outputs are alive, and pins the texts and the byte figures).

Bars, as in tests/test_gpu_feature_width.py and no wider: every stage's output, every model's output and the logits bit for bit
(0 ulp) against the oracle; scores within 1 ulp of the oracle's and bit for bit the restated sigmoid's (check_scores); rows outside
a stage call's range and the row behind the end untouched; d_logits written by a stage that ends in the sigmoid and by no other.
Off must be today: not fused, 0 stages, layer by layer, the same bits.

The speed guard at the end: embed32 and trunc on ER 1 M / 10 M on one engine each, fused against layer by layer (which this
feature does not touch, so it is the baseline); the fused forward may not be slower than that by more than the spread of the
baseline's own three batches."""
import time

import numpy as np
import pytest

from tools import modelgen_patterns as mp
from tests import generic_harness as gh
from tests import pattern_harness as ph
from tests.generic_harness import bits, graph_of, heavy_counts, ulp
from tests.pattern_harness import assert_fused_as_specified, assert_layer_by_layer, assert_oracle_forward, open_engine, open_fused, want_of
from tests.test_expf_restatement import shim, _run   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)
from tests.test_modelgen_patterns import LDS_BYTES

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_AUDIT = -1, -5, -6
SMALL_GRAPHS = ["er3000", "er1933", "sparse", "one"]
OPEN_ENDED = [n for n in mp.ADMITTED if not ph.ends_in_sigmoid(n)]


def device_forward(e, name, g, audited=False):
    """gnnvc_forward_device (or its audited form) on NaN-filled outputs: (outputs, logits) as numpy, n x out_width each."""
    import torch
    dev = torch.device("cuda:0")
    x = torch.from_numpy(mp.model_input(name, g)).to(dev)
    out = torch.full((g.n, mp.out_width(name)), float("nan"), dtype=torch.float32, device=dev)
    lgt = torch.full((g.n, mp.out_width(name)), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    (e.forward_audited_device if audited else e.forward_device)(x.data_ptr(), out.data_ptr(), lgt.data_ptr())
    e.synchronize()
    return out.cpu().numpy(), lgt.cpu().numpy()


def assert_device_outputs(shim, name, gname, out, lgt, label):
    """The outputs of a device forward against the walk; the logits untouched (still NaN) unless the model ends in the sigmoid."""
    _, w_out, w_pre = want_of(name, gname)[-1]
    if ph.ends_in_sigmoid(name):
        gh.check_scores(shim, out.reshape(-1), lgt.reshape(-1), ph.flat_logits(name, gname), (name, gname, label))
    else:
        bad = np.argwhere(bits(out) != bits(w_out))
        assert bad.size == 0, (name, gname, label, f"{len(bad)} values differ, first (row, column)", bad[:6].tolist())
        assert np.isnan(lgt).all(), (name, gname, label, "d_logits was written by a model that does not end in the sigmoid")


def run_stage_ranges(e, name, g, s, hin, ranges_by_part, want_out, want_pre, label):
    """generic_harness.run_stage_ranges for this family: the stage entry over the ranges of each part in turn, on NaN-filled
    outputs; after every part the rows done so far are the oracle's and every other row (the pad row included) is still NaN.
    Logits are handed over for every stage, and written by the sigmoid stage only."""
    import torch
    dev = torch.device("cuda:0")
    n = g.n
    f, n_out = mp.stage_widths(name)[s]
    sig = mp.stage_ends(name)[s] == mp.END_SIGMOID
    tin = torch.zeros((n + 1, f), dtype=torch.float32, device=dev)
    tin[:n] = torch.from_numpy(np.ascontiguousarray(hin, dtype=np.float32).reshape(n, f)).to(dev)
    out = torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)
    lgt = torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    done = np.zeros(n + 1, dtype=bool)
    for part, todo in enumerate(ranges_by_part):
        for lo, hi in todo:
            e.stage_forward_device(s, lo, hi, tin.data_ptr(), out.data_ptr(), lgt.data_ptr())
            done[lo:hi] = True
        e.synchronize()
        got, gotl = out.cpu().numpy(), lgt.cpu().numpy()
        assert np.isnan(got[~done]).all(), (label, s, part, "rows outside the ranges were written")
        assert np.isnan(gotl[~done]).all() if sig else np.isnan(gotl).all(), (label, s, part, "logits rows")
        d = done[:n]
        if sig:
            assert np.array_equal(bits(gotl[:n][d]), bits(want_pre[d])), (label, s, part, "stage logits")
            assert ulp(got[:n][d], want_out[d]).max(initial=0) <= 1, (label, s, part, "stage scores")
        else:
            bad = np.argwhere(bits(got[:n][d]) != bits(want_out[d]))
            assert bad.size == 0, (label, s, part, f"{len(bad)} values differ, first (row, column)", bad[:6].tolist())
    return done


# ---------------------------------------------------------------- 1. off is today

@pytest.mark.parametrize("name", mp.NAMES)
def test_off_is_today(shim, name):
    e = open_engine(name, graph_of("er3000"))
    try:
        assert_layer_by_layer(e)
        assert e.get_info("generic_patterns") == 0
        first = assert_oracle_forward(shim, e, name, "er3000", "fresh")
        assert e.get_info("generic_stages_active") == 0
        e.set_generic_patterns(0)
        assert_layer_by_layer(e)
        assert e.get_info("generic_patterns") == 0
        again = assert_oracle_forward(shim, e, name, "er3000", "after 0")
        assert e.get_info("generic_stages_active") == 0 and np.array_equal(bits(first), bits(again))
    finally:
        e.close()


def test_trunc_off_is_the_unfused_model_path():
    """tests/test_gpu_parity.py::test_unfused_model_path's case: the trained model's first 14 layers, erdos_renyi(500, 2500, 17)."""
    from tools import graphgen as gg
    g = gg.erdos_renyi(500, 2500, 17)
    e = open_engine("trunc", g)
    try:
        assert not e.fused and e.num_layers == 14 and e.out_width == 16
        out, _ = e.forward(g.x(), want_logits=False)
        want = ph.predict(ph.oracle_at("trunc", g.ws), g, g.x(), stop_after=13)
        assert np.array_equal(bits(out), bits(want))
        e.set_generic_patterns(mp.OPEN_END)
        assert e.fused and e.num_stages == 2
        out2, _ = e.forward(g.x(), want_logits=False)
        assert e.get_info("generic_stages_active") == 1 and np.array_equal(bits(out2), bits(want))
    finally:
        e.close()


# ---------------------------------------------------------------- 2. on is fused

@pytest.mark.parametrize("gname", SMALL_GRAPHS)
@pytest.mark.parametrize("name", mp.ADMITTED)
def test_on_is_fused_forward_and_stage_entry(shim, name, gname):
    g = graph_of(gname)
    want = want_of(name, gname)
    e = open_fused(name, g)
    try:
        assert e.get_info("generic_patterns") == mp.MASK[name]
        assert_fused_as_specified(e, name, LDS_BYTES)
        for rep in range(2):   # (twice: nothing may depend on what an earlier forward left)
            assert_oracle_forward(shim, e, name, gname, rep)
            assert e.get_info("generic_stages_active") == 1
        out, lgt = device_forward(e, name, g)
        assert_device_outputs(shim, name, gname, out, lgt, "forward_device")
        assert len(want) == e.num_stages
        for s, (hin, hout, pre) in enumerate(want):
            done = run_stage_ranges(e, name, g, s, hin, [[(0, g.n)]], hout, pre, (name, gname))
            assert done[:g.n].all() and not done[g.n]
    finally:
        e.close()


@pytest.mark.parametrize("name", mp.ADMITTED)
def test_the_empty_graph(name):
    g = graph_of("empty")
    e = open_fused(name, g)
    try:
        assert e.fused
        out, _ = e.forward(mp.model_input(name, g), want_logits=False)
        assert out.shape == (0, mp.out_width(name))
    finally:
        e.close()


@pytest.mark.parametrize("gname", ph.GOLDEN_GRAPHS)
def test_trunc_equals_the_golden_h2(gname):
    g, h2 = ph.golden_h2(gname)
    e = open_fused("trunc", g)
    try:
        assert e.fused and [e.stage_widths(s) for s in range(e.num_stages)] == [(1, 16), (16, 16)]
        out, _ = e.forward(g.x(), want_logits=False)
        assert e.get_info("generic_stages_active") == 1
        assert np.array_equal(bits(out), bits(h2)), gname
    finally:
        e.close()


# ---------------------------------------------------------------- 3. the mask is needed

@pytest.mark.parametrize("name", mp.ADMITTED)
def test_each_bit_admits_only_its_members(shim, name):
    g = graph_of("er3000")
    e = open_engine(name, g, width=64 if name in mp.NEEDS_FEAT else None, big=mp.FULL_LDS if name in mp.NEEDS_BIG else None)
    try:
        first = None
        for mask in (0, 1, 2, 3, 2, 1, 0):
            e.set_generic_patterns(mask)
            assert e.get_info("generic_patterns") == mask
            if mp.admitted_by(name, mask):
                assert_fused_as_specified(e, name, LDS_BYTES)
            else:
                assert_layer_by_layer(e)
            got = assert_oracle_forward(shim, e, name, "er3000", mask)
            assert e.get_info("generic_stages_active") == int(mp.admitted_by(name, mask))
            first = got if first is None else first
            assert np.array_equal(bits(got), bits(first)), (name, mask)
        assert mp.admitted_by(name, 3) and not mp.admitted_by(name, 0)
    finally:
        e.close()


@pytest.mark.parametrize("name", mp.NEEDS_FEAT + mp.NEEDS_BIG)
def test_the_second_opt_in_is_needed_in_either_order(shim, name):
    g = graph_of("er3000")
    second = (lambda e, on: e.set_generic_feature_width(64 if on else 0)) if name in mp.NEEDS_FEAT else \
             (lambda e, on: e.set_generic_big_stages(mp.FULL_LDS if on else 0))
    e = open_engine(name, g, mask=mp.PROLOGUE)
    try:
        assert_layer_by_layer(e)                       # the mask alone
        lg0 = assert_oracle_forward(shim, e, name, "er3000", "mask alone")
        second(e, True)
        assert_fused_as_specified(e, name, LDS_BYTES)   # the mask, then the second call
        lg1 = assert_oracle_forward(shim, e, name, "er3000", "mask, then the second")
        assert e.get_info("generic_stages_active") == 1
        e.set_generic_patterns(0)
        assert_layer_by_layer(e)                       # the second call alone
        lg2 = assert_oracle_forward(shim, e, name, "er3000", "the second alone")
        e.set_generic_patterns(mp.PROLOGUE)
        assert_fused_as_specified(e, name, LDS_BYTES)   # the second call, then the mask
        lg3 = assert_oracle_forward(shim, e, name, "er3000", "the second, then the mask")
        second(e, False)
        assert_layer_by_layer(e)
        assert all(np.array_equal(bits(lg0), bits(x)) for x in (lg1, lg2, lg3))
    finally:
        e.close()


@pytest.mark.parametrize("name", mp.NOT_FITTING)
def test_the_not_fitting_members_are_never_fused(shim, name):
    e = open_engine(name, graph_of("er3000"), width=64, big=mp.FULL_LDS)
    try:
        for mask in (0, 1, 2, 3):
            e.set_generic_patterns(mask)
            assert_layer_by_layer(e)
            assert_oracle_forward(shim, e, name, "er3000", mask)
            assert e.get_info("generic_stages_active") == 0
    finally:
        e.close()


def test_a_model_within_todays_grammar_keeps_its_launches():
    g = graph_of("er3000")
    e = gh.open_engine("shapes", "narrow", g, expect_fused=True)
    try:
        read = lambda: [(e.stage_widths(s), e.get_info(f"generic_stage_layers_{s}"), e.get_info(f"generic_stage_threads_{s}"),
                         e.get_info(f"generic_stage_lds_bytes_{s}")) for s in range(e.num_stages)]
        before = read()
        _, lg0 = e.forward(gh.FAMILIES["shapes"].model_input("narrow", g))
        e.set_generic_patterns(3)
        assert read() == before
        ns = e.num_stages
        assert [e.get_info(f"generic_stage_dense_{s}") for s in range(ns)] == [0] * ns
        assert [e.get_info(f"generic_stage_end_{s}") for s in range(ns)] == [0] * (ns - 1) + [1]
        _, lg1 = e.forward(gh.FAMILIES["shapes"].model_input("narrow", g))
        assert np.array_equal(bits(lg0), bits(lg1)) and e.get_info("generic_stages_active") == 1
    finally:
        e.close()


def test_invalid_masks_are_refused_and_change_nothing():
    import gnn_mwvc_amd as G
    e = open_engine("both", graph_of("er3000"), mask=3)
    try:
        for bad in (4, 7, 8, 0x80000000, 0xFFFFFFFF):
            with pytest.raises(G.engine.GnnvcError) as ei:
                e.set_generic_patterns(bad)
            assert ei.value.code == ERR_INVALID, bad
            assert e.get_info("generic_patterns") == 3
            assert_fused_as_specified(e, "both", LDS_BYTES)
        e.set_generic_patterns(0)
        with pytest.raises(G.engine.GnnvcError) as ei:
            e.set_generic_patterns(4)
        assert ei.value.code == ERR_INVALID and e.get_info("generic_patterns") == 0
        assert_layer_by_layer(e)
        with pytest.raises(G.engine.GnnvcError):
            e.get_info("generic_stage_dense_0")       # (no generic stage list: as "generic_stage_layers_<s>")
    finally:
        e.close()


def test_a_multi_device_handle_refuses_the_call(model_text):
    import gnn_mwvc_amd as G
    e = G.Engine(model_text, devices=[0, 0])
    try:
        for value in (0, 1, 3):
            with pytest.raises(G.engine.GnnvcError) as ei:
                e.set_generic_patterns(value)
            assert ei.value.code == ERR_UNSUPPORTED, value
    finally:
        e.close()


# ---------------------------------------------------------------- 4. ranges

@pytest.mark.parametrize("name", ["embed", "embed32", "both"])
def test_split_ranges_over_a_dense_stage_and_the_graph_stage_behind_it(name):
    gname = "er1933"   # n = 30 * 64 + 13
    g = graph_of(gname)
    want = want_of(name, gname)
    e = open_fused(name, g)
    try:
        assert mp.stage_dense(name)[:2] == [1, 0]
        first, gap = gh.split_ranges(g.n)
        for s in (0, 1):
            hin, hout, pre = want[s]
            done = run_stage_ranges(e, name, g, s, hin, [first, gap], hout, pre, (name, gname, "split"))
            assert done[:g.n].all() and not done[g.n]
    finally:
        e.close()


def test_two_slices_compute_the_whole_of_embeds_stages():
    import torch
    import gnn_mwvc_amd as G
    from gnn_mwvc_amd import distributed as D
    name, gname = "embed", "er1933"
    g = graph_of(gname)
    n = g.n
    want = want_of(name, gname)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(a.astype(np.int64)).to(torch.int32).to(dev)
    rp, col, w, nw = t(g.rowptr), t(g.col), t(g.w), t(g.nw)
    bufs = []
    for s, (hin, _, _) in enumerate(want):
        f, n_out = mp.stage_widths(name)[s]
        tin = torch.zeros((n + 1, f), dtype=torch.float32, device=dev)
        tin[:n] = torch.from_numpy(np.ascontiguousarray(hin)).to(dev)
        bufs.append((tin, torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev),
                     torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)))
    for lo, hi in ((0, 701), (701, n)):
        sl = D.slice_csr(n, rp, col, w, nw, lo, hi)
        e = G.Engine(ph.text_of(name), device=0)
        try:
            e.set_weight_scale(g.ws)
            e.set_generic_patterns(mp.PROLOGUE)
            assert e.fused and e.num_stages == 3
            torch.cuda.synchronize()
            e.attach_graph_slice(n, lo, hi, sl.nnz, sl.rowptr.data_ptr(), sl.col.data_ptr(), sl.w.data_ptr(), sl.nw.data_ptr(), keepalive=sl)
            for s, (tin, out, lgt) in enumerate(bufs):
                e.stage_forward_device(s, lo, hi, tin.data_ptr(), out.data_ptr(), lgt.data_ptr())
            e.synchronize()
        finally:
            e.close()
    for s, ((_, hout, pre), (_, out, lgt)) in enumerate(zip(want, bufs)):
        got, gotl = out.cpu().numpy(), lgt.cpu().numpy()
        assert np.isnan(got[n]).all() and np.isnan(gotl[n]).all(), (s, "the pad row was written")
        if s + 1 == len(want):
            assert np.array_equal(bits(gotl[:n]), bits(pre)), "logits"
            assert ulp(got[:n], hout).max(initial=0) <= 1, "scores"
        else:
            assert np.isnan(gotl).all(), (s, "logits")
            bad = np.argwhere(bits(got[:n]) != bits(hout))
            assert bad.size == 0, (s, f"{len(bad)} values differ, first (row, column)", bad[:6].tolist())


# ---------------------------------------------------------------- 5. heavy and giant rows behind a prologue

@pytest.mark.parametrize("name", ["embed", "embed32"])
def test_heavy_and_giant_rows_behind_a_prologue(shim, name):
    gname = "hubs"
    g = graph_of(gname)
    want = want_of(name, gname)
    e = open_fused(name, g, heavy=512)
    try:
        # the dense stage alone classes nothing: the graph was handed over to a layer-by-layer model, so no row is listed yet
        hin, hout, pre = want[0]
        run_stage_ranges(e, name, g, 0, hin, [[(0, g.n)]], hout, pre, (name, "dense stage alone"))
        assert e.get_info("generic_heavy_rows") == 0 and e.get_info("generic_heavy_last_rows") == 0
        assert e.get_info("generic_giant_rows") == 0 and e.get_info("generic_giant_last_rows") == 0
        hin, hout, pre = want[1]
        run_stage_ranges(e, name, g, 1, hin, [[(0, g.n)]], hout, pre, (name, "the graph stage behind it"))
        assert e.get_info("generic_heavy_rows") == heavy_counts(g, 512)[0] == e.get_info("generic_heavy_last_rows") == 7
        first = None
        for heavy, giant in ((0, 0), (512, 0), (1, 0), (512, 1024), (1, 1024), (0, 1024)):
            e.set_generic_heavy_rows(heavy)
            e.set_generic_giant_rows(giant, 1)
            lg = assert_oracle_forward(shim, e, name, gname, (heavy, giant))
            first = lg if first is None else first
            assert np.array_equal(bits(lg), bits(first)), (name, heavy, giant)
            assert e.get_info("generic_heavy_last_rows") == heavy_counts(g, heavy)[0] == e.get_info("generic_heavy_rows"), (heavy, giant)
            grows = heavy_counts(g, max(giant, heavy))[0] if giant and heavy else 0
            assert e.get_info("generic_giant_last_rows") == grows == e.get_info("generic_giant_rows"), (heavy, giant)
            assert e.get_info("generic_stages_active") == 1
    finally:
        e.close()


# ---------------------------------------------------------------- 6. the audit

@pytest.mark.parametrize("name", mp.ADMITTED)
def test_forward_audited_device_is_clean(shim, name):
    gname = "er3000"
    g = graph_of(gname)
    e = open_fused(name, g)
    try:
        out, lgt = device_forward(e, name, g, audited=True)
        rep = e.audit_report()
        assert rep["audit_runs"] == e.num_stages == len(mp.stages_of(name)) and rep["audit_failures"] == 0 and rep["audit_repairs"] == 0, rep
        assert_device_outputs(shim, name, gname, out, lgt, "forward_audited_device")
        for _ in range(3):   # "audit_period" goes on auditing nothing on a generic model
            e.set_option("audit_period", 1)
            device_forward(e, name, g)
            assert e.audit_report()["audit_runs"] == rep["audit_runs"]
    finally:
        e.close()


# (member, the stage whose row is flipped): a dense stage, and a last stage that ends in its bare linear layer
FLIPS = [("embed", 0), ("embed32", 0), ("both", 0), ("mlp", 0), ("linear_end", 1), ("linear_end17", 0)]


@pytest.mark.parametrize("name,stage", FLIPS)
def test_a_flipped_value_is_found_named_and_repaired(shim, name, stage):
    import gnn_mwvc_amd as G
    gname = "er1933"
    g = graph_of(gname)
    assert mp.stage_dense(name)[stage] == 1 or mp.stage_ends(name)[stage] == mp.END_NONE
    row = g.n // 3 + 7
    e = open_fused(name, g)
    try:
        e.set_option("audit_flip_stage", stage)
        e.set_option("audit_flip_row", row)
        with pytest.raises(G.GnnvcError) as err:
            device_forward(e, name, g, audited=True)
        assert err.value.code == ERR_AUDIT and err.value.is_audit
        msg = str(err.value)
        rep = e.audit_report()
        assert rep["audit_failures"] == 1 and rep["audit_repairs"] == 0, rep
        assert (rep["audit_last_stage"], rep["audit_last_row"], rep["audit_last_col"], rep["audit_last_mismatches"]) == (stage, row, 0, 1), rep
        assert (rep["audit_last_fused_bits"] ^ rep["audit_last_plain_bits"]) == 1, rep
        assert f"stage {stage}" in msg and f"row {row}" in msg and "plan: k_stage_any" in msg and "of the logits" not in msg, msg
        assert ("dense rows" in msg) == bool(mp.stage_dense(name)[stage]), msg
        e.set_option("audit_repair", 1)   # the same flip, repaired: the call succeeds with the oracle's values
        out, lgt = device_forward(e, name, g, audited=True)
        assert_device_outputs(shim, name, gname, out, lgt, "repaired")
        assert e.get_info("audit_repairs") == 1 and e.get_info("audit_failures") == 2
        e.set_option("audit_repair", 0)
        e.set_option("audit_flip_stage", -1)   # the hook off: clean
        out, lgt = device_forward(e, name, g, audited=True)
        assert_device_outputs(shim, name, gname, out, lgt, "hook off")
        assert e.get_info("audit_failures") == 2
    finally:
        e.close()


@pytest.mark.parametrize("name", ["embed", "linear_end17", "trunc"])
def test_repairing_zeros_writes_the_oracles_stage(shim, name):
    import torch
    gname = "er1933"
    g = graph_of(gname)
    n = g.n
    want = want_of(name, gname)
    e = open_fused(name, g, opts={"audit_repair": 1})
    try:
        dev = torch.device("cuda:0")
        for s, (hin, hout, pre) in enumerate(want):
            f, n_out = mp.stage_widths(name)[s]
            sig = mp.stage_ends(name)[s] == mp.END_SIGMOID
            w_out = _run(shim.sigmoid_restated, np.ascontiguousarray(pre.reshape(-1))).reshape(n, n_out) if sig else hout   # the device's scores, bit for bit
            tin = torch.zeros((n + 1, f), dtype=torch.float32, device=dev)
            tin[:n] = torch.from_numpy(np.ascontiguousarray(hin)).to(dev)
            out = torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)
            lgt = torch.full((n + 1, n_out), float("nan"), dtype=torch.float32, device=dev)
            out[:n] = 0.0
            if sig:
                lgt[:n] = 0.0
            torch.cuda.synchronize()
            before = e.audit_report()
            e.audit_stage_device(s, 0, n, tin.data_ptr(), out.data_ptr(), lgt.data_ptr())
            rep = e.audit_report()
            expect = int((bits(w_out) != 0).sum()) + (int((bits(pre) != 0).sum()) if sig else 0)
            assert expect > 0
            assert rep["audit_repairs"] - before["audit_repairs"] == expect, (name, s, rep, expect)
            got, gotl = out.cpu().numpy(), lgt.cpu().numpy()
            assert np.array_equal(bits(got[:n]), bits(w_out)), (name, s, "stage output")
            assert np.array_equal(bits(gotl[:n]), bits(pre)) if sig else np.isnan(gotl).all(), (name, s, "logits")
            assert np.isnan(got[n]).all() and np.isnan(gotl[n]).all(), (name, s, "the row behind the end was written")
    finally:
        e.close()


# ---------------------------------------------------------------- 7. live changes under a resident graph

def test_live_changes_under_a_resident_graph(shim):
    name, gname = "both", "hubs"
    g = graph_of(gname)
    x = mp.model_input(name, g)
    e = open_engine(name, g)   # off; heavy rows at their default (512)
    try:
        assert_layer_by_layer(e)
        off = assert_oracle_forward(shim, e, name, gname, "off")
        assert e.get_info("generic_stages_active") == 0
        e.set_generic_patterns(3)
        assert_fused_as_specified(e, name, LDS_BYTES)
        on = assert_oracle_forward(shim, e, name, gname, "3")
        assert e.get_info("generic_stages_active") == 1 and np.array_equal(bits(on), bits(off))
        assert e.get_info("generic_heavy_last_rows") == 7 == e.get_info("generic_heavy_rows")
        e.set_generic_patterns(0)
        assert_layer_by_layer(e)
        e.set_generic_heavy_rows(513)   # a threshold change while off
        assert np.array_equal(bits(assert_oracle_forward(shim, e, name, gname, "0 again")), bits(off))
        assert e.get_info("generic_stages_active") == 0
        e.set_generic_patterns(3)
        assert_fused_as_specified(e, name, LDS_BYTES)
        assert np.array_equal(bits(assert_oracle_forward(shim, e, name, gname, "3 again, heavy 513")), bits(off))
        assert e.get_info("generic_heavy_last_rows") == heavy_counts(g, 513)[0] == e.get_info("generic_heavy_rows")
        # another weight scale: the oracle at that scale, fused and layer by layer
        ws2 = g.ws * 1.75
        e.set_weight_scale(ws2)
        want2 = ph.walk(ph.oracle_at(name, ws2), name, g, ws=ws2)[-1][1]
        out2, _ = e.forward(x, want_logits=False)
        assert np.array_equal(bits(out2), bits(want2)) and not np.array_equal(bits(out2), bits(off))
        e.set_generic_patterns(0)
        out2_off, _ = e.forward(x, want_logits=False)
        assert e.get_info("generic_stages_active") == 0 and np.array_equal(bits(out2_off), bits(want2))
        e.set_weight_scale(g.ws)
        e.set_generic_patterns(3)
        assert np.array_equal(bits(assert_oracle_forward(shim, e, name, gname, "back")), bits(off))
        assert e.get_info("generic_stages_active") == 1
    finally:
        e.close()


# ---------------------------------------------------------------- 8. speed guard

def batches_ms(e, x, out):
    """[ms a forward] of three batches of five after two warm-up forwards (the loop of gh.steady_ms, every batch kept), the outputs."""
    import torch
    for _ in range(2):
        e.forward_device(x.data_ptr(), out.data_ptr(), 0)
    e.synchronize()
    ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(5):
            e.forward_device(x.data_ptr(), out.data_ptr(), 0)
        e.synchronize()
        ms.append((time.perf_counter() - t) * 200.0)
    return ms, out.clone()


def test_fused_is_not_slower_than_layer_by_layer():
    import torch
    import gnn_mwvc_amd as G
    from tools import graphgen_torch as ggt
    dev = torch.device("cuda", 0)
    g = ggt.erdos_renyi(1_000_000, 10_000_000, 2, dev)
    x1 = g.x().contiguous().reshape(g.n, 1)
    try:
        for name in ("embed32", "trunc"):
            w = mp.in_width(name)   # (tools/modelgen_generic.py's input columns: x, 0.37 x, 1 - x, 3 x, 4 x, ...)
            cols = [x1, x1 * 0.37, 1.0 - x1] + [x1 * float(c) for c in range(3, w)]
            x = torch.cat(cols[:w], dim=1).contiguous()
            e = G.Engine(ph.text_of(name), device=0)
            try:
                e.set_weight_scale(g.ws)
                e.attach_graph_device(g.n, g.nnz, g.rowptr.data_ptr(), g.col.data_ptr(), g.w.data_ptr(), g.nw.data_ptr(), keepalive=g)
                out = torch.zeros((g.n, mp.out_width(name)), device=dev)
                torch.cuda.synchronize()
                off, out0 = batches_ms(e, x, out)
                assert e.get_info("generic_stages_active") == 0
                e.set_generic_patterns(mp.MASK[name])
                assert e.fused
                on, out1 = batches_ms(e, x, out)
                assert e.get_info("generic_stages_active") == 1
                spread = max(off) - min(off)
                print(f"er1m {name}: fused {min(on):.3f} ms (batches {on}), layer by layer {min(off):.3f} ms (batches {off}), "
                      f"spread {spread:.3f} ms, {min(off) / min(on):.2f}x")
                assert torch.equal(out0.view(torch.int32), out1.view(torch.int32)), name
                assert min(on) <= min(off) + spread, f"{name}: fused {min(on):.3f} ms vs layer by layer {min(off):.3f} ms (+ {spread:.3f})"
            finally:
                e.close()
            del x, out, out0, out1
    finally:
        del g, x1
        torch.cuda.empty_cache()
