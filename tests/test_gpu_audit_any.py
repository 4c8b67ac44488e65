"""The explicit audit calls (gnnvc_forward_audited, gnnvc_forward_audited_device, gnnvc_audit_stage_device) and the kernel
behind them for generic stages, k_audit_any.

Models: tools/modelgen_shapes.py and tools/modelgen_depths.py, the members at which the kernel can go wrong (small, 64-wide and
odd widths, four outputs through the sigmoid, three input features, d = 1 and d = 6, 64 / 7 alternating, f = 32 with K = 67 > the
wave, a trained-shape stage inside a generic model).  Expected values: the oracle's, as in tests/test_gpu_shapes.py and
tests/test_gpu_depths.py — bit for bit, scores by check_scores.

The audit is shown to be an implementation of its own by making it WRITE the stage: with "audit_repair" 1 and a zero-filled
output it has to repair every value whose bits are not +0.0f's — the number of repairs and the repaired rows are then the
oracle's.  One flipped bit is found and named; flips inside a forward are found and repaired; NaN inputs are no alarm; the
trained model, slices and the refusals; "audit_period" keeps auditing nothing on a generic model."""
import numpy as np
import pytest

from tools import graphgen as gg
from tools import modelgen_depths as md
from tools import modelgen_shapes as ms
from tests import generic_harness as gh
from tests.generic_harness import bits, check_scores, graph_of
from tests.test_expf_restatement import shim, _run   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED, ERR_AUDIT = -1, -5, -6

# name -> family
FAMILY = {name: "shapes" for name in ("narrow", "wide", "odd", "out4", "in3", "first_trained")}
FAMILY.update({name: "depths" for name in ("logit", "six_deep", "late_wide", "in3_f32", "too_big")})
MODELS = [name for name in FAMILY if name != "too_big"]
GRAPHS = ["er3000", "sparse", "er1933", "one", "hub8k"]   # (tests/generic_harness.py has what each is)
FETCH_BATCH = 64   # column ids k_audit_any fetches at a time


def expect_audit_error(call):
    import gnn_mwvc_amd as G
    with pytest.raises(G.GnnvcError) as err:
        call()
    assert err.value.code == ERR_AUDIT and err.value.is_audit, err.value
    return str(err.value)


def test_graphs_are_what_the_names_say():
    deg = {k: np.diff(graph_of(k).rowptr.astype(np.int64)) for k in GRAPHS}
    # the hub rows run far beyond one fetch batch of the audit's gather, and are rows 0 and 1
    assert (deg["hub8k"] > 50 * FETCH_BATCH).sum() == 2 and deg["hub8k"][:2].min() > 50 * FETCH_BATCH
    assert deg["hub8k"][0] % FETCH_BATCH != 0 and deg["hub8k"][0] % 8 != 0
    assert (deg["sparse"] == 0).mean() > 0.2
    assert graph_of("er1933").n % 64 != 0 and graph_of("er3000").n % 64 != 0 and graph_of("one").n == 1


# ---------------------------------------------------------------- 1. clean forwards

CLEAN = [(name, gname) for name in MODELS for gname in ("er3000", "sparse", "er1933")]
CLEAN += [(name, gname) for name in ("narrow", "in3_f32") for gname in ("one", "hub8k")]


@pytest.mark.parametrize("name,gname", CLEAN)
def test_forward_audited_is_clean_and_changes_nothing(name, gname):
    fam = FAMILY[name]
    g = graph_of(gname)
    x = gh.FAMILIES[fam].model_input(name, g)
    e = gh.open_engine(fam, name, g)
    try:
        ns = e.num_stages
        assert e.fused and ns == len(gh.want_of(fam, name, gname))
        sc0, lg0 = e.forward(x)
        assert e.get_info("audit_runs") == 0
        sc1, lg1 = e.forward_audited(x)
        rep = e.audit_report()
        print(name, gname, rep)
        assert rep["audit_runs"] == ns and rep["audit_failures"] == 0 and rep["audit_repairs"] == 0 and rep["audit_nan_pairs"] == 0, rep
        assert np.array_equal(bits(sc1), bits(sc0)) and np.array_equal(bits(lg1), bits(lg0)), (name, gname)
        assert np.array_equal(bits(lg1), bits(gh.want_of(fam, name, gname)[-1][2])), (name, gname)
        assert e.get_info("generic_stages_active") == 1
        e.forward_audited(x, want_logits=False)   # (without logits: the scores alone are checked)
        assert e.get_info("audit_runs") == 2 * ns and e.get_info("audit_failures") == 0
    finally:
        e.close()


def test_forward_audited_device_is_clean():
    import torch
    name, gname = "odd", "er1933"
    g = graph_of(gname)
    dev = torch.device("cuda:0")
    e = gh.open_engine("shapes", name, g)
    try:
        x = torch.from_numpy(ms.model_input(name, g)).to(dev)
        sc = torch.zeros(g.n, dtype=torch.float32, device=dev)
        lg = torch.zeros(g.n, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        e.forward_audited_device(x.data_ptr(), sc.data_ptr(), lg.data_ptr())   # (synchronises the stream itself)
        assert e.get_info("audit_runs") == e.num_stages and e.get_info("audit_failures") == 0
        assert np.array_equal(bits(lg.cpu().numpy()), bits(gh.flat_logits("shapes", name, gname)))
    finally:
        e.close()


# ---------------------------------------------------------------- 2. the audit is an implementation of its own, and covers every value

WRITES = [(name, "er1933") for name in MODELS]
WRITES += [(name, gname) for name in ("narrow", "in3_f32") for gname in ("er3000", "sparse", "one", "hub8k")]


@pytest.mark.parametrize("name,gname", WRITES)
def test_repairing_zeros_writes_the_oracles_stage(shim, name, gname):
    import torch
    fam = FAMILY[name]
    g = graph_of(gname)
    n = g.n
    want = gh.want_of(fam, name, gname)
    restated = _run(shim.sigmoid_restated, gh.flat_logits(fam, name, gname)).reshape(n, -1)   # the device's scores, bit for bit
    e = gh.open_engine(fam, name, g, {"audit_repair": 1})
    try:
        cuts = sorted({0, n // 5, n // 3, (2 * n) // 3, n})
        ranges = list(zip(cuts[:-1], cuts[1:]))
        order = ranges[0::2] + ranges[1::2]   # with gaps first, then the gaps
        for s, (hin, hout, pre) in enumerate(want):
            last = s + 1 == len(want)
            tin, out, lgt, f, n_out = gh.stage_buffers(fam, name, gname, s)
            w_out = restated if last else np.ascontiguousarray(hout, dtype=np.float32).reshape(n, n_out)
            w_pre = np.ascontiguousarray(pre, dtype=np.float32).reshape(n, n_out)
            done = np.zeros(n + 1, dtype=bool)
            for lo, hi in order:
                out[lo:hi] = 0.0
                if last:
                    lgt[lo:hi] = 0.0
                torch.cuda.synchronize()
                before = e.audit_report()
                e.audit_stage_device(s, lo, hi, tin.data_ptr(), out.data_ptr(), lgt.data_ptr() if last else 0)
                rep = e.audit_report()
                expect = int((bits(w_out[lo:hi]) != 0).sum()) + (int((bits(w_pre[lo:hi]) != 0).sum()) if last else 0)
                assert rep["audit_repairs"] - before["audit_repairs"] == expect, (name, gname, s, lo, hi, rep, expect)
                assert rep["audit_runs"] == before["audit_runs"] + 1
                assert rep["audit_failures"] == before["audit_failures"] + (1 if expect else 0)
                if expect:
                    assert rep["audit_last_stage"] == s and rep["audit_last_mismatches"] == expect and lo <= rep["audit_last_row"] < hi
                    assert rep["audit_last_fused_bits"] == 0
                done[lo:hi] = True
                got, gotl = out.cpu().numpy(), lgt.cpu().numpy()
                assert np.array_equal(bits(got[lo:hi]), bits(w_out[lo:hi])), (name, gname, s, lo, hi, "stage output")
                if last:
                    assert np.array_equal(bits(gotl[lo:hi]), bits(w_pre[lo:hi])), (name, gname, s, lo, hi, "logits")
                assert np.isnan(got[~done]).all(), (name, gname, s, "rows outside the range or the pad row were written")
                assert np.isnan(gotl[~done]).all() if last else np.isnan(gotl).all(), (name, gname, s, "logits rows")
            assert done[:n].all() and not done[n]
            if last:   # the suite's score rule, over the whole stage
                check_scores(shim, got[:n].reshape(-1), gotl[:n].reshape(-1), gh.flat_logits(fam, name, gname), (name, gname))
    finally:
        e.close()


# ---------------------------------------------------------------- 3. one wrong bit is found and named

# where -> (stage, row_lo, row_hi, row, column, in the logits) on out4 (stages 1 -> 16 -> 16 -> 4 + sigmoid), hub8k
def _positions(n):
    lo, hi = n // 5, (2 * n) // 3
    return {
        "first_row": (1, lo, hi, lo, 0, False),
        "last_row": (1, lo, hi, hi - 1, 7, False),
        "last_column": (0, lo, hi, n // 2 + 1, 15, False),
        "last_score": (2, lo, hi, n // 2 + 1, 3, False),
        "logit": (2, lo, hi, n // 2 + 3, 2, True),
        "hub_row": (1, 0, n // 3, 1, 5, False),
    }


@pytest.mark.parametrize("where", ["first_row", "last_row", "last_column", "last_score", "logit", "hub_row"])
def test_one_flipped_bit_is_found_and_named(where):
    import torch
    name, gname = "out4", "hub8k"
    g = graph_of(gname)
    n = g.n
    s, lo, hi, r, c, in_logits = _positions(n)[where]
    last = s + 1 == len(gh.want_of("shapes", name, gname))
    e = gh.open_engine("shapes", name, g)
    try:
        tin, out, lgt, f, n_out = gh.stage_buffers("shapes", name, gname, s)
        assert c < n_out and (last or not in_logits)
        e.stage_forward_device(s, 0, n, tin.data_ptr(), out.data_ptr(), lgt.data_ptr() if last else 0)
        e.synchronize()
        args = (tin.data_ptr(), out.data_ptr(), lgt.data_ptr() if last else 0)
        e.audit_stage_device(s, lo, hi, *args)   # clean as the fused path wrote it
        assert e.get_info("audit_runs") == 1 and e.get_info("audit_failures") == 0
        victim = (lgt if in_logits else out).view(torch.int32)
        good = int(victim[r, c].item()) & 0xFFFFFFFF
        victim[r, c] ^= 1
        torch.cuda.synchronize()
        msg = expect_audit_error(lambda: e.audit_stage_device(s, lo, hi, *args))
        rep = e.audit_report()
        assert (rep["audit_last_stage"], rep["audit_last_row"], rep["audit_last_col"], rep["audit_last_mismatches"]) == (s, r, c, 1), rep
        assert (rep["audit_last_fused_bits"], rep["audit_last_plain_bits"]) == (good ^ 1, good), (rep, hex(good))
        assert rep["audit_failures"] == 1 and rep["audit_repairs"] == 0
        assert f"stage {s}" in msg and f"row {r} column {c}" in msg and ("of the logits" in msg) == in_logits, msg
        assert int(victim[r, c].item()) & 0xFFFFFFFF == good ^ 1   # (no repair asked for: the value stays as it was handed in)
        # the same flip outside [row_lo, row_hi) is not this call's to report
        victim[r, c] ^= 1
        for outside in (lo - 1, hi) if lo > 0 else (hi, n - 1):
            victim[outside, c] ^= 1
            torch.cuda.synchronize()
            e.audit_stage_device(s, lo, hi, *args)
            victim[outside, c] ^= 1
        assert e.get_info("audit_failures") == 1 and e.get_info("audit_runs") == 4
    finally:
        e.close()


# ---------------------------------------------------------------- 4. inside a forward

@pytest.mark.parametrize("name", ["narrow", "six_deep"])
def test_flip_inside_a_forward_is_found_and_repaired(name):
    fam = FAMILY[name]
    gname = "er3000"
    g = graph_of(gname)
    x = gh.FAMILIES[fam].model_input(name, g)
    wl = gh.want_of(fam, name, gname)[-1][2]
    e = gh.open_engine(fam, name, g)
    try:
        ns = e.num_stages
        for s in range(ns):
            r = [g.n // 3 + 7, g.n - 1, 0][s % 3]
            e.set_option("audit_flip_stage", s)
            e.set_option("audit_flip_row", r)
            failures = e.get_info("audit_failures")
            msg = expect_audit_error(lambda: e.forward_audited(x))
            rep = e.audit_report()
            assert rep["audit_failures"] == failures + 1, rep
            assert (rep["audit_last_stage"], rep["audit_last_row"], rep["audit_last_col"], rep["audit_last_mismatches"]) == (s, r, 0, 1), rep
            assert (rep["audit_last_fused_bits"] ^ rep["audit_last_plain_bits"]) == 1, rep
            assert f"stage {s}" in msg and f"row {r}" in msg and "plan: k_stage_any" in msg, msg
            # repaired: the same flip, the call succeeds with the oracle's logits
            e.set_option("audit_repair", 1)
            repairs = e.get_info("audit_repairs")
            _, lg = e.forward_audited(x)
            assert np.array_equal(bits(lg), bits(wl)), (name, s)
            assert e.get_info("audit_repairs") == repairs + 1
            e.set_option("audit_repair", 0)
            # the hook off: clean
            e.set_option("audit_flip_stage", -1)
            failures = e.get_info("audit_failures")
            _, lg = e.forward_audited(x)
            assert np.array_equal(bits(lg), bits(wl)), (name, s)
            assert e.get_info("audit_failures") == failures
        assert e.get_info("audit_runs") == 3 * ns * ns
    finally:
        e.close()


# ---------------------------------------------------------------- 5. NaN pairs

def test_nan_input_is_no_alarm():
    name, gname = "narrow", "er3000"
    g = graph_of(gname)
    x = ms.model_input(name, g).copy()
    x.reshape(-1)[g.n // 2] = np.nan
    e = gh.open_engine("shapes", name, g)
    try:
        sc, lg = e.forward_audited(x)
        rep = e.audit_report()
        assert np.isnan(lg).any()
        assert rep["audit_nan_pairs"] > 0 and rep["audit_failures"] == 0 and rep["audit_runs"] == e.num_stages, rep
    finally:
        e.close()


# ---------------------------------------------------------------- 6. the trained model

def test_trained_model_is_audited_by_the_same_call(model_text, oracle_model):
    import gnn_mwvc_amd as G
    g = graph_of("er3000")
    oracle_model.set_weight_scale(g.ws)
    want = oracle_model.logits(g)
    e = G.Engine(model_text, device=0)
    try:
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
        assert e.get_info("generic_stages_model") == 0 and e.num_stages == 3
        _, lg = e.forward_audited(g.x())
        assert e.get_info("audit_runs") == 3 and e.get_info("audit_failures") == 0
        assert e.get_info("generic_stages_active") == 0
        assert np.array_equal(bits(lg[:, 0]), bits(want))
        e.set_option("audit_flip_stage", 1)
        msg = expect_audit_error(lambda: e.forward_audited(g.x()))
        assert "stage 1" in msg and "plan: sums=" in msg, msg
        assert e.get_info("audit_runs") == 6 and e.get_info("audit_failures") == 1 and e.get_info("audit_last_stage") == 1
    finally:
        e.close()


# ---------------------------------------------------------------- 7. refusals

def test_refusals_and_empty_calls(model_text):
    import torch
    import gnn_mwvc_amd as G
    g = graph_of("er3000")
    t = torch.zeros((g.n + 1, 32), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    # a model that runs layer by layer has no stage to audit
    e = gh.open_engine("depths", "too_big", g)
    try:
        assert not e.fused
        with pytest.raises(G.GnnvcError) as err:
            e.forward_audited(md.model_input("too_big", g))
        assert err.value.code == ERR_UNSUPPORTED
        with pytest.raises(G.GnnvcError) as err:
            e.forward_audited_device(t.data_ptr(), t.data_ptr(), 0)
        assert err.value.code == ERR_UNSUPPORTED
    finally:
        e.close()
    # the stage check is not available on a multi-device handle
    e = G.Engine(model_text, devices=[0, 0])
    try:
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
        with pytest.raises(G.GnnvcError) as err:
            e.audit_stage_device(0, 0, g.n, t.data_ptr(), t.data_ptr(), 0)
        assert err.value.code == ERR_UNSUPPORTED
    finally:
        e.close()
    e = gh.open_engine("shapes", "narrow", g)
    try:
        for stage in (e.num_stages, -1):
            with pytest.raises(G.GnnvcError) as err:
                e.audit_stage_device(stage, 0, g.n, t.data_ptr(), t.data_ptr(), 0)
            assert err.value.code == ERR_INVALID, stage
        with pytest.raises(G.GnnvcError) as err:
            e.audit_stage_device(0, 0, g.n + 1, t.data_ptr(), t.data_ptr(), 0)
        assert err.value.code == ERR_INVALID
        e.audit_stage_device(0, 100, 100, t.data_ptr(), t.data_ptr(), 0)   # an empty range: nothing to check
        assert e.get_info("audit_runs") == 0
        # no vertices: a successful no-op
        e.upload_graph(gg.from_edge_list(0, [], []))
        sc, lg = e.forward_audited(np.zeros((0, 1), dtype=np.float32))
        assert sc.shape == (0, 1) and e.get_info("audit_runs") == 0
        e.forward_audited_device(0, 0, 0)
    finally:
        e.close()


# ---------------------------------------------------------------- 8. slices

def test_a_slice_checks_rows_of_its_slice():
    import torch
    import gnn_mwvc_amd as G
    from gnn_mwvc_amd import distributed as D
    name, gname = "narrow", "er3000"
    g = graph_of(gname)
    dev = torch.device("cuda:0")
    t = lambda v: torch.from_numpy(v.astype(np.int64)).to(torch.int32).to(dev)
    lo, hi = g.n // 2, g.n
    sl = D.slice_csr(g.n, t(g.rowptr), t(g.col), t(g.w), t(g.nw), lo, hi)
    e = G.Engine(gh.text_of("shapes", name), device=0)
    try:
        e.set_weight_scale(g.ws)
        torch.cuda.synchronize()
        e.attach_graph_slice(g.n, lo, hi, sl.nnz, sl.rowptr.data_ptr(), sl.col.data_ptr(), sl.w.data_ptr(), sl.nw.data_ptr(), keepalive=sl)
        s = 1
        tin, out, lgt, f, n_out = gh.stage_buffers("shapes", name, gname, s)
        e.stage_forward_device(s, lo, hi, tin.data_ptr(), out.data_ptr(), 0)
        e.synchronize()
        a, b = lo + 37, hi - 5
        e.audit_stage_device(s, a, b, tin.data_ptr(), out.data_ptr(), 0)
        e.audit_stage_device(s, lo, hi, tin.data_ptr(), out.data_ptr(), 0)
        assert e.get_info("audit_runs") == 2 and e.get_info("audit_failures") == 0
        assert np.array_equal(bits(out[lo:hi].cpu().numpy()), bits(gh.want_of("shapes", name, gname)[s][1][lo:hi]))
        out.view(torch.int32)[hi - 1, n_out - 1] ^= 1
        torch.cuda.synchronize()
        e.audit_stage_device(s, a, b, tin.data_ptr(), out.data_ptr(), 0)       # (the flipped row is outside this range)
        expect_audit_error(lambda: e.audit_stage_device(s, lo, hi, tin.data_ptr(), out.data_ptr(), 0))
        assert (e.get_info("audit_last_row"), e.get_info("audit_last_col"), e.get_info("audit_last_mismatches")) == (hi - 1, n_out - 1, 1)
        for ra, rb in ((lo - 1, hi), (0, lo), (0, g.n)):   # rows outside the slice
            with pytest.raises(G.GnnvcError) as err:
                e.audit_stage_device(s, ra, rb, tin.data_ptr(), out.data_ptr(), 0)
            assert err.value.code == ERR_INVALID, (ra, rb)
    finally:
        e.close()


# ---------------------------------------------------------------- 9. the period path is unchanged

def test_the_period_still_audits_nothing_on_a_generic_model():
    name, gname = "narrow", "er3000"
    g = graph_of(gname)
    x = ms.model_input(name, g)
    e = gh.open_engine("shapes", name, g, {"audit_period": 1})
    try:
        _, lg0 = e.forward(x)
        assert e.get_info("audit_runs") == 0
        _, lg1 = e.forward_audited(x)
        assert e.get_info("audit_runs") == 3 and e.get_info("audit_failures") == 0
        assert np.array_equal(bits(lg0), bits(lg1))
        e.forward(x)
        assert e.get_info("audit_runs") == 3
    finally:
        e.close()
