"""The on-device audit (options "audit_period", "audit_repair", "audit_flip_stage" / "audit_flip_row"; k_audit_stage): every
k-th forward call has each fused stage recomputed by code that uses none of the plans and compared bit for bit.  A flipped bit is
caught in every stage, on the plans and on long / giant rows; repair mode hands back the oracle's logits; nothing is flagged
across a fixed-seed draw of graphs and plan options; unaudited calls launch what they always did; stage calls, slices, the
multi-device handle and the reference CLI audit too."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tools import graphgen as gg

pytestmark = pytest.mark.gpu

ERR_AUDIT = -6


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _engine(model_text, g, opts=(), devices=None):
    import gnn_mwvc_amd as G
    e = G.Engine(model_text, devices=devices) if devices else G.Engine(model_text, device=0)
    for k, v in dict(opts).items():
        e.set_option(k, v)
    e.set_weight_scale(g.ws)
    e.upload_graph(g)
    return e


def _expect_audit_error(e, x):
    import gnn_mwvc_amd as G
    with pytest.raises(G.GnnvcError) as err:
        e.forward(x)
    assert err.value.code == ERR_AUDIT and err.value.is_audit, err.value
    return str(err.value)


# ---------------------------------------------------------------- 1 + 2: a flipped bit is caught (and repaired) in every stage
_PLANNED = {"blocked_min_n": 0, "compact_min_n": 0, "plans_at_handoff": 2}
_LONG = {"long_row_threshold": 64, "giant_row_threshold": 1000}


@pytest.fixture(scope="module")
def er300k():
    return gg.erdos_renyi(300_000, 1_800_000, 11)


@pytest.fixture(scope="module")
def rmat_hubs():
    return gg.rmat(15, 12, 5)


@pytest.mark.parametrize("which", ["er300k_plans", "rmat_long_giant"])
def test_flip_is_caught_and_repaired_in_every_stage(model_text, oracle_model, er300k, rmat_hubs, which):
    g, opts = (er300k, _PLANNED) if which == "er300k_plans" else (rmat_hubs, _LONG)
    oracle_model.set_weight_scale(g.ws)
    want = oracle_model.logits(g)
    x = g.x()
    e = _engine(model_text, g, opts)
    try:
        if which == "er300k_plans":   # the plans are really in force
            assert e.get_info("lds_table_active") or e.get_info("blocked_stage0_active")
            assert e.get_info("compact_gather_active")
        else:
            assert e.get_info("long_rows") > 0 and e.get_info("giant_rows") > 0
        plain_scores, lg = e.forward(x)                       # (unaudited: the scores every later forward must give)
        assert np.array_equal(bits(lg[:, 0]), bits(want))
        e.set_option("audit_period", 1)
        ns = e.num_stages
        deg = np.diff(g.rowptr.astype(np.int64))
        rows = [g.n // 3 + 7, int(np.argmax(deg)), g.n - 1]   # (the R-MAT graph's heaviest row is a giant one)
        for s in range(ns):
            r = rows[s]
            # -- found: the call finishes, says where, the engine stays usable
            e.set_option("audit_flip_stage", s)
            e.set_option("audit_flip_row", r)
            failures = e.get_info("audit_failures")
            msg = _expect_audit_error(e, x)
            rep = e.audit_report()
            assert rep["audit_failures"] == failures + 1, rep
            assert (rep["audit_last_stage"], rep["audit_last_row"], rep["audit_last_col"], rep["audit_last_mismatches"]) == (s, r, 0, 1), rep
            assert (rep["audit_last_fused_bits"] ^ rep["audit_last_plain_bits"]) == 1, rep
            assert f"stage {s}" in msg and f"row {r}" in msg and "plan: sums=" in msg, msg
            if which == "rmat_long_giant":
                assert "long_rows=" in msg, msg
            # -- repaired: same flip, the call succeeds with the oracle's logits
            e.set_option("audit_repair", 1)
            repairs = e.get_info("audit_repairs")
            scores, lg = e.forward(x)
            assert np.array_equal(bits(lg[:, 0]), bits(want)), (which, s)
            assert np.array_equal(bits(scores), bits(plain_scores)), (which, s)
            assert e.get_info("audit_repairs") == repairs + 1
            e.set_option("audit_repair", 0)
            # -- the flip off: clean, and the oracle's logits
            e.set_option("audit_flip_stage", -1)
            failures = e.get_info("audit_failures")
            _, lg = e.forward(x)
            assert np.array_equal(bits(lg[:, 0]), bits(want)), (which, s)
            assert e.get_info("audit_failures") == failures
        assert e.get_info("audit_nan_pairs") == 0
    finally:
        e.close()


# ---------------------------------------------------------------- 3: no false alarms across the plan space
def _graph(rng):
    kind = rng.choice(["er", "rmat", "hub", "chung", "dense"])
    seed = int(rng.integers(1 << 30))
    if kind == "er":
        n = int(rng.integers(2000, 60000))
        return gg.erdos_renyi(n, int(n * rng.uniform(2, 12)), seed)
    if kind == "rmat":
        return gg.rmat(int(rng.integers(11, 16)), int(rng.integers(4, 17)), seed)
    if kind == "hub":
        n = int(rng.integers(5000, 50000))
        return gg.hub_graph(n, int(n * rng.uniform(2, 8)), int(rng.integers(1, 5)), int(rng.integers(300, min(n - 1, 20000))), seed=seed)
    if kind == "chung":
        n = int(rng.integers(5000, 50000))
        return gg.chung_lu_hubs(n, float(rng.uniform(4, 12)), float(rng.uniform(2.0, 2.6)), int(rng.integers(0, 4)),
                                int(rng.integers(300, min(n - 1, 9000))), seed=seed)
    n = int(rng.integers(1500, 4000))
    return gg.erdos_renyi(n, n * int(rng.integers(60, 200)), seed)


def _options(rng):
    o = {"blocked_min_n": 0, "prune_min_entries": 0, "prune_min_drop_percent": int(rng.integers(0, 30))}
    if rng.random() < 0.7:
        o["long_row_threshold"] = int(rng.choice([0, 8, 40, 64, 128, 256, 512]))
    if rng.random() < 0.5:
        o["sorted_long_row_threshold"] = int(rng.choice([64, 256, 512, 1024, 2048]))
    if rng.random() < 0.7:
        o["giant_row_threshold"] = int(rng.choice([0, 64, 300, 1000, 4096, 16384]))
    if rng.random() < 0.4:
        o["giant_row_threshold_f16"] = int(rng.choice([64, 1000, 5000, 65536]))
    o["giant_segments"] = int(rng.choice([-1, 0, 1]))
    o["sorted_tiles"] = int(rng.choice([-1, 0, 1]))
    o["prune_zero_rows"] = int(rng.choice([0, 1, 1]))
    o["prune_class_by_entries_left"] = int(rng.choice([0, 1, 1]))
    o["prune_giant_rows"] = int(rng.choice([0, 1, 1]))
    o["lds_table"] = int(rng.choice([0, 1, 1]))
    o["lds_table_skewed_rows"] = int(rng.choice([0, 64, 512, 2048, 16384]))
    o["compact_gather"] = int(rng.choice([0, 1, 1]))
    o["compact_min_n"] = int(rng.choice([0, 1 << 18]))
    o["plans_at_handoff"] = int(rng.choice([0, 1, 2]))
    o["mfma_dense"] = int(rng.choice([0, 1, 2]))
    o["overlap_dense"] = int(rng.choice([0, 1]))
    if rng.random() < 0.3:
        o["plan_chunk_rows"] = int(rng.choice([16, 48, 256, 4096]))
    o["table_tiles"] = int(rng.choice([0, 1, 1]))
    o["table_tiles_min_n"] = int(rng.choice([0, 0, 49152]))
    o["wide_tiles"] = int(rng.choice([0, 1, 1]))
    o["side_streams"] = int(rng.choice([0, 1, 1, 1]))
    o["long_rows_on_main"] = int(rng.choice([-1, 0, 1]))
    o["poison_features"] = int(rng.choice([0, 1]))
    return o


@pytest.mark.parametrize("block", range(4))
def test_no_false_alarms_across_the_plan_space(model_text, oracle_model, block):
    for case in range(block * 16, block * 16 + 16):
        rng = np.random.default_rng(31_000 + case)
        g, opts = _graph(rng), _options(rng)
        oracle_model.set_weight_scale(g.ws)
        want = oracle_model.logits(g)
        e = _engine(model_text, g, dict(opts, audit_period=1))
        try:
            for rep in range(3):
                _, lg = e.forward(g.x())
                assert np.array_equal(bits(lg[:, 0]), bits(want)), (case, rep, opts)
            r = e.audit_report()
            assert r["audit_failures"] == 0 and r["audit_runs"] == 3 * e.num_stages, (case, r, opts)
        finally:
            e.close()


# ---------------------------------------------------------------- 4: the period; period 0 launches what no option launches
def test_period_and_unaudited_launches(model_text, oracle_model):
    g = gg.rmat(14, 8, 3)
    oracle_model.set_weight_scale(g.ws)
    want = oracle_model.logits(g)
    e = _engine(model_text, g, {"audit_period": 3, "long_row_threshold": 64})
    try:
        for _ in range(7):
            _, lg = e.forward(g.x())
            assert np.array_equal(bits(lg[:, 0]), bits(want))
        assert e.get_info("audit_runs") == 2 * e.num_stages and e.get_info("audit_failures") == 0
    finally:
        e.close()
    names = []
    for opts in ({"kernel_trace": 1}, {"kernel_trace": 1, "audit_period": 0, "audit_repair": 1, "audit_flip_stage": 1}):
        e = _engine(model_text, g, dict(opts, long_row_threshold=64))
        try:
            for _ in range(3):
                e.forward(g.x())
            names.append([n for n, _ in e.kernel_trace(4096)])
            assert e.get_info("audit_runs") == 0
        finally:
            e.close()
    assert names[0] == names[1] and names[0], names
    assert not any("audit" in n for n in names[0])


# ---------------------------------------------------------------- 5: stage calls over row ranges, a slice
def test_stage_calls_and_slices(model_text, oracle_model):
    import torch
    import gnn_mwvc_amd as G
    from gnn_mwvc_amd import distributed as D
    dev = torch.device("cuda:0")
    g = gg.hub_graph(20000, 120000, 3, 3000, seed=4)
    oracle_model.set_weight_scale(g.ws)
    h1 = oracle_model.predict(g, g.x(), stop_after=6)   # stage 1's input
    x = torch.from_numpy(g.x()).to(dev)
    hin = torch.zeros((g.n + 1, 16), dtype=torch.float32, device=dev)
    hin[: g.n] = torch.from_numpy(np.ascontiguousarray(h1, dtype=np.float32)).to(dev)
    e = _engine(model_text, g, {"long_row_threshold": 64, "giant_row_threshold": 1000, "audit_period": 1})
    try:
        a, b = 4096, 12288
        for st, src in ((0, x), (1, hin)):
            clean = torch.full((g.n + 1, 16), 7.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            e.set_option("audit_flip_stage", -1)
            e.stage_forward_device(st, a, b, src.data_ptr(), clean.data_ptr(), 0)
            for r, inside in ((a + 100, True), (b + 5, False), (a - 1, False)):
                e.set_option("audit_flip_stage", st)
                e.set_option("audit_flip_row", r)
                out = torch.full((g.n + 1, 16), 7.0, dtype=torch.float32, device=dev)
                runs, failures = e.get_info("audit_runs"), e.get_info("audit_failures")
                torch.cuda.synchronize()
                if inside:
                    with pytest.raises(G.GnnvcError) as err:
                        e.stage_forward_device(st, a, b, src.data_ptr(), out.data_ptr(), 0)
                    assert err.value.code == ERR_AUDIT and f"row {r}" in str(err.value), err.value
                    assert (e.get_info("audit_last_stage"), e.get_info("audit_last_row")) == (st, r)
                else:
                    e.stage_forward_device(st, a, b, src.data_ptr(), out.data_ptr(), 0)
                assert e.get_info("audit_runs") == runs + 1
                assert e.get_info("audit_failures") == failures + (1 if inside else 0)
                e.synchronize()
                got, ref = out[a:b].cpu().numpy(), clean[a:b].cpu().numpy()
                diff = np.argwhere(bits(got) != bits(ref))
                assert diff.tolist() == ([[r - a, 0]] if inside else []), (st, r, diff[:4])
        e.set_option("audit_flip_stage", -1)
        # a slice audits its own rows (global row ids)
        t = lambda v: torch.from_numpy(v.astype(np.int64)).to(torch.int32).to(dev)
        lo, hi = 6000, 15000
        sl = D.slice_csr(g.n, t(g.rowptr), t(g.col), t(g.w), t(g.nw), lo, hi)
        s = G.Engine(model_text, device=0)
        try:
            s.set_weight_scale(g.ws)
            torch.cuda.synchronize()
            s.attach_graph_slice(g.n, lo, hi, sl.nnz, sl.rowptr.data_ptr(), sl.col.data_ptr(), sl.w.data_ptr(), sl.nw.data_ptr(),
                                 keepalive=sl)
            s.set_option("audit_period", 1)
            out = torch.full((g.n + 1, 16), 7.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            s.stage_forward_device(1, lo, hi, hin.data_ptr(), out.data_ptr(), 0)
            s.synchronize()
            assert s.get_info("audit_runs") == 1 and s.get_info("audit_failures") == 0
            want = oracle_model.predict(g, g.x(), stop_after=13)
            assert np.array_equal(bits(out[lo:hi].cpu().numpy()), bits(want[lo:hi]))
            s.set_option("audit_flip_stage", 1)
            s.set_option("audit_flip_row", hi - 1)
            with pytest.raises(G.GnnvcError) as err:
                s.stage_forward_device(1, lo, hi, hin.data_ptr(), out.data_ptr(), 0)
            assert err.value.code == ERR_AUDIT
            assert (s.get_info("audit_last_row"), s.get_info("audit_last_mismatches")) == (hi - 1, 1)
        finally:
            s.close()
    finally:
        e.close()


# ---------------------------------------------------------------- 6: the multi-device handle
def test_multi_device_handle_reports_after_the_job(model_text, oracle_model):
    g = gg.erdos_renyi(40000, 240000, 21)
    oracle_model.set_weight_scale(g.ws)
    want = oracle_model.logits(g)
    e = _engine(model_text, g, {"audit_period": 1}, devices=[0, 0])
    try:
        rows = [e.get_info(f"part_rows_{r}") for r in range(2)]
        assert sum(rows) == g.n and rows[1] > 0
        r = rows[0] + rows[1] // 2                      # a row part 1 owns
        for s in (0, 1, 2):
            e.set_option("audit_flip_stage", s)
            e.set_option("audit_flip_row", r)
            msg = _expect_audit_error(e, g.x())
            assert msg.split(": ", 1)[1].startswith("part 1:"), msg
            assert (e.get_info("audit_last_stage"), e.get_info("audit_last_row"), e.get_info("audit_last_mismatches")) == (s, r, 1)
            # the same handle, the flip off: the job's barriers were not left broken
            e.set_option("audit_flip_stage", -1)
            _, lg = e.forward(g.x())
            assert np.array_equal(bits(lg[:, 0]), bits(want)), s
        assert e.get_info("audit_failures") == 3
        assert e.get_info("audit_runs") >= 6 * 3       # (every part audits each of its stage calls)
    finally:
        e.close()


# ---------------------------------------------------------------- 7: the reference CLI with GNNVC_OPTIONS=audit_period=1
def _manifest_graph(spec):
    p = spec["graph"]
    if p["kind"] == "erdos_renyi":
        return gg.erdos_renyi(p["n"], p["m"], p["seed"])
    if p["kind"] == "hub_graph":
        return gg.hub_graph(p["n"], p["m"], p["hubs"], p["hub_degree"], seed=p["seed"])
    raise AssertionError(p["kind"])


@pytest.mark.parametrize("devices", [None, "0,0"])
def test_reference_cli_audited(golden_dir, tmp_path, devices):
    cli = golden_dir.parent.parent / "oracle" / "_ref" / "GNN_VC_hip"
    if not cli.exists():
        pytest.fail(f"{cli} is missing: it is built by __graft_entry__.build() and travels with the tree")
    spec = json.loads((golden_dir / "manifest.json").read_text())["er100k"]
    (tmp_path / "er100k.graph").write_text(gg.metis_text(_manifest_graph(spec)))
    # (audit_log: the engine itself reports every audited call; with GNNVC_TRACE the driver's per-call line carries the counters too)
    env = dict(os.environ, GNNVC_OPTIONS="audit_period=1,audit_log=1", GNNVC_TRACE="1")
    if devices:
        env["GNNVC_DEVICES"] = devices
    r = subprocess.run([str(cli), str(tmp_path / "er100k.graph"), str(tmp_path / "er100k.out"), "0", "-1", "0"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.strip().split(",")[1]) == spec["cli"]["final_cost"]
    assert hashlib.md5((tmp_path / "er100k.out").read_bytes()).hexdigest() == spec["cli"]["result_md5"]
    logged = [(int(a), int(b)) for a, b in re.findall(r"gnnvc audit: audit_runs (\d+) audit_failures (\d+)", r.stderr)]
    assert len(logged) >= 5 and logged[-1][0] > 0, r.stderr[-2000:]     # (every predict call of the run is audited)
    assert all(f == 0 for _, f in logged), r.stderr[-2000:]
    found = [(int(a), int(b)) for a, b in re.findall(r"audit_runs (\d+) audit_failures (\d+)", r.stderr)]
    assert all(f == 0 for _, f in found), r.stderr[-2000:]
