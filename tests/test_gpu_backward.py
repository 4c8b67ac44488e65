"""The backward pass on the GPU, bit for bit against tests/backward_reference.py (NaN with NaN): the layer-level entry points, the
model level (train_forward + backward, grad_x included) over the case table of that module, the state rules, the guard bands and a
short training loop.  tests/test_backward_reference.py holds the reference itself to float64 autograd on the CPU.

A model that ends in a sigmoid is compared with the reference run on the restated device sigmoid (tests/support/libexpf_shim.so,
which tests/generic_harness.check_scores holds the engine's scores to bit for bit): the sigmoid's backward reads its output."""
import gc

import numpy as np
import pytest

from gnn_mwvc_amd import training
from tests import backward_reference as R
from tests import generic_harness as H
from tests.generic_harness import bits
from tests.test_expf_restatement import _run, shim   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)
from tests.test_gpu_guard_bands import ALIVE, CHECK, LIVE, OFF, ON, held, probe   # noqa: F401  (probe: a fixture)
from tools import graphgen as gg

pytestmark = pytest.mark.gpu

NO_LAYERS = "layer_level 0 Layers\n"   # an engine for the layer-level entry points
ERR_STATE, ERR_UNSUPPORTED = -4, -5


def same(got, want, label):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (label, f"{int(bad.sum())} of {bad.size} values differ, first at", np.argwhere(bad)[:4].tolist(),
                           got[bad][:4].tolist(), want[bad][:4].tolist())


def engine(text, g=None):
    import gnn_mwvc_amd as G
    e = G.Engine(text, device=0)
    if g is not None:
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
    return e


@pytest.fixture(scope="module")
def bare():
    e = engine(NO_LAYERS)
    yield e
    e.close()


# ---------------------------------------------------------------- layer level

def _linear_inputs(n, k, m):
    h = H.crafted_input(n, k, 1000 + n + k)
    W = H.crafted_input(k, m, 2000 + k + m)
    go = H.crafted_input(n, m, 3000 + n + m)
    old = (H.crafted_input(k, m, 4000 + k), H.crafted_input(1, m, 5000 + m).reshape(m))
    return h, W, go, old


@pytest.mark.parametrize("n,k,m", R.LINEAR_SHAPES)
def test_linear_backward(bare, n, k, m):
    h, W, go, old = _linear_inputs(n, k, m)
    want = R.linear_backward(h, W, go)
    got = bare.linear_backward(h, W, go)
    for name, a, b in zip(("grad_in", "grad_W", "grad_bias"), got, want):
        same(a, b, (n, k, m, name))
    if n <= R.GRAD_BLOCK_ROWS:   # one block: the product itself
        same(got[1], bare.sgemm(h, go, trans_a=True), (n, k, m, "grad_W against sgemm"))
        same(got[2].reshape(1, m), bare.sgemm(np.ones((n, 1), np.float32), go, trans_a=True), (n, k, m, "grad_bias against sgemm"))
    same(got[0], bare.sgemm(go, W, trans_b=True), (n, k, m, "grad_in against sgemm"))
    # accumulate into crafted old values: one more rounded add
    want_acc = R.linear_backward(h, W, go, old)
    got_acc = bare.linear_backward(h, W, go, accumulate_into=old)
    for name, a, b in zip(("grad_in", "grad_W", "grad_bias"), got_acc, want_acc):
        same(a, b, (n, k, m, name, "accumulate"))
    if n <= R.GRAD_BLOCK_ROWS:
        same(got_acc[1], bare.sgemm(h, go, C_in=old[0], beta=1.0, trans_a=True), (n, k, m, "grad_W against sgemm, beta 1"))
    # each output alone
    same(bare.linear_backward(h, W, go, want=("in",))[0], want[0], (n, k, m, "grad_in alone"))
    same(bare.linear_backward(h, W, go, want=("W",))[1], want[1], (n, k, m, "grad_W alone"))
    same(bare.linear_backward(h, W, go, want=("bias",), accumulate_into=old)[2], want_acc[2], (n, k, m, "grad_bias alone, accumulate"))


def test_linear_backward_without_rows(bare):
    old = (np.full((5, 3), 7.0, np.float32), np.full(3, -2.0, np.float32))
    gi, gw, gb = bare.linear_backward(np.zeros((0, 5), np.float32), np.ones((5, 3), np.float32), np.zeros((0, 3), np.float32))
    assert gi.shape == (0, 5) and not bits(gw).any() and not bits(gb).any()
    _, gw, gb = bare.linear_backward(np.zeros((0, 5), np.float32), np.ones((5, 3), np.float32), np.zeros((0, 3), np.float32),
                                     accumulate_into=old)
    same(gw, old[0], "untouched")
    same(gb, old[1], "untouched")


def test_relu_backward(bare):
    z = np.array([-1.0, -0.0, 0.0, np.nan, np.inf, 1e-45, -1e-45, -np.inf, 3.5, -2.5e-38], dtype=np.float32)
    z = np.concatenate([z, H.crafted_input(1, 1000, 7).reshape(-1)])
    go = H.crafted_input(1, z.size, 8).reshape(-1)
    go[:10] = np.array([2.0, 3.0, -4.0, 5.0, np.nan, -0.0, 7.0, 8.0, np.inf, 9.0], dtype=np.float32)
    got = bare.relu_backward(z, go)
    same(got, R.relu_backward(z, go), "relu")
    assert got[:4].tolist() == [0.0, 3.0, -4.0, 0.0] and np.isnan(got[4]) and bits(got[5:6])[0] == 0x80000000


def test_sigmoid_backward(bare):
    rng = np.random.default_rng(9)
    s = np.concatenate([np.array([0.0, 1.0, 0.5, 1e-45, np.float32(1.0) - np.float32(2.0 ** -24), 2.0 ** -24, 0.25, 0.75], dtype=np.float32),
                        rng.uniform(0.0, 1.0, 2000).astype(np.float32)])
    go = H.crafted_input(1, s.size, 10).reshape(-1)
    same(bare.sigmoid_backward(s, go), R.sigmoid_backward(s, go), "sigmoid")


@pytest.mark.parametrize("f", R.GRAPH_LAYER_F)
def test_graph_layer_backward(f):
    e = engine(NO_LAYERS)
    try:
        for gname in R.GRAPH_LAYER_GRAPHS:
            g = R.graph_of(gname)
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            assert e.get_info("graph_symmetric") == -1
            go = H.crafted_input(g.n, 2 * f + 3, 100 * f + len(gname))
            same(e.graph_layer_backward(go), R.graph_layer_backward(g, go), (f, gname))
            assert e.get_info("graph_symmetric") == 1
    finally:
        e.close()


def _shuffled_rows(g, seed):
    """g with every row's entries in another order: still symmetric, no row ascends."""
    rng = np.random.default_rng(seed)
    col = g.col.copy()
    rp = g.rowptr.astype(np.int64)
    for v in range(g.n):
        rng.shuffle(col[rp[v]: rp[v + 1]])
    return gg.CsrGraph(g.n, g.rowptr, col, g.w, g.nw)


def test_symmetry_check_on_rows_in_any_order():
    g = _shuffled_rows(R.graph_of("er1933"), 3)
    e = engine(NO_LAYERS, g)
    try:
        go = H.crafted_input(g.n, 2 * 5 + 3, 77)
        same(e.graph_layer_backward(go), R.graph_layer_backward(g, go), "rows in any order")
        assert e.get_info("graph_symmetric") == 1
        # a doubled entry on one side only: (0, 1) twice, (1, 0) once — symmetric as a set, not with multiplicities; in
        # ascending rows (two searches), then with a row that descends (a scan)
        for n, rowptr, col in ((2, [0, 2, 3], [1, 1, 0]), (3, [0, 3, 4, 5], [2, 1, 1, 0, 0])):
            bad = gg.CsrGraph(n, np.array(rowptr, np.uint64), np.array(col, np.uint32), np.full(n, 5, np.uint32), np.full(n, 5, np.uint32))
            e.upload_graph(bad)
            with pytest.raises(Exception) as ei:
                e.graph_layer_backward(np.ones((n, 5), np.float32))
            assert ei.value.code == ERR_UNSUPPORTED and e.get_info("graph_symmetric") == 0, col
    finally:
        e.close()


def test_long_rows_that_do_not_ascend_are_refused_not_scanned():
    """An entry of a row that does not ascend scans its row: d * d loads for d entries.  Past 65 536 entries the engine refuses
    the graph before it launches the scans, and leaves "graph_symmetric" open; the same star with its hub row ascending is checked
    (two searches an entry) and summed as one chain of 70 001 terms."""
    n = 70002
    rowptr = np.concatenate([[0], n - 1 + np.arange(n, dtype=np.uint64)]).astype(np.uint64)
    w = np.full(n, 50, np.uint32)
    up = np.concatenate([np.arange(1, n), np.zeros(n - 1)]).astype(np.uint32)
    down = np.concatenate([np.arange(n - 1, 0, -1), np.zeros(n - 1)]).astype(np.uint32)
    go = H.crafted_input(n, 5, 91)
    e = engine(NO_LAYERS)
    try:
        e.upload_graph(gg.CsrGraph(n, rowptr, down, w, w))
        with pytest.raises(Exception) as ei:
            e.graph_layer_backward(go)
        assert ei.value.code == ERR_UNSUPPORTED and e.get_info("graph_symmetric") == -1
        g = gg.CsrGraph(n, rowptr, up, w, w)
        e.upload_graph(g)
        same(e.graph_layer_backward(go), R.graph_layer_backward(g, go), "a star of 70 001 rays")
        assert e.get_info("graph_symmetric") == 1
    finally:
        e.close()


# ---------------------------------------------------------------- model level

def _restated(shim_lib):
    return lambda z: _run(shim_lib.sigmoid_restated, np.ascontiguousarray(z, dtype=np.float32))


def _run_case(e, c, label):
    g = c["g"]
    scores = e.train_forward(c["x"], c["params"])
    gp, gx = e.backward(c["grad_scores"], want_grad_x=True)
    if g.n:
        same(scores, c["scores"], (label, "scores"))
    same(gx, c["grad_x"], (label, "grad_x"))
    layout, _ = training.param_layout(c["text"])
    for (k, m, w_off, b_off), (i, gw, gb) in zip(layout, c["layers"]):
        same(gp[w_off: w_off + k * m].reshape(k, m), gw, (label, "grad_W of layer", i))
        same(gp[b_off: b_off + m], gb, (label, "grad_bias of layer", i))
    same(gp, c["grad_params"], (label, "grad_params"))
    return scores, gp, gx


@pytest.mark.parametrize("model", list(R.MODELS))
def test_model_backward(model, shim):   # noqa: F811
    sig = _restated(shim)
    e = engine(R.text_of(model))
    try:
        assert e.num_params() == training.param_layout(R.text_of(model))[1]
        for gname in R.MODEL_GRAPHS:
            g = R.graph_of(gname)
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            for variant in ("own", "perturbed"):
                c = R.case(model, gname, variant, sigmoid=sig)
                scores, gp, gx = _run_case(e, c, (model, gname, variant))
                if variant == "own":
                    same(scores, e.forward(c["x"])[0], (model, gname, "train_forward against forward"))
                    same(e.params(), R.flat_params(R.oracle_py.OracleModel(c["text"])), (model, "params"))
                # a second run, with an ordinary forward between the training forward and the backward: the same bits
                again = e.train_forward(c["x"], c["params"])
                e.forward(c["x"])
                gp2, gx2 = e.backward(c["grad_scores"], want_grad_x=True)
                same(again, scores, (model, gname, variant, "second run: scores"))
                same(gp2, gp, (model, gname, variant, "second run: grad_params"))
                same(gx2, gx, (model, gname, variant, "second run: grad_x"))
            if model in ("trained", "odd") and gname in ("er4097", "empty"):
                # accumulate: old + total, one rounded add; without grad_x the same parameter gradient
                c = R.case(model, gname, "perturbed", sigmoid=sig)
                old = H.crafted_input(1, e.num_params(), 21).reshape(-1) * np.float32(2.0 ** -10)
                want = R.backward(c["text"], g, c["x"], c["grad_scores"], c["params"], old=old, sigmoid=sig)["grad_params"]
                acc = old.copy()
                assert e.backward(c["grad_scores"], accumulate_into=acc) is acc
                same(acc, want, (model, gname, "accumulate"))
                same(e.backward(c["grad_scores"]), c["grad_params"], (model, gname, "without grad_x"))
        assert e.get_info("backward_workspace_bytes") > 0
    finally:
        e.close()


def test_device_forms(shim):   # noqa: F811
    import torch
    c = R.case("odd", "er4097", "perturbed", sigmoid=_restated(shim))
    g = c["g"]
    e = engine(c["text"], g)
    try:
        dev = torch.device("cuda:0")
        x, p, gs = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (c["x"], c["params"], c["grad_scores"]))
        sc = torch.full(c["scores"].shape, float("nan"), device=dev)
        gp = torch.full((e.num_params(),), float("nan"), device=dev)
        gx = torch.full(c["x"].shape, float("nan"), device=dev)
        torch.cuda.synchronize()
        e.train_forward_device(x.data_ptr(), sc.data_ptr(), p.data_ptr())
        e.backward_device(gs.data_ptr(), gp.data_ptr(), gx.data_ptr())
        e.synchronize()
        same(sc.cpu().numpy(), c["scores"], "device scores")
        same(gp.cpu().numpy(), c["grad_params"], "device grad_params")
        same(gx.cpu().numpy(), c["grad_x"], "device grad_x")
        e.backward_device(gs.data_ptr(), gp.data_ptr(), 0, accumulate=True)
        e.synchronize()
        with np.errstate(all="ignore"):
            same(gp.cpu().numpy(), (c["grad_params"] + c["grad_params"]).astype(np.float32), "device accumulate")
    finally:
        e.close()


# ---------------------------------------------------------------- state

def _code(fn):
    import gnn_mwvc_amd as G
    with pytest.raises(G.GnnvcError) as ei:
        fn()
    return ei.value.code


def test_state_rules(model_text):
    import gnn_mwvc_amd as G
    g, g2 = R.graph_of("er1933"), R.graph_of("sparse")
    gs = R.grad_scores_of(g.n, 1, 1)
    e = G.Engine(model_text, device=0)
    try:
        assert _code(lambda: e.backward(gs[:0])) == ERR_STATE                 # no graph at all
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
        assert _code(lambda: e.backward(gs)) == ERR_STATE                     # no training forward yet
        assert e.get_info("backward_workspace_bytes") == 0
        e.train_forward(g.x())
        first = e.backward(gs)
        same(e.backward(gs), first, "a second backward over the same forward")
        for route in H.ROUTES:                                                # every hand-off discards the saved forward
            e.train_forward(g.x())
            H.hand_over(e, g2, route)
            assert _code(lambda: e.backward(R.grad_scores_of(g2.n, 1, 2))) == ERR_STATE, route
            e.train_forward(g2.x())
            e.backward(R.grad_scores_of(g2.n, 1, 2))
            H.hand_over(e, g, "upload")
            assert _code(lambda: e.backward(gs)) == ERR_STATE, route
        e.train_forward(g.x())
        same(e.backward(gs), first, "after the hand-offs")
    finally:
        e.close()


def test_directed_graph_is_refused(model_text):
    g = gg.CsrGraph(3, np.array([0, 1, 2, 2], np.uint64), np.array([1, 2], np.uint32), np.array([30, 40, 50], np.uint32),
                    np.array([40, 50, 0], np.uint32))
    e = engine(model_text, g)
    try:
        assert e.get_info("graph_symmetric") == -1
        e.train_forward(g.x())
        assert _code(lambda: e.backward(np.ones((3, 1), np.float32))) == ERR_UNSUPPORTED
        assert e.get_info("graph_symmetric") == 0
        assert _code(lambda: e.graph_layer_backward(np.ones((3, 5), np.float32))) == ERR_UNSUPPORTED
        e.forward(g.x())   # inference is not the backward's business
    finally:
        e.close()


def test_multi_device_and_sliced_engines_are_refused(model_text):
    import torch
    import gnn_mwvc_amd as G
    g = R.graph_of("er1933")
    m = G.Engine(model_text, devices=[0, 0])
    try:
        m.set_weight_scale(g.ws)
        m.upload_graph(g)
        assert m.num_params() == 6209 and m.params().size == 6209
        assert _code(lambda: m.train_forward(g.x())) == ERR_UNSUPPORTED
        assert _code(lambda: m.backward(np.ones((g.n, 1), np.float32))) == ERR_UNSUPPORTED
        assert _code(lambda: m.graph_layer_backward(np.ones((g.n, 5), np.float32))) == ERR_UNSUPPORTED
    finally:
        m.close()
    from gnn_mwvc_amd.engine import COL_PAD
    lo, hi = 64, 1024
    rp = g.rowptr.astype(np.int64)
    col = np.zeros(int(rp[hi] - rp[lo]) + COL_PAD, np.int64)
    col[: rp[hi] - rp[lo]] = g.col[rp[lo]: rp[hi]]
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(a.astype(np.int64)).to(torch.int32).to(dev) for a in (rp[lo: hi + 1] - rp[lo], col, g.w[lo:hi], g.nw[lo:hi])]
    torch.cuda.synchronize()
    e = G.Engine(model_text, device=0)
    try:
        e.set_weight_scale(g.ws)
        e.attach_graph_slice(g.n, lo, hi, int(rp[hi] - rp[lo]), *[x.data_ptr() for x in t], keepalive=t)
        assert _code(lambda: e.train_forward(g.x())) == ERR_UNSUPPORTED
        assert _code(lambda: e.backward(np.ones((g.n, 1), np.float32))) == ERR_UNSUPPORTED
        assert _code(lambda: e.graph_layer_backward(np.ones((g.n, 5), np.float32))) == ERR_UNSUPPORTED
    finally:
        e.close()


# ---------------------------------------------------------------- guard bands

@pytest.mark.parametrize("model", ["trained", "odd"])
def test_no_band_is_damaged(model, probe, shim):   # noqa: F811
    gc.collect()
    start = probe(LIVE)
    assert probe(ON) == 0
    try:
        assert probe(CHECK) == 0
        sig = _restated(shim)
        e = engine(R.text_of(model), R.graph_of("hub8k"))
        try:
            for variant in ("own", "perturbed"):
                _run_case(e, R.case(model, "hub8k", variant, sigmoid=sig), (model, "hub8k", variant, "guarded"))
            held(probe, (model, "hub8k"))
            # a smaller graph, then the large one again: buffers that stay large, and an exact fit of none
            for gname in ("er1933", "hub8k"):
                g = R.graph_of(gname)
                e.set_weight_scale(g.ws)
                e.upload_graph(g)
                _run_case(e, R.case(model, gname, "own", sigmoid=sig), (model, gname, "guarded"))
                held(probe, (model, gname))
        finally:
            e.close()
        assert probe(CHECK) == 0, "bands found damaged when their buffers were freed: see the stderr lines"
        assert probe(ALIVE) == 0
        assert probe(LIVE) == start, "close() left objects alive"
    finally:
        assert probe(OFF) == 0


# ---------------------------------------------------------------- a loop

def test_training_loop_lowers_the_loss(model_text):
    import gnn_mwvc_amd as G
    g = R.graph_of("er1933")
    x = g.x()
    target = np.random.default_rng(5).uniform(0.0, 1.0, (g.n, 1)).astype(np.float32)
    e = engine(model_text, g)
    try:
        p, vel = e.params(), np.zeros(e.num_params(), np.float32)
        losses = []
        for _ in range(20):
            scores = e.train_forward(x, p)
            losses.append(training.mse_loss(scores, target))
            grad = e.backward(training.mse_grad(scores, target))
            p, vel = training.sgd_step(p, vel, grad, batch=g.n, lr=0.05, momentum=0.5, weight_decay=0.0)
        last = e.train_forward(x, p)
        losses.append(training.mse_loss(last, target))
        print("MSE per step:", " ".join(f"{v:.6f}" for v in losses))
        assert all(b < a for a, b in zip(losses, losses[1:])), losses
        same(e.forward(x)[0], e.train_forward(x), "the engine's own parameters are untouched")
    finally:
        e.close()
    fresh = G.Engine(training.text_with_params(model_text, p), device=0)
    try:
        fresh.set_weight_scale(g.ws)
        fresh.upload_graph(g)
        same(fresh.forward(x)[0], last, "a fresh inference engine on the trained text")
        same(fresh.params(), p, "the text carries the parameters bit for bit")
    finally:
        fresh.close()
