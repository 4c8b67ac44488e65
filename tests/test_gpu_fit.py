"""The loss, the read-outs and the optimizer step on the GPU (include/gnnvc.h "loss and step"), bit for bit (NaN with NaN): the
gradient against training.mse_grad, the loss total and run_model's counts against tests/fit_reference.py, the step against
training.sgd_step, host and device forms; the argument rules; training.Trainer against the same loop written with the host API;
the guard bands.  tests/test_fit_reference.py holds the reference itself to float64 and to the reference trainer's own loops."""
import ctypes as C
import gc
import itertools

import numpy as np
import pytest

from gnn_mwvc_amd import training
from gnn_mwvc_amd.engine import FitStats
from tests import backward_reference as R
from tests import fit_reference as FR
from tests import generic_harness as H
from tests.generic_harness import bits
from tests.test_fit_reference import edge_rows
from tests.test_gpu_backward import NO_LAYERS, _code, engine, same
from tests.test_gpu_guard_bands import ALIVE, CHECK, LIVE, OFF, ON, held, probe   # noqa: F401  (probe: a fixture)

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -5
F32 = np.float32


@pytest.fixture(scope="module")
def bare():
    e = engine(NO_LAYERS)   # no model layer, no graph: neither call needs one
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def dev_stats(fields=(0.0, 0, 0, 0, 0)):
    """A gnnvc_fit_stats in device memory holding `fields`."""
    raw = np.zeros(5, np.int64)
    raw[:1].view(np.float64)[0] = fields[0]
    raw[1:] = fields[1:]
    return dev(raw)


def stats_fields(s):
    if isinstance(s, FitStats):
        return s.loss_sum, s.rows, s.positives, s.positive_hits, s.negative_hits
    raw = s.cpu().numpy()
    return (float(raw[:1].view(np.float64)[0]),) + tuple(int(v) for v in raw[1:])


def same_stats(got, want, label):
    got, want = stats_fields(got), want.fields() if isinstance(want, FR.Stats) else want
    assert got[1:] == tuple(want[1:]), (label, got, want)
    a, b = np.float64(got[0]), np.float64(want[0])
    assert (np.isnan(a) and np.isnan(b)) or a.view(np.uint64) == b.view(np.uint64), (label, got, want)


# ---------------------------------------------------------------- the loss

def _mse_inputs(rows, width):
    x, y = H.crafted_input(rows, width, 300 + rows + width), H.crafted_input(rows, width, 900 + rows + width)
    if rows >= 64:   # scores equal to targets: d = +0.0f, a gradient of +0.0f
        x[32:48] = y[32:48]
    sx, sy = edge_rows(x, y)   # column 0: 0.5f, just above, just below, signed zeros, inf, NaN
    if rows >= 64 and width > 1:   # ... and specials off column 0, which the counts must not see
        sx[48:52, 1], sy[48:52, 1] = np.array([np.inf, np.nan, -0.0, 0.5], F32), np.array([np.inf, 1.0, 0.0, 0.5], F32)
    return (x, y), (sx, sy)


@pytest.mark.parametrize("width", [1, 3, 16])
@pytest.mark.parametrize("rows", [1, 255, 4096, 4097, 8209])
def test_mse(bare, rows, width):
    import torch
    for kind, (x, y) in zip(("crafted", "special"), _mse_inputs(rows, width)):
        label = (rows, width, kind)
        with np.errstate(all="ignore"):
            want_grad = training.mse_grad(x, y)
        once, twice = FR.Stats().add(x, y), FR.Stats().add(x, y).add(x, y)
        if kind == "crafted":
            assert np.isfinite(once.loss_sum) and once.loss_sum > 0.0   # a total whose bits depend on the order of its terms
        # the host form: both outputs, then the stats accumulate over a second call; each output alone
        s = FitStats()
        same(bare.mse(x, y, stats=s), want_grad, (label, "host grad"))
        same_stats(s, once, (label, "host stats"))
        assert bare.mse(x, y, want_grad=False, stats=s) is None
        same_stats(s, twice, (label, "host stats, second call"))
        same(bare.mse(x, y), want_grad, (label, "host grad alone"))
        # the device form
        dx, dy = dev(x), dev(y)
        dg, ds = torch.full(x.shape, float("nan"), device=dx.device), dev_stats()
        torch.cuda.synchronize()
        bare.mse_device(rows, width, dx.data_ptr(), dy.data_ptr(), dg.data_ptr(), ds.data_ptr())
        bare.mse_device(rows, width, dx.data_ptr(), dy.data_ptr(), 0, ds.data_ptr())
        bare.synchronize()
        same(dg.cpu().numpy(), want_grad, (label, "device grad"))
        same_stats(ds, twice, (label, "device stats over two calls"))
        dg.fill_(float("nan"))
        torch.cuda.synchronize()
        bare.mse_device(rows, width, dx.data_ptr(), dy.data_ptr(), dg.data_ptr(), 0)
        bare.synchronize()
        same(dg.cpu().numpy(), want_grad, (label, "device grad alone"))
        same_stats(ds, twice, (label, "stats untouched by a call without them"))
        same(dx.cpu().numpy(), x, (label, "scores untouched"))
        same(dy.cpu().numpy(), y, (label, "target untouched"))


def test_mse_gradient_in_place(bare):
    """d_grad may be d_scores itself: the stats are those of the scores as they were."""
    import torch
    rows, width = 4097, 3
    x, y = _mse_inputs(rows, width)[1]
    with np.errstate(all="ignore"):
        want = training.mse_grad(x, y)
    dx, dy, ds = dev(x), dev(y), dev_stats()
    torch.cuda.synchronize()
    bare.mse_device(rows, width, dx.data_ptr(), dy.data_ptr(), dx.data_ptr(), ds.data_ptr())
    bare.synchronize()
    same(dx.cpu().numpy(), want, "gradient written over the scores")
    same_stats(ds, FR.Stats().add(x, y), "stats of a call in place")


def test_mse_adds_to_what_the_stats_hold(bare):
    import torch
    x, y = _mse_inputs(255, 3)[0]
    start = (1234.5, 7, 3, 2, 1)
    t = float(FR.loss_total(x, y))
    p, ph, nh = FR.counts(x, y)
    want = (1234.5 + t, 7 + 255, 3 + p, 2 + ph, 1 + nh)
    s = FitStats(*start)
    bare.mse(x, y, want_grad=False, stats=s)
    same_stats(s, want, "host")
    dx, dy, ds = dev(x), dev(y), dev_stats(start)
    torch.cuda.synchronize()
    bare.mse_device(255, 3, dx.data_ptr(), dy.data_ptr(), 0, ds.data_ptr())
    bare.synchronize()
    same_stats(ds, want, "device")


# ---------------------------------------------------------------- the step

def _sgd_inputs(count):
    w = H.crafted_input(1, count, 11 + count).reshape(-1) * F32(2.0 ** -18)
    vel = H.crafted_input(1, count, 12 + count).reshape(-1) * F32(2.0 ** -20)
    grad = H.crafted_input(1, count, 13 + count).reshape(-1)
    if count >= 63:
        sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-38, 3.4e38, -3.4e38, 1.0, -1.0], F32)
        grad[:12], w[12:24], vel[24:36] = sp, sp, sp
        grad[36:48], w[36:48] = sp, sp[::-1]
    return w, vel, grad


@pytest.mark.parametrize("count", [1, 63, 6209, 100003])
def test_sgd_step(bare, count):
    import torch
    w0, v0, g0 = _sgd_inputs(count)
    lr = 0.05
    for batch, momentum, wd, zero in itertools.product([1, 1933, 500001], [0.0, 0.9], [0.0, 1e-4], [False, True]):
        label = (count, batch, momentum, wd, zero)
        with np.errstate(all="ignore"):
            want_w, want_v = training.sgd_step(w0, v0, g0, batch=batch, lr=lr, momentum=momentum, weight_decay=wd)
        want_g = np.zeros_like(g0) if zero else g0   # +0.0f, or the bits as they were: the decayed gradient is not stored back
        w, v, g = w0.copy(), v0.copy(), g0.copy()
        bare.sgd_step(w, v, g, batch, lr, momentum, wd, zero_grad=zero)
        same(w, want_w, (label, "host params"))
        same(v, want_v, (label, "host velocity"))
        same(g, want_g, (label, "host grad"))
        dw, dv, dg = dev(w0), dev(v0), dev(g0)
        torch.cuda.synchronize()
        bare.sgd_step_device(count, dw.data_ptr(), dv.data_ptr(), dg.data_ptr(), batch, lr, momentum, wd, zero_grad=zero)
        bare.synchronize()
        same(dw.cpu().numpy(), want_w, (label, "device params"))
        same(dv.cpu().numpy(), want_v, (label, "device velocity"))
        same(dg.cpu().numpy(), want_g, (label, "device grad"))
        if zero:
            assert not bits(g).any() and not bits(dg.cpu().numpy()).any(), (label, "+0.0f, not -0.0f")


# ---------------------------------------------------------------- argument and state rules

def test_argument_rules(bare):
    import torch
    import gnn_mwvc_amd as G
    L, h = G.load_library(), bare._h
    x, y = _mse_inputs(255, 3)[0]
    g, s = np.full_like(x, np.nan), FitStats(2.5, 1, 1, 1, 0)
    px, py, pg = (a.ctypes.data_as(C.c_void_p) for a in (x, y, g))
    dx, dy, dg, ds = dev(x), dev(y), dev(g), dev_stats((2.5, 1, 1, 1, 0))
    torch.cuda.synchronize()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    # gnnvc_mse, gnnvc_mse_device
    assert L.gnnvc_mse(h, 255, 0, px, py, pg, C.byref(s)) == ERR_INVALID                       # width == 0
    assert L.gnnvc_mse_device(h, 255, 0, ptr(dx), ptr(dy), ptr(dg), ptr(ds)) == ERR_INVALID
    assert L.gnnvc_mse(h, 255, 3, px, py, None, None) == ERR_INVALID                           # neither output
    assert L.gnnvc_mse_device(h, 255, 3, ptr(dx), ptr(dy), None, None) == ERR_INVALID
    assert L.gnnvc_mse(h, 0, 3, px, py, None, None) == ERR_INVALID                             # ... also without rows
    for a, b in ((None, py), (px, None)):                                                      # a null required buffer
        assert L.gnnvc_mse(h, 255, 3, a, b, pg, C.byref(s)) == ERR_INVALID
    for a, b in ((None, ptr(dy)), (ptr(dx), None)):
        assert L.gnnvc_mse_device(h, 255, 3, a, b, ptr(dg), ptr(ds)) == ERR_INVALID
    assert L.gnnvc_mse(h, 0, 3, None, None, pg, C.byref(s)) == 0                               # rows == 0: nothing is written
    assert L.gnnvc_mse_device(h, 0, 3, None, None, ptr(dg), ptr(ds)) == 0
    assert bare.mse(np.zeros((0, 3), F32), np.zeros((0, 3), F32), stats=s).shape == (0, 3)
    bare.synchronize()
    same_stats(s, (2.5, 1, 1, 1, 0), "host stats after the refused and the empty calls")
    same_stats(ds, (2.5, 1, 1, 1, 0), "device stats after the refused and the empty calls")
    assert np.isnan(g).all() and np.isnan(dg.cpu().numpy()).all()
    # gnnvc_sgd_step, gnnvc_sgd_step_device
    w, v, gr = _sgd_inputs(63)
    keep = [a.copy() for a in (w, v, gr)]
    pw, pv, pgr = (a.ctypes.data_as(C.c_void_p) for a in (w, v, gr))
    dw, dv, dgr = dev(w), dev(v), dev(gr)
    torch.cuda.synchronize()
    f = C.c_float
    assert L.gnnvc_sgd_step(h, 63, pw, pv, pgr, 0, f(0.1), f(0.9), f(0.0), 1) == ERR_INVALID   # batch == 0
    assert L.gnnvc_sgd_step_device(h, 63, ptr(dw), ptr(dv), ptr(dgr), 0, f(0.1), f(0.9), f(0.0), 1) == ERR_INVALID
    for args in ((None, pv, pgr), (pw, None, pgr), (pw, pv, None)):
        assert L.gnnvc_sgd_step(h, 63, *args, 5, f(0.1), f(0.9), f(0.0), 1) == ERR_INVALID
    for args in ((None, ptr(dv), ptr(dgr)), (ptr(dw), None, ptr(dgr)), (ptr(dw), ptr(dv), None)):
        assert L.gnnvc_sgd_step_device(h, 63, *args, 5, f(0.1), f(0.9), f(0.0), 1) == ERR_INVALID
    assert L.gnnvc_sgd_step(h, 0, None, None, None, 5, f(0.1), f(0.9), f(0.0), 1) == 0         # count == 0
    assert L.gnnvc_sgd_step_device(h, 0, None, None, None, 5, f(0.1), f(0.9), f(0.0), 1) == 0
    bare.synchronize()
    for got, dgot, want in zip((w, v, gr), (dw, dv, dgr), keep):
        same(got, want, "host arrays after the refused and the empty calls")
        same(dgot.cpu().numpy(), want, "device arrays after the refused and the empty calls")


def test_multi_device_handle_is_refused(model_text):
    import torch
    import gnn_mwvc_amd as G
    x, y = _mse_inputs(255, 1)[0]
    w, v, g = _sgd_inputs(63)
    dx, dy, dg, ds = dev(x), dev(y), dev(np.zeros_like(x)), dev_stats()
    dw, dv, dgr = dev(w), dev(v), dev(g)
    torch.cuda.synchronize()
    m = G.Engine(model_text, devices=[0, 0])
    try:
        assert _code(lambda: m.mse(x, y, stats=FitStats())) == ERR_UNSUPPORTED
        assert _code(lambda: m.mse_device(255, 1, dx.data_ptr(), dy.data_ptr(), dg.data_ptr(), ds.data_ptr())) == ERR_UNSUPPORTED
        assert _code(lambda: m.sgd_step(w.copy(), v.copy(), g.copy(), 5, 0.1, 0.9)) == ERR_UNSUPPORTED
        assert _code(lambda: m.sgd_step_device(63, dw.data_ptr(), dv.data_ptr(), dgr.data_ptr(), 5, 0.1, 0.9)) == ERR_UNSUPPORTED
    finally:
        m.close()
    same_stats(ds, (0.0, 0, 0, 0, 0), "nothing was added")
    same(dw.cpu().numpy(), w, "nothing was stepped")


# ---------------------------------------------------------------- the trainer

TRAINER_GRAPHS = ["hub8k", "er1933", "er4097"]
HYPER = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)


def _pairs():
    out = []
    for i, name in enumerate(TRAINER_GRAPHS):
        g = R.graph_of(name)
        out.append((g, np.random.default_rng(70 + i).uniform(0.0, 1.0, (g.n, 1)).astype(F32)))
    return out


def _host_pass(e, pairs, state, fit, batch_vertices):
    """run_model's loop with the host API: train_forward, training.mse_grad, backward accumulating into `acc`, training.sgd_step.
    state = [params, velocity, accumulator]; returns the pass's Stats, the number of steps taken and the last scores."""
    stats, t, steps, scores = FR.Stats(), 0, [], None

    def step(batch):
        with np.errstate(all="ignore"):
            state[0], state[1] = training.sgd_step(state[0], state[1], state[2], batch=batch, **HYPER)
        state[2][:] = F32(0.0)
        steps.append(batch)
    for g, target in pairs:
        e.set_weight_scale(g.ws)
        e.upload_graph(g)
        scores = e.train_forward(g.x(), state[0])
        stats.add(scores, target)
        if fit:
            assert e.backward(training.mse_grad(scores, target), accumulate_into=state[2]) is state[2]
            t += g.n
            if t > batch_vertices:
                step(t)
                t = 0
    if t > 0:
        step(t)
    return stats, steps, scores


def test_trainer_is_the_host_loop(model_text):
    import gnn_mwvc_amd as G
    pairs = _pairs()
    n = [g.n for g, _ in pairs]
    batch_vertices = n[0] + n[1] - 1   # a step behind the second graph, a trailing one behind the third
    assert n[0] <= batch_vertices and 0 < n[2] <= batch_vertices
    e = engine(model_text)
    try:
        own = e.params()
        state = [own.copy(), np.zeros(own.size, F32), np.zeros(own.size, F32)]
        tr = training.Trainer(e, model_text, batch_vertices=batch_vertices, **HYPER)
        for epoch in range(2):
            got = tr.run(pairs, fit=True)
            stats, steps, _ = _host_pass(e, pairs, state, True, batch_vertices)
            assert steps == [n[0] + n[1], n[2]], steps
            print(f"epoch {epoch}: loss {got[0]:.6f}, total accuracy {got[1]:.4f}, true accuracy {got[2]:.4f}")
            same_stats(tr.stats, stats, ("stats of epoch", epoch))
            assert got == stats.metrics(), (epoch, got, stats.metrics())
            same(tr.params(), state[0], ("params after epoch", epoch))
            same(tr.velocity(), state[1], ("velocity after epoch", epoch))
        assert (bits(state[0]) != bits(own)).any(), "the steps changed the parameters"
        # an evaluation pass: no step, and the last training forward ran with the final parameters
        got = tr.run(pairs, fit=False)
        stats, steps, last = _host_pass(e, pairs, state, False, batch_vertices)
        assert steps == [] and got == stats.metrics()
        same_stats(tr.stats, stats, "stats of the evaluation")
        same(tr.params(), state[0], "an evaluation leaves the parameters")
        same(tr.scores(), last, "the trainer's last training forward")
        g = pairs[-1][0]
        same(e.params(), own, "the engine's own parameters are untouched")
        same(e.forward(g.x())[0], e.train_forward(g.x()), "the engine still scores with its own parameters")
        text = tr.text()
        tr.close()
        assert e.forward(g.x())[0].shape == (g.n, 1)   # on the engine's own stream again
    finally:
        e.close()
    fresh = G.Engine(text, device=0)
    try:
        fresh.set_weight_scale(g.ws)
        fresh.upload_graph(g)
        same(fresh.forward(g.x())[0], last, "a fresh inference engine on the trainer's text")
        same(fresh.params(), state[0], "the text carries the parameters bit for bit")
    finally:
        fresh.close()


# ---------------------------------------------------------------- guard bands

def test_no_band_is_damaged(model_text, probe):   # noqa: F811
    gc.collect()
    start = probe(LIVE)
    assert probe(ON) == 0
    try:
        assert probe(CHECK) == 0
        g = R.graph_of("er4097")
        e = engine(model_text, g)
        try:
            x, y = _mse_inputs(8209, 3)[0]
            s = FitStats()
            with np.errstate(all="ignore"):
                same(e.mse(x, y, stats=s), training.mse_grad(x, y), "guarded mse")
            same_stats(s, FR.Stats().add(x, y), "guarded mse stats")
            w, v, gr = _sgd_inputs(6209)
            with np.errstate(all="ignore"):
                want_w, want_v = training.sgd_step(w, v, gr, batch=1933, **HYPER)
            e.sgd_step(w, v, gr, 1933, zero_grad=True, **HYPER)
            same(w, want_w, "guarded step: params")
            same(v, want_v, "guarded step: velocity")
            held(probe, "mse and sgd_step")
            target = np.random.default_rng(3).uniform(0.0, 1.0, (g.n, 1)).astype(F32)
            tr = training.Trainer(e, model_text, batch_vertices=1000, **HYPER)
            tr.run([(g, target)], fit=True)
            state = [e.params(), np.zeros(e.num_params(), F32), np.zeros(e.num_params(), F32)]
            _host_pass(e, [(g, target)], state, True, 1000)
            same(tr.params(), state[0], "guarded trainer graph")
            held(probe, "a trainer graph")
            tr.close()
        finally:
            e.close()
        assert probe(CHECK) == 0, "bands found damaged when their buffers were freed: see the stderr lines"
        assert probe(ALIVE) == 0
        assert probe(LIVE) == start, "close() left objects alive"
    finally:
        assert probe(OFF) == 0
