"""gnn_mwvc_amd.training on the CPU: the parameter layout, a model text that the oracle's parser reads back bit for bit, and the SGD
step against a scalar restatement of the old trainer's formulas (reference old_files/src/lib/gnn_training.cpp, SGD_step, MSE_grad)."""
import numpy as np

from gnn_mwvc_amd import training
from oracle import oracle_py
from tests import backward_reference as R


def test_param_layout_of_the_trained_text(model_text):
    layout, total = training.param_layout(model_text)
    assert total == 6209
    assert [(k, m) for k, m, _, _ in layout] == [(5, 32), (32, 32), (32, 16), (35, 32), (32, 32), (32, 16), (35, 32), (32, 16), (16, 1)]
    off = 0
    for k, m, w_off, b_off in layout:
        assert (w_off, b_off) == (off, off + k * m)
        off += k * m + m
    assert R.flat_params(oracle_py.OracleModel(model_text)).size == total


def _crafted(total, seed):
    rng = np.random.default_rng(seed)
    p = np.ldexp(rng.uniform(1.0, 2.0, total), rng.integers(-60, 40, total)).astype(np.float32)
    p = np.where(rng.random(total) < 0.5, -p, p).astype(np.float32)
    p[:8] = np.array([0.0, -0.0, 1e-45, -1e-45, np.finfo(np.float32).max, np.finfo(np.float32).tiny, 1.0, 0.1], dtype=np.float32)
    u = rng.integers(0, 0x7F800000, 64, dtype=np.uint32)   # any finite bit pattern, denormals included
    p[8:72] = u.view(np.float32)
    return p


def test_text_with_params_round_trips_bit_for_bit(model_text):
    for text in (model_text, R.text_of("odd"), R.text_of("two_graphs"), R.text_of("linear_end")):
        total = training.param_layout(text)[1]
        for p in (R.flat_params(oracle_py.OracleModel(text)), _crafted(total, 5)):
            new = training.text_with_params(text, p)
            om = oracle_py.OracleModel(new)
            back = R.flat_params(om)
            assert np.array_equal(back.view(np.uint32), p.view(np.uint32))
            assert om.layer_kinds() == oracle_py.OracleModel(text).layer_kinds()
            assert training.param_layout(new) == training.param_layout(text)


def test_sgd_step_matches_the_scalar_formulas():
    rng = np.random.default_rng(11)
    n = 257
    w = rng.standard_normal(n).astype(np.float32)
    v = (0.1 * rng.standard_normal(n)).astype(np.float32)
    g = (3.0 * rng.standard_normal(n)).astype(np.float32)
    f = np.float32
    for batch, lr, mom, wd in ((1, 0.05, 0.9, 0.0), (7, 0.01, 0.5, 1e-4), (32, 0.1, 0.0, 0.01)):
        nw, nv = training.sgd_step(w, v, g, batch, lr, mom, wd)
        assert nw.dtype == np.float32 and nv.dtype == np.float32
        for i in range(n):
            grad = g[i]
            if wd > 0.0:
                grad = f(grad + f(f(f(2.0) * f(wd)) * w[i]))
            vel = f(f(f(mom) * v[i]) + f(grad / f(batch)))
            par = f(w[i] - f(f(lr) * vel))
            assert vel.view(np.uint32) == nv[i].view(np.uint32) and par.view(np.uint32) == nw[i].view(np.uint32), i
    assert np.array_equal(w, np.asarray(w)) and training.sgd_step(w, v, g, 1, 0.05, 0.9, 0.0)[0] is not w


def test_mse_grad_is_two_differences_over_the_width():
    x = np.array([[0.25, 0.5], [1.0, 0.0]], dtype=np.float32)
    y = np.array([[0.0, 1.0], [0.5, 0.5]], dtype=np.float32)
    assert np.array_equal(training.mse_grad(x, y), np.array([[0.25, -0.5], [0.5, -0.5]], dtype=np.float32))
    assert training.mse_grad(x[:, :1], y[:, :1]).tolist() == [[0.5], [1.0]]
