"""tests/fit_reference.py, the float32 restatement the GPU tests hold gnnvc_mse to bit for bit, held itself to two things on the CPU:
an independent float64 evaluation of the same inputs, within the forward error bound of the float32 chains it is made of, and —
up to one block of rows — the reference trainer's own loops (MSE_loss's `loss += se / width`, run_model's if / else), bit for bit."""
import numpy as np
import pytest

from tests import fit_reference as FR
from tests import generic_harness as H

F32 = np.float32
ROWS, WIDTHS = [1, 255, 4096, 4097, 8209], [1, 3, 16]


def _inputs(n, width):
    return H.crafted_input(n, width, 100 * n + width), H.crafted_input(n, width, 7 + 100 * n + width)


def _gamma(k):
    """Higham's gamma_k = k u / (1 - k u) for float32, u = eps / 2: the relative error bound of k rounded operations in a row."""
    u = float(np.finfo(np.float32).eps) / 2.0
    assert k * u < 1.0
    return k * u / (1.0 - k * u)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n", ROWS)
def test_loss_total_against_float64(n, width):
    """Every term is a square, so nothing cancels and the error of the total is relative.  A row value passes the subtraction
    (1 rounding), the square (the subtraction's error twice, 1 rounding: 3 in all), `width` adds and the division: width + 4
    roundings at the most.  It then passes the adds of its block's chain, at most min(n, 4096) of them, and the adds of the
    chain over the blocks, one per block.  The bound is gamma of that count; no value here overflows or falls below the
    normal range (magnitudes 2^-20 .. 2^20, squares 2^-40 .. 2^42)."""
    x, y = _inputs(n, width)
    d = x.astype(np.float64) - y.astype(np.float64)
    want = float(((d * d).sum(axis=1) / width).sum())
    got = float(FR.loss_total(x, y))
    blocks = -(-n // FR.GRAD_BLOCK_ROWS)
    bound = _gamma(width + 4 + min(n, FR.GRAD_BLOCK_ROWS) + blocks)
    print(f"n {n} width {width}: relative error {abs(got - want) / want:.3e}, bound {bound:.3e}")
    assert want > 0.0 and abs(got - want) <= bound * want


def _trainer_loops(x, y):
    """MSE_loss's chain before its division by the height, and run_model's three counters, as the reference writes them."""
    n, width = x.shape
    loss, fw = F32(0.0), F32(width)
    num_true = true_acc = total_acc = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            se = F32(0.0)
            for j in range(width):
                se = F32(se + F32((x[i, j] - y[i, j]) * (x[i, j] - y[i, j])))
            loss = F32(loss + F32(se / fw))
            if y[i, 0] > 0.5:
                num_true += 1
                if x[i, 0] > 0.5:
                    true_acc += 1
            elif x[i, 0] < 0.5:
                total_acc += 1
    return loss, (num_true, true_acc, total_acc)


def edge_rows(x, y):
    """Copies of x and y whose first 16 rows (where there are as many) hold in column 0 what run_model's comparisons have to
    place: the threshold, either side of it, signed zeros, inf, NaN — against each other and against a positive target."""
    x, y = x.copy(), y.copy()
    if x.shape[0] >= 16:
        edge = np.array([0.5, np.nextafter(F32(0.5), F32(1)), np.nextafter(F32(0.5), F32(0)), 0.0, -0.0, np.inf, -np.inf, np.nan], F32)
        x[:8, 0], y[:8, 0] = edge, edge[::-1]
        x[8:16, 0], y[8:16, 0] = edge, F32(0.75)
    return x, y


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n", [r for r in ROWS if r <= FR.GRAD_BLOCK_ROWS])
def test_one_block_is_the_trainers_own_loop(n, width):
    for x, y in (_inputs(n, width), edge_rows(*_inputs(n, width))):
        loss, cnt = _trainer_loops(x, y)
        got = FR.loss_total(x, y)
        assert (np.isnan(got) and np.isnan(loss)) or got.view(np.uint32) == loss.view(np.uint32), (got, loss)
        assert FR.counts(x, y) == cnt


def test_stats_add_up_and_report_run_models_formulas():
    a, b = _inputs(4097, 3), _inputs(255, 3)
    s = FR.Stats().add(*a).add(*b).add(np.zeros((0, 3), F32), np.zeros((0, 3), F32))
    assert s.loss_sum == (0.0 + float(FR.loss_total(*a))) + float(FR.loss_total(*b)) and s.rows == 4097 + 255
    ca, cb = FR.counts(*a), FR.counts(*b)
    assert (s.positives, s.positive_hits, s.negative_hits) == tuple(u + v for u, v in zip(ca, cb))
    assert s.metrics() == (s.loss_sum / s.rows, (s.positive_hits + s.negative_hits) / s.rows, s.positive_hits / s.positives)
    assert all(np.isnan(v) for v in FR.Stats().metrics())
