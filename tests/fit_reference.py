"""The CPU reference of the loss read-outs of include/gnnvc.h "loss and step" ("Loss and step"): the loss
total of one gnnvc_mse call and run_model's three counts, in float32 numpy, one rounded operation at a time, in the order the
header states.  The gradient and the step have their reference in gnn_mwvc_amd.training (mse_grad, sgd_step).
tests/test_fit_reference.py holds this module to float64 and to the reference trainer's own loops; tests/test_gpu_fit.py holds the
engine to it bit for bit.  A plain module: nothing here touches a GPU.
"""
import numpy as np

GRAD_BLOCK_ROWS = 4096   # GNNVC_GRAD_BLOCK_ROWS
F32 = np.float32


def _shaped(scores, target):
    x = np.ascontiguousarray(scores, dtype=F32)
    x = x.reshape(x.shape[0], int(np.prod(x.shape[1:]))) if x.ndim > 1 else x.reshape(-1, 1)
    return x, np.ascontiguousarray(target, dtype=F32).reshape(x.shape)


def row_values(scores, target):
    """r_i = se_i / width, se_i one float32 chain over the row's columns from +0.0f of se + d * d, d = x - y."""
    x, y = _shaped(scores, target)
    se = np.zeros(x.shape[0], F32)
    with np.errstate(all="ignore"):
        for j in range(x.shape[1]):
            d = (x[:, j] - y[:, j]).astype(F32)
            se = (se + (d * d).astype(F32)).astype(F32)
        return (se / F32(x.shape[1])).astype(F32)


def loss_total(scores, target):
    """The float32 total one call adds to loss_sum: per block of GRAD_BLOCK_ROWS rows one chain over its row values in ascending
    order from +0.0f, then one chain over the blocks' partials in ascending order from +0.0f."""
    r = row_values(scores, target)
    total = F32(0.0)
    with np.errstate(all="ignore"):
        for lo in range(0, r.size, GRAD_BLOCK_ROWS):
            part = F32(0.0)
            for v in r[lo: lo + GRAD_BLOCK_ROWS]:
                part = F32(part + v)
            total = F32(total + part)
    return total


def counts(scores, target):
    """(positives, positive_hits, negative_hits) on column 0: run_model's num_true, true_accuracy and total_accuracy counters."""
    x, y = _shaped(scores, target)
    with np.errstate(invalid="ignore"):
        pos = y[:, 0] > F32(0.5)
        return int(pos.sum()), int((pos & (x[:, 0] > F32(0.5))).sum()), int((~pos & (x[:, 0] < F32(0.5))).sum())


class Stats:
    """gnnvc_fit_stats on the host: add() is one gnnvc_mse call with stats."""

    def __init__(self):
        self.loss_sum, self.rows, self.positives, self.positive_hits, self.negative_hits = 0.0, 0, 0, 0, 0

    def add(self, scores, target):
        x, _ = _shaped(scores, target)
        if x.shape[0] == 0:
            return self
        with np.errstate(all="ignore"):
            self.loss_sum = self.loss_sum + float(loss_total(scores, target))   # a double add of the fp32 total
        p, ph, nh = counts(scores, target)
        self.rows += x.shape[0]
        self.positives += p
        self.positive_hits += ph
        self.negative_hits += nh
        return self

    def metrics(self):
        """run_model's three read-outs: (loss, total accuracy, true accuracy), NaN where the divisor is zero."""
        nan = float("nan")
        return (self.loss_sum / self.rows if self.rows else nan,
                (self.positive_hits + self.negative_hits) / self.rows if self.rows else nan,
                self.positive_hits / self.positives if self.positives else nan)

    def fields(self):
        return self.loss_sum, self.rows, self.positives, self.positive_hits, self.negative_hits
