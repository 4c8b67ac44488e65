"""What a trainer needs around Engine.train_forward / Engine.backward: the layout of the flat parameter array, a model text with
new parameters, the MSE gradient and the SGD step of the reference's old trainer (reference old_files/src/lib/gnn_training.cpp:
MSE_grad, SGD_step), in float32 numpy.  Plain host code: the gradients themselves come from the engine's HIP kernels.

The loop ("Retraining"):

    p, vel = engine.params(), np.zeros(engine.num_params(), np.float32)
    scores = engine.train_forward(x, p)
    grad = engine.backward(mse_grad(scores, target))
    p, vel = sgd_step(p, vel, grad, batch=1, lr=0.05, momentum=0.9, weight_decay=0.0)
    ...
    text = text_with_params(model_text, p)      # a fresh inference Engine(text) scores with exactly these bits

The same loop on the device — the engine's gnnvc_mse_device and gnnvc_sgd_step_device kernels in the arithmetic of mse_grad and
sgd_step below, which stay as the reference they are tested against — is Trainer, at the end of this module.
"""
from __future__ import annotations

import numpy as np

_RECORDS = ("Linear_Layer", "Graph_Layer", "ReLU_Activation", "Sigmoid_Activation")


def _walk(text: str):
    """(name, [record]) of a model text, read the way the engine's parser reads it: a record is (kind,) or
    ("Linear_Layer", w_label, k, m, W tokens, b_label, bh, bw, bias tokens); unknown records are skipped."""
    tok = text.split()
    if len(tok) < 3:
        raise ValueError("model header: expected '<name> <n> Layers'")
    name, n, at, out = tok[0], int(tok[1]), 3, []
    for _ in range(n):
        if at >= len(tok):
            raise ValueError("model text ends early")
        kind = tok[at]
        at += 1
        if kind == "Linear_Layer":
            wl, k, m = tok[at], int(tok[at + 1]), int(tok[at + 2])
            at += 3
            W = tok[at: at + k * m]
            at += k * m
            bl, bh, bw = tok[at], int(tok[at + 1]), int(tok[at + 2])
            at += 3
            b = tok[at: at + bh * bw]
            at += bh * bw
            if len(W) != k * m or bh != 1 or bw != m or len(b) != m:
                raise ValueError("malformed Linear_Layer record")
            out.append((kind, wl, k, m, W, bl, bh, bw, b))
        elif kind in _RECORDS:
            out.append((kind,))
    return name, out


def param_layout(text: str):
    """([(k, m, w_off, b_off)] per Linear_Layer in the order of the text, total): W is params[w_off: w_off + k * m] as k x m
    row-major, the bias params[b_off: b_off + m] — the order of gnnvc_get_params and of every gradient."""
    off, out = 0, []
    for rec in _walk(text)[1]:
        if rec[0] == "Linear_Layer":
            k, m = rec[2], rec[3]
            out.append((k, m, off, off + k * m))
            off += k * m + m
    return out, off


def text_with_params(text: str, params) -> str:
    """The model text with its parameters replaced by `params` (flat, param_layout's order), every value written as %.9g: nine
    significant digits name one float32, so the parser reads back the same bits (NaN payloads aside)."""
    p = np.ascontiguousarray(params, dtype=np.float32).reshape(-1)
    name, recs = _walk(text)
    layout, total = param_layout(text)
    if p.size != total:
        raise ValueError(f"params: {p.size} values, the model has {total}")
    lines, li = [name, f"{len(recs)} Layers"], 0

    def row(v):
        return " ".join("%.9g" % float(x) for x in v) + " "
    for rec in recs:
        lines.append(rec[0])
        if rec[0] == "Linear_Layer":
            k, m, w_off, b_off = layout[li]
            li += 1
            lines.append(f"{rec[1]} {k} {m}")
            lines += [row(p[w_off + r * m: w_off + (r + 1) * m]) for r in range(k)]
            lines.append(f"{rec[5]} 1 {m}")
            lines.append(row(p[b_off: b_off + m]))
        lines.append("")
    return "\n".join(lines)


def mse_grad(scores, target) -> np.ndarray:
    """MSE_grad: (2 (x - y)) / width per element (not divided by the number of rows, as there), float32."""
    x = np.ascontiguousarray(scores, dtype=np.float32)
    y = np.ascontiguousarray(target, dtype=np.float32).reshape(x.shape)
    width = np.float32(x.shape[-1] if x.ndim > 1 else 1)
    return ((np.float32(2.0) * (x - y)) / width).astype(np.float32)


def mse_loss(scores, target) -> float:
    """MSE_loss as a float64 mean of squared float32 differences (a read-out: nothing is trained on its bits)."""
    x = np.ascontiguousarray(scores, dtype=np.float32)
    y = np.ascontiguousarray(target, dtype=np.float32).reshape(x.shape)
    d = (x - y).astype(np.float64)
    return float(np.mean(d * d)) if d.size else 0.0


def sgd_step(params, vel, grad, batch: int, lr: float, momentum: float, weight_decay: float):
    """SGD_step: with weight_decay > 0 first grad = grad + (2 weight_decay) w; then vel = (momentum vel) + (grad / batch) and
    w = w - (lr vel), every operation rounded to float32 on its own.  Returns the new (params, vel); the inputs are not changed."""
    f = np.float32
    w = np.ascontiguousarray(params, dtype=np.float32)
    g = np.ascontiguousarray(grad, dtype=np.float32).reshape(w.shape)
    v = np.ascontiguousarray(vel, dtype=np.float32).reshape(w.shape)
    if weight_decay > 0.0:
        g = (g + (f(2.0) * f(weight_decay)) * w).astype(np.float32)
    v = ((f(momentum) * v).astype(np.float32) + (g / f(batch)).astype(np.float32)).astype(np.float32)
    w = (w - (f(lr) * v).astype(np.float32)).astype(np.float32)
    return w, v


class Trainer:
    """run_model of the reference's old trainer (old_files/src/apps/gnn_train.cpp) with everything between two graphs on the device:
    parameters, velocity, the gradient accumulator, a gnnvc_fit_stats and the per-graph x, target, scores and loss-gradient
    buffers are torch tensors on the engine's device, used by pointer.  The trainer takes a stream from torch and installs it
    in the engine (Engine.set_stream) for as long as it lives, so that torch's copies and the engine's kernels queue in one place
    and torch never holds a stream the engine may destroy; close() hands the engine its own stream back.  Per graph: the hand-off, x = W / ws
    and the target copied up, Engine.train_forward_device with the trainer's parameters, Engine.mse_device (the gradient only when
    fitting), Engine.backward_device accumulating.  No row and no parameter is copied to the host between graphs; run() reads
    the stats back once, at its end.

    The batch rule: t += n after a graph's backward, a step with batch = t once t > batch_vertices, then t = 0; a trailing step at
    the end of run() if t > 0.  (run_model does not count the rows of the graph that triggers a step — an accident of its
    if / else; here the divisor is the number of rows whose gradients are in the sum.  DESIGN.md section 3, "Loss and step".)

    The engine's own inference parameters are never touched; text() is the model text with the trained ones."""

    def __init__(self, engine, model_text: str, batch_vertices: int = 500_000, lr: float = 0.01, momentum: float = 0.9,
                 weight_decay: float = 0.0, params=None, device: int = 0):
        """engine: an Engine of model_text on `device` (single-device).  params: the parameters to start from, default the model's own."""
        import torch
        self._torch = torch
        if engine.in_width != 1:
            raise ValueError(f"the trainer's input is x = W / ws, one column: the model takes {engine.in_width}")
        self.engine, self.model_text = engine, model_text
        self.batch_vertices, self.lr, self.momentum, self.weight_decay = int(batch_vertices), lr, momentum, weight_decay
        self.count = param_layout(model_text)[1]
        if self.count != engine.num_params():
            raise ValueError(f"model_text has {self.count} parameters, the engine's model {engine.num_params()}")
        p = np.ascontiguousarray(engine.params() if params is None else params, dtype=np.float32).reshape(-1)
        if p.size != self.count:
            raise ValueError(f"params: {p.size} values, the model has {self.count}")
        self.device = torch.device("cuda", device)
        # torch's stream, installed in the engine: torch's streams outlive every engine, which an engine's own stream would not
        # (torch's page-locked allocator records an event on the stream of a block's last copy when the block is freed)
        self._stream = torch.cuda.Stream(device=self.device)
        engine.set_stream(self._stream.cuda_stream)
        self._copied = torch.cuda.Event()
        self._width = engine.out_width
        with torch.cuda.stream(self._stream):
            self._params = torch.from_numpy(p.copy()).to(self.device)
            self._vel = torch.zeros(max(self.count, 1), dtype=torch.float32, device=self.device)
            self._grad = torch.zeros(max(self.count, 1), dtype=torch.float32, device=self.device)   # the accumulator: +0.0f
            self._stats = torch.zeros(5, dtype=torch.int64, device=self.device)                     # a gnnvc_fit_stats
        self._stream.synchronize()
        self._rows, self.stats = 0, None
        self._x = self._target = self._scores = self._loss_grad = self._pin_x = self._pin_target = None

    def close(self):
        """Waits for the trainer's work and hands the engine its own stream back (if the engine is still open)."""
        if self._stream is not None:
            self._stream.synchronize()
            if getattr(self.engine, "_h", None) and self.engine._h.value:
                self.engine.set_stream(None)
            self._stream = None

    def _reserve(self, n: int):
        torch = self._torch
        if n <= self._rows:
            return
        self._copied.synchronize()   # (nothing reads the old page-locked buffers any more)
        rows, w = max(n, 1), self._width
        with torch.cuda.stream(self._stream):
            self._x = torch.empty(rows, dtype=torch.float32, device=self.device)
            self._target, self._scores, self._loss_grad = (torch.empty(rows * w, dtype=torch.float32, device=self.device)
                                                           for _ in range(3))
        self._pin_x = torch.empty(rows, dtype=torch.float32).pin_memory()
        self._pin_target = torch.empty(rows * w, dtype=torch.float32).pin_memory()
        self._rows = rows

    def _step(self, batch: int):
        self.engine.sgd_step_device(self.count, self._params.data_ptr(), self._vel.data_ptr(), self._grad.data_ptr(), batch, self.lr,
                                    self.momentum, self.weight_decay, zero_grad=True)

    def run(self, pairs, fit: bool, hand_off: bool = True):
        """One pass over pairs = [(graph, target[n, out_width])] — an epoch with fit, an evaluation without.  Returns (loss, total
        accuracy, true accuracy) by run_model's formulas: loss_sum / rows, (positive_hits + negative_hits) / rows, positive_hits /
        positives (NaN where the divisor is zero); the sums themselves stay in self.stats, a FitStats.  hand_off = False: every
        pair's graph is the engine's resident graph already (one graph trained on again and again) and is not handed over."""
        from .engine import FitStats
        torch, e, w = self._torch, self.engine, self._width
        with torch.cuda.stream(self._stream):
            self._stats.zero_()
        t = 0
        for g, target in pairs:
            n = int(g.n)
            if hand_off:
                e.set_weight_scale(g.ws)
                e.upload_graph(g)
            self._reserve(n)
            if n:
                y = np.ascontiguousarray(target, dtype=np.float32).reshape(n * w)
                self._copied.synchronize()   # the page-locked buffers' last copies are done (long ago, as a rule)
                self._pin_x[:n].copy_(torch.from_numpy(np.ascontiguousarray(g.x(), dtype=np.float32).reshape(n)))
                self._pin_target[: n * w].copy_(torch.from_numpy(y))
                with torch.cuda.stream(self._stream):
                    self._x[:n].copy_(self._pin_x[:n], non_blocking=True)
                    self._target[: n * w].copy_(self._pin_target[: n * w], non_blocking=True)
                    self._copied.record()
            e.train_forward_device(self._x.data_ptr(), self._scores.data_ptr(), self._params.data_ptr())
            e.mse_device(n, w, self._scores.data_ptr(), self._target.data_ptr(), self._loss_grad.data_ptr() if fit else 0,
                         self._stats.data_ptr())
            if fit:
                e.backward_device(self._loss_grad.data_ptr(), self._grad.data_ptr(), 0, accumulate=True)
                t += n
                if t > self.batch_vertices:
                    self._step(t)
                    t = 0
        if t > 0:
            self._step(t)
        with torch.cuda.stream(self._stream):
            raw = self._stats.cpu().numpy()   # the one read-back
        out = FitStats()
        out.loss_sum = float(raw[:1].view(np.float64)[0])
        out.rows, out.positives, out.positive_hits, out.negative_hits = (int(v) for v in raw[1:].view(np.uint64))
        self.stats = out
        return out.loss, out.total_accuracy, out.true_accuracy

    def params(self) -> np.ndarray:
        with self._torch.cuda.stream(self._stream):
            return self._params[: self.count].cpu().numpy()

    def velocity(self) -> np.ndarray:
        with self._torch.cuda.stream(self._stream):
            return self._vel[: self.count].cpu().numpy()

    def scores(self) -> np.ndarray:
        """The last graph's training-forward scores, [n, out_width]."""
        n = self.engine.n
        with self._torch.cuda.stream(self._stream):
            return self._scores[: n * self._width].cpu().numpy().reshape(n, self._width)

    def text(self) -> str:
        return text_with_params(self.model_text, self.params())
