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
