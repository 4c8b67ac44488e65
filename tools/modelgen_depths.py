"""Synthetic models whose stages have OTHER DEPTHS than the trained one's three dense layers, for the generic fused stage
(k_stage_any), from seeds.

Same text format and the same weight draw as tools/modelgen_shapes.py: a name line, `<count> Layers`, then per stage
`Graph_Layer` followed by d pairs (`Linear_Layer`, activation), 1 <= d <= 6 and d free per stage; every activation is
`ReLU_Activation` except the model's last, which is `Sigmoid_Activation`.  Weights and biases are uniform in [-s, s),
s = min(0.5, 1.1 / sqrt(k)) per layer, every value printed with repr(float(np.float32(v))).  The first linear layer of a stage
whose input is f wide has k = 2 f + 3 (the graph layer's row).

That the logits of every member vary over the vertices and are finite is asserted on oracle outputs by
tests/test_modelgen_depths.py, not assumed here; a member that turned out dead gets another seed in SEEDS, not a lower bar.
"""
from __future__ import annotations

import numpy as np

from tools.modelgen import _f

MAX_DENSE_LAYERS = 6

# name -> (input width, [layer widths per stage])
SPECS = {
    "logit": (1, [(1,)]),                                            # one stage, d = 1: the last layer reads the graph row
    "one_each": (1, [(8,), (4,), (1,)]),                             # d = 1 in every stage
    "two_deep": (1, [(24, 12), (24, 1)]),                            # even d
    "four_deep": (1, [(32, 32, 32, 16), (32, 32, 16, 1)]),           # even d, trained-like widths
    "six_deep": (1, [(16, 16, 16, 16, 16, 8), (16, 16, 16, 16, 16, 1)]),   # the maximum
    "mixed": (1, [(32, 32, 16), (20,), (9, 7, 13, 11, 1)]),          # depths 3 / 1 / 5, odd widths, stage 0 of the trained shape
    "late_wide": (1, [(8, 8, 8, 64, 4), (8, 64, 7, 64, 1)]),         # the widest layer late; alternating 64 / 7
    "in3_f32": (3, [(40, 32), (61, 3, 50, 1)]),                      # f = 32 second stage (k = 67), 32 outputs from a last layer
    "too_big": (1, [(64, 64, 64, 64, 64, 32), (64, 64, 64, 64, 64, 1)]),   # outside the LDS bound: stays layer by layer
}
FITTING = [name for name in SPECS if name != "too_big"]

# seed per member (changed here, and only here, if a member's logits turn out dead)
SEEDS = {name: 0 for name in SPECS}


def stage_widths(name: str):
    """[(f, last width)] per stage: what gnnvc_stage_widths reports."""
    f, stages = SPECS[name]
    out = []
    for ws in stages:
        out.append((f, ws[-1]))
        f = ws[-1]
    return out


def stage_depths(name: str):
    """Dense layers per stage: what gnnvc_get_info "generic_stage_layers_<s>" reports."""
    return [len(ws) for ws in SPECS[name][1]]


def linear_shapes(name: str):
    """(k, n) of every linear layer, in order."""
    f, stages = SPECS[name]
    out = []
    for ws in stages:
        k = 2 * f + 3
        for n in ws:
            out.append((k, n))
            k = n
        f = ws[-1]
    return out


def in_width(name: str) -> int:
    return SPECS[name][0]


def out_width(name: str) -> int:
    return SPECS[name][1][-1][-1]


def num_layers(name: str) -> int:
    return sum(1 + 2 * len(ws) for ws in SPECS[name][1])


def model_text(layers, depths, name: str) -> str:
    """layers: (W[k, n], bias[n]) pairs, stage after stage; depths: how many of them each stage takes."""
    assert sum(depths) == len(layers) and all(b.shape == (W.shape[1],) for W, b in layers)
    starts = set(np.cumsum([0] + list(depths[:-1])).tolist())
    out = [name, f"{len(depths) + 2 * len(layers)} Layers"]
    for i, (W, b) in enumerate(layers):
        if i in starts:
            out += ["Graph_Layer", ""]
        out += ["Linear_Layer", f"Weights: {W.shape[0]} {W.shape[1]}"]
        out += [" ".join(_f(v) for v in row) + " " for row in W]
        out += ["", f"Bias: 1 {b.size}", " ".join(_f(v) for v in b) + " ", "", ""]
        out += ["ReLU_Activation" if i + 1 < len(layers) else "Sigmoid_Activation", ""]
    return "\n".join(out) + "\n"


def draw(rng, shapes):
    """The family's weight draw: per (k, n), W[k, n] then bias[n], uniform in [-s, s), s = min(0.5, 1.1 / sqrt(k)).
    (tools/modelgen_big.py draws its members with this function too.)"""
    out = []
    for (k, n) in shapes:
        scale = min(0.5, 1.1 / np.sqrt(k))
        out.append((rng.uniform(-scale, scale, (k, n)).astype(np.float32), rng.uniform(-scale, scale, n).astype(np.float32)))
    return out


def layers_of(name: str, seed: int | None = None):
    seed = SEEDS[name] if seed is None else seed
    return draw(np.random.default_rng([13, list(SPECS).index(name), seed]), linear_shapes(name))


def build(name: str, seed: int | None = None) -> str:
    seed = SEEDS[name] if seed is None else seed
    return model_text(layers_of(name, seed), stage_depths(name), f"depths_{name}_{seed}")


FAMILY = {name: (lambda name=name: build(name)) for name in SPECS}


def model_input(name: str, g) -> np.ndarray:
    """The forward's input for graph g, as tools/modelgen_shapes.model_input: x = W / ws, n x 1 — and for a model of input
    width w > 1 the columns x, 0.37 x, 1 - x, ... (n x w)."""
    x = np.ascontiguousarray(g.x(), dtype=np.float32).reshape(g.n, 1)
    w = in_width(name)
    if w == 1:
        return x
    cols = [x, (x * np.float32(0.37)).astype(np.float32), (np.float32(1.0) - x).astype(np.float32)]
    while len(cols) < w:
        cols.append((x * np.float32(len(cols))).astype(np.float32))
    return np.ascontiguousarray(np.concatenate(cols[:w], axis=1), dtype=np.float32)


if __name__ == "__main__":
    import sys
    sys.stdout.write(FAMILY[sys.argv[1]]())
