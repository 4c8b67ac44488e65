"""Synthetic models of OTHER layer widths than the trained one, for the generic fused stage (k_stage_any), from seeds.

Same text format as tools/modelgen.py (a name line, `<count> Layers`, then `Graph_Layer`, `Linear_Layer` / `Weights: k n` /
k rows / `Bias: 1 n` / one row, `ReLU_Activation`, ..., `Sigmoid_Activation`), every value printed with
repr(float(np.float32(v))) so that the oracle and the engine parse the same fp32 weights.  The layer pattern is the trained
model's, (Graph, Linear, ReLU, Linear, ReLU, Linear, ReLU | Sigmoid) per stage with the sigmoid on the last stage only; what
varies is the number of stages, the widths (n1, n2, n3) of each stage's three linear layers, the input width and the output
width.  The first linear layer of a stage whose input is f wide has k = 2 f + 3 (the graph layer's row).

Weights and biases are uniform in [-scale, scale) as modelgen.dense draws them, with scale = min(0.5, 1.1 / sqrt(k)) per
layer so that a 64-wide layer does not blow its sums up and an 8-wide one is not starved.  Random ReLU units die; that the
logits of every member still vary over the vertices and are finite is asserted on oracle outputs by
tests/test_modelgen_shapes.py, not assumed here.

These models are kept out of modelgen.FAMILY on purpose: that family is the trained SHAPE under other weights (three stages,
21 layers), and its tests say so.
"""
from __future__ import annotations

import numpy as np

from tools.modelgen import _f

TRAINED = [(32, 32, 16), (32, 32, 16), (32, 16, 1)]

# name -> (input width, [(n1, n2, n3) per stage])
SPECS = {
    "narrow": (1, [(8, 8, 4), (8, 8, 4), (8, 4, 1)]),
    "wide": (1, [(64, 64, 32), (64, 64, 32), (64, 32, 1)]),
    "odd": (1, [(7, 13, 5), (19, 3, 9), (11, 6, 1)]),
    "two_stage": (1, [(24, 24, 12), (24, 12, 1)]),
    "deep5": (1, [(16, 16, 8)] * 4 + [(16, 8, 1)]),
    "in3": (3, [(32, 32, 16), (32, 32, 16), (32, 16, 1)]),           # the first k is 2 * 3 + 3 = 9
    "out4": (1, [(32, 32, 16), (32, 32, 16), (32, 16, 4)]),
    "first_trained": (1, [(32, 32, 16), (40, 40, 20), (40, 20, 1)]),  # stage 0 of the trained shape, the rest not
}


def stage_widths(name: str):
    """[(f, n3)] per stage: what gnnvc_stage_widths reports."""
    f, stages = SPECS[name]
    out = []
    for (_, _, n3) in stages:
        out.append((f, n3))
        f = n3
    return out


def linear_shapes(name: str):
    """(k, n) of every linear layer, in order."""
    f, stages = SPECS[name]
    out = []
    for (n1, n2, n3) in stages:
        out += [(2 * f + 3, n1), (n1, n2), (n2, n3)]
        f = n3
    return out


def in_width(name: str) -> int:
    return SPECS[name][0]


def out_width(name: str) -> int:
    return SPECS[name][1][-1][2]


def num_layers(name: str) -> int:
    return 7 * len(SPECS[name][1])


def model_text(layers, name: str) -> str:
    """layers: 3 s (W[k, n], bias[n]) pairs, stage after stage."""
    assert len(layers) % 3 == 0 and all(b.shape == (W.shape[1],) for W, b in layers)
    out = [name, f"{len(layers) // 3 * 7} Layers"]
    for i, (W, b) in enumerate(layers):
        if i % 3 == 0:
            out += ["Graph_Layer", ""]
        out += ["Linear_Layer", f"Weights: {W.shape[0]} {W.shape[1]}"]
        out += [" ".join(_f(v) for v in row) + " " for row in W]
        out += ["", f"Bias: 1 {b.size}", " ".join(_f(v) for v in b) + " ", "", ""]
        out += ["ReLU_Activation" if i + 1 < len(layers) else "Sigmoid_Activation", ""]
    return "\n".join(out) + "\n"


def layers_of(name: str, seed: int = 0):
    rng = np.random.default_rng([7, sorted(SPECS).index(name), seed])
    out = []
    for (k, n) in linear_shapes(name):
        scale = min(0.5, 1.1 / np.sqrt(k))
        out.append((rng.uniform(-scale, scale, (k, n)).astype(np.float32), rng.uniform(-scale, scale, n).astype(np.float32)))
    return out


def build(name: str, seed: int = 0) -> str:
    return model_text(layers_of(name, seed), f"shapes_{name}_{seed}")


FAMILY = {name: (lambda name=name: build(name)) for name in SPECS}


def model_input(name: str, g) -> np.ndarray:
    """The forward's input for graph g: x = W / ws, n x 1 — and for a model of input width w > 1 the columns
    x, 0.37 x, 1 - x, ... (n x w), so that no two columns carry the same values."""
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
