"""Synthetic models whose LAYER SEQUENCE lies outside the default pattern of the generic fused stage (k_stage_any:
(Graph_Layer, (Linear_Layer, activation){1..6})+, every activation a ReLU but the model's last, a sigmoid) and inside — or just
outside — what gnnvc_set_generic_patterns admits: a dense stage in front of the first graph layer (bit 1, PROLOGUE), and a model that
ends in a ReLU or in its bare Linear_Layer (bit 2, OPEN_END).

This module is the family's table of members and its own text writer (tools/modelgen_generic.py's writes the default pattern only).
The weight draw, the model's input and the Python restatement of the kernel's LDS layout are tools/modelgen_generic.py's.

A member is (input width, prologue widths or None, [layer widths per graph stage], ending): ending "sigmoid", "relu" or "none".
`trunc` is not drawn: it is the first 14 layers of the trained model's text, the model a caller who wants the 16-wide h2 rows
builds.  Four members are admitted by no mask; they are given as their layer sequence (G = Graph_Layer, L<n> = Linear_Layer of n
outputs, R = ReLU_Activation, S = Sigmoid_Activation).

That every member's outputs vary over the vertices and are finite is asserted on oracle outputs by tests/test_modelgen_patterns.py,
not assumed here; a member that turned out dead gets another seed in SEEDS, not a lower bar.
"""
from __future__ import annotations

import pathlib
import sys

import numpy as np

from tools.modelgen import _f
from tools.modelgen_generic import Family, draw, stage_lds_bytes

PROLOGUE, OPEN_END = 1, 2                      # GNNVC_PATTERN_PROLOGUE, GNNVC_PATTERN_OPEN_END
END_RELU, END_SIGMOID, END_NONE = 0, 1, 2      # "generic_stage_end_<s>"
_END = {"relu": END_RELU, "sigmoid": END_SIGMOID, "none": END_NONE}
FULL_LDS = 163840

SPECS = {
    "embed": (3, (8,), [(16, 8), (8, 1)], "sigmoid"),              # K = 3: the scalar k tail only
    "embed1": (1, (4, 4), [(8, 1)], "sigmoid"),                    # K = 1, then K = 4 with no tail
    "embed_deep": (5, (16, 16, 16, 16, 16, 12), [(16, 1)], "sigmoid"),   # six layers; hands over f = 12
    "embed32": (32, (64, 32), [(32, 16), (16, 1)], "sigmoid"),     # the default bounds' edge
    "mlp": (7, (16, 8, 1), [], "sigmoid"),                         # no graph layer
    "relu_end": (1, None, [(16, 16), (16, 4)], "relu"),
    "trunc": (1, None, [(32, 32, 16), (32, 32, 16)], "relu"),      # the trained model's first two stages, its own weights
    "linear_end": (1, None, [(16, 8), (8, 1)], "none"),
    "linear_end17": (2, None, [(16, 17)], "none"),                 # d = 1, two outputs a lane
    "both": (4, (8,), [(8, 8)], "relu"),
    "embed48": (48, (32, 40), [(16, 1)], "sigmoid"),               # needs set_generic_feature_width(64) too
    "embed_h128": (16, (128, 16), [(16, 1)], "sigmoid"),           # needs set_generic_big_stages too
}
# member -> the least mask that admits it
MASK = {"embed": 1, "embed1": 1, "embed_deep": 1, "embed32": 1, "mlp": 1, "relu_end": 2, "trunc": 2, "linear_end": 2,
        "linear_end17": 2, "both": 3, "embed48": 1, "embed_h128": 1}
NEEDS_FEAT, NEEDS_BIG = ["embed48"], ["embed_h128"]
ADMITTED = list(SPECS)

# admitted by no mask: (input width, layer sequence)
ODD = {
    "mid_sigmoid": (1, "G L16 R L8 S G L8 R L1 S"),       # a sigmoid inside the model
    "two_graphs": (1, "G G L8 R L1 S"),                   # a stage with no dense layer
    "prologue7": (4, "L8 R L8 R L8 R L8 R L8 R L8 R L8 R G L8 R L1 S"),   # a block of seven dense layers
    "bare_pair": (3, "L4 L1"),                            # two linear layers without an activation between them
}
NOT_FITTING = list(ODD)
NAMES = ADMITTED + NOT_FITTING

# seed per member (changed here, and only here, if a member's outputs turn out dead)
SEEDS = {name: 0 for name in NAMES}
SEEDS["relu_end"] = 2   # (under seed 0 three of its four outputs, under seed 1 one, take a single value over every vertex of er3000)
TAG, PREFIX = 29, "patterns"   # rng seed list [29, NAMES.index(name), seed], first line patterns_<name>_<seed>


def sequence(name: str) -> str:
    """The member's layer sequence, in ODD's notation."""
    if name in ODD:
        return ODD[name][1]
    _, pro, stages, ending = SPECS[name]
    blocks = ([list(pro)] if pro else []) + [list(ws) for ws in stages]
    out = []
    for b, ws in enumerate(blocks):
        if not (pro and b == 0):
            out.append("G")
        for n in ws:
            out += [f"L{n}", "R"]
    out.pop()   # the model's last activation
    if ending != "none":
        out.append("S" if ending == "sigmoid" else "R")
    return " ".join(out)


def in_width(name: str) -> int:
    return ODD[name][0] if name in ODD else SPECS[name][0]


def linear_shapes(name: str):
    """(k, n) of every linear layer, in order."""
    w, out = in_width(name), []
    for tok in sequence(name).split():
        if tok == "G":
            w = 2 * w + 3
        elif tok[0] == "L":
            out.append((w, int(tok[1:])))
            w = int(tok[1:])
    return out


def out_width(name: str) -> int:
    w = in_width(name)
    for tok in sequence(name).split():
        w = 2 * w + 3 if tok == "G" else int(tok[1:]) if tok[0] == "L" else w
    return w


def num_layers(name: str) -> int:
    return len(sequence(name).split())


def _trained_text() -> str:
    return (pathlib.Path(__file__).resolve().parent.parent / "gnn-mwvc_amd" / "data" / "mwvc_model.txt").read_text()


def layers_of(name: str, seed: int | None = None):
    """(W[k, n], bias[n]) of every linear layer, in order (trunc: None — its weights are the trained text's)."""
    if name == "trunc":
        return None
    seed = SEEDS[name] if seed is None else seed
    return draw(np.random.default_rng([TAG, NAMES.index(name), seed]), linear_shapes(name))


def model_text(seq: str, layers, first_line: str) -> str:
    """The family's own writer: any sequence of records, in tools/modelgen_generic.model_text's format record by record."""
    toks = seq.split()
    out = [first_line, f"{len(toks)} Layers"]
    it = iter(layers)
    for tok in toks:
        if tok == "G":
            out += ["Graph_Layer", ""]
        elif tok == "R":
            out += ["ReLU_Activation", ""]
        elif tok == "S":
            out += ["Sigmoid_Activation", ""]
        else:
            W, b = next(it)
            assert W.shape[1] == int(tok[1:]) == b.size
            out += ["Linear_Layer", f"Weights: {W.shape[0]} {W.shape[1]}"]
            out += [" ".join(_f(v) for v in row) + " " for row in W]
            out += ["", f"Bias: 1 {b.size}", " ".join(_f(v) for v in b) + " ", "", ""]
    return "\n".join(out) + "\n"


def build(name: str, seed: int | None = None) -> str:
    if name == "trunc":   # the first 14 layers of the trained model's text
        head = _trained_text().split("Graph_Layer")
        return "patterns_trunc\n14 Layers\nGraph_Layer" + head[1] + "Graph_Layer" + head[2]
    seed = SEEDS[name] if seed is None else seed
    return model_text(sequence(name), layers_of(name, seed), f"{PREFIX}_{name}_{seed}")


FAMILY = {name: (lambda name=name: build(name)) for name in NAMES}


# ---------------------------------------------------------------- what the engine reports of an admitted member

def stages_of(name: str):
    """[(dense, f, widths, end)] per stage of an admitted member: the dense stage first where there is one."""
    f, pro, stages, ending = SPECS[name]
    blocks = ([(1, tuple(pro))] if pro else []) + [(0, tuple(ws)) for ws in stages]
    out = []
    for b, (dense, ws) in enumerate(blocks):
        out.append((dense, f, ws, _END[ending] if b + 1 == len(blocks) else END_RELU))
        f = ws[-1]
    return out


def stage_widths(name: str):
    return [(f, ws[-1]) for _, f, ws, _ in stages_of(name)]


def stage_depths(name: str):
    return [len(ws) for _, _, ws, _ in stages_of(name)]


def stage_dense(name: str):
    return [dense for dense, _, _, _ in stages_of(name)]


def stage_ends(name: str):
    return [end for _, _, _, end in stages_of(name)]


def lds_bytes(name: str, rows: int = 16):
    """Per stage: "generic_stage_lds_bytes_<s>" (rows = 16) — a dense stage's first K is f."""
    return [stage_lds_bytes(f, ws, rows, first_k=f if dense else 0) for dense, f, ws, _ in stages_of(name)]


def stage_threads(name: str, limit: int = 0):
    """Per stage: "generic_stage_threads_<s>" — 256 within the default bounds, else the largest of 1024 / 512 / 256 that fits."""
    out = []
    for (dense, f, ws, _), b256 in zip(stages_of(name), lds_bytes(name)):
        if all(n <= 64 for n in ws[:-1]) and b256 <= 65536:
            out.append(256)
        else:
            out.append(next(t for t in (1024, 512, 256) if stage_lds_bytes(f, ws, t // 16, first_k=f if dense else 0) <= limit))
    return out


def admitted_by(name: str, mask: int) -> bool:
    return name in MASK and (mask & MASK[name]) == MASK[name]


_input = Family(PREFIX, TAG, list, {name: (in_width(name), []) for name in NAMES})


def model_input(name: str, g):
    """The forward's input for graph g: tools/modelgen_generic.py's columns x, 0.37 x, 1 - x, 3 x, ... for the member's width."""
    return _input.model_input(name, g)


if __name__ == "__main__":
    sys.stdout.write(FAMILY[sys.argv[1]]())
