"""The one implementation behind the synthetic-model families of the generic fused stage (k_stage_any): tools/modelgen_shapes.py
(other widths), tools/modelgen_depths.py (other depths), tools/modelgen_big.py (stages outside the default LDS and hidden-width
bounds) and tools/modelgen_feat.py (feature widths above 32).  Those modules hold their tables of members; everything that turns a table into model texts, weights and inputs is here, once.

A family is data: SPECS (name -> (input width, [layer widths per stage])), the tag that opens its rng seed list, how a member's
index in that list is taken (`sorted` or `list`, over SPECS), the prefix of the text's first line, and optionally SEEDS
(name -> seed; 0 where absent) and members borrowed from another family, text and weights included.

Text format, as tools/modelgen.py's: a name line, `<count> Layers`, then per stage `Graph_Layer` followed by d pairs
(`Linear_Layer` / `Weights: k n` / k rows / `Bias: 1 n` / one row, activation), 1 <= d <= 6 and d free per stage; every
activation is `ReLU_Activation` except the model's last, which is `Sigmoid_Activation`.  Every value is printed with
repr(float(np.float32(v))) so that the oracle and the engine parse the same fp32 weights.  The first linear layer of a stage
whose input is f wide has k = 2 f + 3 (the graph layer's row).

Weights and biases are uniform in [-s, s), s = min(0.5, 1.1 / sqrt(k)) per layer, so that a 64-wide layer does not blow its sums
up and an 8-wide one is not starved.  tests/test_modelgen_generic.py pins the SHA-256 of every member's text: the rng seed list
[tag, index, seed] and the order of the draws are part of every generic-stage test's weights.

stage_lds_bytes restates the kernel's LDS layout (stage_any_layout of csrc/gnnvc_stage_any.hip) in Python, for any family's
stages: the layers' transposed weights at a pitch of an odd number of 16-byte slots, the biases, then per row of a pass two
vectors A and B.
"""
from __future__ import annotations

import numpy as np

from tools.modelgen import _f

MAX_DENSE_LAYERS = 6
SMALL_LDS, MAX_LDS = 64 * 1024, 160 * 1024
SMALL_HIDDEN, BIG_HIDDEN, MAX_LAST, MAX_F = 64, 128, 32, 32


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
    """The weight draw: per (k, n), W[k, n] then bias[n], uniform in [-s, s), s = min(0.5, 1.1 / sqrt(k))."""
    out = []
    for (k, n) in shapes:
        scale = min(0.5, 1.1 / np.sqrt(k))
        out.append((rng.uniform(-scale, scale, (k, n)).astype(np.float32), rng.uniform(-scale, scale, n).astype(np.float32)))
    return out


def _round4(v: int) -> int:
    return (v + 3) // 4 * 4


def _pitch(k: int) -> int:
    return 4 * (((k + 3) // 4) | 1)


def stage_lds_bytes(f: int, widths, rows: int = 16, first_k: int = 0) -> int:
    """stage_any_layout(...).total * 4 for a stage of input width f and these layer widths, `rows` rows a pass (threads / 16).
    first_k: the first layer's K — 0 = a graph stage's 2 f + 3, f for a dense stage (tools/modelgen_patterns.py)."""
    k0 = first_k if first_k else 2 * f + 3
    k, wsum, nsum, a, b = k0, 0, 0, k0, 0
    for l, n in enumerate(widths):
        wsum += n * _pitch(k)
        nsum += n
        if l + 1 < len(widths):
            if l & 1:
                a = max(a, n)
            else:
                b = max(b, n)
        k = n
    return 4 * (wsum + _round4(nsum) + rows * (_round4(a) + _round4(b)))


def stage_is_small(f: int, widths) -> bool:
    """Does the stage pass the default bounds (and so run the 256-thread kernel it always ran)?"""
    return (1 <= f <= MAX_F and 1 <= len(widths) <= MAX_DENSE_LAYERS and all(1 <= n <= SMALL_HIDDEN for n in widths[:-1])
            and 1 <= widths[-1] <= MAX_LAST and stage_lds_bytes(f, widths) <= SMALL_LDS)


def stage_threads(f: int, widths, limit: int) -> int:
    """The launcher's workgroup size ("generic_stage_threads_<s>"): 256 for a small stage, else the largest of 1024 / 512 / 256
    whose layout fits the limit."""
    if stage_is_small(f, widths):
        return 256
    for t in (1024, 512, 256):
        if stage_lds_bytes(f, widths, t // 16) <= limit:
            return t
    raise ValueError("not admitted")


class Family:
    """One family of models.  FAMILY is name -> a function that gives the member's text, as tools/modelgen.FAMILY."""

    def __init__(self, prefix: str, tag: int, order, specs, seeds=None, borrowed=None):
        self.prefix, self.tag, self.order, self.specs = prefix, tag, order, specs
        self.seeds = seeds if seeds is not None else {name: 0 for name in specs}
        self.borrowed = borrowed or {}            # name -> the family whose member (text and weights) this one is
        self.FAMILY = {name: (lambda name=name: self.build(name)) for name in specs}

    def stage_widths(self, name: str):
        """[(f, last width)] per stage: what gnnvc_stage_widths reports."""
        f, stages = self.specs[name]
        out = []
        for ws in stages:
            out.append((f, ws[-1]))
            f = ws[-1]
        return out

    def stage_depths(self, name: str):
        """Dense layers per stage: what gnnvc_get_info "generic_stage_layers_<s>" reports."""
        return [len(ws) for ws in self.specs[name][1]]

    def linear_shapes(self, name: str):
        """(k, n) of every linear layer, in order."""
        f, stages = self.specs[name]
        out = []
        for ws in stages:
            k = 2 * f + 3
            for n in ws:
                out.append((k, n))
                k = n
            f = ws[-1]
        return out

    def in_width(self, name: str) -> int:
        return self.specs[name][0]

    def out_width(self, name: str) -> int:
        return self.specs[name][1][-1][-1]

    def num_layers(self, name: str) -> int:
        return sum(1 + 2 * len(ws) for ws in self.specs[name][1])

    def lds_bytes(self, name: str, rows: int = 16):
        """Per stage: what gnnvc_get_info "generic_stage_lds_bytes_<s>" reports (rows = 16)."""
        return [stage_lds_bytes(f, ws, rows) for (f, _), ws in zip(self.stage_widths(name), self.specs[name][1])]

    def layers_of(self, name: str, seed: int | None = None):
        if name in self.borrowed:
            return self.borrowed[name].layers_of(name, seed)
        seed = self.seeds[name] if seed is None else seed
        return draw(np.random.default_rng([self.tag, self.order(self.specs).index(name), seed]), self.linear_shapes(name))

    def build(self, name: str, seed: int | None = None) -> str:
        if name in self.borrowed:
            return self.borrowed[name].build(name, seed)
        seed = self.seeds[name] if seed is None else seed
        return model_text(self.layers_of(name, seed), self.stage_depths(name), f"{self.prefix}_{name}_{seed}")

    def model_input(self, name: str, g) -> np.ndarray:
        """The forward's input for graph g: x = W / ws, n x 1 — and for a model of input width w > 1 the columns
        x, 0.37 x, 1 - x, ... (n x w), so that no two columns carry the same values."""
        x = np.ascontiguousarray(g.x(), dtype=np.float32).reshape(g.n, 1)
        w = self.in_width(name)
        if w == 1:
            return x
        cols = [x, (x * np.float32(0.37)).astype(np.float32), (np.float32(1.0) - x).astype(np.float32)]
        while len(cols) < w:
            cols.append((x * np.float32(len(cols))).astype(np.float32))
        return np.ascontiguousarray(np.concatenate(cols[:w], axis=1), dtype=np.float32)

    def main(self, argv):
        """python -m tools.modelgen_<family> <member>: the member's text on stdout."""
        import sys
        sys.stdout.write(self.FAMILY[argv[1]]())


if __name__ == "__main__":
    import importlib
    import sys
    importlib.import_module(f"tools.modelgen_{sys.argv[1]}").family.main(sys.argv[1:])
