"""Synthetic models whose stages lie OUTSIDE the default bounds of the generic fused stage (k_stage_any: hidden widths <= 64, a
stage's LDS layout within 64 KiB) and inside — or just outside — the opt-in ones of gnnvc_set_generic_big_stages (hidden widths
<= 128, the layout at 256 threads within the limit passed, at most 163 840 bytes), from seeds.

Same text format and the same weight draw as tools/modelgen_depths.py (its model_text and its draw, imported); `too_big` IS that
file's too_big, so both families mean the same weights.

stage_lds_bytes restates the kernel's LDS layout (stage_any_layout of csrc/gnnvc_stage_any.hip) in Python: the layers' transposed
weights at a pitch of an odd number of 16-byte slots, the biases, then per row of a pass two vectors A and B.

That the logits of every member vary over the vertices and are finite is asserted on oracle outputs by
tests/test_modelgen_big.py, not assumed here; a member that turned out dead gets another seed in SEEDS, not a lower bar.
"""
from __future__ import annotations

import numpy as np

from tools import modelgen_depths as md
from tools.modelgen_depths import draw, model_text

# name -> (input width, [layer widths per stage])
SPECS = {
    "too_big": md.SPECS["too_big"],                                  # the LDS bound only: widths <= 64
    "h128": (1, [(128, 128, 16), (128, 64, 1)]),                     # 128-wide layers; stage 1 is 32 bytes over 64 KiB
    "odd_wide": (3, [(97, 65, 32), (113, 80, 7, 1)]),                # no multiples of 16 on either side of 64; stage 0 fits 64 KiB but
                                                                     # needs the wide loop; f = 32 in stage 1
    "edge": (1, [(128, 128, 106, 32), (1,)]),                        # fits 163 840 bytes at 256 threads only; stage 1 runs the small kernel
    "over": (1, [(128, 128, 128, 32), (128, 1)]),                    # admitted at no limit: stays layer by layer
}
ADMITTED = ["too_big", "h128", "odd_wide", "edge"]                   # fused under set_generic_big_stages(163840)
NOT_FITTING = ["over"]

# seed per member (changed here, and only here, if a member's logits turn out dead)
SEEDS = {name: 0 for name in SPECS}

SMALL_LDS, MAX_LDS = 64 * 1024, 160 * 1024
SMALL_HIDDEN, BIG_HIDDEN, MAX_LAST, MAX_F = 64, 128, 32, 32


def stage_widths(name: str):
    """[(f, last width)] per stage: what gnnvc_stage_widths reports."""
    f, stages = SPECS[name]
    out = []
    for ws in stages:
        out.append((f, ws[-1]))
        f = ws[-1]
    return out


def stage_depths(name: str):
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


def _round4(v: int) -> int:
    return (v + 3) // 4 * 4


def _pitch(k: int) -> int:
    return 4 * (((k + 3) // 4) | 1)


def stage_lds_bytes(f: int, widths, rows: int = 16) -> int:
    """stage_any_layout(...).total * 4 for a stage of input width f and these layer widths, `rows` rows a pass (threads / 16)."""
    k, wsum, nsum, a, b = 2 * f + 3, 0, 0, 2 * f + 3, 0
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


def lds_bytes(name: str, rows: int = 16):
    """Per stage: what gnnvc_get_info "generic_stage_lds_bytes_<s>" reports (rows = 16)."""
    return [stage_lds_bytes(f, ws, rows) for (f, _), ws in zip(stage_widths(name), SPECS[name][1])]


def stage_is_small(f: int, widths) -> bool:
    """Does the stage pass the default bounds (and so run the 256-thread kernel it always ran)?"""
    return (1 <= f <= MAX_F and 1 <= len(widths) <= md.MAX_DENSE_LAYERS and all(1 <= n <= SMALL_HIDDEN for n in widths[:-1])
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


def layers_of(name: str, seed: int | None = None):
    if name == "too_big":
        return md.layers_of(name, seed)
    seed = SEEDS[name] if seed is None else seed
    return draw(np.random.default_rng([17, list(SPECS).index(name), seed]), linear_shapes(name))


def build(name: str, seed: int | None = None) -> str:
    if name == "too_big":
        return md.build(name, seed)
    seed = SEEDS[name] if seed is None else seed
    return model_text(layers_of(name, seed), stage_depths(name), f"big_{name}_{seed}")


FAMILY = {name: (lambda name=name: build(name)) for name in SPECS}


def model_input(name: str, g) -> np.ndarray:
    """As tools/modelgen_depths.model_input: x = W / ws, and for an input width w > 1 the columns x, 0.37 x, 1 - x, ..."""
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
