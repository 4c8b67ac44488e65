"""Synthetic models whose FEATURE WIDTHS lie outside the default bounds of the generic fused stage (k_stage_any: a stage's feature
width f — the model's input width, for later stages the previous stage's last layer — and its own last layer at most 32) and
inside — or just outside — the opt-in ones of gnnvc_set_generic_feature_width (both at most the width passed, 33 .. 64), from seeds.

This module is the family's table of members.  The text format, the weight draw, the model's input, every function over the
table and the Python restatement of the kernel's LDS layout are tools/modelgen_generic.py's, shared with
tools/modelgen_shapes.py, tools/modelgen_depths.py and tools/modelgen_big.py; the names below are this family's instances of them.

That the logits of every member vary over the vertices and are finite is asserted on oracle outputs by
tests/test_modelgen_feat.py, not assumed here; a member that turned out dead gets another seed in SEEDS, not a lower bar.
"""
from __future__ import annotations

import sys

from tools.modelgen_generic import (BIG_HIDDEN, MAX_DENSE_LAYERS, MAX_LDS, SMALL_HIDDEN, SMALL_LDS, Family,   # noqa: F401
                                    stage_lds_bytes, stage_threads)

MAX_FEATURE_WIDTH, DEFAULT_FEATURE_WIDTH = 64, 32   # the most gnnvc_set_generic_feature_width takes, and the bound when it is off

# name -> (input width, [layer widths per stage]); the last of a stage's widths is the next stage's f
SPECS = {
    "f33": (1, [(16, 33), (16, 1)]),                      # one column in the third slot; a 33-wide last layer
    "f47": (1, [(24, 47), (24, 47), (8, 1)]),             # wide in and wide out in one stage
    "f48_49": (1, [(32, 48), (32, 49), (16, 1)]),         # three full slots, then a fourth with one column; 48 against 49
    "f64": (1, [(32, 64), (64, 64), (32, 1)]),            # the widest; stage 1 is 64 256 bytes at 256 threads, inside 64 KiB
    "in40": (40, [(32, 16), (16, 1)]),                    # a wide stage 0: n x 40 input
    "out64": (1, [(16, 16), (32, 64)]),                   # 64 sigmoid outputs: scores and logits n x 64
    "big_f64": (1, [(64, 64), (128, 64), (64, 1)]),       # needs big stages too: stage 1 is 118 784 bytes at 256 threads
    "f65": (1, [(32, 65), (16, 1)]),                      # admitted by no setting: stays layer by layer
}
ADMITTED = ["f33", "f47", "f48_49", "f64", "in40", "out64"]   # fused under set_generic_feature_width(64) alone
NEEDS_BIG = ["big_f64"]                                       # ... only with set_generic_big_stages as well
NOT_FITTING = ["f65"]

# seed per member (changed here, and only here, if a member's logits turn out dead)
SEEDS = {name: 0 for name in SPECS}

# rng seed list [23, list(SPECS).index(name), seed], first line feat_<name>_<seed>
family = Family("feat", 23, list, SPECS, SEEDS)
FAMILY, build, layers_of, model_input = family.FAMILY, family.build, family.layers_of, family.model_input
stage_widths, stage_depths, linear_shapes = family.stage_widths, family.stage_depths, family.linear_shapes
in_width, out_width, num_layers, lds_bytes = family.in_width, family.out_width, family.num_layers, family.lds_bytes


def feature_width_needed(name: str) -> int:
    """The widest f or last width of the member's stages: the least value of gnnvc_set_generic_feature_width that could admit it."""
    return max(max(f, last) for f, last in stage_widths(name))


def stage_fits(f: int, widths, feature_width: int = 0, limit: int = 0) -> bool:
    """stage_any_route's yes / no: feature_width as passed to gnnvc_set_generic_feature_width (0 = off), limit as passed to
    gnnvc_set_generic_big_stages (0 = off)."""
    fw = feature_width if DEFAULT_FEATURE_WIDTH < feature_width <= MAX_FEATURE_WIDTH else DEFAULT_FEATURE_WIDTH
    if not (1 <= f <= fw and 1 <= len(widths) <= MAX_DENSE_LAYERS and 1 <= widths[-1] <= fw):
        return False
    if not all(1 <= n <= BIG_HIDDEN for n in widths[:-1]):
        return False
    lds = stage_lds_bytes(f, widths)
    if all(n <= SMALL_HIDDEN for n in widths[:-1]) and lds <= SMALL_LDS:
        return True
    return SMALL_LDS <= limit <= MAX_LDS and lds <= limit


def stage_threads_feat(f: int, widths, limit: int = 0) -> int:
    """The launcher's workgroup size for an admitted stage ("generic_stage_threads_<s>"): 256 within the default LDS and
    hidden-width bounds, else the largest of 1024 / 512 / 256 whose layout fits the limit."""
    if all(n <= SMALL_HIDDEN for n in widths[:-1]) and stage_lds_bytes(f, widths) <= SMALL_LDS:
        return 256
    for t in (1024, 512, 256):
        if stage_lds_bytes(f, widths, t // 16) <= limit:
            return t
    raise ValueError("not admitted")


def model_fits(name: str, feature_width: int = 0, limit: int = 0) -> bool:
    return all(stage_fits(f, ws, feature_width, limit) for (f, _), ws in zip(stage_widths(name), SPECS[name][1]))


if __name__ == "__main__":
    family.main(sys.argv)
