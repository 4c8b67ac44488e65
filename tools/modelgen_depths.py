"""Synthetic models whose stages have OTHER DEPTHS than the trained one's three dense layers, for the generic fused stage
(k_stage_any), from seeds.

This module is the family's table of members: per stage d layer widths, 1 <= d <= 6 and d free per stage.  The text format,
the weight draw, the model's input and every function over the table (stage_widths, stage_depths, linear_shapes, build,
model_input, ...) are tools/modelgen_generic.py's, shared with tools/modelgen_shapes.py and tools/modelgen_big.py; the names
below are this family's instances of them.

That the logits of every member vary over the vertices and are finite is asserted on oracle outputs by
tests/test_modelgen_depths.py, not assumed here; a member that turned out dead gets another seed in SEEDS, not a lower bar.
"""
from __future__ import annotations

import sys

from tools.modelgen_generic import MAX_DENSE_LAYERS, Family   # noqa: F401  (MAX_DENSE_LAYERS: what this family's callers read here)

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

family = Family("depths", 13, list, SPECS, SEEDS)   # rng seed list [13, list(SPECS).index(name), seed], first line depths_<name>_<seed>
FAMILY, build, layers_of, model_input = family.FAMILY, family.build, family.layers_of, family.model_input
stage_widths, stage_depths, linear_shapes = family.stage_widths, family.stage_depths, family.linear_shapes
in_width, out_width, num_layers = family.in_width, family.out_width, family.num_layers

if __name__ == "__main__":
    family.main(sys.argv)
