"""Synthetic models of OTHER layer widths than the trained one, for the generic fused stage (k_stage_any), from seeds.

This module is the family's table of members.  The text format, the weight draw, the model's input and every function over the
table (stage_widths, linear_shapes, build, model_input, ...) are tools/modelgen_generic.py's, shared with
tools/modelgen_depths.py and tools/modelgen_big.py; the names below are this family's instances of them.

The layer pattern is the trained model's, (Graph, Linear, ReLU, Linear, ReLU, Linear, ReLU | Sigmoid) per stage with the sigmoid
on the last stage only; what varies is the number of stages, the widths (n1, n2, n3) of each stage's three linear layers, the
input width and the output width.

Random ReLU units die; that the logits of every member still vary over the vertices and are finite is asserted on oracle outputs
by tests/test_modelgen_shapes.py, not assumed here.

These models are kept out of modelgen.FAMILY on purpose: that family is the trained SHAPE under other weights (three stages,
21 layers), and its tests say so.
"""
from __future__ import annotations

import sys

from tools.modelgen_generic import Family

TRAINED = [(32, 32, 16), (32, 32, 16), (32, 16, 1)]

# name -> (input width, [(n1, n2, n3) per stage]): modelgen_generic's [layer widths per stage], three layers a stage
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

family = Family("shapes", 7, sorted, SPECS)   # rng seed list [7, sorted(SPECS).index(name), seed], first line shapes_<name>_<seed>
FAMILY, build, layers_of, model_input = family.FAMILY, family.build, family.layers_of, family.model_input
stage_widths, stage_depths, linear_shapes = family.stage_widths, family.stage_depths, family.linear_shapes
in_width, out_width, num_layers = family.in_width, family.out_width, family.num_layers

if __name__ == "__main__":
    family.main(sys.argv)
