"""Synthetic models for the live-column gather of the generic fused stage (gnnvc_set_generic_live_columns: a graph stage gathers
only the columns of its input that are not +-0.0 in every row), from seeds.

Two kinds of members:
  in<w>      (w, [(16, 8), (8, 1)]) — a stage 0 whose n x w input is the test's own: the tests overwrite columns of it so that
             exactly the columns they choose are live.  w = 2, 16, 17, 32 run within the default bounds; w = 33, 48, 49, 64 need
             gnnvc_set_generic_feature_width(64) (the FEAT instantiations, three and four columns a lane);
  sparse32   (1, [(64, 32), (64, 32), (32, 1)]) — dead output units BY CONSTRUCTION: DEAD_UNITS (24 of the 32) of both 32-wide last
             layers have their weight column zeroed and their bias made <= 0 (every third of them -0.0f), so that stages 1 and 2 see
             at most 8 live columns of 32 whatever the graph.

This module is the family's table of members and one override: the weight draw is tools/modelgen_generic.py's, sparse32's dead
units are cut out of it afterwards (layers_of).  The text format, the model's input and every function over the table are the
shared ones.  tests/test_modelgen_live.py pins the texts and, on the oracle, the masks the GPU tests expect.
"""
from __future__ import annotations

import sys

import numpy as np

from tools.modelgen_generic import Family

# name -> (input width, [layer widths per stage]); the last of a stage's widths is the next stage's f
SPECS = {
    "in2": (2, [(16, 8), (8, 1)]),
    "in16": (16, [(16, 8), (8, 1)]),
    "in17": (17, [(16, 8), (8, 1)]),
    "in32": (32, [(16, 8), (8, 1)]),
    "in33": (33, [(16, 8), (8, 1)]),
    "in48": (48, [(16, 8), (8, 1)]),
    "in49": (49, [(16, 8), (8, 1)]),
    "in64": (64, [(16, 8), (8, 1)]),
    "sparse32": (1, [(64, 32), (64, 32), (32, 1)]),
}
DEFAULT_BOUNDS = ["in2", "in16", "in17", "in32", "sparse32"]   # fused as they are
NEEDS_FEAT = ["in33", "in48", "in49", "in64"]                  # ... under set_generic_feature_width(64)

# sparse32: the output units of each 32-wide last layer that can never fire (24 of 32; 1, 6, 9, 14, 17, 22, 25, 30 stay)
DEAD_UNITS = [u for u in range(32) if u % 8 not in (1, 6)]
MINUS_ZERO_BIAS = DEAD_UNITS[::3]                              # ... and those among them whose bias is -0.0f


class LiveFamily(Family):
    def layers_of(self, name: str, seed: int | None = None):
        layers = super().layers_of(name, seed)
        if name != "sparse32":
            return layers
        lasts = set((np.cumsum(self.stage_depths(name)) - 1).tolist())   # each stage's last layer
        out = []
        for i, (W, b) in enumerate(layers):
            if i in lasts and W.shape[1] == 32:
                W, b = W.copy(), b.copy()
                W[:, DEAD_UNITS] = np.float32(0.0)
                b[DEAD_UNITS] = -np.abs(b[DEAD_UNITS])
                b[MINUS_ZERO_BIAS] = np.float32(-0.0)
            out.append((W, b))
        return out


# rng seed list [37, list(SPECS).index(name), seed], first line live_<name>_<seed>
family = LiveFamily("live", 37, list, SPECS)
FAMILY, build, layers_of, model_input = family.FAMILY, family.build, family.layers_of, family.model_input
stage_widths, stage_depths, linear_shapes = family.stage_widths, family.stage_depths, family.linear_shapes
in_width, out_width, num_layers, lds_bytes = family.in_width, family.out_width, family.num_layers, family.lds_bytes


def live_mask(h) -> int:
    """The 64-bit mask of the live columns of the stage input h (n x f): bit c set iff some row has bits other than +-0.0 there."""
    h = np.ascontiguousarray(h, dtype=np.float32)
    if h.size == 0:
        return 0
    alive = ((h.view(np.uint32) & np.uint32(0x7FFFFFFF)) != 0).reshape(h.shape[0], -1).any(axis=0)
    return sum(1 << c for c in np.flatnonzero(alive).tolist())


def used_by_rule(kept: int, f: int, max_percent: int) -> int:
    """include/gnnvc.h's rule: the table is used iff kept * 100 <= max_percent * f."""
    return 1 if kept * 100 <= max_percent * f else 0


if __name__ == "__main__":
    family.main(sys.argv)
