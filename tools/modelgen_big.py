"""Synthetic models whose stages lie OUTSIDE the default bounds of the generic fused stage (k_stage_any: hidden widths <= 64, a
stage's LDS layout within 64 KiB) and inside — or just outside — the opt-in ones of gnnvc_set_generic_big_stages (hidden widths
<= 128, the layout at 256 threads within the limit passed, at most 163 840 bytes), from seeds.

This module is the family's table of members.  The text format, the weight draw, the model's input, every function over the
table and the Python restatement of the kernel's LDS layout (stage_lds_bytes, stage_is_small, stage_threads and their constants)
are tools/modelgen_generic.py's, shared with tools/modelgen_shapes.py and tools/modelgen_depths.py; the names below are this
family's instances of them.  `too_big` IS tools/modelgen_depths.py's too_big, text and weights, so both families mean the same
model.

That the logits of every member vary over the vertices and are finite is asserted on oracle outputs by
tests/test_modelgen_big.py, not assumed here; a member that turned out dead gets another seed in SEEDS, not a lower bar.
"""
from __future__ import annotations

import sys

from tools import modelgen_depths as md
from tools.modelgen_generic import (MAX_LDS, SMALL_LDS, Family,   # noqa: F401  (what this family's callers read here)
                                    stage_is_small, stage_lds_bytes, stage_threads)

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

# rng seed list [17, list(SPECS).index(name), seed], first line big_<name>_<seed>; too_big is modelgen_depths' member
family = Family("big", 17, list, SPECS, SEEDS, borrowed={"too_big": md.family})
FAMILY, build, layers_of, model_input = family.FAMILY, family.build, family.layers_of, family.model_input
stage_widths, stage_depths, linear_shapes = family.stage_widths, family.stage_depths, family.linear_shapes
in_width, out_width, num_layers, lds_bytes = family.in_width, family.out_width, family.num_layers, family.lds_bytes

if __name__ == "__main__":
    family.main(sys.argv)
