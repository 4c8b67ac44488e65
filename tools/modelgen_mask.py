"""Synthetic models of the trained shape for the liveness mask the dense kernels hand from layer to layer (relu_live / dense_live
in csrc/gnnvc_kernels.hip) and for the compact-table emit (c4_emit_regs).  Same text format as tools/modelgen.py; h1 and h2 keep
to the four columns tools/modelgen_units.LIVE, so that the compact-table plan's k_dense_f16 runs the 16-wide stages' dense layers.

  mask_units  in every layer whose ReLU output a skipped chain multiplies (modelgen_units.FEEDERS) three units sit on the edges
              of "can be non-zero in some lane":
                ZERO  all-zero weights and a +0.0 bias: the pre-activation is exactly +0.0 in every row — live for the mask
                      (!(t < 0)), dead for a test of the values;
                NEG   weights < 0 on inputs >= 0 and a bias < 0: negative in every row, dead either way;
                MIX   64 * (W/ws) - 64: exactly +0.0 for the vertices of weight ws (one in a hundred with the generators'
                      weights, uniform integers in [20, 120] at ws = 120) and negative for all others, so a wave with such a
                      row has the unit live for the mask although every lane's value is zero.  In the 32 -> 32 layers W/ws
                      arrives through unit CARRY of the layer before (relu(W/ws) = W/ws).
  emit_strays(d_low, d_high)
              the rows a stage hands to the compact table with a few values outside the table's columns and, in h2, a NaN
              inside them.  Vertices of weight ws and degree <= d_low light column STRAY (outside LIVE) of h1 and of h2; vertices
              of weight ws and degree >= d_high get an infinite unit in stage 1's second layer whose weight row in the third is
              0 for column NAN_COL of LIVE (inf * 0 = NaN) and -1 elsewhere (-inf, zero after the ReLU): h2 has a NaN in that
              one table column and nothing else changes.  (h1 gets no NaN: a NaN in h1 makes all sixteen values of every
              neighbour's h2 row NaN, twelve stray values a row — more than the plan takes, n / 512.)  The caller picks the two
              degrees for its graph; weights are finite everywhere, so every layer may skip.

What the names promise is asserted on oracle outputs by the tests that use them (tests/test_gpu_live_mask.py)."""
from __future__ import annotations

import numpy as np

from tools import modelgen as mg
from tools import modelgen_units as mu

ZERO, NEG, MIX, CARRY = 5, 11, 19, 23
STRAY, NAN_COL = 6, 9
SEL_LOW, SEL_HIGH, BLOWN = 3, 13, 27   # units of emit_strays


def _w_column(layer: int) -> int:
    return 3 if layer == 0 else 18


def _deg_column(layer: int) -> int:
    return 2 if layer == 0 else 17


def mask_units(seed: int = 1) -> str:
    rng = np.random.default_rng([11, seed])
    L = mg._uniform(rng, 0.2)
    mu._four_columns(rng, L)
    for i in mu.FEEDERS:
        W, b = L[i]
        W[:, ZERO] = 0.0
        b[ZERO] = np.float32(0.0)
        W[:, NEG] = -np.abs(W[:, NEG]) - np.float32(0.01)
        b[NEG] = np.float32(-0.5)
        W[:, MIX] = 0.0
        b[MIX] = np.float32(-64.0)
        if i in (0, 3, 6):
            W[_w_column(i), MIX] = 64.0
        else:
            W[CARRY, MIX] = 64.0
        if i in (0, 3):
            W[:, CARRY] = 0.0
            W[_w_column(i), CARRY] = 1.0
            b[CARRY] = np.float32(0.0)
    return mg.model_text(L, f"mask_units_{seed}")


def _select_low(L, first, unit, d_low):
    """Unit `unit` of layers first and first + 1: positive (>= 0.005) for weight ws and degree <= d_low, zero otherwise."""
    mg._pass_through(L, first, unit, {_w_column(first): 64.0, _deg_column(first): -0.01}, -(64.0 - 0.01 * d_low - 0.005))


def emit_strays(d_low: int, d_high: int, seed: int = 1) -> str:
    rng = np.random.default_rng([12, seed])
    L = mg._uniform(rng, 0.2)
    mu._four_columns(rng, L)
    for first in (0, 3):
        _select_low(L, first, SEL_LOW, d_low)
        W, b = L[first + 2]
        W[SEL_LOW, :] = 0.0
        W[SEL_LOW, STRAY] = 1000.0          # (the column's bias is in [-0.5, -0.05]: 0.005 * 1000 clears it)
    # stage 1: SEL_HIGH of its first layer is positive for weight ws and degree >= d_high (steps of 1e26 a degree against 8.3e27
    # a unit of weight), BLOWN of its second layer is that times 1e30: infinite
    W3, b3 = L[3]
    W3[:, SEL_HIGH] = 0.0
    W3[_w_column(3), SEL_HIGH] = 1e30
    W3[_deg_column(3), SEL_HIGH] = 1e26
    b3[SEL_HIGH] = -(1e30 + 1e26 * d_high - 0.5e26)
    W4, b4 = L[4]
    W4[SEL_HIGH, :] = 0.0
    W4[:, BLOWN] = 0.0
    W4[SEL_HIGH, BLOWN] = 1e30
    b4[BLOWN] = 0.0
    W5, _ = L[5]
    W5[BLOWN, :] = -1.0
    W5[BLOWN, NAN_COL] = 0.0
    return mg.model_text(L, f"emit_strays_{d_low}_{d_high}_{seed}")


FAMILY = {"mask_units": mask_units}


if __name__ == "__main__":
    import sys
    sys.stdout.write(FAMILY[sys.argv[1]]())
