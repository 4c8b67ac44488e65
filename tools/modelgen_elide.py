"""A synthetic model of the trained shape whose INPUT x decides which columns of h1 are live, for the forwards in which the
compact-table plan's producers leave out full feature rows (tests/test_gpu_elided_rows.py; csrc/gnnvc_kernels.hip: kSkipElide).

  gated(d_low, d_high)
      tools/modelgen_mask.emit_strays(d_low, d_high) — h1 and h2 keep to the columns modelgen_units.LIVE, a few vertices light
      column STRAY outside them, h2 holds a NaN inside them — with two more units in stage 0:
        GATE   relu(x), handed unchanged to column GATED of h1 (one of LIVE), which is nothing else: an input of zeros leaves that
               column dead in every row and another column takes its place among the four fullest — a choice that still fits;
        FIFTH  relu(x - 2) into column EXTRA (outside LIVE): zero for the driver's input (x = W / ws <= 1), positive in every row
               for x = 3: a fifth live column, more stray values than the plan takes.
      Weights are finite everywhere, so every layer may skip.

What the names promise is asserted on oracle outputs by the test that uses them."""
from __future__ import annotations

import numpy as np

from oracle import oracle_py
from tools import modelgen as mg
from tools import modelgen_mask as mm

GATE, FIFTH = 29, 30
GATED, EXTRA = 12, 7
X_COLUMN = 1            # of the first linear layer's input: [aggregate, x, degree, W/ws, NW/ws]


def gated(d_low: int, d_high: int, seed: int = 1) -> str:
    L = [(W.copy(), b.copy()) for W, b in oracle_py.OracleModel(mm.emit_strays(d_low, d_high, seed)).linear_params()]
    mg._pass_through(L, 0, GATE, {X_COLUMN: 1.0}, 0.0)
    mg._pass_through(L, 0, FIFTH, {X_COLUMN: 1.0}, -2.0)
    W, b = L[2]
    W[GATE, :] = 0.0
    W[FIFTH, :] = 0.0
    W[:, GATED] = 0.0
    W[GATE, GATED] = 1.0
    b[GATED] = np.float32(0.0)
    W[FIFTH, EXTRA] = 1.0            # (the column's bias is in [-0.5, -0.05]: x - 2 = 1 clears it)
    return mg.model_text(L, f"gated_{d_low}_{d_high}_{seed}")
