"""Synthetic models of the trained shape (tools/modelgen.SHAPES) built for the edges of the hidden-unit skip (dense_live in
csrc/gnnvc_kernels.hip): a term of a hidden layer's fma chains is left out when its input unit is zero in all 64 rows of a wave.

The skipped layers are the 32 -> 32 and 32 -> 16 layers of stages 0 and 1 and the 32 -> 16 layer of stage 2: linear layers
1, 2, 4, 5 and 7 of the nine (SKIPPED).  What a chain multiplies is the ReLU output of the layer before: layers 0, 1, 3, 4, 6
(FEEDERS).  Same text format and the same printing of values as tools/modelgen.py.

  one_row     (a) unit UNIT of every feeder is 64 * (W/ws - 119.5/120) after its ReLU: non-zero for the vertices of weight 120
              only (one in a hundred with the generators' weights, uniform integers in [20, 120] at ws = 120), so that some
              group of 64 consecutive rows holds exactly one such row — the term that must NOT be skipped — and others none.
              The unit's row of the next layer keeps its random weights (for the 32 -> 32 layers: a pass-through to the same
              unit of the 32 -> 16 layer's input), so leaving the term out changes that row's output.
  all_dead    (b) every unit of layers 0 and 4 is zero for every row (weights <= 0 on inputs >= 0, biases <= 0, some of them
              0): every term of layers 1 and 5 is skipped and their outputs are relu(bias).
  all_live    (c) every unit of every feeder is positive for every row (weights >= 0, biases > 0): nothing is skipped.
  neg_zero_bias  (d) a bias with the bits of -0.0f in layer 2 (stage 0's 32 -> 16) and in layer 3 (stage 1's first layer):
              the engine must refuse the skip for those two layers.
  inf_weight  (e) W[UNIT][5] = +inf in layer 7 (stage 2's 32 -> 16), on the row of a unit of layer 6 that is dead for every
              vertex: 0 * inf is NaN, so every logit is NaN and h1, h2 are finite — and the engine must refuse the skip for
              that layer (a skipped term would lose the NaN).

Every model keeps h1 and h2 to the four columns LIVE (the other twelve columns of layers 2 and 5 are zero and their biases
not positive, modelgen._restrict), so that both inputs of the 16-wide stages fit one four-column table of the compact-table plan
(k_c4_choose: at most n / 512 non-zeros outside the four fullest columns) and the plan's k_dense_f16 — not the gathering tile
kernel — runs their dense layers.

What (a), (b), (c) and the four columns promise is asserted on oracle outputs by tests/test_modelgen_units.py, not assumed from
the construction.
"""
from __future__ import annotations

import numpy as np

from tools import modelgen as mg

SKIPPED = (1, 2, 4, 5, 7)    # linear layers whose zero terms the kernels may leave out
FEEDERS = (0, 1, 3, 4, 6)    # the layers whose ReLU outputs those chains multiply
UNIT = 7
HEAVIEST = 119.5 / 120.0     # between the two largest values of W/ws
# bit 3 s + l of gnnvc_get_info "dense_skip_layers": dense layer l + 1 of stage s may leave out its zero terms
ALL_LAYERS = 0o777


LIVE = (2, 4, 9, 12)         # the columns of h1 and h2 that may be non-zero


def _four_columns(rng, L):
    for i in (2, 5):
        mg._restrict(rng, *L[i], np.asarray(LIVE))


def _w_column(layer: int) -> int:
    """Column of W/ws in the input of the first linear layer of a stage (modelgen's module text)."""
    return 3 if layer == 0 else 18


def one_row(seed: int = 1) -> str:
    rng = np.random.default_rng([5, seed])
    L = mg._uniform(rng, 0.2)
    _four_columns(rng, L)
    for first in (0, 3):
        mg._pass_through(L, first, UNIT, {_w_column(first): 64.0}, -64.0 * HEAVIEST)
        L[first + 2][0][UNIT, list(LIVE)] = rng.uniform(0.5, 1.0, len(LIVE)).astype(np.float32)
    W6, b6 = L[6]
    W6[:, UNIT] = 0.0
    W6[18, UNIT] = 64.0
    b6[UNIT] = -64.0 * HEAVIEST
    L[7][0][UNIT, :] = rng.uniform(0.5, 1.0, 16).astype(np.float32)
    return mg.model_text(L, f"units_one_row_{seed}")


def all_dead(seed: int = 1) -> str:
    rng = np.random.default_rng([6, seed])
    L = mg._uniform(rng, 0.2)
    _four_columns(rng, L)
    for i in (0, 4):
        W, b = L[i]
        W[:] = -np.abs(W)
        b[:] = -np.abs(b)
        b[::5] = 0.0
    # (relu(bias) of layers 1 and 5 is what the rest of the model sees: half of those biases positive)
    return mg.model_text(L, f"units_all_dead_{seed}")


def all_live(seed: int = 1) -> str:
    rng = np.random.default_rng([7, seed])
    L = mg._uniform(rng, 0.06)
    _four_columns(rng, L)
    for i in FEEDERS:
        W, b = L[i]
        W[:] = np.abs(W)
        b[:] = np.abs(b) + np.float32(0.01)
    return mg.model_text(L, f"units_all_live_{seed}")


def neg_zero_bias(seed: int = 1) -> str:
    rng = np.random.default_rng([8, seed])
    L = mg._uniform(rng, 0.2)
    _four_columns(rng, L)
    L[2][1][3] = np.float32(-0.0)        # (a dead column's bias: not positive)
    L[3][1][11] = np.float32(-0.0)
    return mg.model_text(L, f"units_neg_zero_bias_{seed}")


def inf_weight(seed: int = 1) -> str:
    rng = np.random.default_rng([9, seed])
    L = mg._uniform(rng, 0.2)
    _four_columns(rng, L)
    W6, b6 = L[6]
    W6[:, UNIT] = -np.abs(W6[:, UNIT])   # (its inputs are sums of ReLU outputs, ReLU outputs, degree and weights: none negative)
    b6[UNIT] = -1.0
    L[7][0][UNIT, 5] = np.inf
    return mg.model_text(L, f"units_inf_weight_{seed}")


FAMILY = {
    "one_row": one_row,
    "all_dead": all_dead,
    "all_live": all_live,
    "neg_zero_bias": neg_zero_bias,
    "inf_weight": inf_weight,
}
# the layers the engine may skip in, as "dense_skip_layers" reports them
SKIP_LAYERS = {
    "one_row": ALL_LAYERS,
    "all_dead": ALL_LAYERS,
    "all_live": ALL_LAYERS,
    "neg_zero_bias": ALL_LAYERS & ~(1 << 2) & ~(1 << 3),
    "inf_weight": ALL_LAYERS & ~(1 << 7),
}


if __name__ == "__main__":
    import sys
    sys.stdout.write(FAMILY[sys.argv[1]]())
