"""Random generic-stage models, graphs and opt-ins: the case table of the generic path's differential fuzz
(tests/test_gpu_generic_fuzz.py against the oracle; tests/test_modelgen_fuzz.py pins the table and shows what it reaches).

case(i) is a pure function of i through np.random.default_rng([TAG, i]).  A case is a model — an input width, an optional dense
prologue of 1 .. 6 layers, 0 .. 4 graph stages of 1 .. 6 dense layers each (0 only behind a prologue), an ending "sigmoid", "relu"
or "none" — with widths drawn from edge values (LAST for the input width and every stage's last layer, HIDDEN for the layers
between), the least configuration that admits it (patterns mask, feature width, big-stage LDS limit) plus a drawn surplus, the
order in which the opt-ins are made and whether they are made before the graph or under it, a graph name, the heavy and giant
thresholds, and what the multi-device test and the stage-entry test draw.  About one case in seven is built so that NO setting
admits it (KINDS[1:]); it carries every opt-in at its most generous and must still run layer by layer.

What the engine must answer for a case is restated here in Python from include/gnnvc.h's rules (route, expect): per stage whether
it is dense, f, its widths, its end code, "generic_stage_lds_bytes_<s>", "generic_stage_threads_<s>", and whether its launches
are a BIG, a FEAT or an OPEN instantiation of k_stage_any.  tests/test_modelgen_fuzz.py holds that restatement to the figures
the big, feat and patterns families' own tests pin.

The text writer is tools/modelgen_patterns.model_text, the weight draw and the LDS layout tools/modelgen_generic's draw and
stage_lds_bytes; the model's input is Family.model_input's columns.  A case whose outputs turn out dead gets another seed in
SEEDS — never a lower bar; REGRESSIONS names cases beyond the first N that a long run (python -m tests.fuzz_harness) found.
"""
from __future__ import annotations

import sys
import types

import numpy as np

from tools import graphgen as gg
from tools.modelgen_generic import Family, draw, stage_lds_bytes
from tools.modelgen_patterns import END_NONE, END_RELU, END_SIGMOID, OPEN_END, PROLOGUE, model_text

TAG, PREFIX = 31, "fuzz"    # rng seed lists [31, i] (the case) and [31, i, seed] (its weights), first line fuzz_<i>_<seed>
N = 240                     # the cases tests/test_gpu_generic_fuzz.py runs: 0 .. N - 1, then REGRESSIONS

# (6 and 66 stand in the sets for the k loop of any_chains: no other value gives a layer K >= 4 with K mod 4 = 2 — a graph stage's
# first K, 2 f + 3, is odd — so without them the four-wide body followed by a scalar tail of two is never run)
LAST = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
HIDDEN = LAST + [65, 66, 96, 97, 113, 127, 128]
HEAVY = [0, 1, 17, 64, 512]
GIANT = [None, 1024, 2048]   # None: the engine's default (16 384: no giant row on these graphs)
SEGMENTS = [-1, 0, 1]
PARTS, PIECES, PUSH = [2, 3, 5, 8], [0, 1, 3, 8], [0, 1]
SETTERS = ["big", "feat", "mask", "heavy", "giant"]

# admitted, then the kinds that no setting admits
KINDS = ["admitted", "hidden129", "last65", "f65", "lds", "seven", "mid_sigmoid", "two_graphs"]
NOT_ADMITTED_SHARE = 0.15

# case -> seed of its weight draw (0 where absent); changed here, and only here, if a case's outputs turn out dead
SEEDS = {15: 1, 24: 1, 25: 1, 57: 1, 68: 1, 130: 1, 156: 1, 162: 1, 164: 1, 185: 1, 190: 3, 233: 1}
# cases beyond N that a long run found to mismatch: kept in the pinned table for good
REGRESSIONS = []

DEFAULT_F, FEAT_MAX, SMALL_HIDDEN, BIG_HIDDEN, MAX_DEPTH = 32, 64, 64, 128, 6
SMALL_LDS, FULL_LDS = 65536, 163840
_END = {"relu": END_RELU, "sigmoid": END_SIGMOID, "none": END_NONE}

# ---------------------------------------------------------------- graphs

# tests/generic_harness.GRAPHS' names, and the two graphs below (tests/fuzz_harness.py registers them there)
GRAPH_NAMES = ["er1933", "sparse", "hubs", "one", "empty", "tiny13", "rounds"]
_GRAPH_P = [0.16, 0.10, 0.26, 0.08, 0.08, 0.10, 0.22]
ROUND_DEGREES = [15, 16, 17, 31, 32, 33, 63, 64, 65]   # the round sizes of any_gather, any_gather_n and any_gather1, and one either side
ROUNDS_N = 12 * 64 + 9


def tiny13():
    """13 vertices — fewer rows than one 16-row pass — with a row of no entry (vertex 12)."""
    edges = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 9), (9, 10),
             (10, 11), (1, 11), (2, 9)]
    return gg.from_edge_list(13, edges, np.random.default_rng([TAG, 13]).integers(20, 121, size=13))


def rounds():
    """777 vertices, hubs 0 .. 8 of exactly ROUND_DEGREES entries, neighbours and a sparse background among the other vertices only."""
    rng = np.random.default_rng([TAG, 777])
    nh = len(ROUND_DEGREES)
    others = np.arange(nh, ROUNDS_N)
    edges = []
    for h, d in enumerate(ROUND_DEGREES):
        edges += [(h, int(v)) for v in rng.choice(others, size=d, replace=False)]
    edges += list(zip(rng.integers(nh, ROUNDS_N, size=900).tolist(), rng.integers(nh, ROUNDS_N, size=900).tolist()))
    return gg.from_edge_list(ROUNDS_N, edges, rng.integers(20, 121, size=ROUNDS_N))


NEW_GRAPHS = {"tiny13": tiny13, "rounds": rounds}

# ---------------------------------------------------------------- the engine's rules, restated


def route(dense, f, widths, end, model_last, mask=0, feature_width=0, big_lds=0):
    """What include/gnnvc.h says of one stage under a configuration: None if it is not admitted, else a record of
    lds_bytes ("generic_stage_lds_bytes_<s>": the layout at 256 threads), threads ("generic_stage_threads_<s>"), and big / feat /
    open — which instantiation of k_stage_any its launches are."""
    fw = feature_width if DEFAULT_F < feature_width <= FEAT_MAX else DEFAULT_F
    if not (1 <= f <= fw and 1 <= len(widths) <= MAX_DEPTH):
        return None
    if not (all(1 <= n <= BIG_HIDDEN for n in widths[:-1]) and 1 <= widths[-1] <= fw):
        return None
    if dense and not mask & PROLOGUE:
        return None
    if end != (END_SIGMOID if model_last else END_RELU) and not (model_last and mask & OPEN_END):
        return None
    first_k = f if dense else 0
    lds256 = stage_lds_bytes(f, widths, 16, first_k=first_k)
    r = types.SimpleNamespace(lds_bytes=lds256, threads=256, big=False, feat=f > DEFAULT_F or widths[-1] > DEFAULT_F,
                              open=bool(dense) or end == END_NONE)
    if all(n <= SMALL_HIDDEN for n in widths[:-1]) and lds256 <= SMALL_LDS:
        return r    # within the default bounds: the kernels it always ran, whatever the big-stage limit says
    if not (SMALL_LDS <= big_lds <= FULL_LDS) or lds256 > big_lds:
        return None
    r.big = True
    r.threads = next((t for t in (1024, 512) if stage_lds_bytes(f, widths, t // 16, first_k=first_k) <= big_lds), 256)
    return r


def blocks_of(in_width, prologue, stages, ending):
    """[(dense, f, widths, end code, is the model's last)] per stage: the dense stage first where there is one."""
    blocks = ([(1, tuple(prologue))] if prologue else []) + [(0, tuple(ws)) for ws in stages]
    out, f = [], in_width
    for b, (dense, ws) in enumerate(blocks):
        last = b + 1 == len(blocks)
        out.append((dense, f, ws, _END[ending] if last else END_RELU, last))
        f = ws[-1]
    return out


def expect(in_width, prologue, stages, ending, mask=0, feature_width=0, big_lds=0):
    """Per stage: route's record with dense, f, widths and end added — or None if one stage is not admitted (the whole model
    then runs layer by layer)."""
    out = []
    for dense, f, ws, end, last in blocks_of(in_width, prologue, stages, ending):
        r = route(dense, f, ws, end, last, mask, feature_width, big_lds)
        if r is None:
            return None
        r.dense, r.f, r.widths, r.end = dense, f, ws, end
        out.append(r)
    return out or None


def least_config(in_width, prologue, stages, ending):
    """(mask, feature_width, big_lds): the least of each opt-in under which the model is admitted; None if under none."""
    if expect(in_width, prologue, stages, ending, PROLOGUE | OPEN_END, FEAT_MAX, FULL_LDS) is None:
        return None
    blocks = blocks_of(in_width, prologue, stages, ending)
    mask = (PROLOGUE if prologue else 0) | (OPEN_END if ending != "sigmoid" else 0)
    widest = max(max(f, ws[-1]) for _, f, ws, _, _ in blocks)
    feat = widest if widest > DEFAULT_F else 0
    full = expect(in_width, prologue, stages, ending, mask, feat, FULL_LDS)
    big = max([max(SMALL_LDS, r.lds_bytes) for r in full if r.big], default=0)
    assert expect(in_width, prologue, stages, ending, mask, feat, big) is not None
    return mask, feat, big


# ---------------------------------------------------------------- the draw

def sequence_of(prologue, stages, ending):
    """The layer sequence in tools/modelgen_patterns.py's notation (G, L<n>, R, S)."""
    out = []
    for b, ws in enumerate(([list(prologue)] if prologue else []) + [list(ws) for ws in stages]):
        if not (prologue and b == 0):
            out.append("G")
        for n in ws:
            out += [f"L{n}", "R"]
    out.pop()   # the model's last activation
    if ending != "none":
        out.append("S" if ending == "sigmoid" else "R")
    return out


def linear_shapes(in_width, seq):
    """(k, n) of every linear layer of a sequence, in order."""
    w, out = in_width, []
    for tok in seq:
        if tok == "G":
            w = 2 * w + 3
        elif tok[0] == "L":
            out.append((w, int(tok[1:])))
            w = int(tok[1:])
    return out


def _pick(rng, values, p=None):
    p = None if p is None else np.asarray(p, dtype=np.float64) / np.sum(p)
    return values[int(rng.choice(len(values), p=p))]


def _draw_model(rng):
    """(in_width, prologue or None, stages, ending) that some configuration admits."""
    while True:
        wide_hidden, wide_feat = rng.random() < 0.5, rng.random() < 0.5
        last_set = LAST if wide_feat else [v for v in LAST if v <= DEFAULT_F]
        hid_set = HIDDEN if wide_hidden else [v for v in HIDDEN if v <= SMALL_HIDDEN]
        hid_p = [0.3 if v <= 3 else 1.0 for v in hid_set]   # (a ReLU behind one to three units is mostly a dead one)
        in_width = 1 if rng.random() < 0.12 else _pick(rng, last_set)
        has_pro = rng.random() < 0.35
        depth = lambda: _pick(rng, [1, 2, 3, 4, 5, 6], [0.22, 0.24, 0.2, 0.12, 0.1, 0.12])
        block = lambda: tuple([_pick(rng, hid_set, hid_p) for _ in range(depth() - 1)] + [_pick(rng, last_set)])
        prologue = block() if has_pro else None
        n_stages = _pick(rng, [0, 1, 2, 3, 4], [0.15, 0.3, 0.25, 0.15, 0.15]) if has_pro else _pick(rng, [1, 2, 3, 4], [0.3, 0.3, 0.2, 0.2])
        stages = [block() for _ in range(n_stages)]
        ending = _pick(rng, ["sigmoid", "relu", "none"], [0.45, 0.2, 0.35])
        if least_config(in_width, prologue, stages, ending) is not None:   # (else: a layout over 160 KiB — drawn again)
            return in_width, prologue, stages, ending


def _spoil(rng, kind, in_width, prologue, stages, ending):
    """An admitted model turned into one of KINDS[1:]: (in_width, layer sequence)."""
    stages = [list(ws) for ws in stages] or [[16, 1]]
    if kind == "hidden129":
        s = int(rng.integers(len(stages)))
        stages[s] = [129] + stages[s] if len(stages[s]) < MAX_DEPTH else [129] + stages[s][1:]
    elif kind == "last65":
        stages[int(rng.integers(len(stages)))][-1] = 65
    elif kind == "f65":
        in_width = 65
    elif kind == "lds":   # three 128 x 128 layers: 202 752 bytes of weights alone
        stages[int(rng.integers(len(stages)))] = [128, 128, 128, 128, _pick(rng, [1, 16, 32])]
    elif kind == "seven":
        s = int(rng.integers(len(stages)))
        stages[s] = [_pick(rng, [4, 8, 16]) for _ in range(7 - len(stages[s]))] + stages[s]
    seq = sequence_of(prologue, stages, ending)
    if kind == "mid_sigmoid":
        acts = [i for i, t in enumerate(seq[:-1]) if t == "R"]
        if not acts:   # (one linear layer in all: give it a stage in front)
            seq = ["G", "L8", "R"] + seq
            acts = [2]
        seq[acts[int(rng.integers(len(acts)))]] = "S"
    elif kind == "two_graphs":
        in_width = min(in_width, 16)
        at = [i for i, t in enumerate(seq) if t == "G"]
        seq.insert(at[int(rng.integers(len(at)))], "G")
    return in_width, seq


_cases = {}


def case(i: int):
    """The record of case i (cached; the text is not part of it: text(i))."""
    if i in _cases:
        return _cases[i]
    rng = np.random.default_rng([TAG, i])
    c = types.SimpleNamespace(index=i, seed=SEEDS.get(i, 0))
    c.kind = "admitted" if rng.random() >= NOT_ADMITTED_SHARE else _pick(rng, KINDS[1:])
    c.in_width, c.prologue, c.stages, c.ending = _draw_model(rng)
    c.seq = sequence_of(c.prologue, c.stages, c.ending)
    c.admitted = c.kind == "admitted"
    least = least_config(c.in_width, c.prologue, c.stages, c.ending)
    if c.admitted:
        mask, feat, big = least
        # the surplus: both pattern bits, the widest feature rows, a larger LDS limit (also where no stage needs one)
        if rng.random() < 0.3:
            mask = PROLOGUE | OPEN_END
        if rng.random() < 0.3:
            feat = FEAT_MAX
        how = rng.random()
        if how < 0.25:
            big = FULL_LDS
        elif how < 0.5:
            big = int(rng.integers(max(big, SMALL_LDS), FULL_LDS + 1))
        c.mask, c.feature_width, c.big_lds = mask, feat, big
        c.expect = expect(c.in_width, c.prologue, c.stages, c.ending, mask, feat, big)
        assert c.expect is not None
    else:
        c.in_width, c.seq = _spoil(rng, c.kind, c.in_width, c.prologue, c.stages, c.ending)
        c.prologue = c.stages = None   # (no stage list: the sequence is all there is)
        c.mask, c.feature_width, c.big_lds = PROLOGUE | OPEN_END, FEAT_MAX, FULL_LDS
        c.expect = None
    c.shapes = linear_shapes(c.in_width, c.seq)
    c.out_width = c.shapes[-1][1]
    c.sigmoid_end = c.seq[-1] == "S"
    c.late = bool(rng.random() < 1.0 / 3.0)                      # the opt-ins under the resident graph, not before it
    c.order = [SETTERS[j] for j in rng.permutation(len(SETTERS))]
    c.graph = _pick(rng, GRAPH_NAMES, _GRAPH_P)
    c.heavy = _pick(rng, HEAVY)
    c.giant = _pick(rng, GIANT)
    c.segments = _pick(rng, SEGMENTS)
    c.stage_pick = int(rng.integers(1 << 16))                    # which graph stage meets the crafted input: modulo their number
    c.parts, c.pieces, c.push = _pick(rng, PARTS), _pick(rng, PIECES), _pick(rng, PUSH)
    c.graph2 = _pick(rng, [g for g in GRAPH_NAMES if g != c.graph])
    _cases[i] = c
    return c


def layers_of(i: int):
    c = case(i)
    return draw(np.random.default_rng([TAG, i, c.seed]), c.shapes)


def text(i: int) -> str:
    c = case(i)
    return model_text(" ".join(c.seq), layers_of(i), f"{PREFIX}_{i}_{c.seed}")


def model_input(i: int, g):
    """The forward's input for graph g: tools/modelgen_generic.py's columns x, 0.37 x, 1 - x, 3 x, ... for the case's width."""
    return Family(PREFIX, TAG, list, {i: (case(i).in_width, [])}).model_input(i, g)


def describe(i: int) -> str:
    """One line that names the case: what a failure report carries."""
    c = case(i)
    forms = "" if not c.admitted else " stages " + " | ".join(
        f"{'dense ' if r.dense else ''}f={r.f} {'-'.join(map(str, r.widths))} end={r.end} {r.threads}t"
        f"{' BIG' if r.big else ''}{' FEAT' if r.feat else ''}{' OPEN' if r.open else ''} lds={r.lds_bytes}" for r in c.expect)
    return (f"fuzz case {i} [{c.kind}] in={c.in_width} seq={' '.join(c.seq)} seed={c.seed} mask={c.mask} feat={c.feature_width} "
            f"big={c.big_lds} late={c.late} order={','.join(c.order)} graph={c.graph} heavy={c.heavy} giant={c.giant} "
            f"segments={c.segments}{forms}")


if __name__ == "__main__":
    sys.stdout.write(text(int(sys.argv[1])))
