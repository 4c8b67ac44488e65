"""The graph and the crafted inputs of the giant-row tests of generic stages (tests/test_gpu_giant_rows.py), and the plain numpy
chain they are judged by.  tests/test_giant_rows_inputs.py proves on the CPU that they are what the GPU test needs.

hub_graph()    12 000 vertices; hubs 0 .. 7 of exactly 1023, 1024, 1025, 2049, 4096, 4097, 9000 and 0 entries: around a window of
               the exact scan (1024 addends), around a segment (4096), three segments, and an empty row.  A hub's neighbours are
               drawn without replacement among the other vertices; the sparse background touches no hub and leaves every other
               degree below 64.
scan_input()   a NON-NEGATIVE input for the integer route of the scan (csrc/exact_sum.h): values m * 2^e, m an integer below 2^24
               and e from -24 to 20, whose scale rises with the vertex id — a row's neighbours are stored in ascending order, so
               a hub's accumulator climbs through dozens of binades and meets addends around its last place all the way, exact
               half-ulp ties among them; zeros, -0.0f, a few denormals; and per hub one neighbour whose value lifts that hub's
               accumulator several binades in one add.
chain()        acc = acc + v, one fp32 add per neighbour in stored order from +0.0f, per column: the reference's sum.
chain_facts()  what a chain does on the way: binades crossed, adds that were exact ties, the largest jump of one add.
"""
from __future__ import annotations

import numpy as np

from tools import graphgen as gg

HUB_DEGREES = [1023, 1024, 1025, 2049, 4096, 4097, 9000, 0]
HUB_N = 12000
BIG_HUB = 6          # the 9000-entry row
SPIKE_LIFT = 8       # binades a hub's spike lifts its accumulator by (chain_facts' `jump` sees at least SPIKE_LIFT - 1)


def hub_graph():
    rng = np.random.default_rng(2049)
    nh = len(HUB_DEGREES)
    others = np.arange(nh, HUB_N)
    edges = []
    for h, d in enumerate(HUB_DEGREES):
        for v in rng.choice(others, size=d, replace=False):
            edges.append((h, int(v)))
    a = rng.integers(nh, HUB_N, size=18000)
    b = rng.integers(nh, HUB_N, size=18000)
    edges += list(zip(a.tolist(), b.tolist()))
    return gg.from_edge_list(HUB_N, edges, rng.integers(20, 121, size=HUB_N))


def neighbours(g, u):
    return g.col[int(g.rowptr[u]): int(g.rowptr[u + 1])].astype(np.int64)


def chain(g, u, hin, reverse=False):
    """Row u's neighbour sums, one fp32 add per neighbour in stored (or reversed) order from +0.0f; hin: n x f."""
    nb = neighbours(g, u)
    acc = np.zeros(hin.shape[1], dtype=np.float32)
    for v in (nb[::-1] if reverse else nb):
        acc = (acc + hin[v]).astype(np.float32)
    return acc


def _exponent(a):
    """The binade of |a| as frexp counts it (0 for zero; denormals get their own, below -125)."""
    return np.frexp(a.astype(np.float64))[1]


def chain_facts(g, u, hin):
    """Per column of row u's stored-order chain: `binades` = how many times an add left the accumulator in a higher binade than
    any before (counted from the first non-zero accumulator), `ties` = adds whose exact result lay exactly half-way between two
    floats, `jump` = the most binades one add lifted a non-zero accumulator by."""
    nb = neighbours(g, u)
    f = hin.shape[1]
    acc = np.zeros(f, dtype=np.float32)
    binades = np.zeros(f, dtype=np.int64)
    ties = np.zeros(f, dtype=np.int64)
    jump = np.zeros(f, dtype=np.int64)
    for v in nb:
        x = hin[v]
        exact = acc.astype(np.float64) + x.astype(np.float64)   # exact whenever it matters: a tie needs x within 25 bits of acc's last place
        new = exact.astype(np.float32)
        err = np.abs(exact - new.astype(np.float64))
        half = np.abs(np.spacing(new).astype(np.float64)) / 2.0
        half_down = np.abs(new.astype(np.float64) - np.nextafter(new, np.float32(0)).astype(np.float64)) / 2.0
        ties += ((err != 0) & ((err == half) | (err == half_down))).astype(np.int64)
        lifted = (_exponent(new) - _exponent(acc)) * ((acc != 0) & (new != 0))
        binades += (lifted > 0).astype(np.int64)
        jump = np.maximum(jump, lifted)
        acc = new
    return {"sum": acc, "binades": binades, "ties": ties, "jump": jump}


def scan_input(g, f, seed):
    """n x f float32, no negative value (see the module's docstring)."""
    n = g.n
    rng = np.random.default_rng([4097, f, seed])
    trend = -24 + (44 * np.arange(n, dtype=np.int64)[:, None]) // n                   # -24 .. 19, rising with the vertex id
    e = np.clip(trend + rng.integers(-5, 2, (n, f)), -24, 20)
    bits = rng.integers(1, 25, (n, f))                                                # the length of m in bits
    m = rng.integers(0, 1 << 24, (n, f)) >> (24 - bits) | (1 << (bits - 1))            # exactly `bits` long
    v = np.ldexp(m.astype(np.float64), e).astype(np.float32)                          # (exact: m < 2^24)
    r = rng.random((n, f))
    v[r < 0.04] = np.float32(0.0)
    v[(r >= 0.04) & (r < 0.07)] = np.float32(-0.0)
    den = (r >= 0.07) & (r < 0.075)
    v[den] = rng.integers(1, 1 << 23, int(den.sum())).astype(np.uint32).view(np.float32)   # denormals
    v = np.ascontiguousarray(v, dtype=np.float32)
    # one spike per hub, a third of the way into its row: SPIKE_LIFT binades above where that hub's accumulator stands
    for h, d in enumerate(HUB_DEGREES):
        if d == 0:
            continue
        nb = neighbours(g, h)
        at = d // 3
        acc = np.zeros(f, dtype=np.float32)
        for u in nb[:at]:
            acc = (acc + v[u]).astype(np.float32)
        assert (acc > 0).all()
        v[nb[at]] = np.ldexp(np.float32(1.25), _exponent(acc) - 1 + SPIKE_LIFT).astype(np.float32)
    assert np.isfinite(v).all() and not ((v < 0).any())
    return v
