"""How many hidden units a wave of 64 rows really needs: the evidence behind the hidden-unit skip (dense_live in
csrc/gnnvc_kernels.hip), on the CPU with the oracle's layer functions and tools/graphgen.py.

    python -m tools.unit_sparsity [--model FILE] GRAPH [GRAPH ...]

GRAPH is a generator call of tools/graphgen.py written with colons: er:200000:2000000:7 = erdos_renyi(200000, 2000000, 7),
rmat:16:16:3 = rmat(16, 16, 3).  The model is the shipped one unless --model names a text of the trained shape.

Per layer input that a skipped chain multiplies (the ReLU output of linear layers 0, 1, 3, 4, 6) it prints
  never      units that are zero for every row of the graph (dead for this input),
  per row    the share of (row, unit) pairs that are non-zero — what a per-lane test could skip at best,
  per group  the share of (group of 64 consecutive rows, unit) pairs with a non-zero value in at least one row — the terms a
             wave-uniform branch still has to run (the last group of a graph may be part full).
"""
from __future__ import annotations

import argparse
import pathlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
NAMES = {0: "stage 0, input of 32 -> 32", 1: "stage 0, input of 32 -> 16", 3: "stage 1, input of 32 -> 32",
         4: "stage 1, input of 32 -> 16", 6: "stage 2, input of 32 -> 16"}


def parse_graph(spec: str):
    from tools import graphgen as gg
    kind, *args = spec.split(":")
    make = {"er": gg.erdos_renyi, "rmat": gg.rmat}[kind]
    return make(*[int(a) for a in args])


def hidden_outputs(om, g):
    """{linear layer index: its ReLU output} for the layers in NAMES, by the oracle's own layer functions."""
    from oracle import oracle_py
    h = np.ascontiguousarray(g.x(), dtype=np.float32).reshape(g.n, 1)
    out = {}
    for i, (W, b) in enumerate(om.linear_params()):
        if i % 3 == 0:
            h = oracle_py.graph_layer(g, g.ws, h)
        h = oracle_py.linear_layer(h, W, b)
        if i < 8:
            h = oracle_py.relu(h)
        if i in NAMES:
            out[i] = h
    return out


def group_live(h: np.ndarray, group: int = 64) -> np.ndarray:
    """[groups, units] bool: the unit is non-zero (NaN counts) in at least one row of the group of `group` consecutive rows."""
    nz = h != 0
    pad = (-nz.shape[0]) % group
    if pad:
        nz = np.concatenate([nz, np.zeros((pad, nz.shape[1]), dtype=bool)])
    return nz.reshape(-1, group, nz.shape[1]).any(axis=1)


def table(om, g):
    om.set_weight_scale(g.ws)
    rows = []
    for i, h in hidden_outputs(om, g).items():
        nz = h != 0
        rows.append((NAMES[i], int((~nz.any(axis=0)).sum()), h.shape[1], float(nz.mean()), float(group_live(h).mean())))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", default=str(ROOT / "gnn-mwvc_amd" / "data" / "mwvc_model.txt"))
    ap.add_argument("graphs", nargs="+", metavar="GRAPH")
    a = ap.parse_args(argv)
    from oracle import oracle_py
    om = oracle_py.OracleModel(pathlib.Path(a.model).read_text())
    for spec in a.graphs:
        g = parse_graph(spec)
        print(f"{spec}: {g.n} vertices, {g.nnz} entries")
        print("| layer input (what the chain multiplies) | never non-zero (of units) | live per row | live per 64-row group |")
        print("|---|---|---:|---:|")
        for name, dead, units, per_row, per_group in table(om, g):
            print(f"| {name} | {dead} of {units} | {per_row:.3f} | {per_group:.3f} |")
        print()


if __name__ == "__main__":
    import sys
    if str(ROOT) not in sys.path:
        sys.path.insert(0, str(ROOT))
    main()
