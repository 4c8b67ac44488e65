"""Times of the backward pass on one device, by the method of profiles/generic_stages/README.md: the graph attached on the
device, three calls to settle, then the best and the median of five batches of three, host wall clock around a synchronised
batch.  Prints one JSON line; profiles/backward/README.md holds what it printed.

    python -m tools.backward_timing [n] [m]            # Erdős–Rényi n / m (default 1 000 000 / 10 000 000), the trained model
    python -m tools.backward_timing n m once           # one settled forward + backward and out: the run to put under a kernel trace

Figures: train_forward_device, backward_device (parameter gradients only, and with grad_x), the symmetry check (a backward
right behind a hand-off minus a steady one), and for every linear layer the algorithmic bytes n (k + m) 4 of k_bwd_linear_dw.
"""
import json
import statistics
import sys
import time

import numpy as np
import torch

import gnn_mwvc_amd as G
from gnn_mwvc_amd import training
from tools import graphgen_torch as ggt


def timed(sync, fn, settle=3, batches=5, per=3):
    for _ in range(settle):
        fn()
    sync()
    out = []
    for _ in range(batches):
        t = time.perf_counter()
        for _ in range(per):
            fn()
        sync()
        out.append((time.perf_counter() - t) * 1000.0 / per)
    return {"best_ms": round(min(out), 4), "median_ms": round(statistics.median(out), 4)}


def main(argv):
    n = int(argv[1]) if len(argv) > 1 else 1_000_000
    m = int(argv[2]) if len(argv) > 2 else 10_000_000
    once = len(argv) > 3 and argv[3] == "once"
    dev = torch.device("cuda:0")
    g = ggt.erdos_renyi(n, m, 2, dev)
    text = G.default_model_text()
    e = G.Engine(text, device=0)
    try:
        def attach():
            e.set_weight_scale(g.ws)
            e.attach_graph_device(g.n, g.nnz, g.rowptr.data_ptr(), g.col.data_ptr(), g.w.data_ptr(), g.nw.data_ptr(), keepalive=g)
        attach()
        x = g.x().contiguous()
        sc = torch.zeros(g.n, device=dev)
        gs = torch.rand(g.n, device=dev) * 0.75 + 0.25
        gp = torch.zeros(e.num_params(), device=dev)
        gx = torch.zeros(g.n, device=dev)
        torch.cuda.synchronize()

        def fwd():
            e.train_forward_device(x.data_ptr(), sc.data_ptr())

        def bwd():
            e.backward_device(gs.data_ptr(), gp.data_ptr())

        def bwd_x():
            e.backward_device(gs.data_ptr(), gp.data_ptr(), gx.data_ptr())

        fwd()
        bwd()
        e.synchronize()
        if once:
            fwd()
            bwd_x()
            e.synchronize()
            return
        out = {"graph": f"erdos_renyi {n} / {m}", "entries": g.nnz, "device": torch.cuda.get_device_name(0),
               "workspace_bytes": e.get_info("backward_workspace_bytes"),
               "train_forward": timed(e.synchronize, fwd), "backward": timed(e.synchronize, bwd),
               "backward_with_grad_x": timed(e.synchronize, bwd_x)}
        first = []
        for _ in range(5):   # a backward right behind a hand-off runs the symmetry check
            attach()
            fwd()
            e.synchronize()
            t = time.perf_counter()
            bwd()
            e.synchronize()
            first.append((time.perf_counter() - t) * 1000.0)
            assert e.get_info("graph_symmetric") == 1
        out["first_backward_ms"] = {"best_ms": round(min(first), 4), "median_ms": round(statistics.median(first), 4)}
        out["symmetry_check_ms"] = round(min(first) - out["backward"]["best_ms"], 4)
        out["dw_algorithmic_bytes"] = {f"{k}x{mm}": n * (k + mm) * 4 for k, mm, _, _ in training.param_layout(text)[0]}
        assert np.isfinite(gp.cpu().numpy()).all()
        print(json.dumps(out))
    finally:
        e.close()


if __name__ == "__main__":
    main(sys.argv)
