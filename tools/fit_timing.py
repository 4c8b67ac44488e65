"""One training step per graph, two ways, by the method of profiles/backward/README.md: a few steps to settle, then the best and the
median of five batches, host wall clock around a batch that ends synchronised.  Prints one JSON line per graph;
profiles/fit_step/README.md holds what it printed.

    python -m tools.fit_timing                     # Erdős–Rényi 20 000 / 100 000 and 1 000 000 / 10 000 000, the trained model
    python -m tools.fit_timing n m                 # one graph
    python -m tools.fit_timing n m once            # two settled Trainer steps and out: the run to put under a kernel trace

The two ways, each a forward, the loss, a backward and an SGD step with batch = n:
    host_loop   the loop of tests/test_gpu_backward.py, test_training_loop_lowers_the_loss, as written there: Engine.train_forward,
                training.mse_loss and mse_grad in numpy, Engine.backward, training.sgd_step in numpy — scores down, loss gradient
                up, parameter gradient down, parameters up;
    trainer     training.Trainer.run on the one pair: everything on the device, one read-back of the stats behind the step.
"resident": the graph stays the engine's resident graph (the test's loop); "hand_off": every step begins with
Engine.upload_graph of the same graph from host memory, as a trainer that walks a list of graphs does (graphs up to 100 000
vertices only).
"""
import json
import statistics
import sys
import time
import types

import numpy as np
import torch

import gnn_mwvc_amd as G
from gnn_mwvc_amd import training
from tools import graphgen as gg
from tools import graphgen_torch as ggt

HYPER = dict(lr=0.05, momentum=0.5, weight_decay=0.0)


def timed(fn, per, settle=3, batches=5):
    """fn ends synchronised: the host loop's calls wait for the stream, Trainer.run reads its stats back."""
    for _ in range(settle):
        fn()
    out = []
    for _ in range(batches):
        t = time.perf_counter()
        for _ in range(per):
            fn()
        out.append((time.perf_counter() - t) * 1000.0 / per)
    return {"best_ms": round(min(out), 4), "median_ms": round(statistics.median(out), 4)}


def measure(n, m, once=False):
    text = G.default_model_text()
    small = n <= 100_000
    e = G.Engine(text, device=0)
    try:
        if small:
            g = gg.erdos_renyi(n, m, 3)
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            x, nnz = g.x(), int(g.rowptr[-1])
        else:   # generated and attached on the device; the loops see its size and x = W / ws
            gd = ggt.erdos_renyi(n, m, 2, torch.device("cuda:0"))
            e.set_weight_scale(gd.ws)
            e.attach_graph_device(gd.n, gd.nnz, gd.rowptr.data_ptr(), gd.col.data_ptr(), gd.w.data_ptr(), gd.nw.data_ptr(), keepalive=gd)
            x, nnz = gd.x().cpu().numpy(), int(gd.nnz)
            g = types.SimpleNamespace(n=gd.n, ws=gd.ws, x=lambda: x)
        target = np.random.default_rng(5).uniform(0.0, 1.0, (g.n, 1)).astype(np.float32)
        per = 20 if small else 3
        state = {"p": e.params(), "vel": np.zeros(e.num_params(), np.float32)}

        def host_step():
            scores = e.train_forward(x, state["p"])
            state["loss"] = training.mse_loss(scores, target)
            grad = e.backward(training.mse_grad(scores, target))
            state["p"], state["vel"] = training.sgd_step(state["p"], state["vel"], grad, batch=g.n, **HYPER)

        def host_step_hand_off():
            e.upload_graph(g)
            host_step()

        if once:
            tr = training.Trainer(e, text, batch_vertices=0, **HYPER)
            for _ in range(3):
                tr.run([(g, target)], fit=True, hand_off=False)
            tr.close()
            return None
        out = {"graph": f"erdos_renyi {n} / {m}", "entries": nnz, "device": torch.cuda.get_device_name(0), "steps_per_batch": per,
               "host_loop_resident": timed(host_step, per)}
        if small:
            out["host_loop_hand_off"] = timed(host_step_hand_off, per)
        assert np.isfinite(state["p"]).all()
        tr = training.Trainer(e, text, batch_vertices=0, **HYPER)
        out["trainer_resident"] = timed(lambda: tr.run([(g, target)], fit=True, hand_off=False), per)
        if small:
            out["trainer_hand_off"] = timed(lambda: tr.run([(g, target)], fit=True), per)
        assert np.isfinite(tr.params()).all() and tr.stats.rows == g.n
        tr.close()
        return out
    finally:
        e.close()


def main(argv):
    once = len(argv) > 3 and argv[3] == "once"
    sizes = [(int(argv[1]), int(argv[2]))] if len(argv) > 2 else [(20_000, 100_000), (1_000_000, 10_000_000)]
    for n, m in sizes:
        out = measure(n, m, once)
        if out is not None:
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv)
