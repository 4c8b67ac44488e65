"""Runs tools/optionflips.py's cases (tests/test_gpu_option_flips.py): one engine of the trained shape that has options set under
its resident graph, is handed the same graph again, a graph of another class, another weight scale, another stream — and is held
to the oracle after every step.  A plain module; the oracle's values come from tests/test_gpu_models.py::want_of's cache, computed
once per (model, graph, input, weight scale) and never changed.

The bars are the suite's own and no others: after every forward the logits are the oracle's bit for bit and the scores pass
generic_harness.check_scores (within 1 ulp of the oracle's, bit for bit the restated sigmoid of the device's own logits); after
every stage call the rows written are the oracle's bit for bit, every other row and the pad row keep their 7.0 fill
(tests/test_gpu_models.py::stages_on_device).

Two checks of the engine's state catch what happens not to change a bit on these inputs:

  re-upload equals fresh       after every ("reupload",) and ("graph", name) step a second engine is opened, given every
                               gnnvc_set_option call the first one has had, in their order, before its first graph, and handed the
                               same graph: the read-outs of AT_HANDOFF agree, and after three forwards on both those of
                               AFTER_FORWARDS (include/gnnvc.h: options "take effect at the next graph upload")
  flip back equals never flipped   a directed case records both lists on its first hand-off; its last step hands the same graph
                               over again with the key back at its first value: the same read-outs

python -m tests.flip_harness --from A --to B runs random cases A .. B - 1 beyond the pinned table (tools/optionflips.long_case),
once each, and stops at the first failure with the case, the step and the options in force on stderr."""
import numpy as np

from tools import optionflips as of
from tests import test_gpu_models as tm
from tests.generic_harness import bits, check_scores, ulp
from tests.test_expf_restatement import _run

# gnnvc_get_info read-outs compared between two engines in the same state
AT_HANDOFF = ["long_rows", "giant_rows", "giant_entries", "giant_segments", "lds_table_active", "compact_gather_active",
              "table_tiles_active", "pruned_predicted_stage1"]
AFTER_FORWARDS = ["wide_tiles_used", "lds_table_last_ok", "compact_gather_last_ok", "pruned_last_ok_stage1", "pruned_entries_stage1",
                  "table_tiles_fit_stage1", "table_tiles_fit_stage2"]
FORWARDS_BEFORE_READOUT = 3
# What an engine keeps across graphs on purpose (gnnvc_engine_state.h: t4.choice_live): once a forward has run on table tiles, the
# next graph that qualifies for them is offered them from its FIRST forward, on the columns chosen last, where a fresh engine's first
# forward runs without (on wide tiles, up to "wide_tiles_max_n_f16" vertices) and its tiles fit a forward later.  Same bits either
# way; these read-outs of the first three forwards are then not a fresh engine's, and are left out of both state checks for a
# hand-off at which the first engine carries a choice and the graph has table tiles.  The rest of the list is compared as ever.
CARRIED_BY_TABLE_TILES = ("wide_tiles_used", "table_tiles_fit_stage1", "table_tiles_fit_stage2")


class FlipFailure(AssertionError):
    pass


def model_text(name):
    """tools/modelgen.py's members, and "trained": the model the package ships (seeded into want_of's cache under that name)."""
    if name == "trained" and ("text", name) not in tm._cache:
        import pathlib
        tm._cache["text", name] = (pathlib.Path(__file__).resolve().parents[1] / "gnn-mwvc_amd" / "data" / "mwvc_model.txt").read_text()
    return tm.text_of(name)


def want(name, gname, what="logits", scale=1):
    model_text(name)
    return tm.want_of(name, gname, what, scale)


def needs(c):
    """[(model, graph, scale)] a case's steps compare against, in order: run the oracle ahead of the engines."""
    out, graph, scale = [], c.graph, 1
    for s in c.steps:
        if s[0] == "graph":
            graph = s[1]
        elif s[0] == "weight_scale":
            scale = s[1]
        if s[0] in ("forward", "stage", "reupload", "graph") and (c.model, graph, scale) not in out:
            out.append((c.model, graph, scale))
    return out


def prepare(cases):
    for c in cases:
        for name, gname, scale in needs(c):
            want(name, gname, "logits", scale)
            want(name, gname, "other", scale)


def readouts(e, keys, left_out=()):
    return {k: e.get_info(k) for k in keys if k not in left_out}


class Run:
    """One case on one engine (or, devices=[...], on a multi-device handle)."""

    def __init__(self, c, shim, devices=None, log=None):
        self.c, self.shim, self.devices, self.log = c, shim, devices, log
        self.e = None
        self.history = []          # every gnnvc_set_option call so far, in order
        self.graph, self.scale = c.graph, 1
        self.step = -1
        self.uploads = 0
        self.streams = []
        self.dev_inputs = {}
        self.first = None          # a directed case's read-outs on its first hand-off
        self.last = None           # the last forward's (scores, logits): what a multi-device run is compared by
        self.trace = []            # [(step index, scores, logits)] of every forward, kept on request
        self.keep_trace = False
        self.left_out = tuple(k for k, _ in c.left_out)
        self.forwards_here = 0     # whole forwards since the last hand-off
        self.choice_carried = False   # a forward has run on this engine with table tiles offered (see CARRIED_BY_TABLE_TILES)

    # -- reporting
    def in_force(self):
        o = {}
        for k, v in self.history:
            o[k] = v
        return o

    def where(self):
        s = self.c.steps[self.step] if 0 <= self.step < len(self.c.steps) else "hand-off"
        return (f"{of.describe(self.c)}\n  step {self.step}: {s}\n  graph {self.graph}, weight scale x{self.scale}, "
                f"devices {self.devices}\n  options in force: {self.in_force()}")

    def check(self, ok, what):
        if not ok:
            raise FlipFailure(f"{what}\n  {self.where()}")

    # -- the engine
    def open(self):
        import gnn_mwvc_amd as G
        text = model_text(self.c.model)
        self.e = G.Engine(text, devices=self.devices) if self.devices else G.Engine(text, device=0)
        self.check(self.e.fused and self.e.num_stages == 3 and self.e.num_layers == 21, "not the trained shape")
        for k, v in self.c.options.items():
            self.set(k, v)
        self.hand_over(self.e, staged=False)

    def close(self):
        if self.e is not None:
            self.e.close()
            self.e = None
        self.streams.clear()
        self.dev_inputs.clear()

    def set(self, k, v):
        self.e.set_option(k, v)
        self.history.append((k, v))

    def g(self):
        return tm.graph_of(self.graph)

    def ws(self):
        return float(np.float32(self.g().ws * self.scale))

    def hand_over(self, e, staged):
        e.set_weight_scale(self.ws())
        if staged and not self.devices:
            e.upload_graph_staged(self.g())
        else:
            e.upload_graph(self.g())

    def fresh(self):
        """A second engine in the state the header promises for the first: the same set calls, then the graph."""
        import gnn_mwvc_amd as G
        e = G.Engine(model_text(self.c.model), device=0)
        try:
            for k, v in self.history:
                e.set_option(k, v)
            self.hand_over(e, staged=False)
        except BaseException:
            e.close()
            raise
        return e

    # -- the steps
    def forward(self, which, e=None):
        g = self.g()
        x = g.x() if which == "x" else tm.other_input(g)
        w = want(self.c.model, self.graph, "logits" if which == "x" else "other", self.scale)
        tiles = e is None and not self.devices and self.e.get_info("table_tiles_active") == 1
        sc, lg = (e or self.e).forward(x)
        if e is None:
            self.choice_carried = self.choice_carried or (tiles and self.forwards_here >= 1)
            self.forwards_here += 1
        diff = np.flatnonzero(bits(lg[:, 0]) != bits(w))
        self.check(diff.size == 0, f"forward({which}): {diff.size} of {g.n} logits differ from the oracle's, first rows {diff[:8].tolist()}"
                                   + (" (the second, fresh engine)" if e is not None else ""))
        try:
            check_scores(self.shim, sc[:, 0], lg[:, 0], w, "scores")
        except FlipFailure:
            raise
        except AssertionError as err:
            self.check(False, f"forward({which}): {err}")
        if e is None:
            self.last = (sc, lg)
            if self.keep_trace:
                self.trace.append((self.step, sc.copy(), lg.copy()))

    def stage(self, st, lo, hi):
        import torch
        g, name = self.g(), self.c.model
        dev = torch.device("cuda:0")
        key = (self.graph, self.scale, st)
        if key not in self.dev_inputs:
            if st == 0:
                t = torch.from_numpy(g.x()).to(dev)
            else:
                t = torch.zeros((g.n + 1, 16), dtype=torch.float32, device=dev)
                t[: g.n] = torch.from_numpy(np.ascontiguousarray(want(name, self.graph, f"h{st}", self.scale))).to(dev)
            self.dev_inputs[key] = t
        t = self.dev_inputs[key]
        out = torch.full((g.n + 1, 16 if st < 2 else 1), 7.0, dtype=torch.float32, device=dev)
        lg = torch.full((g.n + 1,), 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        self.forwards_here += 1 if st == 0 else 0   # (a call of stage 0 counts as a use of the graph: the next forward is offered the tiles)
        self.e.stage_forward_device(st, lo, hi, t.data_ptr(), out.data_ptr(), lg.data_ptr() if st == 2 else 0)
        self.e.synchronize()
        got, seven = out.cpu().numpy(), bits(np.float32(7.0))
        outside = np.ones(g.n + 1, dtype=bool)
        outside[lo:hi] = False
        if st < 2:
            w = want(name, self.graph, f"h{st + 1}", self.scale)
            bad = np.argwhere(bits(got[lo:hi]) != bits(w[lo:hi]))
            self.check(bad.size == 0, f"stage {st} over [{lo}, {hi}): {len(bad)} values of h{st + 1} differ, first (row - lo, column) {bad[:6].tolist()}")
        else:
            w = want(name, self.graph, "logits", self.scale)
            lgh = lg.cpu().numpy()
            bad = np.flatnonzero(bits(lgh[lo:hi]) != bits(w[lo:hi]))
            self.check(bad.size == 0, f"stage 2 over [{lo}, {hi}): {bad.size} logits differ, first rows - lo {bad[:8].tolist()}")
            self.check(bool((bits(lgh[outside]) == seven).all()), f"stage 2 over [{lo}, {hi}): a logit outside the range, or the pad row's, was written")
            sc = np.ascontiguousarray(got[lo:hi, 0])
            self.check(np.array_equal(bits(sc), bits(_run(self.shim.sigmoid_restated, np.ascontiguousarray(lgh[lo:hi])))),
                       f"stage 2 over [{lo}, {hi}): scores differ from sigmoid_restated(logits)")
            from oracle import oracle_py
            self.check(int(ulp(sc, oracle_py.sigmoid(np.ascontiguousarray(w[lo:hi]))).max(initial=0)) <= 1, f"stage 2 over [{lo}, {hi}): a score more than 1 ulp from the oracle's")
        self.check(bool((bits(got[outside]) == seven).all()), f"stage {st} over [{lo}, {hi}): a row outside the range, or the pad row, was written")

    def same_as_fresh(self, forwards=True):
        """Re-upload equals fresh — and, on a directed case's first and last hand-off, flip back equals never flipped.
        forwards=False (a ("reupload", "plain") step): the read-outs at hand-off alone, the engine is left before its first forward."""
        if self.devices:
            return
        f = self.fresh()
        try:
            a, b = readouts(self.e, AT_HANDOFF, self.left_out), readouts(f, AT_HANDOFF, self.left_out)
            carried = CARRIED_BY_TABLE_TILES if self.choice_carried and a["table_tiles_active"] == 1 else ()
            self.check(a == b, f"read-outs at hand-off differ from a fresh engine's with the same options: {_diff(a, b)}")
            if not forwards:
                return a
            for _ in range(FORWARDS_BEFORE_READOUT):
                self.forward("x")
                self.forward("x", e=f)
            a2, b2 = readouts(self.e, AFTER_FORWARDS, self.left_out + carried), readouts(f, AFTER_FORWARDS, self.left_out + carried)
            self.check(a2 == b2, f"read-outs after {FORWARDS_BEFORE_READOUT} forwards differ from a fresh engine's with the same options: {_diff(a2, b2)}")
        finally:
            f.close()
        return dict(a, **a2)

    def run(self):
        from gnn_mwvc_amd.engine import GnnvcError
        try:
            self._run()
        except GnnvcError as err:   # (a call the engine refused or that failed: the case's failure, with its step)
            failure = FlipFailure(f"{err}\n  {self.where()}")
            failure.code = err.code
            raise failure from err

    def _run(self):
        c = self.c
        self.open()
        if c.kind == "directed":   # (the engine IS fresh here: its read-outs are the ones the flip back has to restore)
            self.first = readouts(self.e, AT_HANDOFF, self.left_out)
        forwards = 0
        for self.step, s in enumerate(c.steps):
            if self.log:
                self.log(f"  step {self.step}: {s}")
            kind = s[0]
            if kind == "set":
                self.set(s[1], s[2])
            elif kind == "forward":
                self.forward(s[1])
                forwards += 1
                if c.kind == "directed" and forwards == FORWARDS_BEFORE_READOUT:
                    self.first.update(readouts(self.e, AFTER_FORWARDS, self.left_out))
            elif kind == "stage":
                self.stage(s[1], s[2], s[3])
            elif kind == "weight_scale":
                self.scale = s[1]
                self.e.set_weight_scale(self.ws())
            elif kind in ("reupload", "graph"):
                if kind == "graph":
                    self.graph = s[1]
                self.uploads += 1
                self.hand_over(self.e, staged=self.uploads % 2 == 1)
                self.forwards_here = 0
                now = self.same_as_fresh(forwards=len(s) == 1)
                if c.kind == "directed" and self.step == len(c.steps) - 1:
                    before = {k: v for k, v in self.first.items() if k in now}
                    self.check(now == before, f"the key is back at its first value and the graph handed over again, the read-outs are not "
                                                  f"the ones before the first flip: {_diff(now, before)}")
            elif kind == "stream":
                if s[1] == "caller":
                    import torch
                    self.streams.append(torch.cuda.Stream())
                    self.e.set_stream(self.streams[-1].cuda_stream)
                else:
                    self.e.synchronize()
                    self.e.set_stream(None)
            elif kind == "expect":
                got = self.e.get_info(s[1])
                self.check(got == s[2], f"{s[1]} is {got}, the case expects {s[2]}: it did not reach the transition it is named for")
            else:
                raise ValueError(s)


def _diff(a, b):
    return {k: (a.get(k), b.get(k)) for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)}


def run_case(c, shim, log=None):
    """A directed or random case on a single engine; raises FlipFailure with the case, the step and the options in force."""
    r = Run(c, shim, log=log)
    try:
        r.run()
    finally:
        r.close()


def run_multi(c, shim, devices=(0, 0, 0), log=None):
    """A multi case on a handle of several parts and on a single engine that has the same set calls: both against the oracle
    after every forward (Run.forward), and every forward's scores and logits equal between the two."""
    traces = []
    for dv in (list(devices), None):
        r = Run(c, shim, devices=dv, log=log)
        r.keep_trace = True
        try:
            r.run()
            if dv:
                r.check(r.e.get_info("devices") == len(devices), "not a multi-device handle")
        finally:
            r.close()
        traces.append(r.trace)
    multi, single = traces
    assert len(multi) == len(single) and len(multi) >= 3, of.describe(c)
    for (step, sc, lg), (_, sc1, lg1) in zip(multi, single):
        if not (np.array_equal(bits(lg), bits(lg1)) and np.array_equal(bits(sc), bits(sc1))):
            raise FlipFailure(f"step {step} ({c.steps[step]}): the handle's scores or logits differ from a single engine's\n  {of.describe(c)}")


def main(argv=None):
    import argparse
    import sys
    from tests.fuzz_harness import load_shim
    ap = argparse.ArgumentParser(description="random option-flip cases beyond the pinned table, once each")
    ap.add_argument("--from", dest="lo", type=int, default=of.N)
    ap.add_argument("--to", dest="hi", type=int, default=of.N + 100)
    ap.add_argument("--verbose", action="store_true")
    a = ap.parse_args(argv)
    shim = load_shim()
    for seed in range(max(a.lo, of.N), a.hi):
        c = of.long_case(seed)
        prepare([c])
        try:
            run_case(c, shim, log=(lambda m: print(m, flush=True)) if a.verbose else None)
        except FlipFailure as err:
            print(f"FAILED {err}", file=sys.stderr)
            return 1
        print(f"case {seed} ok ({len(c.steps)} steps)", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
