"""The hidden-unit skip of the VALU dense layers (dense_live: k_stage_f1, k_dense_f16; option "dense_skip_zeros") against the
oracle and against itself switched off.

Models: the trained one, the dense members of tools/modelgen.py's family, its live_four and live_pairs, and
tools/modelgen_units.py's models, built for the skip's edges (tests/test_modelgen_units.py shows on the oracle what they do in
groups of 64 rows, and that their h1 and h2 fit one table of the compact-table plan).
Graphs: er3000 — 46 full waves and one of 56 rows; wide tiles off, so that k_stage_f1 has stage 0 — and PLAN_GRAPH, the
smallest graph of tests/test_modelgen.py on which the plans built at hand-off include the compact-table plan.  There the
device takes the plan for a 16-wide stage — and k_dense_f16, not the gathering tile kernel, runs its dense layers — only
if the stage's input has at most n / 512 non-zeros outside its four fullest columns.  FITS says for which stages of which model
that holds on PLAN_GRAPH: both for the unit models, live_four and live_pairs; stage 2 alone for the trained model (its h1 has ten
live columns on so small a graph); neither for the dense members, which reach k_stage_f1 only.  After each whole-range call of
such a stage the test asserts that the device did take the plan ("compact_gather_last_passes" == 1).

Bars: logits, h1 and h2 bit for bit against the oracle over five forwards, a second input and the stage entry point, as in
tests/test_gpu_models.py, with the option at 1 and at 0, and the two settings bit for bit against each other.  inf_weight's
logits are NaN for every vertex (0 * inf): against the oracle they must be NaN where its are (a NaN's sign and payload are the
FPU's own), between the two settings bit for bit like everything else; h1 and h2 bit for bit against the oracle as always."""
import numpy as np
import pytest

from tools import modelgen_units as mu
from tests.test_expf_restatement import shim   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)
from tests import test_gpu_models as tm
from tests.test_gpu_models import DENSE, PLANNED, bits, forwards, graph_of, open_engine, stages_on_device, want_of

pytestmark = pytest.mark.gpu

PLAN_GRAPH = "er1933"
UNITS = ["units_" + k for k in mu.FAMILY]
LIVE = ["live_four", "live_pairs"]
MODELS = ["trained"] + DENSE + LIVE + UNITS
# the 16-wide stages whose input fits the plan's table on PLAN_GRAPH (tests/test_modelgen_units.py)
FITS = dict({m: (1, 2) for m in UNITS + LIVE}, trained=(2,))
GRAPH_OPTS = {"er3000": {"wide_tiles": 0, "poison_features": 1}, PLAN_GRAPH: dict(PLANNED, poison_features=1)}


@pytest.fixture(scope="module", autouse=True)
def texts(model_text):
    """tests/test_gpu_models.py's helpers look a model's text up by name: the trained model and the new ones under theirs."""
    tm._cache["text", "trained"] = model_text
    for k, make in mu.FAMILY.items():
        tm._cache["text", "units_" + k] = make()
    assert tm.text_of("trained") is model_text and tm.text_of(UNITS[0]).startswith("units_")   # (the helpers do find them there)


def skip_layers_of(name):
    return mu.SKIP_LAYERS[name[len("units_"):]] if name in UNITS else mu.ALL_LAYERS


def stage_outputs(e, name, gname, ins):
    """h1, h2 and the logits through the stage entry point, each stage fed the oracle's input (`ins` of stages_on_device); on
    PLAN_GRAPH the stages in FITS must have run on the compact-table plan: k_dense_f16 did their dense layers."""
    import torch
    g = graph_of(gname)
    dev = torch.device("cuda:0")
    got = []
    for st in (0, 1, 2):
        out = torch.zeros((g.n + 1, 16 if st < 2 else 1), dtype=torch.float32, device=dev)
        lg = torch.zeros((g.n + 1,), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        e.stage_forward_device(st, 0, g.n, ins[st].data_ptr(), out.data_ptr(), lg.data_ptr() if st == 2 else 0)
        e.synchronize()
        if gname == PLAN_GRAPH and st in FITS.get(name, ()):
            assert e.get_info("compact_gather_last_passes") == 1, (name, gname, st, "the plan did not take this input")
        got.append((out if st < 2 else lg)[: g.n].cpu().numpy())
    return got


def nan_forwards(e, name, gname):
    """forwards() for a model whose logits are NaN: NaN where the oracle's are, and scores that are NaN with them."""
    g = graph_of(gname)
    for x, what in [(g.x(), "logits")] * 5 + [(tm.other_input(g), "other"), (g.x(), "logits")]:
        want = want_of(name, gname, what)
        sc, lg = e.forward(x)
        nan = np.isnan(want)
        assert nan.all(), (name, gname, "the oracle's logits are expected to be NaN everywhere")
        assert np.array_equal(np.isnan(lg[:, 0]), nan), (name, gname, what)
        assert np.array_equal(np.isnan(sc[:, 0]), nan), (name, gname, what)


@pytest.mark.parametrize("gname", list(GRAPH_OPTS))
@pytest.mark.parametrize("name", MODELS)
def test_hidden_unit_skip_is_bit_identical(shim, name, gname):
    g = graph_of(gname)
    nan_model = name == "units_inf_weight"
    seen = {}
    for skip in (1, 0):
        e = open_engine(name, g, dict(GRAPH_OPTS[gname], dense_skip_zeros=skip))
        try:
            # which layers the model's weights allow to skip in does not depend on the option
            assert e.get_info("dense_skip_layers") == skip_layers_of(name), (name, oct(e.get_info("dense_skip_layers")))
            if gname == PLAN_GRAPH:
                assert e.get_info("compact_gather_active") == 1 and e.get_info("lds_table_active") == 1, (name, gname)
            if nan_model:
                nan_forwards(e, name, gname)
                import torch
                dev = torch.device("cuda:0")
                ins = {0: torch.from_numpy(g.x()).to(dev)}
                for st, h in ((1, "h1"), (2, "h2")):
                    t = torch.zeros((g.n + 1, 16), dtype=torch.float32, device=dev)
                    t[: g.n] = torch.from_numpy(np.ascontiguousarray(want_of(name, gname, h))).to(dev)
                    ins[st] = t
            else:
                forwards(e, shim, name, gname, label=("dense_skip_zeros", skip))
                ins = stages_on_device(e, name, gname)
            if gname == "er3000":
                assert e.get_info("wide_tiles_used") == 0, name   # (k_stage_f1 had stage 0, not the wide tiles)
            sc, lg = e.forward(g.x())
            if gname == PLAN_GRAPH and 2 in FITS.get(name, ()):
                assert e.get_info("compact_gather_last_passes") == 1, name   # (the forward's last stage ran on the plan)
            h1, h2, lg2 = stage_outputs(e, name, gname, ins)
            seen[skip] = (sc.copy(), lg.copy(), h1, h2, lg2)
        finally:
            e.close()
        h1, h2, lg2 = seen[skip][2:]
        assert np.array_equal(bits(h1), bits(want_of(name, gname, "h1"))), (name, gname, skip, "h1")
        assert np.array_equal(bits(h2), bits(want_of(name, gname, "h2"))), (name, gname, skip, "h2")
        if nan_model:
            assert np.isnan(lg2).all() and np.isnan(want_of(name, gname)).all(), (name, gname, skip, "stage 2 logits")
        else:
            assert np.array_equal(bits(lg2), bits(want_of(name, gname))), (name, gname, skip, "stage 2 logits")
    for a, b, what in zip(seen[1], seen[0], ("scores", "logits", "h1", "h2", "stage 2 logits")):
        assert np.array_equal(bits(a), bits(b)), (name, gname, what, "dense_skip_zeros 1 against 0")


def test_the_skip_is_refused_per_layer():
    """(d), (e): a bias of -0.0f or a weight that is not finite takes the skip away from its own layer, whatever the option says,
    and from no other; the first layer's bit governs the routes that leave out its known zeros."""
    import gnn_mwvc_amd as G
    for k in mu.FAMILY:
        e = G.Engine(mu.FAMILY[k](), device=0)
        try:
            for opt in (1, 0):
                e.set_option("dense_skip_zeros", opt)
                assert e.get_info("dense_skip_layers") == mu.SKIP_LAYERS[k], (k, opt, oct(e.get_info("dense_skip_layers")))
        finally:
            e.close()
