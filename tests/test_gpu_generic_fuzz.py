"""Randomised differential test of the generic fused stages (k_stage_any and its launchers, k_audit_any, the heavy- and giant-row
kernels, forward_part_generic with k_push_rows): tools/modelgen_fuzz.py's cases — random layer sequences, widths from edge values,
graphs, thresholds, opt-ins in a drawn order before the graph or under it, part counts and stage inputs — against the CPU
oracle.  tests/test_modelgen_fuzz.py pins the table on the CPU and shows that its cases reach every specialisation; the runs
themselves are tests/fuzz_harness.py's.  (`python -m tests.fuzz_harness --from 240 --to 2240` is the long form:
2 000 cases, 0 mismatches.)

Bars, tests/generic_harness.py's and no others: logits bit for bit the oracle's, scores within 1 ulp of the oracle's and bit for
bit the restated sigmoid's (check_scores); a model that does not end in the sigmoid has its outputs compared bit for bit and its
logits buffer left untouched.  "poison_features" is 1 on every handle."""
import pytest

from tools import modelgen_fuzz as mz
from tests import fuzz_harness as fh
from tests.test_expf_restatement import shim   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)

pytestmark = pytest.mark.gpu

CASES = list(range(mz.N)) + list(mz.REGRESSIONS)
ADMITTED = [i for i in CASES if mz.case(i).admitted]
OFF = ADMITTED[0::3]          # a third of the admitted cases
MULTI = ADMITTED[1::3][:60]   # every admitted case is one gnnvc_create_multi_generic accepts


def _blocks(cases, size):
    return [cases[at: at + size] for at in range(0, len(cases), size)]


@pytest.mark.parametrize("block", _blocks(CASES, 30), ids=lambda b: f"{b[0]}-{b[-1]}")
def test_random_models_single_engine(shim, block):
    """Per admitted case: the engine's read-outs against the record; three host forwards; one with the input scaled by 0.37 and the
    first input again; one audited forward (k_audit_any clean, audit_runs grown by the number of stages); one device-pointer
    forward into NaN-filled tensors; a drawn graph stage, and the dense stage where there is one, through the stage entry on the
    crafted input over split ranges, then gnnvc_audit_stage_device.  A case that no setting admits reports fused == False and
    takes the host forwards on the layer-by-layer path."""
    for i in block:
        fh.one_case(i, shim)


@pytest.mark.parametrize("block", _blocks(OFF, 23), ids=lambda b: f"{b[0]}-{b[-1]}")
def test_random_models_generic_stages_off(shim, block):
    """Option "generic_stages" 0: the layer-by-layer kernels at widths no table ever gave them, the same values as the oracle's."""
    for i in block:
        fh.one_case_off(i, shim)


@pytest.mark.parametrize("block", _blocks(MULTI, 10), ids=lambda b: f"{b[0]}-{b[-1]}")
def test_random_models_on_several_parts(shim, block):
    """gnnvc_create_multi_generic with 2, 3, 5 or 8 parts on device 0, "multi_pieces" and "multi_push" drawn: two graphs handed to
    the same handle in turn (upload, then staged in 7 pieces), three forwards each, and on the second an audited one — zero
    failures, audit_runs = non-empty pieces x stages.  All parts share device 0, as in tests/test_gpu_multi_generic.py: this is
    k_push_rows at every row width and the exchange's ordering, and says nothing about a link."""
    for i in block:
        fh.one_case_multi(i, shim)


def test_a_handle_forgets_the_heavy_rows_of_the_graph_before(shim):
    """What the fuzz found (case 9 on three parts, `hubs` then `one`): a part whose slice of the next graph is empty kept the
    classing of its slice of the graph before, and a handle given the graph of no vertices attaches it to no part, so the handle's
    summed "generic_heavy_rows" and "generic_giant_rows" went on reporting the hub rows of a graph that was gone."""
    import gnn_mwvc_amd as G
    from tests import generic_harness as gh
    keys = ("generic_heavy_rows", "generic_heavy_entries", "generic_giant_rows", "generic_giant_entries")
    e = G.Engine(gh.text_of("shapes", "odd"), devices=[0, 0, 0], generic={"heavy_rows": 512, "giant_rows": 2048})
    try:
        for gname in ("hubs", "one", "hubs", "empty", "hubs", "er1933"):
            g = gh.graph_of(gname)
            gh.hand_over(e, g, "upload")
            e.forward(gh.FAMILIES["shapes"].model_input("odd", g))
            want = gh.heavy_counts(g, 512) + gh.heavy_counts(g, 2048)
            assert tuple(e.get_info(k) for k in keys) == want, gname
            assert want == ((7, 7354, 1, 3000) if gname == "hubs" else (0, 0, 0, 0))
    finally:
        e.close()
