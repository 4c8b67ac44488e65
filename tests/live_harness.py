"""What tests/test_modelgen_live.py (CPU) and tests/test_gpu_live_columns.py (GPU) share about the live-column gather
(gnnvc_set_generic_live_columns): the families it adds to tests/generic_harness.py's registry — tools/modelgen_live.py's, and the
trained model as a family of one member, so that the oracle's stage-by-stage walk serves it too — and the oracle's answer to
"which columns of stage s's input are live", taken from that walk's stage inputs.  A plain module."""
import pathlib

from oracle import oracle_py
from tools import modelgen_feat, modelgen_live
from tools.modelgen_generic import Family
from tests import generic_harness as gh

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _trained_family():
    text = (ROOT / "gnn-mwvc_amd" / "data" / "mwvc_model.txt").read_text()
    shapes = [W.shape for W, _ in oracle_py.OracleModel(text).linear_params()]
    assert len(shapes) == 9 and shapes[0][0] == 5   # three stages of three dense layers, one input feature
    fam = Family("trained", 0, list, {"model": (1, [tuple(n for _, n in shapes[3 * s: 3 * s + 3]) for s in range(3)])})
    fam.FAMILY = {"model": lambda: text}
    return fam


gh.FAMILIES.setdefault("live", modelgen_live.family)
gh.FAMILIES.setdefault("feat", modelgen_feat.family)
gh.FAMILIES.setdefault("trained", _trained_family())


def stage_masks(family, name, gname):
    """[(f, mask)] per stage: the live columns of the stage's input on the oracle's walk from the member's own model input."""
    return [(hin.shape[1] if hin.ndim > 1 else 1, modelgen_live.live_mask(hin)) for hin, _, _ in gh.want_of(family, name, gname)]


def eligible(family, name):
    """Per stage: does gnnvc_set_generic_live_columns examine it — a graph stage with f >= 2 (these families have no dense stage
    and no open ending)."""
    return [f >= 2 for f, _ in gh.FAMILIES[family].stage_widths(name)]


def expected_readouts(family, name, gname, max_percent):
    """Per stage (kept, used, mask) as "generic_live_{kept,used,mask_lo|hi}_<s>" must read after a forward on the graph: -1 / 0 / 0 for a
    stage that is not examined (or on a graph without vertices)."""
    out = []
    if gh.graph_of(gname).n == 0 or not max_percent:
        return [(-1, 0, 0)] * len(eligible(family, name))
    for (f, mask), ok in zip(stage_masks(family, name, gname), eligible(family, name)):
        if not ok:
            out.append((-1, 0, 0))
        else:
            kept = bin(mask).count("1")
            out.append((kept, modelgen_live.used_by_rule(kept, f, max_percent), mask))
    return out
