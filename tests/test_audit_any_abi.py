"""CPU-side checks of the explicit audit calls (gnnvc_forward_audited, gnnvc_forward_audited_device, gnnvc_audit_stage_device):
the header declares and documents them, the library exports them, the binding has their methods, a null engine is refused,
and the ABI version has not moved.  No compute calls here (tests/test_gpu_audit_any.py has those)."""
import ctypes as C
import pathlib
import re

import pytest

import gnn_mwvc_amd as G

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "gnnvc.h").read_text()

ENTRY_POINTS = {
    "gnnvc_forward_audited": r"int gnnvc_forward_audited\(gnnvc_engine \*e, const float \*x, float \*scores, float \*logits\);",
    "gnnvc_forward_audited_device":
        r"int gnnvc_forward_audited_device\(gnnvc_engine \*e, const float \*d_x, float \*d_scores, float \*d_logits\);",
    "gnnvc_audit_stage_device":
        r"int gnnvc_audit_stage_device\(gnnvc_engine \*e, int stage, uint32_t row_lo, uint32_t row_hi,\s*"
        r"const float \*d_in, float \*d_out, float \*d_logits\);",
}


@pytest.fixture(scope="module")
def lib():
    G.build_library()
    return G.load_library()


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_header_declares_and_documents_the_entry_point(name):
    m = re.search(ENTRY_POINTS[name], HEADER)
    assert m, f"{name} is not declared with the agreed signature"
    # documented: named in a comment outside its own declaration (the option paragraphs and the block above the prototypes)
    comments = " ".join(re.findall(r"/\*.*?\*/", HEADER, flags=re.S))
    assert re.search(rf"\b{name}\b", comments), f"{name} is not mentioned in any comment of the header"


def test_header_says_what_the_period_does_on_generic_models():
    period = HEADER[HEADER.index('"audit_period" k >= 0'): HEADER.index('"audit_repair" 0|1')]
    generic = HEADER[HEADER.index('"generic_stages" 0|1|2'): HEADER.index("gnnvc_get_info keys (further)")]
    for para in (period, generic):
        assert "gnnvc_forward_audited" in para and "gnnvc_audit_stage_device" in para
    assert "audit nothing" in period or "audits nothing" in period
    assert "audits nothing" in generic and "k_audit_any" in generic


def test_abi_version_is_still_1(lib):
    assert re.search(r"#define GNNVC_ABI_VERSION 1\b", HEADER)
    assert lib.gnnvc_abi_version() == 1


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_library_exports_the_entry_point(lib, name):
    assert name in G.engine.ABI_SYMBOLS
    assert getattr(lib, name) is not None
    assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes


def test_null_engine_is_rejected(lib):
    assert lib.gnnvc_forward_audited(None, None, None, None) == -1
    assert lib.gnnvc_forward_audited_device(None, None, None, None) == -1
    assert lib.gnnvc_audit_stage_device(None, 0, 0, 0, None, None, None) == -1


def test_binding_has_the_methods():
    for name in ("forward_audited", "forward_audited_device", "audit_stage_device"):
        assert callable(getattr(G.Engine, name, None)), name
    assert G.GnnvcError(-6, "x").is_audit
