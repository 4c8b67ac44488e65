"""CPU-side checks of gnnvc_set_generic_patterns (generic models with a dense prologue or an open ending fused too, opt-in): the
header declares and documents it, the library exports it, the binding lists it with its argument types and has its method, a
null engine is refused, the documents name the call and its info key, the option table does not hold it, and the ABI version has
not moved.  No compute calls here (tests/test_gpu_patterns.py has those)."""
import ctypes as C
import pathlib
import re

import pytest

import gnn_mwvc_amd as G

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "gnnvc.h").read_text()

NAME = "gnnvc_set_generic_patterns"
PROTOTYPE = r"int gnnvc_set_generic_patterns\(gnnvc_engine \*e, uint32_t mask\);"
INFO_KEY = "generic_patterns"


@pytest.fixture(scope="module")
def lib():
    G.build_library()
    return G.load_library()


def test_header_declares_the_entry_point_next_to_feature_width():
    assert re.search(PROTOTYPE, HEADER), f"{NAME} is not declared with the agreed signature"
    feat = HEADER.index("int gnnvc_set_generic_feature_width(gnnvc_engine *e")
    mine = HEADER.index("int gnnvc_set_generic_patterns(gnnvc_engine *e")
    assert feat < mine < HEADER.index("int gnnvc_num_layers(")
    assert not re.search(r"^int gnnvc_", HEADER[feat + 10: mine], flags=re.M), "another entry point stands between the two"


def test_the_bits_are_defined():
    assert re.search(r"^#define GNNVC_PATTERN_PROLOGUE 1u?$", HEADER, flags=re.M)
    assert re.search(r"^#define GNNVC_PATTERN_OPEN_END 2u?$", HEADER, flags=re.M)
    assert (G.engine.PATTERN_PROLOGUE, G.engine.PATTERN_OPEN_END) == (1, 2)


def test_the_comment_in_front_of_the_prototype_is_its_own():
    doc = HEADER[HEADER.index("int gnnvc_set_generic_feature_width(gnnvc_engine *e"): HEADER.index("int gnnvc_set_generic_patterns(gnnvc_engine *e")]
    for word in ("mask", "GNNVC_PATTERN_PROLOGUE", "GNNVC_PATTERN_OPEN_END", "GNNVC_ERR_UNSUPPORTED", "GNNVC_ERR_INVALID", "at once",
                 "gnnvc_set_generic_big_stages", "gnnvc_set_generic_feature_width", "k_audit_any", "d_logits", "audit_period",
                 f'"{INFO_KEY}"', '"generic_stage_dense_<s>"', '"generic_stage_end_<s>"'):
        assert word in doc, word


def test_the_generic_stages_paragraph_names_the_call_and_its_keys():
    generic = HEADER[HEADER.index('"generic_stages" 0|1|2'): HEADER.index("gnnvc_get_info keys (further)")]
    assert NAME in generic and f'"{INFO_KEY}"' in generic
    assert '"generic_stage_dense_<s>"' in generic and '"generic_stage_end_<s>"' in generic


def test_abi_version_is_still_1(lib):
    assert re.search(r"#define GNNVC_ABI_VERSION 1\b", HEADER)
    assert lib.gnnvc_abi_version() == 1


def test_library_exports_the_entry_point_and_the_binding_types_it(lib):
    assert NAME in G.engine.ABI_SYMBOLS
    fn = getattr(lib, NAME)
    assert fn is not None and fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_uint32]


def test_null_engine_is_rejected(lib):
    for value in (0, 1, 2, 3, 4, 0xFFFFFFFF):
        assert lib.gnnvc_set_generic_patterns(None, value) == -1
        assert lib.gnnvc_set_generic_patterns(None, value) == lib.gnnvc_set_generic_feature_width(None, 0) == lib.gnnvc_set_generic_big_stages(None, 0)


def test_binding_has_the_method():
    fn = getattr(G.Engine, "set_generic_patterns", None)
    assert callable(fn)
    assert f'"{INFO_KEY}"' in fn.__doc__ and NAME in fn.__doc__
    assert '"generic_stage_dense_<s>"' in fn.__doc__ and '"generic_stage_end_<s>"' in fn.__doc__


def test_the_option_table_is_not_where_it_lives():
    table = (ROOT / "gnn-mwvc_amd" / "csrc" / "gnnvc_options.h").read_text()
    assert "generic_patterns" not in table and "prologue" not in table.lower() and "open_end" not in table.lower()


@pytest.mark.parametrize("doc", ["INTEGRATION.md", "README.md"])
def test_the_documents_name_the_call_and_its_key(doc):
    text = (ROOT / doc).read_text()
    assert NAME in text and INFO_KEY in text and "set_generic_patterns" in text, doc
    assert "generic_stage_dense_" in text and "generic_stage_end_" in text, doc


def test_design_names_the_call():
    assert NAME in (ROOT / "DESIGN.md").read_text()
