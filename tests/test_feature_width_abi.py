"""CPU-side checks of gnnvc_set_generic_feature_width (generic stages whose feature width and last layer are up to 64 wide, opt-in):
the header declares and documents it, the library exports it, the binding lists it with its argument types and has its method, a
null engine is refused, the documents name the call and its info key, and the ABI version has not moved.  No compute calls here
(tests/test_gpu_feature_width.py has those)."""
import ctypes as C
import pathlib
import re

import pytest

import gnn_mwvc_amd as G

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "gnnvc.h").read_text()

NAME = "gnnvc_set_generic_feature_width"
PROTOTYPE = r"int gnnvc_set_generic_feature_width\(gnnvc_engine \*e, uint32_t max_width\);"
INFO_KEY = "generic_feature_width"


@pytest.fixture(scope="module")
def lib():
    G.build_library()
    return G.load_library()


def test_header_declares_the_entry_point_next_to_big_stages():
    assert re.search(PROTOTYPE, HEADER), f"{NAME} is not declared with the agreed signature"
    big = HEADER.index("int gnnvc_set_generic_big_stages(gnnvc_engine *e")
    mine = HEADER.index("int gnnvc_set_generic_feature_width(gnnvc_engine *e")
    assert big < mine < HEADER.index("int gnnvc_num_layers(")
    assert not re.search(r"^int gnnvc_", HEADER[big + 10: mine], flags=re.M), "another entry point stands between the two"


def test_the_comment_in_front_of_the_prototype_is_its_own():
    doc = HEADER[HEADER.index("int gnnvc_set_generic_big_stages(gnnvc_engine *e"): HEADER.index("int gnnvc_set_generic_feature_width(gnnvc_engine *e")]
    for word in ("max_width", "33 .. 64", "GNNVC_ERR_UNSUPPORTED", "GNNVC_ERR_INVALID", "at once", "gnnvc_set_generic_big_stages",
                 "k_audit_any", "k_any_heavy_sums", "k_any_giant_gather", f'"{INFO_KEY}"'):
        assert word in doc, word


def test_the_generic_stages_paragraph_names_the_call_and_its_key():
    generic = HEADER[HEADER.index('"generic_stages" 0|1|2'): HEADER.index("gnnvc_get_info keys (further)")]
    assert NAME in generic and f'"{INFO_KEY}"' in generic


def test_abi_version_is_still_1(lib):
    assert re.search(r"#define GNNVC_ABI_VERSION 1\b", HEADER)
    assert lib.gnnvc_abi_version() == 1


def test_library_exports_the_entry_point_and_the_binding_types_it(lib):
    assert NAME in G.engine.ABI_SYMBOLS
    fn = getattr(lib, NAME)
    assert fn is not None and fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_uint32]


def test_null_engine_is_rejected(lib):
    for value in (0, 1, 32, 33, 48, 64, 65, 0xFFFFFFFF):
        assert lib.gnnvc_set_generic_feature_width(None, value) == -1


def test_binding_has_the_method():
    fn = getattr(G.Engine, "set_generic_feature_width", None)
    assert callable(fn)
    assert f'"{INFO_KEY}"' in fn.__doc__ and NAME in fn.__doc__


def test_the_option_table_is_not_where_it_lives():
    table = (ROOT / "gnn-mwvc_amd" / "csrc" / "gnnvc_options.h").read_text()
    assert "feature_width" not in table


@pytest.mark.parametrize("doc", ["INTEGRATION.md", "README.md"])
def test_the_documents_name_the_call_and_its_key(doc):
    text = (ROOT / doc).read_text()
    assert NAME in text and INFO_KEY in text and "set_generic_feature_width" in text, doc


def test_design_names_the_call():
    assert NAME in (ROOT / "DESIGN.md").read_text()
