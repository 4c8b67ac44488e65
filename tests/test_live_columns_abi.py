"""CPU-side checks of gnnvc_set_generic_live_columns (generic graph stages gather only the live columns of their input, opt-in): the
header declares and documents it in its place, the library exports it, the binding lists it with its argument types and has its
method, a null engine is refused, the documents name the call and its info keys, the option table does not hold it, and the ABI
version has not moved.  No compute calls here (tests/test_gpu_live_columns.py has those)."""
import ctypes as C
import pathlib
import re

import pytest

import gnn_mwvc_amd as G

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "gnnvc.h").read_text()

NAME = "gnnvc_set_generic_live_columns"
PROTOTYPE = r"int gnnvc_set_generic_live_columns\(gnnvc_engine \*e, uint32_t max_percent\);"
INFO_KEY = "generic_live_columns"
STAGE_KEYS = ['"generic_live_kept_<s>"', '"generic_live_used_<s>"', '"generic_live_mask_lo_<s>"', '"generic_live_mask_hi_<s>"']


@pytest.fixture(scope="module")
def lib():
    G.build_library()
    return G.load_library()


def test_header_declares_the_entry_point_behind_patterns():
    assert re.search(PROTOTYPE, HEADER), f"{NAME} is not declared with the agreed signature"
    patterns = HEADER.index("int gnnvc_set_generic_patterns(gnnvc_engine *e")
    mine = HEADER.index("int gnnvc_set_generic_live_columns(gnnvc_engine *e")
    assert patterns < mine < HEADER.index("int gnnvc_num_layers(")
    assert not re.search(r"^int gnnvc_", HEADER[patterns + 10: mine], flags=re.M), "another entry point stands between the two"
    assert not re.search(r"^int gnnvc_", HEADER[mine + 10: HEADER.index("int gnnvc_num_layers(")], flags=re.M)
    feat = HEADER.index("int gnnvc_set_generic_feature_width(gnnvc_engine *e")
    assert not re.search(r"^int gnnvc_", HEADER[feat + 10: patterns], flags=re.M), "nothing may stand between feature_width and patterns"


def test_the_comment_in_front_of_the_prototype_is_its_own():
    doc = HEADER[HEADER.index("int gnnvc_set_generic_patterns(gnnvc_engine *e"): HEADER.index("int gnnvc_set_generic_live_columns(gnnvc_engine *e")]
    for word in ("max_percent", "kept * 100 <= max_percent * f", "0x7fffffff", "denormal", "GNNVC_ERR_UNSUPPORTED", "GNNVC_ERR_INVALID",
                 "next forward", "bit-identical", "k_any_live_mask", "k_any_live_pack", "k_audit_any", "f == 1", "bare linear layer",
                 "gnnvc_stage_forward_device", "gnnvc_audit_stage_device", "sliced", "gnnvc_create_multi_generic", "Heavy and giant rows",
                 "gnnvc_set_generic_big_stages", "gnnvc_set_generic_feature_width", "gnnvc_set_generic_patterns", "one copy and one wait",
                 f'"{INFO_KEY}"', *STAGE_KEYS):
        assert word in doc, word


def test_the_generic_stages_paragraph_names_the_call_and_its_keys():
    generic = HEADER[HEADER.index('"generic_stages" 0|1|2'): HEADER.index("gnnvc_get_info keys (further)")]
    assert NAME in generic and f'"{INFO_KEY}"' in generic
    for key in STAGE_KEYS:
        assert key in generic, key


def test_abi_version_is_still_1(lib):
    assert re.search(r"#define GNNVC_ABI_VERSION 1\b", HEADER)
    assert lib.gnnvc_abi_version() == 1


def test_library_exports_the_entry_point_and_the_binding_types_it(lib):
    assert NAME in G.engine.ABI_SYMBOLS
    fn = getattr(lib, NAME)
    assert fn is not None and fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_uint32]


def test_null_engine_is_rejected(lib):
    for value in (0, 1, 100, 101, 0xFFFFFFFF):
        assert lib.gnnvc_set_generic_live_columns(None, value) == -1
        assert lib.gnnvc_set_generic_live_columns(None, value) == lib.gnnvc_set_generic_patterns(None, 0)


def test_binding_has_the_method():
    fn = getattr(G.Engine, "set_generic_live_columns", None)
    assert callable(fn)
    assert f'"{INFO_KEY}"' in fn.__doc__ and NAME in fn.__doc__
    for key in STAGE_KEYS:
        assert key in fn.__doc__, key


def test_the_option_table_is_not_where_it_lives():
    table = (ROOT / "gnn-mwvc_amd" / "csrc" / "gnnvc_options.h").read_text()
    assert "generic_live" not in table and "live_columns" not in table.lower()


def test_the_config_struct_of_the_multi_device_call_is_untouched():
    struct = HEADER[HEADER.index("typedef struct gnnvc_generic_config"): HEADER.index("} gnnvc_generic_config;")]
    assert "live" not in struct


@pytest.mark.parametrize("doc", ["INTEGRATION.md", "README.md"])
def test_the_documents_name_the_call_and_its_keys(doc):
    text = (ROOT / doc).read_text()
    assert NAME in text and INFO_KEY in text and "set_generic_live_columns" in text, doc
    for key in ("generic_live_kept_", "generic_live_used_", "generic_live_mask_lo_", "generic_live_mask_hi_"):
        assert key in text, (doc, key)


def test_design_names_the_call_and_restates_the_lemma():
    text = (ROOT / "DESIGN.md").read_text()
    assert NAME in text and "Live columns" in text
    section = text[text.index("Live columns"):]
    for word in ("-0.0f", "+0.0f", "round-to-nearest", "k_any_live_mask", "k_any_live_pack"):
        assert word in section, word
