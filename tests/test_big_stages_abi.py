"""CPU-side checks of gnnvc_set_generic_big_stages (generic stages of up to 160 KiB of LDS and 128-wide hidden layers, opt-in): the
header declares and documents it, the library exports it, the binding has its method, a null engine is refused, and the ABI
version has not moved.  No compute calls here (tests/test_gpu_big_stages.py has those)."""
import ctypes as C
import pathlib
import re

import pytest

import gnn_mwvc_amd as G

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "gnnvc.h").read_text()

NAME = "gnnvc_set_generic_big_stages"
PROTOTYPE = r"int gnnvc_set_generic_big_stages\(gnnvc_engine \*e, uint32_t lds_bytes\);"
INFO_KEYS = ("generic_big_lds", "generic_stage_lds_bytes_<s>", "generic_stage_threads_<s>")


@pytest.fixture(scope="module")
def lib():
    G.build_library()
    return G.load_library()


def test_header_declares_and_documents_the_entry_point():
    assert re.search(PROTOTYPE, HEADER), f"{NAME} is not declared with the agreed signature"
    comments = " ".join(re.findall(r"/\*.*?\*/", HEADER, flags=re.S))
    assert re.search(rf"\b{NAME}\b", comments), f"{NAME} is not mentioned in any comment of the header"
    for key in INFO_KEYS:
        assert f'"{key}"' in comments, key


def test_the_comment_in_front_of_the_prototype_is_its_own():
    doc = HEADER[HEADER.index("int gnnvc_set_generic_giant_rows(gnnvc_engine *e"): HEADER.index("int gnnvc_set_generic_big_stages(gnnvc_engine *e")]
    for word in ("lds_bytes", "65 536", "163 840", "128", "256", "512", "1024", "GNNVC_ERR_UNSUPPORTED", "GNNVC_ERR_INVALID",
                 "at once", "k_audit_any") + INFO_KEYS:
        assert word in doc, word


def test_the_generic_stages_paragraph_names_the_call_and_its_keys():
    generic = HEADER[HEADER.index('"generic_stages" 0|1|2'): HEADER.index("gnnvc_get_info keys (further)")]
    assert NAME in generic
    for key in INFO_KEYS:
        assert f'"{key}"' in generic, key


def test_abi_version_is_still_1(lib):
    assert re.search(r"#define GNNVC_ABI_VERSION 1\b", HEADER)
    assert lib.gnnvc_abi_version() == 1


def test_library_exports_the_entry_point(lib):
    assert NAME in G.engine.ABI_SYMBOLS
    fn = getattr(lib, NAME)
    assert fn is not None and fn.restype is C.c_int and len(fn.argtypes) == 2


def test_null_engine_is_rejected(lib):
    for value in (0, 1, 65535, 65536, 99648, 163840, 163841, 0xFFFFFFFF):
        assert lib.gnnvc_set_generic_big_stages(None, value) == -1


def test_binding_has_the_method():
    fn = getattr(G.Engine, "set_generic_big_stages", None)
    assert callable(fn)
    for key in INFO_KEYS:
        assert f'"{key}"' in fn.__doc__, key
