"""CPU-side checks of gnnvc_set_generic_giant_rows (the giant rows of generic stages): the header declares and documents it, the
library exports it, the binding has its method, a null engine is refused, and the ABI version has not moved.  No compute calls
here (tests/test_gpu_giant_rows.py has those)."""
import ctypes as C
import pathlib
import re

import pytest

import gnn_mwvc_amd as G

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "gnnvc.h").read_text()

NAME = "gnnvc_set_generic_giant_rows"
PROTOTYPE = r"int gnnvc_set_generic_giant_rows\(gnnvc_engine \*e, uint32_t from_degree, int segments\);"
INFO_KEYS = ("generic_giant_from", "generic_giant_segments", "generic_giant_rows", "generic_giant_entries",
             "generic_giant_last_rows", "generic_giant_last_segmented")


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
    assert "k_any_giant_gather" in comments and "k_giant_sum" in comments and "16 384" in comments


def test_the_comment_in_front_of_the_prototype_is_its_own():
    doc = HEADER[HEADER.index("int gnnvc_set_generic_heavy_rows(gnnvc_engine *e"): HEADER.index("int gnnvc_set_generic_giant_rows(gnnvc_engine *e")]
    for word in ("from_degree", "segments", "-1", "GNNVC_ERR_UNSUPPORTED", "GNNVC_ERR_INVALID") + INFO_KEYS:
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
    assert fn is not None and fn.restype is C.c_int and len(fn.argtypes) == 3


def test_null_engine_is_rejected(lib):
    for value in (0, 1, 16384, 0xFFFFFFFF):
        for seg in (-1, 0, 1):
            assert lib.gnnvc_set_generic_giant_rows(None, value, seg) == -1


def test_binding_has_the_method():
    assert callable(getattr(G.Engine, "set_generic_giant_rows", None))
