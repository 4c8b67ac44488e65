"""CPU-side checks of gnnvc_set_generic_heavy_rows (the heavy rows of generic stages): the header declares and documents it, the
library exports it, the binding has its method, a null engine is refused, and the ABI version has not moved.  No compute calls
here (tests/test_gpu_heavy_rows.py has those)."""
import ctypes as C
import pathlib
import re

import pytest

import gnn_mwvc_amd as G

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "gnnvc.h").read_text()

NAME = "gnnvc_set_generic_heavy_rows"
PROTOTYPE = r"int gnnvc_set_generic_heavy_rows\(gnnvc_engine \*e, uint32_t from_degree\);"
INFO_KEYS = ("generic_heavy_from", "generic_heavy_rows", "generic_heavy_entries", "generic_heavy_last_rows")


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
    assert "k_any_heavy_sums" in comments and "512" in comments


def test_the_generic_stages_paragraph_names_the_call():
    generic = HEADER[HEADER.index('"generic_stages" 0|1|2'): HEADER.index("gnnvc_get_info keys (further)")]
    assert NAME in generic


def test_abi_version_is_still_1(lib):
    assert re.search(r"#define GNNVC_ABI_VERSION 1\b", HEADER)
    assert lib.gnnvc_abi_version() == 1


def test_library_exports_the_entry_point(lib):
    assert NAME in G.engine.ABI_SYMBOLS
    fn = getattr(lib, NAME)
    assert fn is not None and fn.restype is C.c_int and fn.argtypes


def test_null_engine_is_rejected(lib):
    for value in (0, 1, 512, 0xFFFFFFFF):
        assert lib.gnnvc_set_generic_heavy_rows(None, value) == -1


def test_binding_has_the_method():
    assert callable(getattr(G.Engine, "set_generic_heavy_rows", None))
