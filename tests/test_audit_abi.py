"""CPU-side checks of the on-device audit's ABI (options "audit_*", GNNVC_ERR_AUDIT): the header defines the code and
documents the options and read-outs, the library names the code, the binding exposes it.  No compute calls here."""
import pathlib
import re

import pytest

import gnn_mwvc_amd as G

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "gnnvc.h").read_text()


@pytest.fixture(scope="module")
def lib():
    G.build_library()
    return G.load_library()


def test_header_defines_the_audit_code():
    m = re.search(r"\bGNNVC_ERR_AUDIT\s*=\s*(-?\d+)", HEADER)
    assert m and int(m.group(1)) == -6
    assert re.search(r"#define GNNVC_ABI_VERSION 1\b", HEADER)


def test_strerror_names_the_audit_code(lib):
    text = lib.gnnvc_strerror(-6)
    assert text and text != lib.gnnvc_strerror(-99)   # its own text, not the default one
    assert b"audit" in text


@pytest.mark.parametrize("key", ["audit_period", "audit_repair", "audit_flip_stage", "audit_flip_row", "audit_quiet"])
def test_audit_options_are_documented(key):
    assert f'"{key}"' in HEADER


@pytest.mark.parametrize("key", G.engine.AUDIT_KEYS)
def test_audit_read_outs_are_documented(key):
    assert f'"{key}"' in HEADER


def test_binding_exposes_the_code():
    assert G.ERR_AUDIT == -6
    assert G.GnnvcError(-6, "x").is_audit and not G.GnnvcError(-4, "x").is_audit
    assert hasattr(G.Engine, "audit_report")
