"""The engine's host state keeps its three lifetimes apart (csrc/gnnvc_engine_state.h), checked without a GPU.

What belongs to the resident graph sits in gnnvc_engine::PerGraph, and reset_graph_state replaces it in one assignment.  That is
safe only while PerGraph is plain data: the header says so in two static asserts, which a translation unit that does nothing but
include the header exercises here.  The second test reads the two host sources: one body of reset_graph_state, of one statement,
and no hand-written clearing of the row classes outside the functions that own them."""
import pathlib
import re
import subprocess

import pytest

from tests.test_kernel_waves import CSRC, _hipcc, _make_var

SOURCES = ("gnnvc_engine.cpp", "gnnvc_plans.cpp")


def test_per_graph_state_is_plain_data(tmp_path):
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc on this machine")
    mk = (CSRC / "Makefile").read_text()
    header = (CSRC / "gnnvc_engine_state.h").read_text()
    for trait in ("is_trivially_destructible_v", "is_trivially_copyable_v"):
        assert re.search(rf"static_assert\(std::{trait}<gnnvc_engine::PerGraph>\)", header), trait
    tu = tmp_path / "layout.cpp"
    tu.write_text('#include "gnnvc_engine_state.h"\n'
                  "static_assert(sizeof(gnnvc_engine::PerGraph) > 0);\n"
                  "int main() { return 0; }\n")
    r = subprocess.run([hipcc, f"--offload-arch={_make_var(mk, 'ARCH')}", *_make_var(mk, "CXXFLAGS").split(), "-fsyntax-only",
                        f"-I{CSRC}", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def _functions(text):
    """{name: [body, ...]} of the functions defined at the left margin (a body ends at the first closing brace there)."""
    out = {}
    for m in re.finditer(r"^[A-Za-z_][^\n;{}]*?\b(\w+)\([^;{}]*\)\s*\{\n(.*?)^\}", text, re.M | re.S):
        out.setdefault(m.group(1), []).append(m.group(2))
    return out


def test_one_reset_and_no_hand_patches():
    bodies, strays = [], []
    for name in SOURCES:
        text = (CSRC / name).read_text()
        funcs = _functions(text)
        bodies += funcs.get("reset_graph_state", [])
        owned = "".join(b for f in ("find_long", "find_giant") for b in funcs.get(f, []))
        for pat in (r"n_long = ", r"n_giant = "):
            strays += [f"{name}: {pat}"] * (len(re.findall(pat, text)) - len(re.findall(pat, owned)))
    assert len(bodies) == 1, bodies
    statements = [s for s in bodies[0].split(";") if s.strip()]
    assert len(statements) == 1 and re.fullmatch(r"\s*e->pg = gnnvc_engine::PerGraph\{\}", statements[0]), bodies[0]
    assert not strays, strays
