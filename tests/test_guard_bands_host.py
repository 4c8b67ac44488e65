"""The guard-band registry of gnn-mwvc_amd/csrc/gnnvc_device_mem.h on the host: tests/support/guard_host.cpp, a program of its
own, instantiates Buffer and GuardRegistry over malloc memory and runs every scenario under the address and undefined-behaviour
sanitizers (nothing is loaded into Python).  The device side of the same code is tests/test_gpu_guard_bands.py."""
import os
import pathlib
import subprocess

import pytest

HERE = pathlib.Path(__file__).resolve().parent
SRC = HERE / "support" / "guard_host.cpp"
HDR = HERE.parent / "gnn-mwvc_amd" / "csrc" / "gnnvc_device_mem.h"
EXE = HERE / "support" / "guard_host"
ROCM = pathlib.Path(os.environ.get("ROCM_PATH", "/opt/rocm"))   # (the header names HIP's types; no HIP call is linked)

SCENARIOS = ["switch_on_off_on", "sizes_and_edges", "hooks", "damage_found_at_free", "growth", "moves", "threads", "devices",
             "allocated_on_freed_off", "nothing_left"]


@pytest.fixture(scope="module")
def ran():
    if not EXE.exists() or EXE.stat().st_mtime < max(SRC.stat().st_mtime, HDR.stat().st_mtime):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-isystem", str(ROCM / "include"),
                        "-pthread", "-o", str(EXE), str(SRC)], check=True)
    try:   # (seconds on one core; a program that stalls fails here, with the scenarios it got through)
        return subprocess.run([str(EXE)], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as stalled:
        done = stalled.stdout.decode() if isinstance(stalled.stdout, bytes) else (stalled.stdout or "")
        pytest.fail(f"{EXE.name} did not finish in 120 s; scenarios printed so far:\n{done}")


def test_every_scenario_passes(ran):
    assert ran.returncode == 0, ran.stdout + ran.stderr     # (a sanitizer report ends the program with a non-zero code)
    assert ran.stdout.splitlines() == [f"{name}: ok" for name in SCENARIOS]


def test_each_damaged_band_is_reported_once(ran):
    """One stderr line per damaged band, with what finds the buffer among the reserve sites: bytes, element size, side and the
    offset of the first damaged byte.  The hooks scenario hits a 12-byte buffer of floats after its end, before its start and
    at the trailing band's end, then the 20-byte one before its start."""
    lines = [line for line in ran.stderr.splitlines() if line.startswith("gnnvc guard")]
    hooks = [line for line in lines if " 12 bytes, element size 4," in line and "(check)" in line and "0x5a" in line]
    assert [line.rsplit(": ", 1)[1] for line in hooks] == [
        "trailing band damaged, first at offset 0, value 0x5a",
        "leading band damaged, first at offset 4095, value 0x5a",
        "trailing band damaged, first at offset 4095, value 0x5a"]
    assert sum(" 20 bytes, element size 4," in line and "0x5a" in line for line in lines) == 1
    # damage_found_at_free: both bands of a 6-byte buffer of 2-byte elements, seen by the free
    at_free = [line for line in lines if "(free)" in line and " 6 bytes, element size 2," in line]
    assert [line.rsplit(": ", 1)[1] for line in at_free] == [
        "leading band damaged, first at offset 4095, value 0x00",
        "trailing band damaged, first at offset 0, value 0x00"]
