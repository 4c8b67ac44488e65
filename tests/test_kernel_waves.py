"""Registers, LDS and waves per SIMD of the dense kernels on the metric route, as the compiler reports them (no GPU).

k_stage_f1 on the LDS-table route and the two k_dense_f16 instantiations run with seven and six waves per SIMD only as long as
nothing grows their LDS region or their register peak (csrc/gnnvc_kernels.hip: kSlimRegionFloats, GNNVC_ROUTE_C_GROUPS;
DESIGN.md section 5).  This compiles csrc/gnnvc_kernels.hip for the device with the Makefile's flags and reads the
kernel-resource-usage remarks of those kernels: resource figures only, no instructions.  Kernels are found by their template
arguments, decoded from the mangled names in the remarks."""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "gnn-mwvc_amd" / "csrc"


def _make_var(text, name):
    m = re.search(rf"^{name}\s*[:?]?=\s*(.*)$", text, re.M)
    assert m, name
    return m.group(1).strip()


def _hipcc():
    mk = (CSRC / "Makefile").read_text()
    exe = _make_var(mk, "HIPCC")
    return exe if pathlib.Path(exe).exists() else shutil.which("hipcc")


def template_args(mangled, kernel):
    """k_stage_f1ILi32ELi32ELi16ELi4ELb0ELb1EE... -> (32, 32, 16, 4, False, True); None for another function."""
    m = re.search(rf"\d+{kernel}I((?:L[ib]\d+E)+)E", mangled)
    if not m:
        return None
    return tuple(bool(int(v)) if t == "b" else int(v) for t, v in re.findall(r"L([ib])(\d+)E", m.group(1)))


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{(kernel, template arguments): {figure: value}} of every k_stage_f1 and k_dense_f16 instantiation."""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc on this machine")
    mk = (CSRC / "Makefile").read_text()
    flags = _make_var(mk, "CXXFLAGS").split()
    arch = _make_var(mk, "ARCH")
    obj = tmp_path_factory.mktemp("waves") / "gnnvc_kernels.o"
    r = subprocess.run([hipcc, f"--offload-arch={arch}", *flags, "--offload-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", "-o", str(obj), "gnnvc_kernels.hip"], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:\S+: )?\s*Function Name: (\S+)", line)
        if m:
            cur = None
            for kernel in ("k_stage_f1", "k_dense_f16"):
                args = template_args(m.group(1), kernel)
                if args is not None:
                    cur = out.setdefault((kernel, args), {})
            continue
        m = re.search(r"remark: (?:\S+: )?\s*([A-Za-z][A-Za-z /\[\]]*?): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    assert out, "no resource remarks read:\n" + r.stderr[-2000:]
    return out


SLIM = ("k_stage_f1", (32, 32, 16, 4, False, True))
FULL = [("k_stage_f1", (32, 32, 16, 4, False, False)), ("k_stage_f1", (32, 32, 16, 4, True, False))]
DENSE = [("k_dense_f16", (32, 32, 16, False)), ("k_dense_f16", (32, 16, 1, True))]


def test_template_arguments_are_decoded():
    name = "_ZN5gnnvc12_GLOBAL__N_110k_stage_f1ILi32ELi32ELi16ELi4ELb0ELb1EEEvNS_8GraphDevEfPKfPfS4_jj"
    assert template_args(name, "k_stage_f1") == (32, 32, 16, 4, False, True)
    assert template_args(name, "k_dense_f16") is None
    assert template_args("_ZN5gnnvc12_GLOBAL__N_111k_dense_f16ILi32ELi16ELi1ELb1EEEvNS_8GraphDevEf", "k_dense_f16") == (32, 16, 1, True)


def test_the_kernels_are_all_there(usage):
    for key in [SLIM] + FULL + DENSE:
        assert key in usage, (key, sorted(usage))
        for figure in ("VGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
            assert figure in usage[key], (key, figure, usage[key])


@pytest.mark.parametrize("key", [SLIM] + FULL + DENSE, ids=lambda k: f"{k[0]}<{', '.join(str(a).lower() for a in k[1])}>")
def test_no_scratch_and_no_spills(usage, key):
    u = usage[key]
    print(key, u)
    assert int(u["ScratchSize [bytes/lane]"]) == 0 and int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0, (key, u)


def test_slim_stage_kernel_runs_seven_waves(usage):
    u = usage[SLIM]
    print(SLIM, u)
    assert int(u["LDS Size [bytes/block]"]) == 17408, u
    assert int(u["Occupancy [waves/SIMD]"]) >= 7, u


@pytest.mark.parametrize("key", FULL, ids=["valu", "mfma"])
def test_full_region_instantiations_keep_their_lds(usage, key):
    assert int(usage[key]["LDS Size [bytes/block]"]) == 33792, (key, usage[key])


@pytest.mark.parametrize("key", DENSE, ids=["feature_stage", "last_stage"])
def test_dense_kernels_run_six_waves(usage, key):
    u = usage[key]
    print(key, u)
    assert int(u["Occupancy [waves/SIMD]"]) >= 6, (key, u)
