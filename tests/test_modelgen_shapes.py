"""tools/modelgen_shapes.py: models of other layer widths than the trained one (what the generic fused stage, k_stage_any,
runs).  On the ORACLE: every text parses, the layer-by-layer walk that tests/test_gpu_shapes.py takes its per-stage references
from equals predict, and every member's logits are finite and vary over the vertices (random ReLU units die; a model whose
output were constant would test nothing).

And a record, not a requirement: at which of the new (k, n) shapes the SciPy-bundled OpenBLAS cblas_sgemm agrees bit for bit
with the oracle's sequential fma chain (tests/test_openblas_seam.py checks the nine trained shapes).  The contract for these
models is the oracle's chain; the record says where a stock OpenBLAS build of the reference would agree with it.  Every shape
is tried in a child process of its own, so that a crash inside the bundled library is a line of the record too."""
import json
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from oracle import oracle_py
from tools import graphgen as gg
from tools import modelgen_shapes as ms
from tests.generic_harness import bits, stage_outputs
from tests.test_openblas_seam import _find_openblas

GRAPHS = {
    "er3000": lambda: gg.erdos_renyi(3000, 15000, 15),
    "hub2k": lambda: gg.hub_graph(2000, 6000, 2, 700, seed=5),
}


@pytest.fixture(scope="module")
def graphs():
    return {k: f() for k, f in GRAPHS.items()}


@pytest.mark.parametrize("name", list(ms.SPECS))
def test_text_parses_and_has_the_named_shapes(name):
    text = ms.FAMILY[name]()
    assert text == ms.FAMILY[name]()   # from the seed alone
    om = oracle_py.OracleModel(text)
    assert om.n_layers == ms.num_layers(name) == 7 * len(ms.SPECS[name][1])
    kinds = om.layer_kinds()
    assert [i for i, k in enumerate(kinds) if k == 0] == [7 * s + d for s in range(om.n_layers // 7) for d in (1, 3, 5)]
    assert [tuple(W.shape) for W, _ in om.linear_params()] == ms.linear_shapes(name)
    assert ms.linear_shapes(name)[0][0] == 2 * ms.in_width(name) + 3
    for (W, b), (W2, b2) in zip(ms.layers_of(name), om.linear_params()):
        assert np.array_equal(bits(W), bits(W2)) and np.array_equal(bits(b), bits(b2))


def test_the_required_members_are_there():
    S = ms.SPECS
    assert S["narrow"] == (1, [(8, 8, 4), (8, 8, 4), (8, 4, 1)])
    assert S["wide"] == (1, [(64, 64, 32), (64, 64, 32), (64, 32, 1)])
    assert S["odd"] == (1, [(7, 13, 5), (19, 3, 9), (11, 6, 1)])
    assert S["two_stage"] == (1, [(24, 24, 12), (24, 12, 1)])
    assert S["deep5"] == (1, [(16, 16, 8)] * 4 + [(16, 8, 1)])
    assert S["in3"][0] == 3 and ms.linear_shapes("in3")[0][0] == 9
    assert S["out4"][1][-1] == (32, 16, 4) and ms.out_width("out4") == 4
    assert S["first_trained"] == (1, [(32, 32, 16), (40, 40, 20), (40, 20, 1)])
    assert S["first_trained"][1][0] == ms.TRAINED[0]
    from tools import modelgen as mg
    assert not set(S) & set(mg.FAMILY)


@pytest.mark.parametrize("name", list(ms.SPECS))
def test_walk_equals_predict_and_logits_are_alive(graphs, name):
    om = oracle_py.OracleModel(ms.FAMILY[name]())
    for gname, g in graphs.items():
        om.set_weight_scale(g.ws)
        x = ms.model_input(name, g)
        assert x.shape == (g.n, ms.in_width(name))
        st = stage_outputs(om, "shapes", name, g)
        assert [(a.shape[1], b.shape[1]) for a, b, _ in st] == ms.stage_widths(name)
        logits = om.predict(g, x, stop_after=om.n_layers - 2)
        scores = om.predict(g, x)
        assert logits.shape == (g.n, ms.out_width(name))
        assert np.array_equal(bits(st[-1][2]), bits(logits)), (name, gname)
        assert np.array_equal(bits(st[-1][1]), bits(scores)), (name, gname)
        # alive: finite, and not one value for every vertex — in every output column
        assert np.isfinite(logits).all() and np.isfinite(scores).all(), (name, gname)
        for c in range(logits.shape[1]):
            assert np.unique(bits(logits[:, c])).size > g.n // 20, (name, gname, c, np.unique(bits(logits[:, c])).size)
        # and every stage hands something on: no stage output is all zero
        for s, (_, h, _) in enumerate(st):
            assert (h != 0).any(), (name, gname, s)


_CHILD = textwrap.dedent("""
    import ctypes as C, json, sys
    import numpy as np
    path, k, n, threads = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    lib = C.CDLL(path)
    fn = lib.scipy_cblas_sgemm
    fn.restype = None
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                   C.c_float, C.c_void_p, C.c_int]
    st = getattr(lib, "scipy_openblas_set_num_threads", None)
    if st is not None:
        st(threads)
    rng = np.random.default_rng([11, k, n])
    rows = 4099
    a = rng.uniform(-3, 3, size=(rows, k)).astype(np.float32)
    a[rng.random(a.shape) < 0.2] = 0.0
    W = rng.uniform(-0.5, 0.5, size=(k, n)).astype(np.float32)
    c = np.full((rows, n), np.nan, dtype=np.float32)
    fn(101, 111, 111, rows, n, k, 1.0, a.ctypes.data, k, W.ctypes.data, n, 0.0, c.ctypes.data, n)
    np.save(sys.argv[5], c)
    print("done")
""")


def test_record_openblas_seam_at_the_new_shapes(tmp_path, capsys):
    """RECORDED, not required (see the module docstring).  The result goes to the captured output (pytest -s shows it) and
    DESIGN.md §3 keeps what was found when this was written."""
    path = _find_openblas()
    if not path:
        pytest.skip("no bundled LP64 OpenBLAS in this environment")
    shapes = sorted({s for name in ms.SPECS for s in ms.linear_shapes(name)})
    record = {}
    for (k, n) in shapes:
        for threads in (1, 4):
            out = tmp_path / f"c_{k}_{n}_{threads}.npy"
            r = subprocess.run([sys.executable, "-c", _CHILD, path, str(k), str(n), str(threads), str(out)],
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0 or "done" not in r.stdout:
                record[f"{k}x{n}/t{threads}"] = f"child ended with status {r.returncode}"
                continue
            rng = np.random.default_rng([11, k, n])
            rows = 4099
            a = rng.uniform(-3, 3, size=(rows, k)).astype(np.float32)
            a[rng.random(a.shape) < 0.2] = 0.0
            W = rng.uniform(-0.5, 0.5, size=(k, n)).astype(np.float32)
            want = oracle_py.linear_layer(a, W, np.zeros(n, dtype=np.float32))
            got = (np.load(out) + np.zeros((1, n), dtype=np.float32)).astype(np.float32)
            diff = int((bits(got) != bits(want)).sum())
            record[f"{k}x{n}/t{threads}"] = "identical" if diff == 0 else f"{diff} of {got.size} values differ"
    with capsys.disabled():
        print("\nOpenBLAS seam at the generic shapes (k x n / threads):", json.dumps(record, indent=1))
    assert len(record) == 2 * len(shapes)
