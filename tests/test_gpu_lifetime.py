"""gnnvc_destroy frees everything an engine allocated.  The library counts the device / page-locked allocations, events and
streams its owning handles hold (csrc/gnnvc_device_mem.h; read through gnnvc_debug_probe(NULL, 1000), which is no part of
include/gnnvc.h), so "nothing is left" is an exact assertion — free-memory readings on a shared device would not give one."""
import ctypes as C
import gc

import numpy as np
import pytest

from tools import graphgen as gg

pytestmark = pytest.mark.gpu

PROBE_LIVE_OBJECTS = 1000


@pytest.fixture(scope="module")
def live():
    import gnn_mwvc_amd as G
    L = G.load_library()
    L.gnnvc_debug_probe.argtypes = [C.c_void_p, C.c_int]
    L.gnnvc_debug_probe.restype = C.c_int
    return lambda: L.gnnvc_debug_probe(None, PROBE_LIVE_OBJECTS)


def _two_hubs(n, degrees, sparse_edges, seed):
    """n vertices, vertex i < len(degrees) adjacent to degrees[i] others, and a few random edges among the rest."""
    rng = np.random.default_rng(seed)
    hubs = len(degrees)
    a = [np.full(d, i) for i, d in enumerate(degrees)]
    b = [rng.choice(np.arange(hubs, n), size=d, replace=False) for d in degrees]
    u = rng.integers(hubs, n, size=sparse_edges)
    v = rng.integers(hubs, n, size=sparse_edges)
    u, v = np.concatenate(a + [u[u != v]]), np.concatenate(b + [v[u != v]])
    key = np.unique(np.minimum(u, v).astype(np.int64) * n + np.maximum(u, v))
    return gg.csr_from_pairs(n, key // n, key % n, rng.integers(20, 121, size=n))


# every plan at these sizes (the options tests/test_gpu_parity.py, test_gpu_fuzz.py force them with): the hubs as long and giant
# rows, the pruned adjacency, the LDS-table, compact-table and column-blocked plans, sorted tiles, table tiles; events of the
# stage timing and the kernel trace
HUB_OPTIONS = {"long_row_threshold": 64, "giant_row_threshold": 64, "prune_min_entries": 0, "prune_min_drop_percent": 1,
               "blocked_min_n": 0, "compact_min_n": 0, "plans_at_handoff": 2, "handoff_min_entries": 1,
               "compact_first_forward_entries": 1, "compact_gather": 2, "lds_table": 2, "sorted_tiles": 1, "sorted_min_nnz": 0,
               "table_tiles_min_n": 0, "forward_timing": 2, "kernel_trace": 1}

CASES = {
    "er_defaults": (lambda: (gg.erdos_renyi(3000, 12000, 3), gg.erdos_renyi(2000, 7000, 4)), {}, None),
    "hubs_every_plan": (lambda: (_two_hubs(600, (300, 500), 1500, 5), _two_hubs(600, (500, 300), 1200, 6)), HUB_OPTIONS, None),
    "er_two_parts": (lambda: (gg.erdos_renyi(3000, 12000, 3), gg.erdos_renyi(2000, 7000, 4)), {}, [0, 0]),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_destroy_frees_everything(model_text, live, case):
    import gnn_mwvc_amd as G
    graphs, options, devices = CASES[case]
    first, second = graphs()
    gc.collect()   # (an engine an earlier test left to the collector goes now, not between the two readings)
    start = live()
    peak = start
    for _ in range(3):
        e = G.Engine(model_text, devices=devices) if devices else G.Engine(model_text, device=0)
        try:
            for k, v in options.items():
                e.set_option(k, v)
            e.set_weight_scale(first.ws)
            e.upload_graph(first)
            e.forward(first.x())
            e.forward(first.x())
            if case == "hubs_every_plan":   # (the test cannot pass by allocating nothing)
                assert e.get_info("long_rows") > 0 and e.get_info("giant_rows") > 0
            e.set_weight_scale(second.ws)
            if devices:
                e.upload_graph(second)
            else:
                e.upload_graph_staged(second)   # (the page-locked staging buffers)
            e.forward(second.x())
            peak = max(peak, live())
        finally:
            e.close()
    assert peak > start + 10, (start, peak)
    assert live() == start


def test_host_entry_points_keep_nothing(model_text, live):
    """gnnvc_linear_forward, gnnvc_sgemm and gnnvc_stream_sum allocate for the call and free on the way out."""
    import gnn_mwvc_amd as G
    rng = np.random.default_rng(11)
    gc.collect()
    start = live()
    e = G.Engine(model_text, device=0)
    try:
        e.relu(np.zeros(64, dtype=np.float32))   # (the engine's own scratch rows, kept until it goes: sized for the calls below)
        h, W, b = (rng.standard_normal(s).astype(np.float32) for s in ((4, 5), (5, 3), (3,)))
        before = live()
        out = e.linear(h, W, b)
        assert live() == before
        np.testing.assert_allclose(out, h @ W + b, rtol=0, atol=1e-5)   # (five products of magnitude < 10: a few fp32 roundings of 6e-7 each)
        before = live()
        out = e.sgemm(h, W)
        assert live() == before
        np.testing.assert_allclose(out, h @ W, rtol=0, atol=1e-5)
        v = rng.uniform(0, 2, (3, 70)).astype(np.float32)
        before = live()
        sums = e.stream_sum(v)
        assert live() == before
        assert np.array_equal(sums, np.cumsum(v, axis=1, dtype=np.float32)[:, -1])   # (the sequential fp32 chain, test_exact_sum_host.py)
    finally:
        e.close()
    assert live() == start
