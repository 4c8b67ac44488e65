"""The backward pass on the GPU at the shapes, graphs, values and calls that tests/test_gpu_backward.py's tables — sized for the
shipped model — never reach: every (TK, TM) form of the parameter gradient's kernel and the edges of its tiles, both paths of the
input gradient and the switch between them, graph layers wider than 64, rows as long as the graph kernel's group of lanes and one
more or less, a symmetric multigraph that is summed, graphs that miss symmetry by one entry of thousands, denormal and non-finite
values through the linear and graph kernels, and the model-level calls and layer sequences nobody made.

Everything is bit for bit against tests/backward_reference.py (NaN with NaN), whose tables (TILE_SHAPES, DX_SHAPES, ...) these
tests run; tests/test_backward_reference.py checks on the CPU that those tables reach every form, and holds the reference at them
to float64."""
import numpy as np
import pytest

from tests import backward_reference as R
from tests import generic_harness as H
from tests.test_expf_restatement import shim   # noqa: F401  (the fixture that builds tests/support/libexpf_shim.so)
from tests.test_gpu_backward import ERR_UNSUPPORTED, NO_LAYERS, _code, _linear_inputs, _restated, _run_case, _shuffled_rows
from tests.test_gpu_backward import bare, engine, same   # noqa: F401  (bare: a fixture)
from tests.test_gpu_backward import test_linear_backward as _linear_case

pytestmark = pytest.mark.gpu

F32 = np.float32
TINY = float(np.finfo(np.float32).tiny)   # 2^-126


# ---------------------------------------------------------------- linear layer

@pytest.mark.parametrize("n,k,m", R.TILE_SHAPES)
def test_linear_backward_in_every_tile(bare, n, k, m):   # noqa: F811
    """As test_linear_backward runs its shapes: all three outputs, accumulated into crafted old values, each output alone (W
    alone: a tile of k rows; the bias alone: of one), and against gnnvc_sgemm where that is the same rule."""
    _linear_case(bare, n, k, m)


@pytest.mark.parametrize("n,k,m", R.DX_SHAPES)
def test_linear_input_gradient_on_both_paths(bare, n, k, m):   # noqa: F811
    h, W, go, _ = _linear_inputs(n, k, m)
    got = bare.linear_backward(h, W, go, want=("in",))[0]
    same(got, R.linear_backward(h, W, go)[0], (n, k, m, "grad_in"))
    same(got, bare.sgemm(go, W, trans_b=True), (n, k, m, "grad_in against sgemm"))


# ---------------------------------------------------------------- special values

def _small_input(n, f, seed):
    """Magnitudes from 2^-14 to 2^-3, both signs, some -0.0f.  Two of these scaled by 2^-60 each give products from 2^-148 to
    2^-126, every one denormal, and sums of them on both sides of 2^-126.  (H.crafted_input's 2^-20 .. 2^20 would leave nearly
    every product of two such factors either normal or zero: at (97, 20, 40) the reference then holds no denormal at all.)"""
    rng = np.random.default_rng(seed)
    v = np.ldexp(rng.uniform(1.0, 2.0, (n, f)), rng.integers(-14, -3, (n, f))).astype(F32)
    v = np.where(rng.random((n, f)) < 0.5, -v, v).astype(F32)
    v[rng.random((n, f)) < 0.05] = F32(-0.0)
    return np.ascontiguousarray(v, dtype=F32)


def _denormals(a):
    a = np.abs(np.asarray(a, dtype=F32))
    return int(((a > 0) & (a < TINY)).sum())


def test_denormals_are_kept(bare):   # noqa: F811
    """The reference keeps denormals (fmaf and adds on the host); a kernel that flushed them, in a product, a partial sum or a
    result, differs.  Each case asserts first that the reference's result holds denormal values and values that are not."""
    s = F32(2.0 ** -60)
    n, k, m = 97, 20, 40
    h, go = _small_input(n, k, 11) * s, _small_input(n, m, 12) * s
    W = H.crafted_input(k, m, 13)
    want = R.linear_backward(h, W, go)
    d = _denormals(want[1])   # (grad_bias has in = 1, unscaled: its sums are normal)
    print(f"grad_W: {d} of {want[1].size} reference values are denormal, {int((want[1] == 0).sum())} zero")
    assert d > want[1].size // 10 and (np.abs(want[1]) >= TINY).any()
    got = bare.linear_backward(h, W, go)
    for name, a, b in zip(("grad_in", "grad_W", "grad_bias"), got, want):
        same(a, b, ("denormal parameter gradient", name))
    # the input gradient on both paths: grad_out and W scaled
    for n, k, m in ((97, 20, 40), (3, 482, 17)):
        go, W = _small_input(n, m, 14 + k) * s, _small_input(k, m, 15 + k) * s
        want = R.linear_backward(np.zeros((n, k), F32), W, go)[0]
        d = _denormals(want)
        print(f"grad_in at k = {k}: {d} of {want.size} reference values are denormal, {int((want == 0).sum())} zero")
        assert d > want.size // 10 and (np.abs(want) >= TINY).any(), k
        same(bare.linear_backward(np.zeros((n, k), F32), W, go, want=("in",))[0], want, ("denormal input gradient", k))
    # the graph layer: every term is denormal
    g = R.graph_of("er1933")
    e = engine(NO_LAYERS, g)
    try:
        for f in (5, 65):
            go = H.crafted_input(g.n, 2 * f + 3, 16 + f) * F32(2.0 ** -130)
            want = R.graph_layer_backward(g, go)
            d = _denormals(want)
            print(f"graph layer f = {f}: {d} of {want.size} reference values are denormal, {int((want == 0).sum())} zero")
            assert d > want.size // 50, f
            same(e.graph_layer_backward(go), want, ("denormal graph layer", f))
    finally:
        e.close()


def test_non_finite_values_stay_where_they_belong(bare):   # noqa: F811
    """One NaN, one +inf and one -inf in grad_out and one +inf in the input: the reference says which outputs they reach — the
    column of grad_W and grad_bias, the input's row of grad_W, the row of grad_in — and every other output is finite, in the
    reference and, bit for bit, on the device.  Neither m = 40 nor ke = 21 fills its tile (48 columns, 32 rows): the padded
    lanes hold 0 * inf = NaN in accumulators that are dropped, and a kernel that let one into a live chain would show here."""
    n, k, m = 97, 20, 40
    h, W, go, old = _linear_inputs(n, k, m)
    go[5, 7], go[40, 13], go[70, 39] = np.nan, np.inf, -np.inf   # column 39: the tile's last live one
    h[50, 19] = np.inf                                             # row 19 of grad_W: the last in front of the bias
    want = R.linear_backward(h, W, go)
    bad_w = np.zeros((k, m), bool)
    bad_w[:, [7, 13, 39]] = True
    bad_w[19, :] = True
    bad_b = np.zeros(m, bool)
    bad_b[[7, 13, 39]] = True
    bad_in = np.zeros((n, k), bool)
    bad_in[[5, 40, 70], :] = True
    for name, w, bad in zip(("grad_in", "grad_W", "grad_bias"), want, (bad_in, bad_w, bad_b)):
        assert np.array_equal(~np.isfinite(w), bad), (name, "the reference's non-finite outputs are not the expected ones")
    assert np.isnan(want[1][:, 7]).all() and np.isnan(want[2][7]) and want[2][13] == np.inf and want[2][39] == -np.inf
    for acc in (None, old):
        got = bare.linear_backward(h, W, go, accumulate_into=acc)
        ref = R.linear_backward(h, W, go, acc)
        for name, a, b, bad in zip(("grad_in", "grad_W", "grad_bias"), got, ref, (bad_in, bad_w, bad_b)):
            same(a, b, ("non-finite", name, acc is not None))
            assert np.array_equal(~np.isfinite(a), bad), (name, acc is not None)
    # the input gradient without LDS: rows 1, 3 and 5 of seven
    n, k, m = 7, 482, 17
    h, W, go, _ = _linear_inputs(n, k, m)
    go[1, 3], go[3, 16], go[5, 0] = np.nan, np.inf, -np.inf
    want = R.linear_backward(h, W, go)[0]
    bad_in = np.zeros((n, k), bool)
    bad_in[[1, 3, 5], :] = True
    assert np.array_equal(~np.isfinite(want), bad_in)
    got = bare.linear_backward(h, W, go, want=("in",))[0]
    same(got, want, "non-finite, grad_in at k = 482")
    assert np.array_equal(~np.isfinite(got), bad_in)


@pytest.mark.parametrize("f", [5, 65])
def test_non_finite_values_reach_the_neighbours_only(f):
    """A non-finite grad_out[u][j], j < f, reaches column j of u's neighbours; one in an own column f + j (not an overwritten
    one) reaches column j of u itself; nothing else."""
    g = R.graph_of("er1933")
    rp, deg = g.rowptr.astype(np.int64), np.diff(g.rowptr.astype(np.int64))
    a, b, c, d = (int(v) for v in np.flatnonzero(deg >= 3)[[3, 400, 900, 1200]])
    go = H.crafted_input(g.n, 2 * f + 3, 31 + f)
    go[a, 2], go[b, 0], go[c, f - 1], go[d, f + 4] = np.nan, np.inf, -np.inf, np.inf
    go[d, f + 2] = np.nan   # an overwritten own column: no term of any output
    bad = np.zeros((g.n, f), bool)
    for u, j in ((a, 2), (b, 0), (c, f - 1)):
        bad[g.col[rp[u]: rp[u + 1]].astype(np.int64), j] = True
    bad[d, 4] = True
    want = R.graph_layer_backward(g, go)
    assert np.array_equal(~np.isfinite(want), bad), "the reference's non-finite outputs are not the expected ones"
    e = engine(NO_LAYERS, g)
    try:
        got = e.graph_layer_backward(go)
    finally:
        e.close()
    same(got, want, ("non-finite graph layer", f))
    assert np.array_equal(~np.isfinite(got), bad)


# ---------------------------------------------------------------- graph layer

@pytest.mark.parametrize("f", R.GRAPH_LAYER_F_WIDE)
def test_graph_layer_backward_wider_than_a_wave(f):
    e = engine(NO_LAYERS)
    try:
        for gname in R.GRAPH_LAYER_WIDE_GRAPHS:
            g = R.graph_of(gname)
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            go = H.crafted_input(g.n, 2 * f + 3, 100 * f + len(gname))
            same(e.graph_layer_backward(go), R.graph_layer_backward(g, go), (f, gname))
            assert e.get_info("graph_symmetric") == 1
    finally:
        e.close()


@pytest.mark.parametrize("f", R.GRAPH_LAYER_F + R.GRAPH_LAYER_F_WIDE)
def test_rows_around_the_group_size(f):
    """R.ladder(): rows of GS - 1, GS, GS + 1 and 2 GS + 1 entries for every group size; as built, then in another stored order,
    which gives the sums other bits."""
    e = engine(NO_LAYERS)
    try:
        built = R.ladder()
        want = []
        for g in (built, _shuffled_rows(built, 5)):
            assert R.is_symmetric(g)
            e.upload_graph(g)
            go = H.crafted_input(g.n, 2 * f + 3, 200 * f + 7)
            want.append(R.graph_layer_backward(g, go))
            same(e.graph_layer_backward(go), want[-1], (f, "ladder"))
            assert e.get_info("graph_symmetric") == 1
        assert (H.bits(want[0]) != H.bits(want[1])).any(), "the stored order does not show in the sums"
    finally:
        e.close()


@pytest.mark.parametrize("f", R.MULTIGRAPH_F)
def test_symmetric_multigraph_is_summed(f):
    """Doubled entries on both sides and self loops, once and twice: symmetric with multiplicities, so accepted and summed."""
    e = engine(NO_LAYERS)
    try:
        built = R.multigraph()
        assert built.nnz == 3258
        for g in (built, _shuffled_rows(built, 9)):
            assert R.is_symmetric(g)
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            assert e.get_info("graph_symmetric") == -1
            go = H.crafted_input(g.n, 2 * f + 3, 300 * f + 3)
            same(e.graph_layer_backward(go), R.graph_layer_backward(g, go), (f, "multigraph"))
            assert e.get_info("graph_symmetric") == 1
    finally:
        e.close()


# ---------------------------------------------------------------- the symmetry check says no

@pytest.mark.parametrize("gname,shuffle", [("er1933", False), ("er1933", True), ("hub8k", False)])
def test_one_entry_from_symmetric(gname, shuffle):
    """Graphs that miss symmetry by one stored entry — deleted at the ends of the graph, of a row, of the partner's row and in
    the middle of a row of 5002, or redirected so that every row keeps its length — are refused, and the intact graph is
    accepted again after each.  shuffle: rows in another order after the defect, which takes the scans instead of the searches."""
    intact = R.graph_of(gname)
    go = H.crafted_input(intact.n, 5, 41)
    e = engine(NO_LAYERS)
    try:
        e.set_weight_scale(intact.ws)
        for label, bad in R.defects(gname):
            if shuffle:
                bad = _shuffled_rows(bad, 13)
            assert not R.is_symmetric(bad), (gname, label)
            assert bad.col.max() < bad.n
            e.upload_graph(bad)
            assert e.get_info("graph_symmetric") == -1
            assert _code(lambda: e.graph_layer_backward(go)) == ERR_UNSUPPORTED, (gname, label)
            assert e.get_info("graph_symmetric") == 0, (gname, label)
            e.upload_graph(intact)
            assert e.get_info("graph_symmetric") == -1
            e.graph_layer_backward(go)
            assert e.get_info("graph_symmetric") == 1, (gname, label, "the intact graph after it")
    finally:
        e.close()


# ---------------------------------------------------------------- model level

@pytest.mark.parametrize("model", ["trained", "embed", "two_graphs"])
def test_each_output_alone(model, shim):   # noqa: F811
    import torch
    c = R.case(model, "er4097", "perturbed", sigmoid=_restated(shim))
    gs = c["grad_scores"]
    e = engine(c["text"], c["g"])
    try:
        _, gp, gx = _run_case(e, c, (model, "er4097", "perturbed"))
        same(e.backward(gs, want_grad_x=True, want_grad_params=False), gx, (model, "grad_x alone"))
        assert e.backward(gs, want_grad_params=False) is None
        # without grad_x: embed walks every layer down to its first, two_graphs stops above its graph layers
        same(e.backward(gs), gp, (model, "grad_params alone"))
        with pytest.raises(ValueError):
            e.backward(gs, want_grad_params=False, accumulate_into=gp.copy())
        dev = torch.device("cuda:0")
        d_gs = torch.from_numpy(np.ascontiguousarray(gs)).to(dev)
        d_gx = torch.full(c["x"].shape, float("nan"), device=dev)
        d_gp = torch.full((e.num_params(),), float("nan"), device=dev)
        torch.cuda.synchronize()
        e.backward_device(d_gs.data_ptr(), 0, d_gx.data_ptr())
        e.synchronize()
        same(d_gx.cpu().numpy(), gx, (model, "device grad_x alone"))
        e.backward_device(d_gs.data_ptr(), 0, 0)
        e.synchronize()
        # nothing has changed: the saved forward gives the same gradients once more
        e.backward_device(d_gs.data_ptr(), d_gp.data_ptr(), d_gx.data_ptr())
        e.synchronize()
        same(d_gp.cpu().numpy(), gp, (model, "device grad_params after the calls without outputs"))
        same(d_gx.cpu().numpy(), gx, (model, "device grad_x after the calls without outputs"))
        gp2, gx2 = e.backward(gs, want_grad_x=True)
        same(gp2, gp, (model, "grad_params after the calls without outputs"))
        same(gx2, gx, (model, "grad_x after the calls without outputs"))
    finally:
        e.close()


def test_directed_graph_under_the_walked_range(shim):   # noqa: F811
    """The symmetry check belongs to the graph layers a backward walks.  two_graphs without grad_x stops at its first linear
    layer, above both graph layers: the call succeeds on a directed graph, the answer stays open, and the parameter gradient is
    the reference's; with grad_x it is refused.  mlp has no graph layer: nothing is checked and nothing refused."""
    sig = _restated(shim)
    g = R.directed3()
    assert not R.is_symmetric(g)
    gs = R.grad_scores_of(g.n, 1, 3)
    for model, refused in (("two_graphs", True), ("mlp", False)):
        text = R.text_of(model)
        x = R.model_input(g, R.in_width_of(text))
        ref = R.backward(text, g, x, gs, sigmoid=sig)
        e = engine(text, g)
        try:
            same(e.train_forward(x), ref["scores"], (model, "scores"))
            same(e.backward(gs), ref["grad_params"], (model, "grad_params on a directed graph"))
            assert e.backward(gs, want_grad_params=False) is None
            assert e.get_info("graph_symmetric") == -1
            if refused:
                assert _code(lambda: e.backward(gs, want_grad_x=True)) == ERR_UNSUPPORTED
                assert _code(lambda: e.backward(gs, want_grad_x=True, want_grad_params=False)) == ERR_UNSUPPORTED
                assert e.get_info("graph_symmetric") == 0
                same(e.backward(gs), ref["grad_params"], (model, "grad_params after the refusal"))
            else:
                gp, gx = e.backward(gs, want_grad_x=True)
                same(gp, ref["grad_params"], (model, "grad_params with grad_x"))
                same(gx, ref["grad_x"], (model, "grad_x on a directed graph"))
                same(e.backward(gs, want_grad_x=True, want_grad_params=False), ref["grad_x"], (model, "grad_x alone"))
                assert e.get_info("graph_symmetric") == -1
        finally:
            e.close()


def test_model_without_layers():
    g = R.graph_of("er1933")
    e = engine(NO_LAYERS, g)
    try:
        assert e.num_params() == 0 and e.params().size == 0
        x = H.crafted_input(g.n, 1, 51)
        gs = H.crafted_input(g.n, 1, 52)
        same(e.train_forward(x), x, "no layer: the scores are the input")
        gp, gx = e.backward(gs, want_grad_x=True)
        assert gp.size == 0
        same(gx, gs, "no layer: grad_x is grad_scores")
        assert e.backward(gs).size == 0
        same(e.backward(gs, want_grad_x=True, want_grad_params=False), gs, "no layer: grad_x alone")
        assert e.backward(gs, want_grad_params=False) is None
        assert e.get_info("graph_symmetric") == -1
    finally:
        e.close()


@pytest.mark.parametrize("model", list(R.MORE_MODELS))
def test_more_models(model, shim):   # noqa: F811
    from gnn_mwvc_amd import training
    sig = _restated(shim)
    text = R.text_of(model)
    e = engine(text)
    try:
        assert e.num_params() == training.param_layout(text)[1]
        assert e.in_width == R.in_width_of(text)
        if model == "linear_end17":
            assert (e.in_width, e.out_width) == (2, 17)
        if model == "relu_end":
            assert e.out_width == 4
        for gname in R.MORE_MODEL_GRAPHS:
            g = R.graph_of(gname)
            e.set_weight_scale(g.ws)
            e.upload_graph(g)
            for variant in ("own", "perturbed"):
                c = R.case(model, gname, variant, sigmoid=sig)
                if g.n:
                    assert c["grad_scores"].shape == (g.n, e.out_width)
                scores, gp, gx = _run_case(e, c, (model, gname, variant))
                if variant == "own":
                    same(scores, e.forward(c["x"])[0], (model, gname, "train_forward against forward"))
                same(e.backward(c["grad_scores"]), c["grad_params"], (model, gname, variant, "without grad_x"))
    finally:
        e.close()
