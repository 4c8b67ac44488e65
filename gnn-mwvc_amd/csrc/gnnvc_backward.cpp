// gnnvc_backward.cpp — the backward pass of include/gnnvc.h: the training forward that keeps what a gradient needs, the model-level
// backward over it, and the layer-level backward entry points.  All arithmetic happens in the kernels of gnnvc_backward.hip, in
// the orders DESIGN.md §3 ("Backward") states; there is no CPU fallback here.  At the end, the loss and the optimizer step a trainer
// runs between a backward and the next forward (gnnvc_mse*, gnnvc_sgd_step*; kernels: gnnvc_fit.hip).
//
// The engine's inference side is never touched: the parameters a training forward ran with are a copy of their own
// (gnnvc_engine::TrainBufs::params), its activations and the gradients' scratch live beside them, and an ordinary forward between
// a training forward and its backward reads and writes none of them.  Whether the buffers hold a forward of the RESIDENT graph is
// per-graph state (pg.train.saved), cleared by every hand-off with the rest of PerGraph.
#include "gnnvc_backward.h"
#include "gnnvc_engine_state.h"

namespace {

size_t param_count(const gnnvc_engine *e) {
    size_t p = 0;
    for (const auto &l : e->layers) p += l.W.size() + l.bias.size();
    return p;
}

// what every model-level call asks first; n = 0 is the caller's to treat
int train_args(gnnvc_engine *e, const char *what) {
    if (e->multi) return fail(e, GNNVC_ERR_UNSUPPORTED, "%s is not available on a multi-device handle", what);
    if (!e->have_graph) return fail(e, GNNVC_ERR_STATE, "%s: no graph attached", what);
    if (e->g.sliced() || e->pg.empty_slice) return fail(e, GNNVC_ERR_UNSUPPORTED, "%s: this engine holds a slice of the graph", what);
    return use_device(e);
}

// The graph layer's backward is the transposed neighbour sum written over adj(v): right only where (v, u) is stored as often as
// (u, v).  Checked once per resident graph, exactly, on the device (two read-backs: the call that asks first waits for its stream).
int ensure_symmetric(gnnvc_engine *e) {
    auto &t = e->pg.train;
    if (t.symmetric < 0) {
        if (e->g.n == 0) {
            t.symmetric = 1;
        } else {
            HIP_TRY(e, e->train.row_ascends.reserve(e->g.n));
            HIP_TRY(e, e->train.sym_flag.reserve(2));
            uint32_t info[2] = {0, 0};
            HIP_TRY(e, gnnvc::launch_bwd_row_ascends(e->g, e->train.row_ascends.p, e->train.sym_flag.p, e->stream));
            HIP_TRY(e, hipMemcpyAsync(info, e->train.sym_flag.p, sizeof info, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(e, hipStreamSynchronize(e->stream));
            // (an entry of a row that does not ascend scans the row: a long one is refused, not scanned; the answer stays open)
            if (info[1] > gnnvc::kSymmetryScanLimit)
                return fail(e, GNNVC_ERR_UNSUPPORTED, "a row of %u entries does not ascend: the symmetry check scans such rows only up to %u entries (sort the lists)",
                            info[1], gnnvc::kSymmetryScanLimit);
            HIP_TRY(e, gnnvc::launch_bwd_symmetry(e->g, e->train.row_ascends.p, e->train.sym_flag.p, e->stream));
            HIP_TRY(e, hipMemcpyAsync(info, e->train.sym_flag.p, sizeof info, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(e, hipStreamSynchronize(e->stream));
            t.symmetric = info[0] ? 0 : 1;
        }
    }
    if (!t.symmetric)
        return fail(e, GNNVC_ERR_UNSUPPORTED, "the resident graph's adjacency is not symmetric: the graph layer's backward is defined for symmetric graphs only");
    return GNNVC_OK;
}

// the width of every layer's input, and of the last layer's output: layers.size() + 1 values
std::vector<uint32_t> layer_widths(const gnnvc_engine *e) {
    std::vector<uint32_t> w{(uint32_t)e->in_width};
    for (const auto &l : e->layers) w.push_back(l.kind == kLinear ? l.m : l.kind == kGraph ? 2 * w.back() + 3 : w.back());
    return w;
}

// the saved forward's buffers for the resident graph (contents are not kept when one grows)
int train_reserve(gnnvc_engine *e) {
    auto &t = e->train;
    const auto w = layer_widths(e);
    t.act_off.assign(1, 0);
    for (uint32_t wd : w) t.act_off.push_back(t.act_off.back() + (size_t)e->g.n * wd);
    HIP_TRY(e, t.params.reserve(param_count(e) + 64));
    HIP_TRY(e, t.acts.reserve(t.act_off.back() + 64));
    return GNNVC_OK;
}

// Layer by layer with the inference launchers, every layer's output kept: train.params and the input rows (acts at act_off[0])
// are in place already.  d_scores: device memory, may be null.
int train_forward_run(gnnvc_engine *e, float *d_scores) {
    auto &t = e->train;
    const uint32_t n = e->g.n;
    const auto w = layer_widths(e);
    for (size_t i = 0; i < e->layers.size(); ++i) {
        const Layer &l = e->layers[i];
        const float *cur = t.acts.p + t.act_off[i];
        float *dst = t.acts.p + t.act_off[i + 1];
        switch (l.kind) {
        case kGraph: HIP_TRY(e, gnnvc::launch_graph_layer(e->g, e->ws, w[i], cur, dst, e->stream)); break;
        case kLinear: HIP_TRY(e, gnnvc::launch_linear(n, l.k, l.m, cur, t.params.p + l.w_off, t.params.p + l.b_off, dst, e->stream)); break;
        case kRelu: HIP_TRY(e, gnnvc::launch_relu((size_t)n * w[i], cur, dst, e->stream)); break;
        case kSigmoid: HIP_TRY(e, gnnvc::launch_sigmoid((size_t)n * w[i], cur, dst, e->stream)); break;
        }
    }
    if (d_scores)
        HIP_TRY(e, hipMemcpyAsync(d_scores, t.acts.p + t.act_off[e->layers.size()], (size_t)n * w.back() * sizeof(float),
                                  hipMemcpyDeviceToDevice, e->stream));
    e->pg.train.saved = true;
    return GNNVC_OK;
}

// The backward over the saved forward, n > 0: device pointers; d_gp and d_gx may be null.  Layers are walked last to first; the
// gradient rows ping-pong between train.grad[0 .. 1], the first read from d_gs and the last written to d_gx.  Without d_gx the walk
// ends at the first linear layer, whose input gradient nobody asked for.
int backward_run(gnnvc_engine *e, const float *d_gs, float *d_gp, float *d_gx, bool accumulate) {
    auto &t = e->train;
    const uint32_t n = e->g.n;
    const auto w = layer_widths(e);
    const size_t L = e->layers.size();
    size_t first_lin = L, part = 0;
    bool graph = false;
    for (size_t i = L; i-- > 0;) {
        const Layer &l = e->layers[i];
        if (l.kind == kLinear) {
            first_lin = i;
            part = std::max(part, (size_t)gnnvc::grad_blocks(n) * (l.k + 1) * l.m);
        }
    }
    const size_t stop = d_gx ? 0 : d_gp ? first_lin : L;
    for (size_t i = stop; i < L; ++i) graph = graph || e->layers[i].kind == kGraph;
    if (graph) {
        int rc = ensure_symmetric(e);
        if (rc) return rc;
    }
    for (auto &gb : t.grad) HIP_TRY(e, gb.reserve((size_t)n * e->max_width + 64));
    if (d_gp) HIP_TRY(e, t.partials.reserve(part + 64));
    const float *cur = d_gs;
    int pp = 0;
    for (size_t i = L; i-- > stop;) {
        const Layer &l = e->layers[i];
        float *dst = (i == 0 && d_gx) ? d_gx : t.grad[pp].p;
        const size_t count = (size_t)n * w[i];
        switch (l.kind) {
        case kSigmoid: HIP_TRY(e, gnnvc::launch_bwd_sigmoid(count, t.acts.p + t.act_off[i + 1], cur, dst, e->stream)); break;
        case kRelu: HIP_TRY(e, gnnvc::launch_bwd_relu(count, t.acts.p + t.act_off[i], cur, dst, e->stream)); break;
        case kGraph: HIP_TRY(e, gnnvc::launch_bwd_graph(e->g, w[i], cur, dst, e->stream)); break;
        case kLinear:
            // (W then the bias, k + 1 rows of m: the parameter buffer's own layout, so one launch pair serves both)
            if (d_gp)
                HIP_TRY(e, gnnvc::launch_bwd_linear_dw(n, l.k, l.m, true, t.acts.p + t.act_off[i], cur, t.partials.p, d_gp + l.w_off,
                                                       accumulate, e->stream));
            if (d_gx || i > first_lin) HIP_TRY(e, gnnvc::launch_bwd_linear_dx(n, l.k, l.m, cur, t.params.p + l.w_off, dst, e->stream));
            break;
        }
        cur = dst;
        pp ^= 1;
    }
    if (L == 0 && d_gx)
        HIP_TRY(e, hipMemcpyAsync(d_gx, d_gs, (size_t)n * w[0] * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    return GNNVC_OK;
}

// host buffers of a layer-level call on the device: freed when the call returns, which has waited for the stream by then
struct HostOp {
    gnnvc_engine *e;
    int up(DevBuf<float> &d, const float *h, size_t count, size_t room = 0) {
        HIP_TRY(e, d.reserve(std::max(count, room) + 1));
        if (h && count) HIP_TRY(e, hipMemcpyAsync(d.p, h, count * sizeof(float), hipMemcpyHostToDevice, e->stream));
        return GNNVC_OK;
    }
    int down(float *h, const float *d, size_t count) {
        if (h && count) HIP_TRY(e, hipMemcpyAsync(h, d, count * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        return GNNVC_OK;
    }
};

int activation_backward(gnnvc_engine *e, size_t count, const float *saved, const float *grad_out, float *grad_in, bool sigmoid) {
    if (!e) return GNNVC_ERR_INVALID;
    if (!count) return GNNVC_OK;
    if (!saved || !grad_out || !grad_in) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
    int rc = use_device(e);
    if (rc) return rc;
    HostOp op{e};
    DevBuf<float> ds, dg, di;
    if ((rc = op.up(ds, saved, count)) || (rc = op.up(dg, grad_out, count)) || (rc = op.up(di, nullptr, count))) return rc;
    HIP_TRY(e, sigmoid ? gnnvc::launch_bwd_sigmoid(count, ds.p, dg.p, di.p, e->stream)
                       : gnnvc::launch_bwd_relu(count, ds.p, dg.p, di.p, e->stream));
    if ((rc = op.down(grad_in, di.p, count))) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return GNNVC_OK;
}

// what the loss and the step ask first: `bad` = the argument rule the caller found broken (null: none)
int fit_args(gnnvc_engine *e, const char *what, const char *bad) {
    if (bad) return fail(e, GNNVC_ERR_INVALID, "%s: %s", what, bad);
    if (e->multi) return fail(e, GNNVC_ERR_UNSUPPORTED, "%s is not available on a multi-device handle", what);
    return use_device(e);
}

// rows > 0, device pointers; d_grad or d_stats may be null.  The block partials and counts are the engine's (train.fit_*).
int mse_run(gnnvc_engine *e, uint32_t rows, uint32_t width, const float *d_x, const float *d_y, float *d_grad, gnnvc_fit_stats *d_stats) {
    auto &t = e->train;
    if (d_stats) {
        const size_t blocks = gnnvc::grad_blocks(rows);
        HIP_TRY(e, t.fit_partials.reserve(blocks + 64));
        HIP_TRY(e, t.fit_counts.reserve(3 * blocks + 64));
    }
    HIP_TRY(e, gnnvc::launch_fit_mse(rows, width, d_x, d_y, d_grad, t.fit_partials.p, t.fit_counts.p, d_stats, e->stream));
    return GNNVC_OK;
}

}  // namespace

bool gnnvc_eng::backward_info(const gnnvc_engine *e, const std::string &key, long *value) {
    if (key == "graph_symmetric") *value = e->pg.train.symmetric;              // -1 before the check, then 0 | 1
    else if (key == "backward_workspace_bytes") *value = (long)e->train.bytes();   // the saved forward and the gradients' scratch
    else return false;
    return true;
}

extern "C" {

int gnnvc_num_params(const gnnvc_engine *e, uint64_t *count) {
    if (!e || !count) return GNNVC_ERR_INVALID;
    *count = param_count(e);
    return GNNVC_OK;
}

int gnnvc_get_params(const gnnvc_engine *e, float *params) {
    if (!e || (!params && param_count(e))) return GNNVC_ERR_INVALID;
    for (const auto &l : e->layers) {   // the order of the model text, which is the device parameter buffer's (w_off, b_off)
        if (l.kind != kLinear) continue;
        memcpy(params + l.w_off, l.W.data(), l.W.size() * sizeof(float));
        memcpy(params + l.b_off, l.bias.data(), l.bias.size() * sizeof(float));
    }
    return GNNVC_OK;
}

int gnnvc_train_forward_device(gnnvc_engine *e, const float *d_params, const float *d_x, float *d_scores) {
    if (!e) return GNNVC_ERR_INVALID;
    int rc = train_args(e, "gnnvc_train_forward_device");
    if (rc) return rc;
    e->pg.train.saved = false;
    const uint32_t n = e->g.n;
    if (n && (!d_x || !d_scores)) return fail(e, GNNVC_ERR_INVALID, "null device buffers");
    if ((rc = train_reserve(e))) return rc;
    auto &t = e->train;
    const size_t np = param_count(e);
    if (np) HIP_TRY(e, hipMemcpyAsync(t.params.p, d_params ? d_params : e->params.p, np * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    if (n) HIP_TRY(e, hipMemcpyAsync(t.acts.p, d_x, (size_t)n * e->in_width * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    return train_forward_run(e, d_scores);
}

int gnnvc_train_forward(gnnvc_engine *e, const float *params, const float *x, float *scores) {
    if (!e) return GNNVC_ERR_INVALID;
    int rc = train_args(e, "gnnvc_train_forward");
    if (rc) return rc;
    e->pg.train.saved = false;
    const uint32_t n = e->g.n;
    if (n && (!x || !scores)) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
    if ((rc = train_reserve(e))) return rc;
    auto &t = e->train;
    const size_t np = param_count(e);
    if (np && params) HIP_TRY(e, hipMemcpyAsync(t.params.p, params, np * sizeof(float), hipMemcpyHostToDevice, e->stream));
    else if (np) HIP_TRY(e, hipMemcpyAsync(t.params.p, e->params.p, np * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    if (n) HIP_TRY(e, hipMemcpyAsync(t.acts.p, x, (size_t)n * e->in_width * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if ((rc = train_forward_run(e, nullptr))) return rc;
    if (n)
        HIP_TRY(e, hipMemcpyAsync(scores, t.acts.p + t.act_off[e->layers.size()], (size_t)n * e->out_width * sizeof(float),
                                  hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return GNNVC_OK;
}

int gnnvc_backward_device(gnnvc_engine *e, const float *d_grad_scores, float *d_grad_params, float *d_grad_x, int accumulate) {
    if (!e) return GNNVC_ERR_INVALID;
    int rc = train_args(e, "gnnvc_backward_device");
    if (rc) return rc;
    if (!e->pg.train.saved) return fail(e, GNNVC_ERR_STATE, "gnnvc_backward_device: no training forward on the resident graph");
    const size_t np = param_count(e);
    if (e->g.n == 0) {   // no row: every sum is empty
        if (d_grad_params && np && !accumulate) HIP_TRY(e, hipMemsetAsync(d_grad_params, 0, np * sizeof(float), e->stream));
        return GNNVC_OK;
    }
    if (!d_grad_scores) return fail(e, GNNVC_ERR_INVALID, "null device buffers");
    return backward_run(e, d_grad_scores, d_grad_params, d_grad_x, accumulate != 0);
}

int gnnvc_backward(gnnvc_engine *e, const float *grad_scores, float *grad_params, float *grad_x, int accumulate) {
    if (!e) return GNNVC_ERR_INVALID;
    int rc = train_args(e, "gnnvc_backward");
    if (rc) return rc;
    if (!e->pg.train.saved) return fail(e, GNNVC_ERR_STATE, "gnnvc_backward: no training forward on the resident graph");
    const size_t np = param_count(e);
    const uint32_t n = e->g.n;
    if (n == 0) {
        if (grad_params && !accumulate) std::fill(grad_params, grad_params + np, 0.0f);
        return GNNVC_OK;
    }
    if (!grad_scores) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
    auto &t = e->train;
    const size_t gs = (size_t)n * e->out_width, gx = (size_t)n * e->in_width;
    HIP_TRY(e, t.host_in.reserve(gs + 64));
    HIP_TRY(e, t.host_out.reserve(np + gx + 64));
    HIP_TRY(e, hipMemcpyAsync(t.host_in.p, grad_scores, gs * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if (grad_params && accumulate && np)
        HIP_TRY(e, hipMemcpyAsync(t.host_out.p, grad_params, np * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if ((rc = backward_run(e, t.host_in.p, grad_params ? t.host_out.p : nullptr, grad_x ? t.host_out.p + np : nullptr, accumulate != 0)))
        return rc;
    if (grad_params && np) HIP_TRY(e, hipMemcpyAsync(grad_params, t.host_out.p, np * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (grad_x) HIP_TRY(e, hipMemcpyAsync(grad_x, t.host_out.p + np, gx * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return GNNVC_OK;
}

// ---- layer-level backward entry points (host pointers in, host pointers out) ----

int gnnvc_graph_layer_backward(gnnvc_engine *e, uint32_t f, const float *grad_out, float *grad_in) {
    if (!e) return GNNVC_ERR_INVALID;
    int rc = train_args(e, "gnnvc_graph_layer_backward");
    if (rc) return rc;
    if (f == 0) return fail(e, GNNVC_ERR_INVALID, "zero feature width");
    const uint32_t n = e->g.n;
    if (n == 0) return GNNVC_OK;
    if (!grad_out || !grad_in) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
    if ((rc = ensure_symmetric(e))) return rc;
    HostOp op{e};
    DevBuf<float> dg, di;
    if ((rc = op.up(dg, grad_out, (size_t)n * (2 * f + 3))) || (rc = op.up(di, nullptr, (size_t)n * f))) return rc;
    HIP_TRY(e, gnnvc::launch_bwd_graph(e->g, f, dg.p, di.p, e->stream));
    if ((rc = op.down(grad_in, di.p, (size_t)n * f))) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return GNNVC_OK;
}

int gnnvc_linear_backward(gnnvc_engine *e, uint32_t n, uint32_t k, uint32_t m, const float *in, const float *W, const float *grad_out,
                          float *grad_in, float *grad_W, float *grad_bias, int accumulate) {
    if (!e) return GNNVC_ERR_INVALID;
    const size_t wsz = (size_t)k * m;
    if (n == 0 || m == 0) {   // empty sums: +0.0f, and old values stay when accumulating
        if (grad_W && !accumulate) std::fill(grad_W, grad_W + wsz, 0.0f);
        if (grad_bias && !accumulate) std::fill(grad_bias, grad_bias + m, 0.0f);
        if (grad_in) std::fill(grad_in, grad_in + (size_t)n * k, 0.0f);
        return GNNVC_OK;
    }
    if (!grad_out || (grad_W && wsz && !in) || (grad_in && wsz && !W)) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
    int rc = use_device(e);
    if (rc) return rc;
    HostOp op{e};
    DevBuf<float> din, dw, dg, di, dp, dpart;
    if ((rc = op.up(dg, grad_out, (size_t)n * m))) return rc;
    const bool want_w = grad_W && wsz;
    if (want_w || grad_bias) {
        // the (k + 1) x m block of the model level: grad_W's rows, then grad_bias; a call that wants the bias alone runs k = 0
        const uint32_t kw = want_w ? k : 0;
        const size_t outs = ((size_t)kw + (grad_bias ? 1 : 0)) * m;
        if (want_w && (rc = op.up(din, in, (size_t)n * k))) return rc;
        if ((rc = op.up(dp, nullptr, outs)) || (rc = op.up(dpart, nullptr, (size_t)gnnvc::grad_blocks(n) * outs))) return rc;
        if (accumulate) {
            if (want_w) HIP_TRY(e, hipMemcpyAsync(dp.p, grad_W, wsz * sizeof(float), hipMemcpyHostToDevice, e->stream));
            if (grad_bias)
                HIP_TRY(e, hipMemcpyAsync(dp.p + (size_t)kw * m, grad_bias, (size_t)m * sizeof(float), hipMemcpyHostToDevice, e->stream));
        }
        HIP_TRY(e, gnnvc::launch_bwd_linear_dw(n, kw, m, grad_bias != nullptr, din.p, dg.p, dpart.p, dp.p, accumulate != 0, e->stream));
        if (want_w && (rc = op.down(grad_W, dp.p, wsz))) return rc;
        if ((rc = op.down(grad_bias, dp.p + (size_t)kw * m, m))) return rc;
    }
    if (grad_in && wsz) {
        if ((rc = op.up(dw, W, wsz)) || (rc = op.up(di, nullptr, (size_t)n * k))) return rc;
        HIP_TRY(e, gnnvc::launch_bwd_linear_dx(n, k, m, dg.p, dw.p, di.p, e->stream));
        if ((rc = op.down(grad_in, di.p, (size_t)n * k))) return rc;
    }
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return GNNVC_OK;
}

int gnnvc_relu_backward(gnnvc_engine *e, size_t count, const float *z, const float *grad_out, float *grad_in) {
    return activation_backward(e, count, z, grad_out, grad_in, false);
}

int gnnvc_sigmoid_backward(gnnvc_engine *e, size_t count, const float *s, const float *grad_out, float *grad_in) {
    return activation_backward(e, count, s, grad_out, grad_in, true);
}

// ---- loss and step (kernels: gnnvc_fit.hip): no resident graph is needed, the _device forms never wait ----

int gnnvc_mse_device(gnnvc_engine *e, uint32_t rows, uint32_t width, const float *d_scores, const float *d_target, float *d_grad,
                     gnnvc_fit_stats *d_stats) {
    if (!e) return GNNVC_ERR_INVALID;
    int rc = fit_args(e, "gnnvc_mse_device", width == 0 ? "zero width" : (!d_grad && !d_stats) ? "neither a gradient nor stats asked for" : nullptr);
    if (rc || !rows) return rc;
    if (!d_scores || !d_target) return fail(e, GNNVC_ERR_INVALID, "null device buffers");
    return mse_run(e, rows, width, d_scores, d_target, d_grad, d_stats);
}

int gnnvc_mse(gnnvc_engine *e, uint32_t rows, uint32_t width, const float *scores, const float *target, float *grad,
              gnnvc_fit_stats *stats) {
    if (!e) return GNNVC_ERR_INVALID;
    int rc = fit_args(e, "gnnvc_mse", width == 0 ? "zero width" : (!grad && !stats) ? "neither a gradient nor stats asked for" : nullptr);
    if (rc || !rows) return rc;
    if (!scores || !target) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
    const size_t count = (size_t)rows * width;
    HostOp op{e};
    DevBuf<float> dx, dy, dg;
    DevBuf<gnnvc_fit_stats> ds;
    if ((rc = op.up(dx, scores, count)) || (rc = op.up(dy, target, count)) || (grad && (rc = op.up(dg, nullptr, count)))) return rc;
    if (stats) {
        HIP_TRY(e, ds.reserve(1));
        HIP_TRY(e, hipMemcpyAsync(ds.p, stats, sizeof *stats, hipMemcpyHostToDevice, e->stream));
    }
    if ((rc = mse_run(e, rows, width, dx.p, dy.p, grad ? dg.p : nullptr, stats ? ds.p : nullptr))) return rc;
    if ((rc = op.down(grad, dg.p, count))) return rc;
    if (stats) HIP_TRY(e, hipMemcpyAsync(stats, ds.p, sizeof *stats, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return GNNVC_OK;
}

int gnnvc_sgd_step_device(gnnvc_engine *e, uint64_t count, float *d_params, float *d_vel, float *d_grad, uint64_t batch, float lr,
                          float momentum, float weight_decay, int zero_grad) {
    if (!e) return GNNVC_ERR_INVALID;
    int rc = fit_args(e, "gnnvc_sgd_step_device", batch == 0 ? "zero batch" : nullptr);
    if (rc || !count) return rc;
    if (!d_params || !d_vel || !d_grad) return fail(e, GNNVC_ERR_INVALID, "null device buffers");
    HIP_TRY(e, gnnvc::launch_fit_sgd_step(count, d_params, d_vel, d_grad, (float)batch, lr, momentum, weight_decay, zero_grad != 0, e->stream));
    return GNNVC_OK;
}

int gnnvc_sgd_step(gnnvc_engine *e, uint64_t count, float *params, float *vel, float *grad, uint64_t batch, float lr, float momentum,
                   float weight_decay, int zero_grad) {
    if (!e) return GNNVC_ERR_INVALID;
    int rc = fit_args(e, "gnnvc_sgd_step", batch == 0 ? "zero batch" : nullptr);
    if (rc || !count) return rc;
    if (!params || !vel || !grad) return fail(e, GNNVC_ERR_INVALID, "null host buffers");
    HostOp op{e};
    DevBuf<float> dw, dv, dg;
    if ((rc = op.up(dw, params, count)) || (rc = op.up(dv, vel, count)) || (rc = op.up(dg, grad, count))) return rc;
    HIP_TRY(e, gnnvc::launch_fit_sgd_step(count, dw.p, dv.p, dg.p, (float)batch, lr, momentum, weight_decay, zero_grad != 0, e->stream));
    if ((rc = op.down(params, dw.p, count)) || (rc = op.down(vel, dv.p, count))) return rc;
    if (zero_grad && (rc = op.down(grad, dg.p, count))) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return GNNVC_OK;
}

}  // extern "C"
