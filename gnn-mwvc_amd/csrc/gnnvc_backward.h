// gnnvc_backward.h — launch interface between the engine's backward pass (gnnvc_backward.cpp) and its gfx950 kernels
// (gnnvc_backward.hip; the loss and the optimizer step: gnnvc_fit.hip).  Internal; the public boundary is include/gnnvc.h, the order
// rules are DESIGN.md §3 "Backward".
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gnnvc.h"
#include "gnnvc_kernels.h"

namespace gnnvc {

// rows per block of a parameter gradient's sum: GNNVC_GRAD_BLOCK_ROWS of include/gnnvc.h, part of the ABI's numerics
constexpr uint32_t kGradBlockRows = 4096;
inline uint32_t grad_blocks(uint32_t n) { return (n + kGradBlockRows - 1) / kGradBlockRows; }

// grad_in[i] = z[i] >= 0 ? grad_out[i] : 0 (z: the ReLU's input) / grad_in[i] = (s[i] * (1 - s[i])) * grad_out[i] (s: the sigmoid's output)
hipError_t launch_bwd_relu(size_t count, const float *z, const float *grad_out, float *grad_in, hipStream_t stream);
hipError_t launch_bwd_sigmoid(size_t count, const float *s, const float *grad_out, float *grad_in, hipStream_t stream);

// grad_in (n x k) = grad_out (n x m) * W^T (W k x m): one fmaf chain over j = 0 .. m - 1 per output, from +0.0f
hipError_t launch_bwd_linear_dx(uint32_t n, uint32_t k, uint32_t m, const float *grad_out, const float *W, float *grad_in,
                                hipStream_t stream);

// The parameter gradient of a linear layer.  Output rows 0 .. k - 1 are grad_W (k x m), and with with_bias row k is grad_bias (the
// input column that is 1 in every row): (k + with_bias) x m floats at `grad`, which is how the parameter buffer lays a layer out.
// k_bwd_linear_dw writes one partial per block of kGradBlockRows rows to `partials` (grad_blocks(n) x (k + with_bias) x m floats),
// k_bwd_reduce_blocks adds them in block order and stores the total, or old + total with accumulate.  k == 0 computes the bias alone
// (`in` is not read then).  n == 0: no partial, the total is +0.0f.
hipError_t launch_bwd_linear_dw(uint32_t n, uint32_t k, uint32_t m, bool with_bias, const float *in, const float *grad_out,
                                float *partials, float *grad, bool accumulate, hipStream_t stream);

// grad_in (n x f) of the graph layer from grad_out (n x (2 f + 3)) on a SYMMETRIC graph: the neighbours' rows of columns 0 .. f - 1
// added in stored order from +0.0f, then the own term of column f + j (none where the forward overwrites that column)
hipError_t launch_bwd_graph(const GraphDev &g, uint32_t f, const float *grad_out, float *grad_in, hipStream_t stream);

// Is the adjacency symmetric, with multiplicities?  Two steps over info[0 .. 1] (zeroed by the first) and row_ascends (n bytes):
//   launch_bwd_row_ascends  row_ascends[v] = 1 iff row v's ids never descend (its look-ups are binary searches, else scans), and
//                           info[1] = the length of the longest row that does not ascend;
//   launch_bwd_symmetry     info[0] becomes non-zero iff some entry (v, u) is stored another number of times in row v than (u, v)
//                           in row u.  A thread per entry: an entry of a row that does not ascend scans that row, so such a row of d
//                           entries costs d * d loads — the engine refuses graphs whose info[1] exceeds kSymmetryScanLimit
//                           instead of launching that (65 536: 4e9 loads for the worst row, a fraction of a second).
constexpr uint32_t kSymmetryScanLimit = 65536;
hipError_t launch_bwd_row_ascends(const GraphDev &g, uint8_t *row_ascends, uint32_t *info, hipStream_t stream);
hipError_t launch_bwd_symmetry(const GraphDev &g, const uint8_t *row_ascends, uint32_t *info, hipStream_t stream);

// ---- loss and step (gnnvc_fit.hip; include/gnnvc.h "loss and step") ----
// x, y: rows x width.  With grad: grad[i][j] = (2.0f * (x[i][j] - y[i][j])) / (float)width; grad may be x or y itself.  With stats
// (device memory): k_mse_block leaves one loss partial and three counts per block of kGradBlockRows rows in `partials`
// (grad_blocks(rows) floats) and `counts` (3 * grad_blocks(rows) words), k_mse_finish adds them in block order onto *stats.  Up to
// kGradBlockRows rows the total added to loss_sum is the reference's MSE_loss chain, loss += se / width over the rows, before its
// division by the height, bit for bit.  rows == 0: nothing is launched.
hipError_t launch_fit_mse(uint32_t rows, uint32_t width, const float *x, const float *y, float *grad, float *partials, uint32_t *counts,
                          gnnvc_fit_stats *stats, hipStream_t stream);
// SGD_step over count parameters: g = grad (+ (2 weight_decay) w where weight_decay > 0), vel = (momentum vel) + (g / batch),
// w = w - (lr vel); with zero_grad grad becomes +0.0f, else it is not written.  batch: the divisor, already a float.
hipError_t launch_fit_sgd_step(size_t count, float *params, float *vel, float *grad, float batch, float lr, float momentum,
                               float weight_decay, bool zero_grad, hipStream_t stream);

}  // namespace gnnvc
