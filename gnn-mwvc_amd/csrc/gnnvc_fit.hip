// gnnvc_fit.hip — the gfx950 kernels of what a trainer does between a training forward and the next one (include/gnnvc.h "loss and
// step"; the order rules: DESIGN.md §3 "Loss and step"): the MSE gradient, the loss and accuracy read-outs, the momentum SGD step.
//
// Every operation is one fp32 operation rounded on its own, in the order written (the library is compiled with -ffp-contract=off,
// and nothing here calls __builtin_fmaf or multiplies by a reciprocal), and every sum has one stated order:
//   k_mse_block    a workgroup per block of kGradBlockRows rows, a thread per row at a time.  grad[i][j] = (2 (x - y)) / width.  The
//                  row value r_i = se_i / width, se_i one chain over the row's columns from +0.0f of se + d * d; the block's loss
//                  partial is one chain over its rows in ascending order from +0.0f, walked by ONE lane over the r_i in LDS; the
//                  three counts of the block are integers, summed in LDS;
//   k_mse_finish   one workgroup: the partials added in ascending block order from +0.0f, one rounded add each (one lane again, the
//                  partials staged through LDS), then the caller's gnnvc_fit_stats updated in place.
//   k_sgd_step     one element a thread.
// Plain loads and stores ordered by the stream, no atomics: a result depends on neither the grid nor the run.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gnnvc_backward.h"

namespace gnnvc {

namespace {

constexpr uint32_t kFitThreads = 256;
constexpr uint32_t kFinishChunk = 1024;   // partials k_mse_finish stages at a time

// the sum over the workgroup of three counts a thread, left in red[0 .. 2][0]: a tree over LDS
__device__ void fit_sum3(unsigned long long (*red)[kFitThreads], unsigned long long a, unsigned long long b, unsigned long long c) {
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    red[2][threadIdx.x] = c;
    __syncthreads();
    for (uint32_t s = kFitThreads / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s)
            for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
        __syncthreads();
    }
}

// One chain over v[0 .. count - 1] (LDS, 16-byte aligned) onto `total`, by the calling lane alone.  Sixteen values a step, the next
// step's four fetches issued ahead of this step's adds: the chain then waits for its adds, not for LDS.
__device__ inline float fit_add16(const float4 (&q)[4], float total) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        total = total + q[k].x;
        total = total + q[k].y;
        total = total + q[k].z;
        total = total + q[k].w;
    }
    return total;
}

__device__ float fit_chain(const float *v, uint32_t count, float total) {
    const float4 *v4 = reinterpret_cast<const float4 *>(v);
    uint32_t i = 0;
    if (count >= 16) {
        float4 cur[4], nxt[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) cur[k] = v4[k];
        for (; i + 32 <= count; i += 16) {
#pragma unroll
            for (int k = 0; k < 4; ++k) nxt[k] = v4[i / 4 + 4 + k];
            total = fit_add16(cur, total);
#pragma unroll
            for (int k = 0; k < 4; ++k) cur[k] = nxt[k];
        }
        total = fit_add16(cur, total);   // the last full step: nothing left to fetch ahead
        i += 16;
    }
    for (; i < count; ++i) total = total + v[i];
    return total;
}

// x, y and grad carry no __restrict__: grad may be x or y itself (every element is read by the thread that then writes it)
__global__ __launch_bounds__(kFitThreads) void k_mse_block(uint32_t rows, uint32_t width, const float *x, const float *y, float *grad,
                                                           float *__restrict__ partials, uint32_t *__restrict__ counts) {
    __shared__ __attribute__((aligned(16))) float rv[kGradBlockRows];
    __shared__ unsigned long long red[3][kFitThreads];
    const uint32_t r0 = blockIdx.x * kGradBlockRows;
    const uint32_t cnt = (rows - r0 > kGradBlockRows) ? kGradBlockRows : rows - r0;
    const float fw = (float)width;
    const bool stats = partials != nullptr;
    uint32_t pos = 0, pos_hit = 0, neg_hit = 0;
    for (uint32_t r = threadIdx.x; r < cnt; r += kFitThreads) {
        const size_t at = (size_t)(r0 + r) * width;
        const float x0 = x[at], y0 = y[at];   // column 0, before a gradient in place replaces it
        float se = 0.0f;
        for (uint32_t j = 0; j < width; ++j) {
            const float d = x[at + j] - y[at + j];
            if (grad) grad[at + j] = (2.0f * d) / fw;
            se = se + d * d;
        }
        if (stats) {
            rv[r] = se / fw;
            if (y0 > 0.5f) {   // run_model's comparisons: a NaN target is no positive, a NaN score no hit
                ++pos;
                if (x0 > 0.5f) ++pos_hit;
            } else if (x0 < 0.5f) {
                ++neg_hit;
            }
        }
    }
    if (!stats) return;
    fit_sum3(red, pos, pos_hit, neg_hit);   // (its first barrier also publishes rv)
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = fit_chain(rv, cnt, 0.0f);
        for (int q = 0; q < 3; ++q) counts[(size_t)blockIdx.x * 3 + q] = (uint32_t)red[q][0];
    }
}

__global__ __launch_bounds__(kFitThreads) void k_mse_finish(uint32_t rows, uint32_t blocks, const float *__restrict__ partials,
                                                            const uint32_t *__restrict__ counts, gnnvc_fit_stats *stats) {
    __shared__ __attribute__((aligned(16))) float pv[kFinishChunk];
    __shared__ unsigned long long red[3][kFitThreads];
    float total = 0.0f;
    for (uint32_t b0 = 0; b0 < blocks; b0 += kFinishChunk) {
        const uint32_t c = min(kFinishChunk, blocks - b0);
        __syncthreads();   // the previous chunk's chain has read LDS
        for (uint32_t i = threadIdx.x; i < c; i += kFitThreads) pv[i] = partials[b0 + i];
        __syncthreads();
        if (threadIdx.x == 0) total = fit_chain(pv, c, total);
    }
    unsigned long long s[3] = {0, 0, 0};
    for (uint32_t b = threadIdx.x; b < blocks; b += kFitThreads)
        for (int q = 0; q < 3; ++q) s[q] += counts[(size_t)b * 3 + q];
    fit_sum3(red, s[0], s[1], s[2]);
    if (threadIdx.x == 0) {
        stats->loss_sum = stats->loss_sum + (double)total;
        stats->rows += rows;
        stats->positives += red[0][0];
        stats->positive_hits += red[1][0];
        stats->negative_hits += red[2][0];
    }
}

__global__ void k_sgd_step(size_t count, float *__restrict__ w, float *__restrict__ vel, float *__restrict__ grad, float batch, float lr,
                           float momentum, float weight_decay, int zero_grad) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        float g = grad[i];
        if (weight_decay > 0.0f) g = g + ((2.0f * weight_decay) * w[i]);
        const float v = (momentum * vel[i]) + (g / batch);
        vel[i] = v;
        w[i] = w[i] - (lr * v);
        if (zero_grad) grad[i] = 0.0f;
    }
}

}  // namespace

hipError_t launch_fit_mse(uint32_t rows, uint32_t width, const float *x, const float *y, float *grad, float *partials, uint32_t *counts,
                          gnnvc_fit_stats *stats, hipStream_t stream) {
    if (!rows || !width || (!grad && !stats)) return hipSuccess;
    const uint32_t blocks = grad_blocks(rows);
    hipLaunchKernelGGL(k_mse_block, dim3(blocks), dim3(kFitThreads), 0, stream, rows, width, x, y, grad, stats ? partials : nullptr,
                       stats ? counts : nullptr);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess || !stats) return rc;
    hipLaunchKernelGGL(k_mse_finish, dim3(1), dim3(kFitThreads), 0, stream, rows, blocks, (const float *)partials,
                       (const uint32_t *)counts, stats);
    return hipGetLastError();
}

hipError_t launch_fit_sgd_step(size_t count, float *params, float *vel, float *grad, float batch, float lr, float momentum,
                               float weight_decay, bool zero_grad, hipStream_t stream) {
    if (!count) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<size_t>((count + 255) / 256, 8192);
    hipLaunchKernelGGL(k_sgd_step, dim3(blocks), dim3(256), 0, stream, count, params, vel, grad, batch, lr, momentum, weight_decay,
                       zero_grad ? 1 : 0);
    return hipGetLastError();
}

}  // namespace gnnvc
