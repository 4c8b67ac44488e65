// gnnvc_backward.hip — the gfx950 kernels of the backward pass (include/gnnvc.h "backward"; the order rules: DESIGN.md §3).
//
// Every sum has one stated order, so a gradient depends on neither the grid nor the run:
//   k_bwd_relu, k_bwd_sigmoid   one element a thread;
//   k_bwd_linear_dx             grad_in[i][kk]: one __builtin_fmaf chain over j = 0 .. m - 1 from +0.0f (gnnvc_sgemm with trans_b);
//   k_bwd_linear_dw             the partial of grad_W[kk][j] (and of grad_bias[j], the input column that is 1) over one block of
//                               kGradBlockRows rows: one __builtin_fmaf chain over the block's rows in ascending order, from +0.0f;
//   k_bwd_reduce_blocks         the partials added in ascending block order, one rounded add each from +0.0f, then — when
//                               accumulating — the old value plus that total, one more rounded add;
//   k_bwd_graph                 the neighbours' gradient rows added in stored (CSR) order from +0.0f, one rounded add each, then the
//                               own term, one more;
//   k_bwd_row_ascends, k_bwd_symmetry   the exact symmetry check k_bwd_graph's rule rests on.
// Compiled with -ffp-contract=off like every kernel of the library: only the explicit __builtin_fmaf calls fuse.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gnnvc_backward.h"

namespace gnnvc {

namespace {

inline unsigned bwd_blocks(size_t work, unsigned block) { return (unsigned)((work + block - 1) / block); }

// ------------------------------------------------------------------ activations
__global__ void k_bwd_relu(size_t count, const float *__restrict__ z, const float *__restrict__ gout, float *__restrict__ gin) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        gin[i] = (z[i] >= 0.0f) ? gout[i] : 0.0f;   // -0.0 passes, NaN gives 0
}

__global__ void k_bwd_sigmoid(size_t count, const float *__restrict__ s, const float *__restrict__ gout, float *__restrict__ gin) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        const float v = s[i];
        const float d = v * (1.0f - v);
        gin[i] = d * gout[i];
    }
}

// ------------------------------------------------------------------ linear layer: the input's gradient
// One thread per (row, input column), 256 consecutive outputs a workgroup.  The chain runs over W's row kk; LDSW stages W sixteen
// columns of all its k rows at a time (pitch 17: consecutive kk fall on different banks), else W is read through the caches.
constexpr int kDxCols = 16;

template <bool LDSW>
__global__ __launch_bounds__(256) void k_bwd_linear_dx(uint32_t n, uint32_t k, uint32_t m, const float *__restrict__ gout,
                                                       const float *__restrict__ W, float *__restrict__ gin) {
    extern __shared__ __attribute__((aligned(16))) float ws[];   // LDSW: k x (kDxCols + 1)
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = gid < (size_t)n * k;
    const uint32_t i = live ? (uint32_t)(gid / k) : 0, kk = live ? (uint32_t)(gid % k) : 0;
    const float *grow = gout + (size_t)i * m;
    float acc = 0.0f;
    if (LDSW) {
        for (uint32_t j0 = 0; j0 < m; j0 += kDxCols) {
            const uint32_t jc = min((uint32_t)kDxCols, m - j0);
            __syncthreads();
            for (uint32_t idx = threadIdx.x; idx < k * kDxCols; idx += 256) {
                const uint32_t r = idx / kDxCols, c = idx % kDxCols;
                ws[r * (kDxCols + 1) + c] = c < jc ? W[(size_t)r * m + j0 + c] : 0.0f;
            }
            __syncthreads();
            if (live)
                for (uint32_t c = 0; c < jc; ++c) acc = __builtin_fmaf(grow[j0 + c], ws[kk * (kDxCols + 1) + c], acc);
        }
    } else if (live) {
        const float *wrow = W + (size_t)kk * m;
        for (uint32_t j = 0; j < m; ++j) acc = __builtin_fmaf(grow[j], wrow[j], acc);
    }
    if (live) gin[gid] = acc;
}

// ------------------------------------------------------------------ linear layer: the parameters' gradient
// One workgroup per (row block, output tile).  256 threads as 16 x 16, each owning TK x TM accumulators: a tile of 16 TK rows of
// grad_W (row k: the bias) by 16 TM columns.  The block's rows of `in` and grad_out pass through LDS kDwRows at a time — fetched
// into registers one chunk ahead, so the next chunk's loads fly under this chunk's chains — and every thread walks them in
// ascending order: each accumulator is one chain.  Rows past the block's end are never fed to a chain (fmaf(0, 0, -0.0f) would
// turn an underflowed -0.0f into +0.0f); columns past the tile's use are zeros and their outputs dropped.
constexpr int kDwRows = 32;

template <int TK, int TM>
__global__ __launch_bounds__(256) void k_bwd_linear_dw(uint32_t n, uint32_t k, uint32_t m, uint32_t ke, const float *__restrict__ in,
                                                       const float *__restrict__ gout, float *__restrict__ partials) {
    constexpr int KW = 16 * TK, MW = 16 * TM;
    constexpr int PA = kDwRows * KW / 256, PG = kDwRows * MW / 256;   // staged elements a thread: 2 TK and 2 TM
    __shared__ __attribute__((aligned(16))) float sa[kDwRows][KW];
    __shared__ __attribute__((aligned(16))) float sg[kDwRows][MW];
    const uint32_t tiles_m = (m + MW - 1) / MW;
    const uint32_t k0 = (blockIdx.y / tiles_m) * KW, j0 = (blockIdx.y % tiles_m) * MW;
    const uint32_t r0 = blockIdx.x * kGradBlockRows;
    const uint32_t r1 = (n - r0 > kGradBlockRows) ? r0 + kGradBlockRows : n;
    const uint32_t tk = threadIdx.x / 16, tm = threadIdx.x % 16;
    float acc[TK][TM], pa[PA], pg[PG];
#pragma unroll
    for (int a = 0; a < TK; ++a)
#pragma unroll
        for (int b = 0; b < TM; ++b) acc[a][b] = 0.0f;
    // element e = threadIdx.x + 256 i of a chunk: row e / width, column e % width (rows past the block's end: zeros, never used)
    auto fetch = [&](uint32_t row) {
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const uint32_t e = threadIdx.x + 256 * i, r = row + e / KW, kk = k0 + e % KW;
            pa[i] = r >= r1 ? 0.0f : kk < k ? in[(size_t)r * k + kk] : kk < ke ? 1.0f : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < PG; ++i) {
            const uint32_t e = threadIdx.x + 256 * i, r = row + e / MW, j = j0 + e % MW;
            pg[i] = (r < r1 && j < m) ? gout[(size_t)r * m + j] : 0.0f;
        }
    };
    auto row_step = [&](uint32_t r) {
        float av[TK], gv[TM];
#pragma unroll
        for (int a = 0; a < TK; ++a) av[a] = sa[r][tk * TK + a];
#pragma unroll
        for (int b = 0; b < TM; ++b) gv[b] = sg[r][tm * TM + b];
#pragma unroll
        for (int a = 0; a < TK; ++a)
#pragma unroll
            for (int b = 0; b < TM; ++b) acc[a][b] = __builtin_fmaf(av[a], gv[b], acc[a][b]);
    };
    fetch(r0);
    for (uint32_t row = r0; row < r1; row += kDwRows) {
        __syncthreads();   // the previous chunk's chains have read LDS
#pragma unroll
        for (int i = 0; i < PA; ++i) (&sa[0][0])[threadIdx.x + 256 * i] = pa[i];
#pragma unroll
        for (int i = 0; i < PG; ++i) (&sg[0][0])[threadIdx.x + 256 * i] = pg[i];
        __syncthreads();
        if (row + kDwRows < r1) fetch(row + kDwRows);
        if (r1 - row >= (uint32_t)kDwRows) {
#pragma unroll 8
            for (uint32_t r = 0; r < (uint32_t)kDwRows; ++r) row_step(r);
        } else {
            for (uint32_t r = 0, rc = r1 - row; r < rc; ++r) row_step(r);
        }
    }
    float *dst = partials + (size_t)blockIdx.x * ke * m;
#pragma unroll
    for (int a = 0; a < TK; ++a) {
        const uint32_t kk = k0 + tk * TK + a;
#pragma unroll
        for (int b = 0; b < TM; ++b) {
            const uint32_t j = j0 + tm * TM + b;
            if (kk < ke && j < m) dst[(size_t)kk * m + j] = acc[a][b];
        }
    }
}

__global__ void k_bwd_reduce_blocks(uint32_t blocks, size_t outputs, const float *__restrict__ partials, float *__restrict__ grad,
                                    int accumulate) {
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= outputs) return;
    float total = 0.0f;
    for (uint32_t b = 0; b < blocks; ++b) total = total + partials[(size_t)b * outputs + o];
    grad[o] = accumulate ? grad[o] + total : total;
}

// ------------------------------------------------------------------ graph layer
// GS lanes (a power of two, at least f up to 64) own a vertex, a lane a column of it; f > 64 takes the columns 64 at a time.  The
// group fetches GS column ids at once and walks them in stored order, whatever the row's length: one chain per (vertex, column).
template <int GS>
__global__ __launch_bounds__(256) void k_bwd_graph(GraphDev g, uint32_t f, const float *__restrict__ gout, float *__restrict__ gin) {
    const uint32_t wd = 2 * f + 3;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t vv = gid / GS;
    const uint32_t sub = threadIdx.x % GS;
    const bool live = vv < g.n;
    const uint32_t v = live ? (uint32_t)vv : 0;
    const uint32_t rs = live ? g.rowptr[v] : 0, re = live ? g.rowptr[v + 1] : 0;
    const int gbase = (int)((threadIdx.x & 63) - sub);
    for (uint32_t jb = 0; jb < f; jb += GS) {
        const uint32_t j = jb + sub;
        const bool has = j < f;
        float acc = 0.0f;
        for (uint32_t e = rs; e < re; e += GS) {
            const uint32_t cnt = min((uint32_t)GS, re - e);
            const uint32_t mine = sub < cnt ? g.col[e + sub] : 0;
            for (uint32_t t = 0; t < cnt; ++t) {
                const uint32_t u = GS == 1 ? mine : (uint32_t)__shfl((int)mine, gbase + (int)t);
                if (has) acc = acc + gout[(size_t)u * wd + j];
            }
        }
        if (has && live) {
            // the forward writes degree, W / ws and NW / ws over columns f + 1 .. f + 3: they carry no own term
            const float own = (j >= 1 && j <= 3) ? 0.0f : gout[(size_t)v * wd + f + j];
            gin[(size_t)v * f + j] = acc + own;
        }
    }
}

// ------------------------------------------------------------------ symmetry of the adjacency, with multiplicities
// info[1] = the longest row that does not ascend: every entry of such a row costs k_bwd_symmetry a scan of the row (and of the
// partner's, if that does not ascend either), so the engine looks at this length before it launches the scans
__global__ void k_bwd_row_ascends(GraphDev g, uint8_t *__restrict__ asc, uint32_t *__restrict__ info) {
    const size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= g.n) return;
    bool up = true;
    const uint32_t rs = g.rowptr[v], re = g.rowptr[v + 1];
    for (uint32_t e = rs + 1; e < re && up; ++e) up = g.col[e - 1] <= g.col[e];
    asc[v] = up ? 1 : 0;
    if (!up) atomicMax(info + 1, re - rs);
}

// how often `target` is stored in row `row`: two binary searches where the row ascends, a scan otherwise
__device__ uint32_t bwd_count_in_row(const GraphDev &g, const uint8_t *asc, uint32_t row, uint32_t target) {
    const uint32_t rs = g.rowptr[row], re = g.rowptr[row + 1];
    if (asc[row]) {
        uint32_t lo = rs, hi = re;
        while (lo < hi) {   // first entry >= target
            const uint32_t mid = lo + (hi - lo) / 2;
            if (g.col[mid] < target) lo = mid + 1; else hi = mid;
        }
        const uint32_t first = lo;
        hi = re;
        while (lo < hi) {   // first entry > target
            const uint32_t mid = lo + (hi - lo) / 2;
            if (g.col[mid] <= target) lo = mid + 1; else hi = mid;
        }
        return lo - first;
    }
    uint32_t c = 0;
    for (uint32_t e = rs; e < re; ++e) c += g.col[e] == target;
    return c;
}

__global__ void k_bwd_symmetry(GraphDev g, const uint8_t *__restrict__ asc, uint32_t *__restrict__ flag) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= g.nnz) return;
    uint32_t lo = 0, hi = g.n;   // the row of entry e: the last v with rowptr[v] <= e (rowptr[n] = nnz > e)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (g.rowptr[mid] <= e) lo = mid; else hi = mid;
    }
    const uint32_t v = lo, u = g.col[e];
    if (u >= g.n || bwd_count_in_row(g, asc, v, u) != bwd_count_in_row(g, asc, u, v)) atomicOr(flag, 1u);
}

template <int TK, int TM>
void dw_launch(uint32_t n, uint32_t k, uint32_t m, uint32_t ke, const float *in, const float *gout, float *partials, hipStream_t stream) {
    const uint32_t tiles = ((ke + 16 * TK - 1) / (16 * TK)) * ((m + 16 * TM - 1) / (16 * TM));
    hipLaunchKernelGGL((k_bwd_linear_dw<TK, TM>), dim3(grad_blocks(n), tiles), dim3(256), 0, stream, n, k, m, ke, in, gout, partials);
}

// The tile per side: 4 above 48 values, 3 above 32, 2 above 16, else 1 — here for m, in launch_bwd_linear_dw for ke.
// tests/test_backward_reference.py (test_tables_cover_every_kernel_form) restates this rule, the LDS limit of
// launch_bwd_linear_dx and the group sizes of launch_bwd_graph as arithmetic on the shapes of the tests' tables, and asserts
// that they reach all sixteen (TK, TM), both k_bwd_linear_dx and every k_bwd_graph with f > 64: change it with the rule.
template <int TK>
void dw_launch_m(uint32_t n, uint32_t k, uint32_t m, uint32_t ke, const float *in, const float *gout, float *partials, hipStream_t stream) {
    if (m > 48) dw_launch<TK, 4>(n, k, m, ke, in, gout, partials, stream);
    else if (m > 32) dw_launch<TK, 3>(n, k, m, ke, in, gout, partials, stream);
    else if (m > 16) dw_launch<TK, 2>(n, k, m, ke, in, gout, partials, stream);
    else dw_launch<TK, 1>(n, k, m, ke, in, gout, partials, stream);
}

}  // namespace

hipError_t launch_bwd_relu(size_t count, const float *z, const float *grad_out, float *grad_in, hipStream_t stream) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(k_bwd_relu, dim3(std::min(bwd_blocks(count, 256), 8192u)), dim3(256), 0, stream, count, z, grad_out, grad_in);
    return hipGetLastError();
}

hipError_t launch_bwd_sigmoid(size_t count, const float *s, const float *grad_out, float *grad_in, hipStream_t stream) {
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(k_bwd_sigmoid, dim3(std::min(bwd_blocks(count, 256), 8192u)), dim3(256), 0, stream, count, s, grad_out, grad_in);
    return hipGetLastError();
}

hipError_t launch_bwd_linear_dx(uint32_t n, uint32_t k, uint32_t m, const float *grad_out, const float *W, float *grad_in,
                                hipStream_t stream) {
    const size_t work = (size_t)n * k;
    if (!work) return hipSuccess;
    const size_t lds = (size_t)k * (kDxCols + 1) * sizeof(float);
    if (lds <= 32768)   // k <= 481: every width the parser's models reach (131), with room
        hipLaunchKernelGGL((k_bwd_linear_dx<true>), dim3(bwd_blocks(work, 256)), dim3(256), lds, stream, n, k, m, grad_out, W, grad_in);
    else
        hipLaunchKernelGGL((k_bwd_linear_dx<false>), dim3(bwd_blocks(work, 256)), dim3(256), 0, stream, n, k, m, grad_out, W, grad_in);
    return hipGetLastError();
}

hipError_t launch_bwd_linear_dw(uint32_t n, uint32_t k, uint32_t m, bool with_bias, const float *in, const float *grad_out,
                                float *partials, float *grad, bool accumulate, hipStream_t stream) {
    const uint32_t ke = k + (with_bias ? 1u : 0u);
    const size_t outputs = (size_t)ke * m;
    if (!outputs) return hipSuccess;
    if (n) {
        if (ke > 48) dw_launch_m<4>(n, k, m, ke, in, grad_out, partials, stream);
        else if (ke > 32) dw_launch_m<3>(n, k, m, ke, in, grad_out, partials, stream);
        else if (ke > 16) dw_launch_m<2>(n, k, m, ke, in, grad_out, partials, stream);
        else dw_launch_m<1>(n, k, m, ke, in, grad_out, partials, stream);
        hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
    }
    hipLaunchKernelGGL(k_bwd_reduce_blocks, dim3(bwd_blocks(outputs, 256)), dim3(256), 0, stream, grad_blocks(n), outputs,
                       (const float *)partials, grad, accumulate ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_bwd_graph(const GraphDev &g, uint32_t f, const float *grad_out, float *grad_in, hipStream_t stream) {
    if (!g.n || !f) return hipSuccess;
#define GNNVC_BWD_GRAPH(GS_)                                                                                                 \
    hipLaunchKernelGGL((k_bwd_graph<GS_>), dim3(bwd_blocks((size_t)g.n * GS_, 256)), dim3(256), 0, stream, g, f, grad_out, grad_in)
    if (f == 1) GNNVC_BWD_GRAPH(1);
    else if (f <= 2) GNNVC_BWD_GRAPH(2);
    else if (f <= 4) GNNVC_BWD_GRAPH(4);
    else if (f <= 8) GNNVC_BWD_GRAPH(8);
    else if (f <= 16) GNNVC_BWD_GRAPH(16);
    else if (f <= 32) GNNVC_BWD_GRAPH(32);
    else GNNVC_BWD_GRAPH(64);
#undef GNNVC_BWD_GRAPH
    return hipGetLastError();
}

hipError_t launch_bwd_row_ascends(const GraphDev &g, uint8_t *row_ascends, uint32_t *info, hipStream_t stream) {
    hipError_t rc = hipMemsetAsync(info, 0, 2 * sizeof(uint32_t), stream);
    if (rc != hipSuccess || !g.n) return rc;
    hipLaunchKernelGGL(k_bwd_row_ascends, dim3(bwd_blocks(g.n, 256)), dim3(256), 0, stream, g, row_ascends, info);
    return hipGetLastError();
}

hipError_t launch_bwd_symmetry(const GraphDev &g, const uint8_t *row_ascends, uint32_t *info, hipStream_t stream) {
    if (!g.n || !g.nnz) return hipSuccess;
    hipLaunchKernelGGL(k_bwd_symmetry, dim3(bwd_blocks(g.nnz, 256)), dim3(256), 0, stream, g, row_ascends, info);
    return hipGetLastError();
}

}  // namespace gnnvc
