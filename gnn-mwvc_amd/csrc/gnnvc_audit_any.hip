// gnnvc_audit_any.hip — k_audit_any: the on-device audit of a GENERIC fused stage (gnnvc_forward_audited*,
// gnnvc_audit_stage_device).  It recomputes one stage — graph layer of input width f, d = 1 .. 6 dense layers of widths
// n[0 .. d), ReLU | sigmoid — for rows [lo, hi) from the stage's own input and compares every value the fused path wrote: the
// n[d - 1]-wide output row, or the scores and the logits on the sigmoid stage.  Bounds: whatever stage_any_fits admits (1 <= f <= 32,
// every width but the last <= 64 — <= 128 in a big stage, gnnvc_set_generic_big_stages — the last <= 32; f and the last width up to
// 64 under gnnvc_set_generic_feature_width).  Under gnnvc_set_generic_patterns a stage may be DENSE — no graph layer: the row is
// the stage's own input row, f columns, and the first K is f — and the model's last stage may end in a ReLU or in its bare linear
// layer, whose pre-activation is then what the fused path stored (`sig`: kEndRelu, kEndSigmoid, kEndNone; logits are compared on a
// sigmoid stage only).
//
// What is computed is the layer-by-layer kernels' arithmetic (k_graph_layer, k_linear, k_relu, k_sigmoid):
//   neighbour-sum column c   one fp32 add chain in stored CSR order from +0.0f;
//   the row                  [sums (f) | own (f) | 0 0 0], then degree, W / ws, NW / ws written LAST into columns f + 1 .. f + 3;
//   each linear output       one __builtin_fmaf chain over k = 0 .. K - 1 from +0.0f, then a separately rounded bias add;
//   relu_ref, or sigmoid_ref on the model's last layer.
// Compile with -ffp-contract=off, like the rest of the library.
//
// The kernel shares no code and no layout with k_stage_any (gnnvc_stage_any.hip) or k_audit_stage (gnnvc_kernels.hip): two
// implementations that agree bit for bit are evidence only while they are two.  Where those give a row to sixteen lanes, deal
// the outputs o = j + 16 t, transpose the weights into LDS at a padded pitch and walk k four at a time, this one is laid out the
// other way round:
//   a WAVE per row (four rows per 256-thread workgroup, grid-stride, no workgroup barrier anywhere);
//   lane o owns output o of every layer — and output o + 64 of a layer wider than the wave (a big stage's, at most 128), a second
//   chain of its own behind the first — and runs its whole chain, k advancing one at a time; the weight W[k][o] is read where the model put it, in the stored [k][n] layout straight from the parameter block (the
//   lanes of a wave read consecutive words; a stage's parameters are a few KiB that stay in the caches), nothing is transposed
//   and nothing copied to LDS;
//   the row's activations live in two per-wave LDS vectors of 132 floats (static LDS, 4224 bytes a workgroup) that the layers
//   ping-pong through; x[k] is one broadcast read;
//   the graph row has K = 2 f + 3 <= 131 columns — more than a wave — so it is written by a loop over c = lane, lane + 64, lane + 128;
//   lanes c < f each run their column's add chain over the neighbours: the wave fetches 64 column ids at a time (the next 64
//   already on their way), takes eight neighbours' rows per lane into registers, then adds them in order.  f = 1 has one
//   column and so one chain: every lane fetches one neighbour's value, and the values are added in stored order through lane
//   reads.  Rows of any degree take this loop; the kernel sees rowptr / col / w / nw and nothing else of the graph.
//
// Two values are equal when their bits are, or when both are NaN (counted apart: every pair of NaNs is counted, also one whose
// payloads agree — two implementations that run the same operations in the same order mostly hand the same NaN on, and a
// caller who feeds NaNs wants to see that they were met).  Record (kAuditWords zeroed 64-bit words, the
// one k_audit_stage writes): [0] the exact number of mismatching values, [1] NaN pairs, [2] repairs, and of the first
// mismatching row its first mismatching value: [3] ~(row << 32 | column code), [4] ~(row << 32 | fused bits), [5] ~(row << 32 |
// audit bits) — atomicMax of the complements; a row is checked by exactly one wave, which submits one triple, so the three
// minima belong together.  Column code: the output column, + 64 for a logit (widths are at most 64: the codes stay below 128).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "expf_glibc.h"
#include "gnnvc_kernels.h"

namespace gnnvc {

namespace {

// (the layer-by-layer kernels' two activations, restated: (x < 0) ? 0 : x, and 1 / (1 + expf(-x)) with glibc's expf)
__device__ __forceinline__ float relu_ref(float x) { return (x < 0.0f) ? 0.0f : x; }
__device__ __forceinline__ float sigmoid_ref(float x) { return 1.0f / (1.0f + expf_glibc(-x)); }

// LDS operations of one wave execute in program order; this keeps the compiler from moving them across a hand-off
__device__ __forceinline__ void wave_handoff() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

constexpr int kBlockThreads = 256, kWaves = kBlockThreads / 64;
constexpr int kVec = 132;   // floats per activation vector: the graph row's 2 * 64 + 3 = 131 columns, hidden widths up to 128
// (f <= 64: a lane has at most ONE sum column, c == lane; a last layer of at most 64 outputs: one per lane, and a column code
// below 64 with 64 left for the logits' flag)
static_assert(kVec >= 2 * kAnyFeatMax + 3 && kVec >= kAnyBigHidden && kAnyBigHidden <= 2 * 64 && kAnyMaxLast <= kAnyFeatMax && kAnyFeatMax <= 64,
              "the vectors, the one sum column and the two outputs a lane owns, and the column code are sized for what stage_any_route admits");

struct AuditGraph {   // the graph as handed over
    const uint32_t *rowptr, *col, *w, *nw;
};
struct AuditShape {
    int f, d;
    int n[kMaxDenseLayers];
};

__device__ __forceinline__ bool is_nan_bits(uint32_t b) { return (b & 0x7FFFFFFFu) > 0x7F800000u; }

__global__ __launch_bounds__(kBlockThreads) void k_audit_any(AuditGraph g, float ws, const float *__restrict__ P,
                                                             const float *__restrict__ in, float *out, float *logits, uint32_t lo,
                                                             uint32_t hi, AuditShape S, int sig, unsigned long long *__restrict__ rec,
                                                             int repair, int dense) {
    __shared__ float vec[kWaves][2][kVec];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t f = (uint32_t)S.f;
    const int d = S.d, k1 = dense ? S.f : 2 * S.f + 3;   // (dense: wave-uniform, a kernel argument)
    const uint32_t cl = min((uint32_t)lane, f - 1u);   // the lane's neighbour column (lanes >= f fetch a copy nobody uses)
    // what this wave has found over all its rows (kept by every lane alike; lane 0 submits it once, at the end)
    unsigned long long n_bad = 0, n_nan = 0, first_row = 0;
    uint32_t first_code = 0, first_fused = 0, first_audit = 0;
    bool have_first = false;
    for (uint64_t u64 = (uint64_t)lo + (uint64_t)blockIdx.x * kWaves + (uint64_t)wave; u64 < hi; u64 += (uint64_t)gridDim.x * kWaves) {
        const uint32_t u = (uint32_t)u64;
        float *a = vec[wave][0], *b = vec[wave][1];
        if (dense) {
            // ---- a dense stage: the row is row u of the input (f <= 64: one column a lane); no array of the graph is read
            if ((uint32_t)lane < f) a[lane] = in[(size_t)u * f + (uint32_t)lane];
        } else {
            // ---- graph layer: column cl's chain
            const uint32_t rs = g.rowptr[u], re = g.rowptr[u + 1];
            float s = 0.0f;
            uint32_t next_ids = (rs + (uint32_t)lane < re) ? g.col[rs + lane] : 0u;
            for (uint32_t e = rs; e < re; e += 64u) {
                const uint32_t ids = next_ids, m = min(64u, re - e);
                next_ids = (e + 64u + (uint32_t)lane < re) ? g.col[e + 64u + lane] : 0u;
                if (f == 1u) {
                    const float mine = in[ids];   // (lanes >= m: ids == 0, a valid row nobody adds)
                    for (uint32_t i = 0; i < m; ++i) s = s + __shfl(mine, (int)i);
                } else {
                    for (uint32_t i0 = 0; i0 < m; i0 += 8u) {
                        float v[8];
#pragma unroll
                        for (uint32_t t = 0; t < 8u; ++t) {
                            const uint32_t nb = (uint32_t)__shfl((int)ids, (int)min(i0 + t, m - 1u));
                            v[t] = in[(size_t)nb * f + cl];
                        }
#pragma unroll
                        for (uint32_t t = 0; t < 8u; ++t)
                            if (i0 + t < m) s = s + v[t];
                    }
                }
            }
            const float deg = (float)(re - rs), wv = (float)g.w[u] / ws, nwv = (float)g.nw[u] / ws;
            for (int c = lane; c < k1; c += 64) {
                float v = 0.0f;
                if (c < (int)f) v = s;   // (f <= 64: c == lane here)
                else if (c < 2 * (int)f) v = in[(size_t)u * f + (uint32_t)(c - (int)f)];
                if (c == (int)f + 1) v = deg;
                if (c == (int)f + 2) v = wv;
                if (c == (int)f + 3) v = nwv;
                a[c] = v;
            }
        }
        wave_handoff();
        // ---- the dense layers: lane o = output o; W[k * N + o] from the parameter block as stored
        const float *W = P;
        int K = k1;
        float r = 0.0f;
        for (int l = 0; l < d; ++l) {
            const int N = S.n[l], o = min(lane, N - 1);   // (lanes >= N run a copy of the last chain and drop it)
            float acc = 0.0f;
#pragma unroll 8   // (the loads of eight steps on their way together; the chain itself stays one fma per k, in k order)
            for (int k = 0; k < K; ++k) acc = __builtin_fmaf(a[k], W[k * N + o], acc);
            r = acc + W[K * N + o];
            if (l + 1 < d) {
                if (lane < N) b[lane] = relu_ref(r);
                if (N > 64) {   // (wave-uniform) a layer wider than the wave: output lane + 64, the same way
                    const int o1 = min(lane + 64, N - 1);
                    float acc1 = 0.0f;
#pragma unroll 8
                    for (int k = 0; k < K; ++k) acc1 = __builtin_fmaf(a[k], W[k * N + o1], acc1);
                    const float r1 = acc1 + W[K * N + o1];
                    if (lane + 64 < N) b[lane + 64] = relu_ref(r1);
                }
                wave_handoff();
                float *t = a;
                a = b;
                b = t;
                W += K * N + N;
                K = N;
            }
        }
        // ---- compare (and repair): lane o < n_out holds output o's pre-activation in r
        const int n_out = S.n[d - 1];
        uint32_t cnt = 0, nan = 0, code = 0, fb = 0, pb = 0;
        if (lane < n_out) {
            auto check = [&](float *p, float want, uint32_t cc) {
                const uint32_t x = __float_as_uint(*p), y = __float_as_uint(want);
                if (is_nan_bits(x) && is_nan_bits(y)) { ++nan; return; }   // (whatever their payloads, the same included)
                if (x == y) return;
                if (cnt++ == 0) { code = cc; fb = x; pb = y; }
                if (repair) *p = want;
            };
            const size_t at = (size_t)u * (uint32_t)n_out + (uint32_t)lane;
            if (sig == kEndSigmoid) {
                check(out + at, sigmoid_ref(r), (uint32_t)lane);
                if (logits) check(logits + at, r, 64u + (uint32_t)lane);
            } else if (sig == kEndNone) {
                check(out + at, r, (uint32_t)lane);
            } else {
                check(out + at, relu_ref(r), (uint32_t)lane);
            }
        }
        wave_handoff();   // (the wave's vectors are rewritten by its next row)
        // exact counts: the sum over the lanes (a lane holds up to two mismatches)
        const unsigned long long any_bad = __ballot(cnt != 0), any_nan = __ballot(nan != 0);
        if (any_bad) {
            n_bad += (unsigned long long)(__popcll(__ballot(cnt & 1u)) + 2 * __popcll(__ballot(cnt & 2u)));
            if (!have_first) {   // rows ascend along the wave's walk: its first failing row is its lowest
                const int L = __ffsll((long long)any_bad) - 1;   // columns ascend with the lane
                have_first = true;
                first_row = (unsigned long long)u << 32;
                first_code = (uint32_t)__shfl((int)code, L);
                first_fused = (uint32_t)__shfl((int)fb, L);
                first_audit = (uint32_t)__shfl((int)pb, L);
            }
        }
        if (any_nan) n_nan += (unsigned long long)(__popcll(__ballot(nan & 1u)) + 2 * __popcll(__ballot(nan & 2u)));
    }
    if (lane == 0) {
        if (n_bad) {
            atomicAdd(rec + 0, n_bad);
            if (repair) atomicAdd(rec + 2, n_bad);
            atomicMax(rec + 3, ~(first_row | first_code));
            atomicMax(rec + 4, ~(first_row | first_fused));
            atomicMax(rec + 5, ~(first_row | first_audit));
        }
        if (n_nan) atomicAdd(rec + 1, n_nan);
    }
}

}  // namespace

hipError_t launch_audit_any(const StageCall &c, unsigned long long *rec, bool repair) {
    if (c.row_hi <= c.row_lo) return hipSuccess;
    const StagePlan &sp = *c.sp;
    const GraphDev &g = *c.g;
    if (!stage_any_fits(sp) || c.row_hi > g.hi() || c.row_lo < g.lo() || !rec) return hipErrorInvalidValue;
    AuditShape S{};
    S.f = sp.f;
    S.d = sp.nd;
    for (int l = 0; l < kMaxDenseLayers; ++l) S.n[l] = (l < sp.nd) ? sp.wn[l] : 0;
    // (stage_any_fits' bounds are what the vectors and the column code are sized for: the static_assert at kVec)
    // the graph as handed over and nothing else: no plan's view can reach the audit
    const AuditGraph plain = sp.dense ? AuditGraph{nullptr, nullptr, nullptr, nullptr} : AuditGraph{g.rowptr, g.col, g.w, g.nw};
    // a persistent grid: a wave per row, up to eight workgroups on each of 256 CUs
    const size_t need = ((size_t)(c.row_hi - c.row_lo) + kWaves - 1) / kWaves;
    const dim3 grid((unsigned)std::min<size_t>(need, 2048u)), block(kBlockThreads);
    hipLaunchKernelGGL(k_audit_any, grid, block, 0, c.stream, plain, c.ws, c.params + sp.param_offset, c.in, c.out,
                       sp.sigmoid_last ? c.logits : nullptr, c.row_lo, c.row_hi, S, sp.end, rec, repair ? 1 : 0, sp.dense ? 1 : 0);
    return hipGetLastError();
}

}  // namespace gnnvc
