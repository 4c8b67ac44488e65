// gnnvc_stage_any.hip — k_stage_any: one fused stage (graph layer, one to six dense layers, ReLU | sigmoid) whose depth and
// widths are kernel ARGUMENTS, for models that are laid out like the trained one but are not of its shape (a retrain with 8-,
// 24- or 64-wide hidden layers, two or four dense layers after a graph layer, another feature width, several input features or
// outputs).  The trained shapes keep their own kernels in gnnvc_kernels.hip; nothing here is shared with them or with
// k_audit_stage.
//
// What is computed is the layer-by-layer kernels' arithmetic (k_graph_layer, k_linear, k_relu, k_sigmoid):
//   neighbour-sum column c   one fp32 add chain in stored CSR order from +0.0f;
//   the row                  [sums (f) | own (f) | 0 0 0], then degree, W / ws, NW / ws written LAST into columns f + 1 .. f + 3
//                            (for f > 1 they land on own-feature columns, as in k_graph_layer);
//   each linear output       one __builtin_fmaf chain over k = 0 .. K - 1 from +0.0f, then a separately rounded bias add;
//   relu_ref, or sigmoid_ref on the last layer of the last stage (the logits are its input).
// Compile with -ffp-contract=off, like the rest of the library.
//
// Bounds (stage_any_route, which stage_any_fits asks), by default: 1 <= f <= 32, 1 <= d <= 6 dense layers, every width but the last 1 .. 64, the
// last 1 .. 32, and the LDS layout below within 64 KiB (the dynamic LDS a launch gets without raising the kernel's limit).  A
// stage within these launches the kernel's default instantiations, whatever else is set.  With gnnvc_set_generic_big_stages a
// stage outside them is admitted when its hidden widths are at most 128 and its layout at 256 threads fits the limit given (at
// most 160 KiB, a CU's LDS): it launches a BIG instantiation (below), whose limit allow_big_stages has raised.  With
// gnnvc_set_generic_feature_width f and the last width may be up to the width given (33 .. 64): a stage that uses the allowance
// launches a FEAT instantiation (below), and must still fit the LDS and hidden-width bounds, default or big, like any other.
// With gnnvc_set_generic_patterns a stage may be DENSE — no graph layer in front: the row is row u of the input itself and the
// first K is f, within the same bounds (the kAnyDense instantiations below) — and the model's last stage may end in a ReLU or in
// its bare linear layer, whose pre-activation is stored (the OPEN instantiations).
//
// Shape of the kernel: 256-thread workgroups walk the row range 16 rows at a time (grid-stride; no workgroup barrier inside
// the walk, so a wave that sits on a very long row holds up nobody else).  Each workgroup first transposes the stage's
// weight matrices into LDS (wt[o * pitch + k], a pitch per layer, any_pitch(K): an odd number of 16-byte slots, so the sixteen
// lanes of a group read sixteen different 16-byte slots of the bank row).  A 16-lane group owns a row and two LDS vectors, A
// and B: the graph row goes to A, layer 1 writes B, layer 2 A, ... (each vector as long as the longest that ever lands in
// it), and the last layer goes from whichever holds its input — A itself when d = 1 — straight to memory:
//   gather   lane j owns neighbour columns j and j + 16.  The group fetches the column ids of a round (32 entries; 16 when
//            f > 16), the next round's already on their way, issues the round's 32 row loads per lane, then adds them in
//            order.  f = 1: every lane fetches one neighbour's value per 16 entries, 64 entries a round, and all lanes add
//            them in the same order.  Rows of any degree can take this loop; the heavy ones get their
//            sums from k_any_heavy_sums instead (below), and the giant ones among those from the exact parallel scan behind
//            k_any_giant_gather (further below): that changes who adds, not what is added.
//   dense    the outputs of a layer are dealt to the lanes (o = j + 16 t); a lane runs its outputs' chains together, four
//            k at a time: one 16-byte read of the group's input vector (same address for the group) and one per output of
//            its transposed weight row.  The number of outputs per lane (1 .. 4) is a template argument chosen by a
//            wave-uniform switch per layer, so the accumulators stay in registers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "expf_glibc.h"
#include "gnnvc_kernels.h"

namespace gnnvc {

namespace {

// (the same two functions as gnnvc_kernels.hip's: (x < 0) ? 0 : x, and 1 / (1 + expf(-x)) with glibc's expf restated)
__device__ __forceinline__ float relu_ref(float x) { return (x < 0.0f) ? 0.0f : x; }
__device__ __forceinline__ float sigmoid_ref(float x) { return 1.0f / (1.0f + expf_glibc(-x)); }

__device__ __forceinline__ void wave_lds_sync() {
    // LDS operations of one wave execute in program order; this keeps the compiler from moving them across the hand-off
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

constexpr int kAnyBlock = 256, kAnyRows = kAnyBlock / 16;

// what the kernel reads of GraphDev: the graph as handed over and nothing else — no plan's view reaches it
struct AnyGraph {
    const uint32_t *rowptr, *col, *w, *nw;
};

}  // namespace

// what the kernel is told of the stage, by value: f, the number of dense layers and their widths
struct AnyShape {
    int f, d;
    int n[kMaxDenseLayers];
};

// LDS layout, in floats (host and device agree through this one function): the layers' transposed weights one after the other
// (layer l: n[l] rows of any_pitch(K_l) floats), the biases, then per group [A | B]
struct StageAnyLayout {
    int bias, grp;   // offsets (the weights start at 0)
    int gs, hb;      // per group: gs floats — [0, hb) vector A, [hb, gs) vector B
    int total;
};
__host__ __device__ inline int any_round4(int v) { return (v + 3) / 4 * 4; }
__host__ __device__ inline int any_pitch(int k) {
    return 4 * (((k + 3) / 4) | 1);   // an odd number of 16-byte slots: rows o .. o + 15 start in sixteen different slots
}
// first_k: the first layer's K — 0 = a graph stage's 2 f + 3 (every call site but a dense stage's), f for a dense stage
__host__ __device__ inline StageAnyLayout stage_any_layout(const AnyShape &S, int rows, int first_k = 0) {   // rows: a workgroup's rows per pass (threads / 16)
    StageAnyLayout L;
    int K = first_k ? first_k : 2 * S.f + 3, wsum = 0, nsum = 0, a = K, b = 0;   // a, b: the longest vector that lands in A, in B
    for (int l = 0; l < S.d; ++l) {
        const int N = S.n[l];
        wsum += N * any_pitch(K);
        nsum += N;
        if (l + 1 < S.d) {   // (the last layer's outputs go to memory)
            if (l & 1) a = a > N ? a : N;
            else b = b > N ? b : N;
        }
        K = N;
    }
    L.bias = wsum;
    L.grp = L.bias + any_round4(nsum);
    L.hb = any_round4(a);
    L.gs = L.hb + any_round4(b);
    L.total = L.grp + rows * L.gs;
    return L;
}
constexpr size_t kAnyLdsBytes = 64u * 1024u;         // the dynamic LDS a launch gets without raising the kernel's limit
constexpr size_t kAnyBigLdsBytes = 160u * 1024u;     // a CU's LDS: the most gnnvc_set_generic_big_stages may allow a workgroup

namespace {

// T outputs per lane (o = j + 16 t, clamped to the layer's last output for lanes that have none there: they compute a copy
// nobody stores): acc[t] = fma-chain over k = 0 .. K - 1 of x[k] * wt[o * pitch + k], from +0.0f; + bias[o] rounded on its own
template <int T>
__device__ __forceinline__ void any_chains(const float *x, int K, const float *wt, int pitch, const float *bias, int N, int j,
                                           float (&res)[T]) {
    const float *wrow[T];
    float acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        wrow[t] = wt + min(j + 16 * t, N - 1) * pitch;
        acc[t] = 0.0f;
    }
    int k = 0;
#pragma unroll 1   // (unrolled, the T = 4 bodies cost 60 VGPRs and a wave per SIMD)
    for (; k + 4 <= K; k += 4) {
        const float4 x4 = *reinterpret_cast<const float4 *>(x + k);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const float4 w4 = *reinterpret_cast<const float4 *>(wrow[t] + k);
            acc[t] = __builtin_fmaf(x4.x, w4.x, acc[t]);
            acc[t] = __builtin_fmaf(x4.y, w4.y, acc[t]);
            acc[t] = __builtin_fmaf(x4.z, w4.z, acc[t]);
            acc[t] = __builtin_fmaf(x4.w, w4.w, acc[t]);
        }
    }
    for (; k < K; ++k) {
        const float xv = x[k];
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = __builtin_fmaf(xv, wrow[t][k], acc[t]);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) res[t] = acc[t] + bias[min(j + 16 * t, N - 1)];
}

// a hidden layer: dst[o] = relu_ref(chain + bias), o < N
template <int T>
__device__ __forceinline__ void any_hidden(const float *x, int K, const float *wt, int pitch, const float *bias, int N, int j,
                                           float *dst) {
    float r[T];
    any_chains<T>(x, K, wt, pitch, bias, N, j, r);
#pragma unroll
    for (int t = 0; t < T; ++t)
        if (j + 16 * t < N) dst[j + 16 * t] = relu_ref(r[t]);
}

__device__ __forceinline__ void any_hidden_n(const float *x, int K, const float *wt, int pitch, const float *bias, int N, int j,
                                             float *dst) {
    switch ((N + 15) >> 4) {   // (wave-uniform)
    case 1: any_hidden<1>(x, K, wt, pitch, bias, N, j, dst); break;
    case 2: any_hidden<2>(x, K, wt, pitch, bias, N, j, dst); break;
    case 3: any_hidden<3>(x, K, wt, pitch, bias, N, j, dst); break;
    default: any_hidden<4>(x, K, wt, pitch, bias, N, j, dst); break;
    }
}

// the stage's last layer, straight to memory: row u of out (and of logits, sigmoid stage, when asked for).  sig: kEndRelu or
// kEndSigmoid — and, in the OPEN instantiations only, kEndNone: the pre-activation itself is stored (a select beside the ReLU's).
// OPEN is a template argument so that the instantiations that were there compile to what they compiled to: as a third runtime
// value of `sig` it changed the code of all of them (67 to 254 more instructions each, other SGPR counts).
template <int T, bool OPEN>
__device__ __forceinline__ void any_last(const float *x, int K, const float *wt, int pitch, const float *bias, int N, int j,
                                         int sig, float *out_row, float *logit_row) {
    float r[T];
    any_chains<T>(x, K, wt, pitch, bias, N, j, r);
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int o = j + 16 * t;
        if (o < N) {
            if (OPEN ? sig == kEndSigmoid : sig != 0) {
                out_row[o] = sigmoid_ref(r[t]);
                if (logit_row) logit_row[o] = r[t];
            } else {
                if constexpr (OPEN) out_row[o] = sig == kEndNone ? r[t] : relu_ref(r[t]);
                else out_row[o] = relu_ref(r[t]);
            }
        }
    }
}

// the neighbour sums of row [rs, re): s0 = column j, s1 = column j + 16 (TWO: f > 16).  A round fetches 32 entries' rows (16
// when a lane owns two columns): 32 loads in flight per lane either way, the next round's column ids already on their way.
// Loads of lanes without a column, and of slots behind the row's end, go to a valid address (row 0 / the lane's last column)
// and are never added.
template <bool TWO>
__device__ __forceinline__ void any_gather(const uint32_t *__restrict__ col, const float *__restrict__ in, uint32_t rs, uint32_t re,
                                           uint32_t f, int j, int gbase, float &s0, float &s1) {
    constexpr int CH = TWO ? 1 : 2;
    const uint32_t c0 = min((uint32_t)j, f - 1u), c1 = min((uint32_t)j + 16u, f - 1u);
    uint32_t cn[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) cn[c] = (rs + 16u * c + j < re) ? col[rs + 16u * c + j] : 0u;
    for (uint32_t e = rs; e < re; e += 16u * CH) {
        const uint32_t m = min(16u * CH, re - e);
        uint32_t cc[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            cc[c] = cn[c];
            cn[c] = (e + 16u * (CH + c) + j < re) ? col[e + 16u * (CH + c) + j] : 0u;
        }
        float v0[16 * CH], v1[16];
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const size_t row = (size_t)(uint32_t)__shfl((int)cc[c], gbase + i) * f;
                v0[16 * c + i] = in[row + c0];
                if (TWO) v1[i] = in[row + c1];
            }
#pragma unroll
        for (int i = 0; i < 16 * CH; ++i)
            if ((uint32_t)i < m) {
                s0 = s0 + v0[i];
                if (TWO) s1 = s1 + v1[i & 15];
            }
    }
}

// The same sums for 32 < f <= 64 (the FEAT instantiations): lane j owns columns j + 16 t, t < NC = ceil(f / 16) = 3 or 4, one chain
// each in s[t].  The group fetches 16 column ids at a time, the next 16 already on their way, and takes them in two rounds of 8
// entries: 8 NC row loads per lane in flight (24 or 32), then their adds in stored order.  A round behind the row's end is not
// issued; within a round, slots behind the end load row 0 and lanes without a column their last one, and neither is added.
template <int NC>
__device__ __forceinline__ void any_gather_n(const uint32_t *__restrict__ col, const float *__restrict__ in, uint32_t rs, uint32_t re,
                                             uint32_t f, int j, int gbase, float (&s)[4]) {
    uint32_t ct[NC];
#pragma unroll
    for (int t = 0; t < NC; ++t) ct[t] = min((uint32_t)j + 16u * t, f - 1u);
    uint32_t cn = (rs + j < re) ? col[rs + j] : 0u;
    for (uint32_t e = rs; e < re; e += 16u) {
        const uint32_t m = min(16u, re - e);
        const uint32_t cc = cn;
        cn = (e + 16u + j < re) ? col[e + 16u + j] : 0u;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if ((uint32_t)(8 * h) >= m) break;   // (uniform over the group, whose lanes are all the shuffles below read)
            float v[8][NC];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const size_t row = (size_t)(uint32_t)__shfl((int)cc, gbase + 8 * h + i) * f;
#pragma unroll
                for (int t = 0; t < NC; ++t) v[i][t] = in[row + ct[t]];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if ((uint32_t)(8 * h + i) < m) {
#pragma unroll
                    for (int t = 0; t < NC; ++t) s[t] = s[t] + v[i][t];
                }
        }
    }
}

// f = 1: every lane fetches one neighbour's value per chunk of 16 (four chunks a round), and all lanes of the group add the
// values in the same — stored — order
__device__ __forceinline__ float any_gather1(const uint32_t *__restrict__ col, const float *__restrict__ in, uint32_t rs, uint32_t re,
                                             int j, int gbase) {
    constexpr int CH = 4;
    float s = 0.0f;
    uint32_t cn[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) cn[c] = (rs + 16u * c + j < re) ? col[rs + 16u * c + j] : 0u;
    for (uint32_t e = rs; e < re; e += 16u * CH) {
        const uint32_t m = min(16u * CH, re - e);
        float mine[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            mine[c] = in[cn[c]];
            cn[c] = (e + 16u * (CH + c) + j < re) ? col[e + 16u * (CH + c) + j] : 0u;
        }
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float t = __shfl(mine[c], gbase + i);
                if ((uint32_t)(16 * c + i) < m) s = s + t;
            }
    }
    return s;
}

// Which rows a launch takes (the arithmetic behind the sums is one source for all three):
//   kAnyAll     every row of [lo, hi) — a graph without heavy rows launches this and nothing else;
//   kAnyLight   the rows of [lo, hi) below `from` entries;
//   kAnyListed  the rows list[0 .. nlist) that lie in [lo, hi): a group's row is list[i], its sums are hsum[i * f + c]
//               (k_any_heavy_sums below wrote them), there is no gather;
//   kAnyDense   every row of [lo, hi) of a DENSE stage (gnnvc_set_generic_patterns: a prologue in front of the first graph
//               layer): vector A is row u of `in`, f floats, and the first K is f.  Nothing of the graph is read — no rowptr, col,
//               w or nw, no gather, no heavy or giant split; everything behind the row build is the same source.  All of it sits
//               behind `if constexpr`, so the other instantiations compile to what they compiled to.
// MODE is a template argument, not a kernel argument: as a wave-uniform runtime value it cost the all-rows launch seven more
// VGPRs and 2 % of a forward on an Erdős–Rényi graph, which has no heavy row (profiles/generic_stages/README.md, "Heavy rows");
// kAnyAll is the kernel as it was.
enum { kAnyAll = 0, kAnyLight = 1, kAnyListed = 2, kAnyDense = 3 };
// the descriptor of a stage's live columns (gnnvc_set_generic_live_columns; the LIVE form below): two 64-bit words on the device
struct AnyLiveDesc {
    unsigned long long mask;   // bit c: column c of the stage's input has a word other than +-0.0
    uint32_t kept, used;       // popcount(mask); 1 = this forward's launches gather from the table
};
static_assert(sizeof(AnyLiveDesc) == 16, "the engine keeps two 64-bit words per stage");
// The two pointers mean one thing to the listed-rows launch (list, hsum) and another to a LIVE all-rows or light-rows launch
// (live, live_table), which reads neither list nor sums: one slot each, named for both, so that the kernel's arguments — and with
// them every instantiation that was there — stay what they were.
struct AnyRowSel {
    uint32_t from, nlist;
    union {
        const uint32_t *list;          // kAnyListed: the listed rows
        const AnyLiveDesc *live;       // LIVE: the stage's descriptor
    };
    union {
        const float *hsum;             // kAnyListed: their sums
        const float *live_table;       // LIVE: the compact table of the live columns
    };
};

// The BIG form (gnnvc_set_generic_big_stages; BIG = true) is the same source with two more template arguments: BLOCK = 256, 512 or
// 1024 threads (16 / 32 / 64 rows a pass: above 80 KiB of LDS one workgroup fits a CU, and its waves are all the CU has to cover
// the LDS reads of the dense layers with), and hidden layers of up to 128 outputs, taken 64 outputs at a time — the chains of
// different outputs are independent, so a layer's second half is the first half's code on the next 64 transposed rows.  The
// defaults are the kernel as it was.
//
// The FEAT form (gnnvc_set_generic_feature_width; FEAT = true, on top of BIG = true) is the same source again for stages whose f
// or last width lies in 33 .. 64: a lane owns up to four sum columns (any_gather_n above; the listed rows read four sums from
// hsum) and up to four outputs of the last layer.  Everything it adds sits behind `if constexpr (FEAT)`, so the other twelve
// instantiations compile to what they compiled to.  A FEAT stage within the default LDS and hidden-width bounds launches the
// 256-thread form; one outside them needs big stages too and follows their rule for 1024 / 512 / 256 threads.
//
// The OPEN form (gnnvc_set_generic_patterns) is the same source once more for a stage that ends in its bare linear layer — and for
// every dense stage, whose instantiations are new anyway: any_last<T, true> knows the third ending.
//
// The LIVE form (gnnvc_set_generic_live_columns; kAnyAll and kAnyLight only, OPEN = false) is the same source for a stage whose
// input may have dead columns (+-0.0 in every row): R.live is the stage's AnyLiveDesc {mask, kept, used} and R.live_table the compact
// table of the live columns (n rows of `kept` floats, k_any_live_pack below) — they share their slots with the listed rows' list
// and sums, which an all-rows or light-rows launch never reads, and the kernel's arguments stay what they were.  The descriptor is wave-uniform.  used == 0: today's gather
// on `in` with f.  used != 0: the SAME gather functions on the table with `kept` in the place of f (none at all for kept == 0,
// whose f - 1u clamps would underflow), columns [0, f) of vector A zeroed, and lane j's sums stored at the positions of the
// (j + 16 t)-th set bits of the mask, computed once per kernel.  A dead column's chain is +0.0f for every row and a live column's
// chain is the one it was ("Live columns").  Everything it adds sits behind `if constexpr (LIVE)`.
template <int MODE, int BLOCK = kAnyBlock, bool BIG = false, bool FEAT = false, bool OPEN = MODE == 3 /* kAnyDense */, bool LIVE = false>
__global__ __launch_bounds__(BLOCK) void k_stage_any(AnyGraph g, float ws, const float *__restrict__ P, const float *__restrict__ in,
                                                        float *__restrict__ out, float *__restrict__ logits, uint32_t lo, uint32_t hi,
                                                        AnyShape S, int sig, AnyRowSel R) {
    extern __shared__ float4 any_lds4[];
    float *lds = reinterpret_cast<float *>(any_lds4);
    constexpr int ROWS = BLOCK / 16;
    constexpr bool dense = MODE == kAnyDense;
    const int f = S.f, d = S.d, k1 = dense ? f : 2 * f + 3;
    const StageAnyLayout L = stage_any_layout(S, ROWS, dense ? f : 0);
    float *bs = lds + L.bias;
    // parameters, transposed: wt[o * pitch + k] = W[k * N + o]   (W1 b1 W2 b2 ... are contiguous from P)
    {
        const float *W = P;
        float *wt = lds, *bl = bs;
        int K = k1;
        for (int l = 0; l < d; ++l) {
            const int N = S.n[l], p = any_pitch(K);
            for (int i = threadIdx.x; i < K * N; i += BLOCK) wt[(i % N) * p + i / N] = W[i];
            for (int i = threadIdx.x; i < N; i += BLOCK) bl[i] = W[K * N + i];
            W += K * N + N;
            wt += N * p;
            bl += N;
            K = N;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, j = lane & 15, grp = threadIdx.x >> 4, gbase = lane & 48;
    float *xs = lds + L.grp + grp * L.gs;   // the group's vector A; B follows at L.hb
    constexpr bool listed = MODE == kAnyListed;
    static_assert(!LIVE || MODE == kAnyAll || MODE == kAnyLight, "the table serves the all-rows and light-rows launches only");
    [[maybe_unused]] uint32_t live_used = 0u, live_kept = 0u;
    [[maybe_unused]] int live_pos[FEAT ? 4 : 2];   // where lane j's sums go: the (j + 16 t)-th live column, -1 = the lane has none
    if constexpr (LIVE) {
        const AnyLiveDesc *ld = R.live;
        live_used = ld->used;
        live_kept = ld->kept;
        const unsigned long long mask = ld->mask;
#pragma unroll
        for (int t = 0; t < (FEAT ? 4 : 2); ++t) {
            unsigned long long m = mask;
            for (int i = 0; i < j + 16 * t && m; ++i) m &= m - 1ull;   // (drop the lower set bits)
            live_pos[t] = (live_used && m && (uint32_t)(j + 16 * t) < live_kept) ? __ffsll((long long)m) - 1 : -1;
        }
    }
    // (the walk is over rows, or over positions of the list)
    const uint64_t walk_lo = listed ? 0u : (uint64_t)lo, walk_hi = listed ? (uint64_t)R.nlist : (uint64_t)hi;
    for (uint64_t base = walk_lo + (uint64_t)blockIdx.x * ROWS; base < walk_hi; base += (uint64_t)gridDim.x * ROWS) {
        const uint64_t u64 = base + (uint64_t)grp;
        if (u64 >= walk_hi) continue;   // (no workgroup barrier below: a group without a row just waits for the next round)
        uint32_t u = (uint32_t)u64;
        if (listed) {
            u = R.list[u64];
            if (u < lo || u >= hi) continue;   // listed, but not in this call's range
        }
        if constexpr (dense) {
            // ---- the row itself: vector A = row u of `in`
            for (int c = j; c < f; c += 16) xs[c] = in[(size_t)u * (uint32_t)f + (uint32_t)c];
        } else {
            // ---- graph layer
            const uint32_t rs = g.rowptr[u], re = g.rowptr[u + 1];
            if (MODE == kAnyLight && re - rs >= R.from) continue;   // a heavy row: the listed-rows launch has it
            float s0 = 0.0f, s1 = 0.0f;
            [[maybe_unused]] float s2 = 0.0f, s3 = 0.0f;   // (FEAT: columns j + 32, j + 48)
            if constexpr (LIVE) {
                // the table's rows are `kept` floats (used), or the input's own f (not used): one dispatch over (gin, gf)
                const float *__restrict__ gin = live_used ? R.live_table : in;
                const uint32_t gf = live_used ? live_kept : (uint32_t)f;
                if (gf == 0u) {
                    // no live column: nothing to gather, every sum is the empty chain's +0.0f
                } else if (FEAT && gf > 32u) {
                    if constexpr (FEAT) {
                        float sn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                        if (gf <= 48u) any_gather_n<3>(g.col, gin, rs, re, gf, j, gbase, sn);
                        else any_gather_n<4>(g.col, gin, rs, re, gf, j, gbase, sn);
                        s0 = sn[0];
                        s1 = sn[1];
                        s2 = sn[2];
                        s3 = sn[3];
                    }
                } else if (gf == 1u) {
                    s0 = any_gather1(g.col, gin, rs, re, j, gbase);
                } else if (gf <= 16u) {
                    any_gather<false>(g.col, gin, rs, re, gf, j, gbase, s0, s1);
                } else {
                    any_gather<true>(g.col, gin, rs, re, gf, j, gbase, s0, s1);
                }
            } else if (listed) {
                const float *hs = R.hsum + (size_t)u64 * (uint32_t)f;
                s0 = hs[min(j, f - 1)];
                s1 = hs[min(j + 16, f - 1)];
                if constexpr (FEAT) {
                    s2 = hs[min(j + 32, f - 1)];
                    s3 = hs[min(j + 48, f - 1)];
                }
            } else if (FEAT && f > 32) {
                if constexpr (FEAT) {
                    float sn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (f <= 48) any_gather_n<3>(g.col, in, rs, re, (uint32_t)f, j, gbase, sn);
                    else any_gather_n<4>(g.col, in, rs, re, (uint32_t)f, j, gbase, sn);
                    s0 = sn[0];
                    s1 = sn[1];
                    s2 = sn[2];
                    s3 = sn[3];
                }
            } else if (f == 1) {
                s0 = any_gather1(g.col, in, rs, re, j, gbase);
            } else if (f <= 16) {
                any_gather<false>(g.col, in, rs, re, (uint32_t)f, j, gbase, s0, s1);
            } else {
                any_gather<true>(g.col, in, rs, re, (uint32_t)f, j, gbase, s0, s1);
            }
            const float deg = (float)(re - rs), wv = (float)g.w[u] / ws, nwv = (float)g.nw[u] / ws;
            for (int c = j; c < k1; c += 16) {
                float v = 0.0f;
                if (c < f) v = (LIVE && live_used) ? 0.0f : c < 16 ? s0 : (!FEAT || c < 32) ? s1 : (c < 48 ? s2 : s3);
                else if (c < 2 * f) v = in[(size_t)u * (uint32_t)f + (uint32_t)(c - f)];
                if (c == f + 1) v = deg;
                if (c == f + 2) v = wv;
                if (c == f + 3) v = nwv;
                xs[c] = v;
            }
            if constexpr (LIVE) {
                if (live_used) {   // (wave-uniform) the sums over the zeros, at their columns' places — all below f, so never on degree, W or NW
                    wave_lds_sync();
                    if (live_pos[0] >= 0) xs[live_pos[0]] = s0;
                    if (live_pos[1] >= 0) xs[live_pos[1]] = s1;
                    if constexpr (FEAT) {
                        if (live_pos[2] >= 0) xs[live_pos[2]] = s2;
                        if (live_pos[3] >= 0) xs[live_pos[3]] = s3;
                    }
                }
            }
        }
        wave_lds_sync();
        // ---- the hidden layers, linear + ReLU each (A -> B -> A ...), then the last: linear + ReLU | sigmoid (-> memory)
        const float *src = xs;
        float *dst = xs + L.hb;
        const float *wt = lds, *bl = bs;
        int K = k1;
        for (int l = 0; l + 1 < d; ++l) {
            const int N = S.n[l], p = any_pitch(K);
            if (BIG) {   // (N <= 128: one or two passes; outputs ob + j + 16 t, the clamp and the k tail as in the one pass)
                for (int ob = 0; ob < N; ob += 64) any_hidden_n(src, K, wt + ob * p, p, bl + ob, N - ob, j, dst + ob);
            } else {
                any_hidden_n(src, K, wt, p, bl, N, j, dst);
            }
            wave_lds_sync();
            wt += N * p;
            bl += N;
            K = N;
            float *t = const_cast<float *>(src);
            src = dst;
            dst = t;
        }
        const int n_out = S.n[d - 1];
        float *out_row = out + (size_t)u * (uint32_t)n_out;
        float *logit_row = logits ? logits + (size_t)u * (uint32_t)n_out : nullptr;   // (null unless this is the sigmoid stage)
        if (n_out <= 16) any_last<1, OPEN>(src, K, wt, any_pitch(K), bl, n_out, j, sig, out_row, logit_row);
        else if (!FEAT || n_out <= 32) any_last<2, OPEN>(src, K, wt, any_pitch(K), bl, n_out, j, sig, out_row, logit_row);
        else if (n_out <= 48) any_last<3, OPEN>(src, K, wt, any_pitch(K), bl, n_out, j, sig, out_row, logit_row);
        else any_last<4, OPEN>(src, K, wt, any_pitch(K), bl, n_out, j, sig, out_row, logit_row);
        wave_lds_sync();   // (the group's LDS is rewritten by its next row)
    }
}

// ---- live columns (gnnvc_set_generic_live_columns): which columns of a stage's input (n x f floats, f <= 64) hold anything but
// +-0.0, and the compact table of those columns.  Both kernels run on the forward's stream ahead of the stage's launches; the
// descriptor was zeroed by the forward's one hipMemsetAsync.
//
// k_any_live_mask: one pass over the n f words.  A thread ORs 1 << column for every word with a bit set below the sign; the
// masks are reduced over the wave (shuffles), over the workgroup (LDS) and leave with ONE 64-bit atomicOr per workgroup.  The
// body takes 16-byte loads from the first 16-byte boundary on (stage 0's input is the caller's, at any 4-byte alignment); the
// words in front of it and behind the last whole 16 bytes are taken one by one by the grid's first threads.
constexpr int kLiveBlock = 256;
constexpr uint32_t kLivePackRows = 256;   // k_any_live_pack: rows per workgroup and pass

__device__ __forceinline__ uint32_t live_wrap(uint32_t c, uint32_t f) {   // c < f + 4, f >= 2 -> c mod f
    c -= c >= f ? f : 0u;
    c -= c >= f ? f : 0u;
    return c;
}

__global__ __launch_bounds__(kLiveBlock) void k_any_live_mask(const float *__restrict__ in, uint64_t total, uint32_t f,
                                                             AnyLiveDesc *__restrict__ desc) {
    __shared__ unsigned long long wave_mask[kLiveBlock / 64];
    const uint32_t *w = reinterpret_cast<const uint32_t *>(in);
    const uint64_t head = std::min<uint64_t>(total, (uint64_t)((4u - (uint32_t)((reinterpret_cast<uintptr_t>(in) >> 2) & 3u)) & 3u));
    const uint64_t nvec = (total - head) / 4u, tail0 = head + 4u * nvec;
    const uint32_t tid = blockIdx.x * kLiveBlock + threadIdx.x, nthr = gridDim.x * kLiveBlock;   // (the grid is at most 2048 workgroups)
    unsigned long long m = 0ull;
    if (tid < head && (w[tid] & 0x7fffffffu)) m |= 1ull << (tid % f);
    if (tid < total - tail0 && (w[tail0 + tid] & 0x7fffffffu)) m |= 1ull << (uint32_t)((tail0 + tid) % f);
    const uint4 *v = reinterpret_cast<const uint4 *>(w + head);
    // The threads that take 16-byte pieces step by a multiple of f words (the grid has at least 256 >= f threads): a thread's four
    // columns never change, so the loop is a load and four ORs, four loads in flight, and the columns are looked at once, behind it.
    const uint32_t stride = nthr / f * f;
    if (tid < stride) {
        uint32_t a0 = 0u, a1 = 0u, a2 = 0u, a3 = 0u;
        uint64_t i = tid;
        for (; i + 3ull * stride < nvec; i += 4ull * stride) {
            const uint4 q0 = v[i], q1 = v[i + stride], q2 = v[i + 2ull * stride], q3 = v[i + 3ull * stride];
            a0 |= q0.x | q1.x | q2.x | q3.x;
            a1 |= q0.y | q1.y | q2.y | q3.y;
            a2 |= q0.z | q1.z | q2.z | q3.z;
            a3 |= q0.w | q1.w | q2.w | q3.w;
        }
        for (; i < nvec; i += stride) {
            const uint4 q = v[i];
            a0 |= q.x;
            a1 |= q.y;
            a2 |= q.z;
            a3 |= q.w;
        }
        const uint32_t c = ((uint32_t)head + 4u * tid) % f;     // the column of the first word of this thread's 16 bytes
        if (a0 & 0x7fffffffu) m |= 1ull << c;
        if (a1 & 0x7fffffffu) m |= 1ull << live_wrap(c + 1u, f);
        if (a2 & 0x7fffffffu) m |= 1ull << live_wrap(c + 2u, f);
        if (a3 & 0x7fffffffu) m |= 1ull << live_wrap(c + 3u, f);
    }
    uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        lo |= (uint32_t)__shfl_xor((int)lo, o);
        hi |= (uint32_t)__shfl_xor((int)hi, o);
    }
    if ((threadIdx.x & 63u) == 0u) wave_mask[threadIdx.x >> 6] = ((unsigned long long)hi << 32) | lo;
    __syncthreads();
    if (threadIdx.x == 0u) {
        unsigned long long all = 0ull;
#pragma unroll
        for (int i = 0; i < kLiveBlock / 64; ++i) all |= wave_mask[i];
        if (all) atomicOr(&desc->mask, all);
    }
}

// k_any_live_pack: every workgroup reads the mask and derives kept = popcount and used = (kept * 100 <= max_percent * f);
// workgroup 0 writes them beside the mask.  Not used: nothing else happens.  Used: table[u * kept + r] = in[u * f + column_r],
// column_r the r-th set bit (a list in LDS), a workgroup per kLivePackRows rows and pass — the index within the pass stays
// below 2^14, everything that scales with n is 64-bit.  The table's row pitch is exactly `kept` floats.
__global__ __launch_bounds__(kLiveBlock) void k_any_live_pack(const float *__restrict__ in, float *__restrict__ table, uint32_t n, uint32_t f,
                                                             uint32_t max_percent, AnyLiveDesc *__restrict__ desc) {
    __shared__ uint32_t cols[64];
    const unsigned long long mask = desc->mask;
    const uint32_t kept = (uint32_t)__popcll(mask), used = kept * 100u <= max_percent * f ? 1u : 0u;
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        desc->kept = kept;
        desc->used = used;
    }
    if (!used || kept == 0u) return;   // (block-uniform)
    const uint32_t inv = (uint32_t)(((1ull << 32) + kept - 1u) / kept);   // ceil(2^32 / kept), kept >= 2 (kept == 1: not used)
    if (threadIdx.x < 64u && ((mask >> threadIdx.x) & 1ull)) cols[__popcll(mask & ((1ull << threadIdx.x) - 1ull))] = threadIdx.x;
    __syncthreads();
    for (uint64_t base = (uint64_t)blockIdx.x * kLivePackRows; base < (uint64_t)n; base += (uint64_t)gridDim.x * kLivePackRows) {
        const uint32_t rows = (uint32_t)std::min<uint64_t>(kLivePackRows, (uint64_t)n - base), cells = rows * kept;
        const float *src = in + base * f;
        float *dst = table + base * kept;
        for (uint32_t t = threadIdx.x; t < cells; t += kLiveBlock) {
            const uint32_t u = kept > 1u ? __umulhi(t, inv) : t, r = t - u * kept;   // t / kept: exact for t < 2^14, kept <= 64
            dst[t] = src[(size_t)u * f + cols[r]];
        }
    }
}

// ---- heavy rows: the neighbour sums of ONE listed row by a whole workgroup (the structure of k_long_f1 / k_long_f16 in
// gnnvc_kernels.hip, for any 1 <= f <= 64; nothing is shared with them or with k_audit_any).  Sums only: the row build, the dense
// layers and the stores stay k_stage_any's (kAnyListed).
//
// The 256 threads form groups of G = 2^gs >= f lanes, a group per neighbour: lane c of a group fetches column c of its
// neighbour's row (lanes c >= f have no column: they fetch column f - 1 and write nothing).  A pass covers 256 / G neighbours, a
// chunk is R passes — R values per thread in registers — so a chunk is CH = 256 R / G neighbours: 1024 for f <= 4 (R = 4, 8, 16 for
// G = 1, 2, 4), 512 for f <= 8, 256 for f <= 16, 128 for f <= 32, 64 above (R = 16; G = 64 is a whole wave, four neighbours a
// pass).  The slab is column-major, f runs of CH + 4 floats (the pad of
// four keeps every column 16-byte aligned and puts the adder lanes' 16-byte reads on different banks); two slabs alternate:
// heavy_lds_bytes(f), at most 34 816 bytes (f = 64; 33 792 at f = 32) — four workgroups a CU by LDS, and the 64 KiB limit is not
// raised.
// While lane c < f of the first wave adds column c of chunk r in stored order (sixteen 16-byte LDS reads ahead of their 64
// adds), the values of chunk r + 1 and the column ids of chunk r + 2 are in flight.  Every fetch is unconditional: entries past
// the row's end clamp to its last entry — a real neighbour, never a pad row of `in` — and what they fetch is written to the slab
// but never added (the adders stop at the row's length).
typedef float any_f32x4 __attribute__((ext_vector_type(4)));
constexpr int kHeavyBlock = 256, kHeavyPad = 4;
__host__ __device__ inline int heavy_shift(int f) {   // G = 1 << heavy_shift(f): the smallest power of two >= f
    int s = 0;
    while ((1 << s) < f) ++s;
    return s;
}
__host__ __device__ inline int heavy_passes(int gs) { return gs >= 2 ? 16 : (gs == 1 ? 8 : 4); }
__host__ __device__ inline size_t heavy_lds_bytes(int f) {
    const int gs = heavy_shift(f), ch = (kHeavyBlock >> gs) * heavy_passes(gs);
    return (size_t)2 * (size_t)f * (size_t)(ch + kHeavyPad) * sizeof(float);
}

template <int R>
__global__ __launch_bounds__(kHeavyBlock) void k_any_heavy_sums(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ col,
                                                               const float *__restrict__ in, const uint32_t *__restrict__ list,
                                                               float *__restrict__ hsum, uint32_t f, uint32_t gs, uint32_t lo,
                                                               uint32_t hi, uint32_t below) {
    extern __shared__ float4 heavy_lds4[];
    float *slab = reinterpret_cast<float *>(heavy_lds4);
    const uint32_t u = list[blockIdx.x];
    if (u < lo || u >= hi) return;   // block-uniform: not in this call's range (k_stage_any skips the same rows)
    const uint32_t tid = threadIdx.x;
    const uint32_t rs = rowptr[u], deg = rowptr[u + 1] - rs;
    if (deg >= below) return;   // block-uniform: a giant row — k_any_giant_gather and the exact scan have its sums (0xFFFFFFFF: none)
    if (deg == 0) {   // (never listed; kept so that nothing below indexes an empty row)
        if (tid < f) hsum[(size_t)blockIdx.x * f + tid] = 0.0f;
        return;
    }
    const uint32_t per = (uint32_t)kHeavyBlock >> gs, CH = per * R, stride = CH + kHeavyPad;
    const uint32_t k0 = tid >> gs, c = tid & ((1u << gs) - 1u);
    const bool has = c < f;
    const uint32_t cc = has ? c : f - 1u;
    const uint32_t nrounds = (deg + CH - 1u) / CH;
    uint32_t idx[R];
    float v[R];
    // (offsets within the row: a row's degree plus three chunks stays far below 2^32 — nnz < 2^32 - GNNVC_COL_PAD)
#define GNNVC_HEAVY_IDX(rd_)                                                  \
    _Pragma("unroll") for (int j = 0; j < R; ++j) {                            \
        const uint32_t o_ = (rd_) * CH + k0 + per * (uint32_t)j;              \
        idx[j] = col[rs + (o_ < deg ? o_ : deg - 1u)];                        \
    }
#define GNNVC_HEAVY_VAL()                                                     \
    _Pragma("unroll") for (int j = 0; j < R; ++j) v[j] = in[(size_t)idx[j] * f + cc];
    float acc = 0.0f;   // threads c < f of the first wave: column c
    GNNVC_HEAVY_IDX(0u)
    GNNVC_HEAVY_VAL()
    GNNVC_HEAVY_IDX(1u)
    for (uint32_t rd = 0; rd < nrounds; ++rd) {
        float *buf = slab + (size_t)(rd & 1u) * f * stride;
        if (has) {
#pragma unroll
            for (int j = 0; j < R; ++j) buf[c * stride + k0 + per * (uint32_t)j] = v[j];
        }
        __syncthreads();
        GNNVC_HEAVY_VAL()            // chunk rd + 1 (unconditional, clamped)
        GNNVC_HEAVY_IDX(rd + 2u)
        if (tid < f) {
            const uint32_t left = deg - rd * CH, cnt = left < CH ? left : CH;
            const float *colv = buf + tid * stride;
            for (uint32_t k = 0; k < cnt; k += 64u) {   // (CH is a multiple of 64: the sixteen reads stay inside the column)
                any_f32x4 t[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) t[j] = *reinterpret_cast<const any_f32x4 *>(&colv[k + 4 * j]);
                if (k + 64u <= cnt) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        acc = acc + t[j][0];
                        acc = acc + t[j][1];
                        acc = acc + t[j][2];
                        acc = acc + t[j][3];
                    }
                } else {   // the row's last entries: what lies behind them in the slab is not added
                    const uint32_t m = cnt - k;
#pragma unroll
                    for (int j = 0; j < 16; ++j)
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if ((uint32_t)(4 * j + i) < m) acc = acc + t[j][i];
                }
            }
        }
        // this slab is rewritten in round rd + 2, behind the barrier of round rd + 1, which the adders reach after these reads
    }
#undef GNNVC_HEAVY_IDX
#undef GNNVC_HEAVY_VAL
    if (tid < f) hsum[(size_t)blockIdx.x * f + tid] = acc;
}

// ---- giant rows: listed rows of at least the giant threshold (gnnvc_set_generic_giant_rows) leave k_any_heavy_sums' single chain
// per column for the trained path's exact parallel scan (exact_sum.h; k_giant_segsum / k_giant_segmap / k_giant_sum of
// gnnvc_kernels.hip, which take the number of streams per row at run time).  What is new here is the gather for any width:
// k_any_giant_gather writes the row's neighbour values column-major into the slab — stream c of giant row i at
// slab + off[i] + c * lpad, lpad = the degree rounded up to the scan's window — and k_any_giant_place copies the aggregates to
// where k_stage_any<kAnyListed> reads a listed row's sums.
//
// One 256-thread workgroup per 256 consecutive entries of one row (lpad / 256 workgroups a row: every float of a stream up to
// lpad is written in every call — the segment sums rely on zero padding).  Groups of G = 2^GS >= f lanes, a group per entry, G
// passes: lane c < f of a group fetches float c of its entry's neighbour row (4-byte loads: f need not be a multiple of 4), all G
// fetches of a thread in flight at once.  Entries past the row's end clamp to its last entry for the fetch — a real neighbour,
// never a pad row — and are stored as +0.0f.  The values cross an LDS tile [f][256 + 4] (at most 33 280 bytes, f = 32) and leave
// with 16-byte stores, 1 KiB per stream and workgroup.  A launch takes the columns c0 .. c0 + min(f - c0, G) of the rows: all of
// them (c0 = 0) for f <= 32, and a row wider than that in two launches of at most 32 columns each, so that GS stays at most 5
// (32 fetches a thread) and the tile within 33 280 bytes.
constexpr int kAnyGiantBlk = 256, kAnyGiantPitch = kAnyGiantBlk + 4;

// meta[i] = {row, first entry, degree, first gather block}, meta[n_giant].w = the number of gather blocks
__device__ __forceinline__ uint32_t any_giant_of_block(const uint4 *__restrict__ meta, uint32_t n_giant, uint32_t b) {
    uint32_t lo = 0, hi = n_giant;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (meta[mid].w <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// the listed rows of at least `thresh` entries, with their position in the list: {row, first entry, degree, position}
__global__ void k_find_any_giant(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ list, uint32_t n_list, uint32_t thresh,
                                 uint4 *__restrict__ meta, uint32_t *__restrict__ count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_list) return;
    const uint32_t u = list[i], rs = rowptr[u], deg = rowptr[u + 1] - rs;
    if (deg >= thresh) meta[atomicAdd(count, 1u)] = make_uint4(u, rs, deg, i);
}

template <int GS>
__global__ __launch_bounds__(kAnyGiantBlk) void k_any_giant_gather(const uint32_t *__restrict__ col, const float *__restrict__ in,
                                                                  float *__restrict__ slab, const uint4 *__restrict__ meta,
                                                                  const unsigned long long *__restrict__ off, uint32_t n_giant, uint32_t f,
                                                                  uint32_t win, uint32_t lo, uint32_t hi, uint32_t c0) {
    extern __shared__ float4 giant_lds4[];
    float *tile = reinterpret_cast<float *>(giant_lds4);
    constexpr uint32_t G = 1u << GS, per = (uint32_t)kAnyGiantBlk >> GS;
    const uint32_t i = any_giant_of_block(meta, n_giant, blockIdx.x);
    const uint4 mt = meta[i];
    if (mt.x < lo || mt.x >= hi) return;   // block-uniform: not in this call's range
    const uint32_t deg = mt.z;
    if (deg == 0) return;                  // (never listed; k_giant_sum writes the sum of no addends)
    const uint32_t j0 = (blockIdx.x - mt.w) * (uint32_t)kAnyGiantBlk;
    const uint32_t lpad = (deg + win - 1u) / win * win;
    if (j0 >= lpad) return;                // (block-uniform; the host lays out exactly lpad / 256 blocks a row)
    const uint32_t tid = threadIdx.x, k0 = tid >> GS, c = tid & (G - 1u);
    const uint32_t fw = min(f - c0, G);    // this launch's columns: c0 .. c0 + fw
    const bool has = c < fw;
    const uint32_t cc = c0 + (has ? c : fw - 1u);
    uint32_t idx[G];
    float v[G];
#pragma unroll
    for (uint32_t p = 0; p < G; ++p) {
        const uint32_t j = j0 + k0 + per * p;
        idx[p] = col[mt.y + (j < deg ? j : deg - 1u)];
    }
#pragma unroll
    for (uint32_t p = 0; p < G; ++p) v[p] = in[(size_t)idx[p] * f + cc];
    if (has) {
#pragma unroll
        for (uint32_t p = 0; p < G; ++p) {
            const uint32_t k = k0 + per * p;
            tile[c * (uint32_t)kAnyGiantPitch + k] = j0 + k < deg ? v[p] : 0.0f;
        }
    }
    __syncthreads();
    float *dst = slab + off[i] + (size_t)c0 * lpad + j0;   // (16-byte aligned: off[i], lpad and j0 are multiples of 256 floats)
    for (uint32_t q = tid; q < fw * (uint32_t)(kAnyGiantBlk / 4); q += (uint32_t)kAnyGiantBlk) {
        const uint32_t cq = q >> 6, k4 = (q & 63u) * 4u;
        *reinterpret_cast<any_f32x4 *>(dst + (size_t)cq * lpad + k4) = *reinterpret_cast<const any_f32x4 *>(&tile[cq * (uint32_t)kAnyGiantPitch + k4]);
    }
}

// aggregate (i, c) of the giant rows -> hsum[pos[i] * f + c], the listed row's sums as k_stage_any<kAnyListed> reads them
__global__ __launch_bounds__(256) void k_any_giant_place(const uint4 *__restrict__ meta, const uint32_t *__restrict__ pos,
                                                         const float *__restrict__ agg, float *__restrict__ hsum, uint32_t n_giant, uint32_t f,
                                                         uint32_t lo, uint32_t hi) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n_giant * f) return;
    const uint32_t i = (uint32_t)(t / f), c = (uint32_t)(t % f), u = meta[i].x;
    if (u < lo || u >= hi) return;         // (its aggregates were not computed in this call)
    hsum[(size_t)pos[i] * f + c] = agg[t];
}

AnyShape any_shape(const StagePlan &sp) {
    AnyShape S{};
    S.f = sp.f;
    S.d = sp.nd;
    for (int l = 0; l < kMaxDenseLayers; ++l) S.n[l] = (l < sp.nd) ? sp.wn[l] : 0;
    return S;
}

}  // namespace

// GNNVC_BIG_THREADS (256 | 512 | 1024, read once per process) forces the big form's workgroup size where that size's layout fits
// the limit, so that one library can be measured three ways (profiles/generic_stages/README.md, "Big stages"); anything else, or
// a size that does not fit, leaves the rule in force.
static int forced_big_threads() {
    static const int v = [] {
        const char *s = getenv("GNNVC_BIG_THREADS");
        const int t = s && *s ? atoi(s) : 0;
        return t == 256 || t == 512 || t == 1024 ? t : 0;
    }();
    return v;
}

// THE function that decides what is admitted and where it goes (plan_model, the launchers here, the engine's read-outs and the
// audit's launcher all ask it, through stage_any_fits where a yes / no is enough).
AnyRoute stage_any_route(const StagePlan &sp) {
    AnyRoute r;
    // the feature width in force (gnnvc_set_generic_feature_width): what f and the last width may be
    const int fw = sp.feat_width > (uint32_t)kAnyMaxF && sp.feat_width <= (uint32_t)kAnyFeatMax ? (int)sp.feat_width : kAnyMaxF;
    static_assert(kAnyMaxF == kAnyMaxLast, "one allowance covers both");
    if (sp.f < 1 || sp.f > fw || sp.nd < 1 || sp.nd > kMaxDenseLayers) return r;
    bool small = true;   // the default bounds: the kernel as it always was
    for (int l = 0; l < sp.nd; ++l) {
        const bool last = l + 1 == sp.nd;
        if (sp.wn[l] < 1 || sp.wn[l] > (last ? fw : kAnyBigHidden)) return r;
        if (!last && sp.wn[l] > kAnySmallHidden) small = false;
    }
    // the patterns in force (gnnvc_set_generic_patterns): a dense stage needs kPatternPrologue; a stage that is not the model's last
    // ends in a ReLU, the model's last in the sigmoid or — with kPatternOpenEnd — in a ReLU or in its bare linear layer
    if (sp.dense && !(sp.patterns & kPatternPrologue)) return r;
    if (sp.end != (sp.model_last ? kEndSigmoid : kEndRelu) && !(sp.model_last && (sp.patterns & kPatternOpenEnd))) return r;
    r.feat = sp.f > kAnyMaxF || sp.wn[sp.nd - 1] > kAnyMaxLast;   // (uses the allowance: a FEAT instantiation)
    const AnyShape S = any_shape(sp);
    const int first_k = sp.dense ? sp.f : 0;   // (a dense stage's first K is f; 0: a graph stage's 2 f + 3)
    r.lds256 = (size_t)stage_any_layout(S, kAnyRows, first_k).total * sizeof(float);
    if (small && r.lds256 <= kAnyLdsBytes) {
        r.ok = true;
        r.lds = r.lds256;
        return r;
    }
    // the opt-in (gnnvc_set_generic_big_stages): admitted by the layout at 256 threads
    if (sp.big_lds < kAnyLdsBytes || sp.big_lds > kAnyBigLdsBytes || r.lds256 > sp.big_lds) return r;
    r.ok = r.big = true;
    r.lds = r.lds256;
    // the workgroup size: the largest whose layout fits the limit (the weights are in LDS once per workgroup, and above 80 KiB a
    // CU holds one workgroup: its waves are all there is to cover the dense layers' LDS reads; measured, 1024 against 512 against
    // 256 threads: profiles/generic_stages/README.md, "Big stages")
    const auto bytes_at = [&](int t) { return (size_t)stage_any_layout(S, t / 16, first_k).total * sizeof(float); };
    const int forced = forced_big_threads();
    const int cap = forced && bytes_at(forced) <= sp.big_lds ? forced : 1024;   // (a forced size that does not fit: the rule)
    for (int t : {1024, 512}) {
        if (t > cap || bytes_at(t) > sp.big_lds) continue;
        r.threads = t;
        r.lds = bytes_at(t);
        break;
    }
    return r;
}

bool stage_any_fits(const StagePlan &sp) { return stage_any_route(sp).ok; }

hipError_t launch_stage_any(const StageCall &c, AnyRows rows, const AnyHeavyRows &hr) {
    if (c.row_hi <= c.row_lo) return hipSuccess;
    const StagePlan &sp = *c.sp;
    const GraphDev &g = *c.g;
    const AnyRoute route = stage_any_route(sp);
    if (!route.ok || c.row_hi > g.hi() || c.row_lo < g.lo()) return hipErrorInvalidValue;
    if (sp.dense && rows != AnyRows::kAll) return hipErrorInvalidValue;   // (a dense stage has no heavy or giant split)
    // the LIVE instantiations (gnnvc_set_generic_live_columns): an all-rows or light-rows launch of a graph stage with f >= 2 that does
    // not end in its bare linear layer, when the call carries the stage's descriptor and table — in the two fields of the row
    // selection that such a launch does not otherwise read
    const bool live = c.live_desc && c.live_table && rows != AnyRows::kListed && !sp.dense && sp.f >= 2 && sp.end != kEndNone;
    AnyRowSel sel{0u, 0u, {nullptr}, {nullptr}};
    if (rows == AnyRows::kLight) sel.from = hr.from;
    if (live) {
        sel.live = reinterpret_cast<const AnyLiveDesc *>(c.live_desc);   // (StageCall carries it untyped: the struct is this file's)
        sel.live_table = c.live_table;
    }
    if (rows == AnyRows::kListed) {
        if (hr.n == 0) return hipSuccess;
        if (!hr.list || !hr.hsum) return hipErrorInvalidValue;
        sel = AnyRowSel{hr.from, hr.n, {hr.list}, {hr.hsum}};
    }
    const AnyGraph plain = sp.dense ? AnyGraph{nullptr, nullptr, nullptr, nullptr} : AnyGraph{g.rowptr, g.col, g.w, g.nw};   // (a dense stage reads none of it)
    const AnyShape S = any_shape(sp);
    const size_t lds = route.lds;   // <= 64 KiB, or (a big stage) <= the limit gnnvc_set_generic_big_stages was given
    // a persistent grid: as many workgroups as the LDS lets a CU hold (at most 8, and 2048 threads), on 256 CUs
    const unsigned per_cu = (unsigned)std::min<size_t>(std::min<size_t>(8, 2048u / (unsigned)route.threads),
                                                       std::max<size_t>(1, (160u * 1024u) / (lds + 1024u)));
    const size_t walk = rows == AnyRows::kListed ? (size_t)hr.n : (size_t)(c.row_hi - c.row_lo);   // rows, or list positions
    const unsigned rows_wg = (unsigned)route.threads / 16u;
    const unsigned need = (unsigned)((walk + rows_wg - 1) / rows_wg);
    const dim3 grid(std::min(need, 256u * per_cu)), block((unsigned)route.threads);
#define GNNVC_ANY_ARGS                                                                                                        \
    grid, block, lds, c.stream, plain, c.ws, c.params + sp.param_offset, c.in, c.out, sp.sigmoid_last ? c.logits : nullptr, \
        c.row_lo, c.row_hi, S, sp.end, sel
#define GNNVC_ANY_FORMS(MODE_, OPEN_, LIVE_)                                                \
    do {                                                                                    \
        if (route.feat) {   /* (also within the default LDS bound: the 256-thread form) */  \
            if (route.threads == 1024) hipLaunchKernelGGL((k_stage_any<MODE_, 1024, true, true, OPEN_, LIVE_>), GNNVC_ANY_ARGS);     \
            else if (route.threads == 512) hipLaunchKernelGGL((k_stage_any<MODE_, 512, true, true, OPEN_, LIVE_>), GNNVC_ANY_ARGS);  \
            else hipLaunchKernelGGL((k_stage_any<MODE_, 256, true, true, OPEN_, LIVE_>), GNNVC_ANY_ARGS); \
        }                                                                                   \
        else if (!route.big) hipLaunchKernelGGL((k_stage_any<MODE_, kAnyBlock, false, false, OPEN_, LIVE_>), GNNVC_ANY_ARGS);      \
        else if (route.threads == 1024) hipLaunchKernelGGL((k_stage_any<MODE_, 1024, true, false, OPEN_, LIVE_>), GNNVC_ANY_ARGS); \
        else if (route.threads == 512) hipLaunchKernelGGL((k_stage_any<MODE_, 512, true, false, OPEN_, LIVE_>), GNNVC_ANY_ARGS);   \
        else hipLaunchKernelGGL((k_stage_any<MODE_, 256, true, false, OPEN_, LIVE_>), GNNVC_ANY_ARGS);           \
    } while (0)
    // (OPEN: only a stage that ends in its bare linear layer leaves the instantiations that were there; a dense stage's are OPEN.
    // LIVE: never OPEN, never the listed rows — fourteen instantiations beside the others)
#define GNNVC_ANY_LAUNCH(MODE_)                                     \
    do {                                                            \
        if (sp.end == kEndNone) GNNVC_ANY_FORMS(MODE_, true, false); \
        else GNNVC_ANY_FORMS(MODE_, false, false);                  \
    } while (0)
    switch (rows) {
    case AnyRows::kAll:
        if (sp.dense) GNNVC_ANY_FORMS(kAnyDense, true, false);
        else if (live) GNNVC_ANY_FORMS(kAnyAll, false, true);
        else GNNVC_ANY_LAUNCH(kAnyAll);
        break;
    case AnyRows::kLight:
        if (live) GNNVC_ANY_FORMS(kAnyLight, false, true);
        else GNNVC_ANY_LAUNCH(kAnyLight);
        break;
    case AnyRows::kListed: GNNVC_ANY_LAUNCH(kAnyListed); break;
    }
#undef GNNVC_ANY_FORMS
#undef GNNVC_ANY_LAUNCH
#undef GNNVC_ANY_ARGS
    return hipGetLastError();
}

// the big instantiations take more than 64 KiB of dynamic LDS: told to the runtime once per device and instantiation
// (allow_dynamic_lds of gnnvc_kernels.hip), by gnnvc_set_generic_big_stages — a refusal surfaces there, never inside a forward.
// The FEAT instantiations likewise (a wide stage may be a big one too), by gnnvc_set_generic_feature_width.
template <bool FEAT>
static hipError_t allow_stage_forms() {
    static std::atomic<uint64_t> done[27];
    hipError_t rc = hipSuccess;
    int i = 0;
#define GNNVC_ANY_ALLOW(MODE_, BLOCK_, OPEN_, LIVE_)                                                                                           \
    if (rc == hipSuccess)                                                                                                               \
        rc = allow_dynamic_lds(reinterpret_cast<const void *>(k_stage_any<MODE_, BLOCK_, true, FEAT, OPEN_, LIVE_>), (int)kAnyBigLdsBytes, done[i]);  \
    ++i
#define GNNVC_ANY_ALLOW3(MODE_, OPEN_, LIVE_) \
    GNNVC_ANY_ALLOW(MODE_, 256, OPEN_, LIVE_); GNNVC_ANY_ALLOW(MODE_, 512, OPEN_, LIVE_); GNNVC_ANY_ALLOW(MODE_, 1024, OPEN_, LIVE_)
    GNNVC_ANY_ALLOW3(kAnyAll, false, false);
    GNNVC_ANY_ALLOW3(kAnyLight, false, false);
    GNNVC_ANY_ALLOW3(kAnyListed, false, false);
    GNNVC_ANY_ALLOW3(kAnyAll, true, false);      // (gnnvc_set_generic_patterns: a last stage that ends in its bare linear layer)
    GNNVC_ANY_ALLOW3(kAnyLight, true, false);
    GNNVC_ANY_ALLOW3(kAnyListed, true, false);
    GNNVC_ANY_ALLOW3(kAnyDense, true, false);    // (... and a dense stage)
    GNNVC_ANY_ALLOW3(kAnyAll, false, true);      // (gnnvc_set_generic_live_columns: the launches that may gather from the table)
    GNNVC_ANY_ALLOW3(kAnyLight, false, true);
#undef GNNVC_ANY_ALLOW3
#undef GNNVC_ANY_ALLOW
    return rc;
}
hipError_t allow_big_stages() { return allow_stage_forms<false>(); }
hipError_t allow_feat_stages() { return allow_stage_forms<true>(); }

hipError_t launch_any_live(const StageCall &c, uint32_t max_percent) {
    const StagePlan &sp = *c.sp;
    const GraphDev &g = *c.g;
    const uint32_t n = g.n;
    if (n == 0) return hipSuccess;
    if (sp.dense || sp.f < 2 || sp.f > kAnyFeatMax || max_percent < 1 || max_percent > 100 || !c.live_desc || !c.live_table || !c.in || g.sliced())
        return hipErrorInvalidValue;
    AnyLiveDesc *desc = reinterpret_cast<AnyLiveDesc *>(c.live_desc);
    const uint64_t total = (uint64_t)n * (uint64_t)sp.f;
    const unsigned mask_need = (unsigned)std::min<uint64_t>((total / 4u + kLiveBlock - 1) / kLiveBlock + 1u, 256u * 8u);
    hipLaunchKernelGGL(k_any_live_mask, dim3(mask_need), dim3(kLiveBlock), 0, c.stream, c.in, total, (uint32_t)sp.f, desc);
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
    const unsigned pack_need = (unsigned)std::min<uint64_t>(((uint64_t)n + kLivePackRows - 1) / kLivePackRows, 256u * 8u);
    hipLaunchKernelGGL(k_any_live_pack, dim3(pack_need), dim3(kLiveBlock), 0, c.stream, c.in, c.live_table, n, (uint32_t)sp.f, max_percent, desc);
    return hipGetLastError();
}

hipError_t launch_any_heavy_sums(const StageCall &c, const AnyHeavyRows &hr) {
    if (c.row_hi <= c.row_lo || hr.n == 0) return hipSuccess;
    const StagePlan &sp = *c.sp;
    const GraphDev &g = *c.g;
    if (sp.f < 1 || sp.f > kAnyFeatMax || !hr.list || !hr.hsum || c.row_hi > g.hi() || c.row_lo < g.lo()) return hipErrorInvalidValue;
    const int gs = heavy_shift(sp.f);           // <= 6: a group is at most a wave, and the adders are lanes of the first wave
    const size_t lds = heavy_lds_bytes(sp.f);   // <= 34 816 bytes (f = 64)
    const dim3 grid(hr.n), block(kHeavyBlock);
#define GNNVC_HEAVY_LAUNCH(R_)                                                                                            \
    hipLaunchKernelGGL((k_any_heavy_sums<R_>), grid, block, lds, c.stream, g.rowptr, g.col, c.in, hr.list, hr.hsum, \
                       (uint32_t)sp.f, (uint32_t)gs, c.row_lo, c.row_hi, hr.below)
    switch (heavy_passes(gs)) {
    case 4: GNNVC_HEAVY_LAUNCH(4); break;
    case 8: GNNVC_HEAVY_LAUNCH(8); break;
    default: GNNVC_HEAVY_LAUNCH(16); break;
    }
#undef GNNVC_HEAVY_LAUNCH
    return hipGetLastError();
}

hipError_t find_any_giant_rows(const GraphDev &g, const uint32_t *list, uint32_t n_list, uint32_t thresh, void *meta, uint32_t *count,
                               hipStream_t stream) {
    hipError_t rc = hipMemsetAsync(count, 0, sizeof(uint32_t), stream);
    if (rc != hipSuccess || n_list == 0) return rc;
    hipLaunchKernelGGL(k_find_any_giant, dim3((n_list + 255) / 256), dim3(256), 0, stream, g.rowptr, list, n_list, thresh,
                       reinterpret_cast<uint4 *>(meta), count);
    return hipGetLastError();
}

hipError_t launch_any_giant(const StageCall &c, const AnyGiantRows &ar, float *hsum, AnyGiantPart part) {
    const GiantRows &gr = ar.gr;
    if (c.row_hi <= c.row_lo || gr.n == 0) return hipSuccess;
    const StagePlan &sp = *c.sp;
    const GraphDev &g = *c.g;
    if (sp.f < 1 || sp.f > kAnyFeatMax || !gr.meta || !gr.off || !gr.slab || !gr.agg || !ar.pos || !hsum || c.row_hi > g.hi() || c.row_lo < g.lo())
        return hipErrorInvalidValue;
    const uint4 *meta = reinterpret_cast<const uint4 *>(gr.meta);
    const uint32_t f = (uint32_t)sp.f;
    if (part == AnyGiantPart::kPlace) {
        const size_t cells = (size_t)gr.n * f;
        hipLaunchKernelGGL(k_any_giant_place, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c.stream, meta, ar.pos, gr.agg, hsum, gr.n,
                           f, c.row_lo, c.row_hi);
        return hipGetLastError();
    }
    const uint32_t win = giant_window();
    if (giant_block() != (uint32_t)kAnyGiantBlk || win % (uint32_t)kAnyGiantBlk != 0 || gr.blocks == 0) return hipErrorInvalidValue;
    const dim3 grid(gr.blocks), block(kAnyGiantBlk);
#define GNNVC_GIANT_GATHER(GS_)                                                                                              \
    hipLaunchKernelGGL((k_any_giant_gather<GS_>), grid, block, lds, c.stream, g.col, c.in, gr.slab, meta, gr.off, gr.n, f, win, \
                       c.row_lo, c.row_hi, c0)
    for (uint32_t c0 = 0; c0 < f; c0 += 32u) {   // (one launch for f <= 32; the columns from 32 on in a second)
        const uint32_t fw = std::min(f - c0, 32u);
        const size_t lds = (size_t)fw * kAnyGiantPitch * sizeof(float);   // <= 33 280 bytes
        switch (heavy_shift((int)fw)) {
        case 0: GNNVC_GIANT_GATHER(0); break;
        case 1: GNNVC_GIANT_GATHER(1); break;
        case 2: GNNVC_GIANT_GATHER(2); break;
        case 3: GNNVC_GIANT_GATHER(3); break;
        case 4: GNNVC_GIANT_GATHER(4); break;
        default: GNNVC_GIANT_GATHER(5); break;
        }
        const hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
    }
#undef GNNVC_GIANT_GATHER
    return hipSuccess;
}

}  // namespace gnnvc
