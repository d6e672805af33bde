// Shared by the two generic-width sources, dpt_train.hip (the training trunk) and dpt_generic.hip (the
// generic-width bandit rollout): the packed blob's offsets, the workspace cursor, the wave helpers, the
// one-query-row attention front and the embedding row as device functions, the compile-time width
// dispatch, and the trunk's enqueue-only host entry points that the rollout drives.
#pragma once

#include <type_traits>

#include "dpt_common.h"

namespace dpt {

constexpr int kTrThreads = 256;
static inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kTrThreads - 1) / kTrThreads); }

// offsets of one layer in the packed blob (dpt_hip.h: [ln1 g b][c_attn W b][c_proj W b][ln2 g b][c_fc W b][mlp.c_proj W b])
struct TrLayer {
    int64_t ln1_g, ln1_b, attn_w, attn_b, proj_w, proj_b, ln2_g, ln2_b, fc_w, fc_b, mp_w, mp_b;
    __host__ __device__ static TrLayer make(int64_t base, int E) {
        TrLayer o;
        int64_t p = base;
        o.ln1_g = p; p += E;
        o.ln1_b = p; p += E;
        o.attn_w = p; p += 3ll * E * E;
        o.attn_b = p; p += 3 * E;
        o.proj_w = p; p += (int64_t)E * E;
        o.proj_b = p; p += E;
        o.ln2_g = p; p += E;
        o.ln2_b = p; p += E;
        o.fc_w = p; p += 4ll * E * E;
        o.fc_b = p; p += 4 * E;
        o.mp_w = p; p += 4ll * E * E;
        o.mp_b = p;
        return o;
    }
};

struct TrBlob {  // offsets of the model-level parameters
    int64_t emb_w, emb_b, wpe, layers, lnf_g, lnf_b, head_w, head_b, total;
    __host__ __device__ static TrBlob make(const TrDims& d) {
        TrBlob b;
        int64_t p = 0;
        b.emb_w = p; p += (int64_t)d.F * d.E;
        b.emb_b = p; p += d.E;
        b.wpe = p; p += (int64_t)d.npos * d.E;
        b.layers = p; p += d.L * d.layer_size();
        b.lnf_g = p; p += d.E;
        b.lnf_b = p; p += d.E;
        b.head_w = p; p += (int64_t)d.E * d.A;
        b.head_b = p; p += d.A;
        b.total = p;
        return b;
    }
};

// Lays a workspace out in floats: take(k) is the offset of the next array of k floats; every array
// starts 16-B aligned (rows are read as float4)
struct WsCursor {
    int64_t p = 0;
    __host__ __device__ int64_t take(int64_t k) { const int64_t at = p; p = (p + k + 3) & ~3ll; return at; }
};

// order this wave's LDS writes before its later LDS reads of other lanes' entries
__device__ inline void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ inline float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// embed_transition(tok) + wpe[pos], column e of one token row (models/net.py:52-54 + GPT2Model
// inputs_embeds + wpe): the bias, then the features in order
__device__ inline float embed_row(const float* __restrict__ tok, const float* __restrict__ blob, const TrDims& d,
                                  const TrBlob& b, int pos, int e) {
    float acc = blob[b.emb_b + e];
    for (int f = 0; f < d.F; ++f) acc = fmaf(tok[f], blob[b.emb_w + (int64_t)f * d.E + e], acc);
    return acc + blob[b.wpe + (int64_t)pos * d.E + e];
}

// The front of the attention of one query row, by one wave: the query qrow into LDS (q, E floats), then
// pr[j] = exp(s_j - max_j s_j) for the keys j < n, s_j = q . key(j) / sqrt(E) (key(j): the key's row of E
// floats; lanes stride over the keys with the columns in order).  Returns 1 / sum_j pr[j].  The callers'
// tails differ in where they apply it: to the probabilities before the weighted sum, or to the sum.
template <class Key>
__device__ inline float attn_row_front(const float* __restrict__ qrow, int E, int n, Key key, float* q, float* pr) {
    const int lane = threadIdx.x & 63;
    for (int e = lane; e < E; e += 64) q[e] = qrow[e];
    wave_lds_sync();
    const float scale = 1.0f / sqrtf((float)E);
    float m = -INFINITY;
    for (int j = lane; j < n; j += 64) {
        const float* k = key(j);
        float s = 0.f;
        for (int e = 0; e < E; ++e) s = fmaf(q[e], k[e], s);
        s *= scale;
        pr[j] = s;
        m = fmaxf(m, s);
    }
    m = wave_max(m);
    float l = 0.f;
    for (int j = lane; j < n; j += 64) {
        const float p = expf(pr[j] - m);
        pr[j] = p;
        l += p;
    }
    return 1.0f / wave_sum(l);
}

// the error of a dispatch that found no kernel (unreachable while predicate and dispatch share a list)
inline int no_width(const char* what, int w) {
    set_error(DPT_EUNSUPPORTED, "%s: no kernel built for width %d", what, w);
    return DPT_EUNSUPPORTED;
}
// The widths a family of kernels is built for, written once: has(w) is the predicate, and
// call(w, f) runs f(std::integral_constant<int, W>) for the W of the list equal to w, so f
// instantiates its kernel for exactly the widths has() admits; false when w is not in the list
// (nothing ran).  run() is call() as a status.
template <int... Ws>
struct Widths {
    static constexpr bool has(int w) { return ((w == Ws) || ...); }
    template <class F>
    static bool call(int w, F&& f) { return ((w == Ws && (f(std::integral_constant<int, Ws>{}), true)) || ...); }
    template <class F>
    static int run(const char* what, int w, F&& f) { return call(w, f) ? DPT_OK : no_width(what, w); }
};
// lanes per row / per key of the float4 row kernels (tr_layernorm_rows, gen_attn_ydecode4): n rounded up
// to a power of two
using Pow2To64 = Widths<1, 2, 4, 8, 16, 32, 64>;
inline int pow2_ceil(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// ---- the trunk's pieces the generic rollout drives (defined in dpt_train.hip, where tr_mm_rows and
// tr_layernorm_rows are instantiated).  They enqueue and do not read the launch error: the rollout is
// launch-bound and checks once per step.
// the forward products, then the data gradients of the first four in the same order (kMmBdQkv + kind)
enum MmKind { kMmQkv, kMmProj, kMmFc, kMmMp, kMmU, kMmLnQkv, kMmLnFc, kMmBdQkv, kMmBdProj, kMmBdFc, kMmBdMp };
// LayerNorm of R rows into y, (mean, rstd) into st
void layernorm(const float* x, const float* g, const float* bb, int R, int E, float* y, float* st, hipStream_t s);
// Y = X W + bias on R rows (the head)
void row_linear(const float* X, const float* W, const float* bias, int R, int IN, int OUT, float* Y, hipStream_t st);
// One forward product of a block on R decode-sized rows (kMmU / kMmProj / kMmFc / kMmMp): the column-split
// matrix-core form at the widths it is built for, else the row kernel.  kMmLnFc (aux = ln_g, ln_b behind it;
// X = the LayerNorm's input) only where dec_ln_in(E).  DPT_EUNSUPPORTED for a kind / width with no kernel.
bool dec_ln_in(int E);
int dec_product(int E, int kind, const float* X, const float* W, const float* bias, const float* res, int R, float* Y,
                hipStream_t st, const float* aux = nullptr);

}  // namespace dpt
