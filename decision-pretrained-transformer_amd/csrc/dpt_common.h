// Shared device-side definitions for libdpt_hip.so (gfx950 / CDNA4 only).
//
// Compiled with -ffp-contract=off: every fused multiply-add below is an
// explicit fmaf()/__builtin_amdgcn_mfma_*, so the fp64 env arithmetic stays
// two-rounding (bit-exact to numpy) and the fp32 model arithmetic is exactly
// the order written here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpt_hip.h"

namespace dpt {

constexpr int kE = 32;          // n_embd (only size built; common_args.py:31 default)
constexpr int kFF = 4 * kE;     // GPT-2 inner dim
constexpr int kWave = 64;
constexpr int kMaxA = 32;       // action_dim limit of the selection / head tiles
constexpr int kMaxF = 64;       // token feature limit (2*sd + A + 1)

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef double doublex2 __attribute__((ext_vector_type(2)));

// ----------------------------------------------------------------------------- error plumbing
void set_error(int code, const char* fmt, ...);
int check_hip(hipError_t e, const char* what);

// host glue of the entry points: argument checks, the stream handle, 16-byte region sizes, launch errors
#define DPT_REQUIRE(cond, ...)                     \
    do {                                           \
        if (!(cond)) {                             \
            set_error(DPT_EINVAL, __VA_ARGS__);    \
            return DPT_EINVAL;                     \
        }                                          \
    } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline int64_t round4(int64_t n) { return (n + 3) & ~int64_t(3); }
inline int launched(const char* what) { return check_hip(hipGetLastError(), what); }
// the cross-entropy entry points and the steps built on them take at most kMaxA actions
inline int check_action_dim(const char* who, int A) {
    if (A <= kMaxA) return DPT_OK;
    set_error(DPT_EUNSUPPORTED, "%s: action_dim=%d above %d", who, A, kMaxA);
    return DPT_EUNSUPPORTED;
}

// ----------------------------------------------------------------------------- model view
// Offsets (in floats) inside one transformer block of the packed blob, dpt_hip.h order.
struct LayerOff {
    static constexpr int ln1_g = 0;
    static constexpr int ln1_b = ln1_g + kE;
    static constexpr int attn_w = ln1_b + kE;
    static constexpr int attn_b = attn_w + kE * 3 * kE;
    static constexpr int proj_w = attn_b + 3 * kE;
    static constexpr int proj_b = proj_w + kE * kE;
    static constexpr int ln2_g = proj_b + kE;
    static constexpr int ln2_b = ln2_g + kE;
    static constexpr int fc_w = ln2_b + kE;
    static constexpr int fc_b = fc_w + kE * kFF;
    static constexpr int mp_w = fc_b + kFF;
    static constexpr int mp_b = mp_w + kFF * kE;
    static constexpr int size = mp_b + kE;  // 12,704 floats per block at E = 32
};
static_assert(LayerOff::size == 12704, "GPT-2 block parameter count at E=32");

// Device pointers into one packed weight blob (passed to kernels by value).
struct ModelView {
    const float* emb_w;   // [F][E]
    const float* emb_b;   // [E]
    const float* wpe;     // [n_positions][E]
    const float* layers;  // n_layer * LayerOff::size
    const float* lnf_g;
    const float* lnf_b;
    const float* head_w;  // [E][A]
    const float* head_b;  // [A]
    // every block's attention folded (L0Off, one block per layer): G = Wq Wk^T,
    // g0 = Wk bq, Wvp = Wv Wproj, bvp = bv Wproj + bproj; then a second set of n_layer blocks with
    // ln_1's g and b folded in for blocks >= 1 (the bandit rollout's packed y cache, derive_l0_kernel)
    const float* l0;
    int n_layer, sd, A, F, n_positions;
    // MLP products on fp16 two-part splits (dpt_mfma_fwd.h Split2): c_fc / mlp.c_proj
    // weights are packed x 2^mlp_ew and the activations split x 2^mlp_ex, powers of two
    // chosen at model creation from static bounds (mlp_scales), so nothing overflows fp16
    int mlp_ew, mlp_ex;
    // the same for the attention's dense products and scores: G and Wvp packed x 2^attn_ew,
    // ln_1 outputs y (keys) and attention outputs x 2^attn_ey, queries u x 2^attn_eq
    int attn_ew, attn_ey, attn_eq;
};

// ----------------------------------------------------------------------------- Philox4x32-10
struct U4 { uint32_t x, y, z, w; };

__host__ __device__ inline uint32_t mulhilo(uint32_t a, uint32_t b, uint32_t* hi) {
    uint64_t p = (uint64_t)a * (uint64_t)b;
    *hi = (uint32_t)(p >> 32);
    return (uint32_t)p;
}

// Philox4x32 with 10 rounds (Salmon et al., SC'11); key = seed, counter =
// (step lo, task lo, stream, task hi ^ step hi).
__host__ __device__ inline U4 philox(uint64_t seed, uint64_t step, int64_t task, uint32_t stream) {
    uint32_t c0 = (uint32_t)step, c1 = (uint32_t)task, c2 = stream;
    uint32_t c3 = (uint32_t)((uint64_t)task >> 32) ^ (uint32_t)(step >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0, hi1;
        uint32_t lo0 = mulhilo(0xD2511F53u, c0, &hi0);
        uint32_t lo1 = mulhilo(0xCD9E8D57u, c2, &hi1);
        uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}

// 53-bit uniform in [0, 1) from two words (numpy's random_sample construction).
__host__ __device__ inline double u53(uint32_t a, uint32_t b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

__host__ __device__ inline double philox_uniform(uint64_t seed, uint64_t step, int64_t task, uint32_t stream) {
    U4 r = philox(seed, step, task, stream);
    return u53(r.x, r.y);
}

// Box-Muller standard normal from one Philox block (u1 in (0,1], u2 in [0,1)).
__device__ inline double philox_normal(uint64_t seed, uint64_t step, int64_t task, uint32_t stream) {
    U4 r = philox(seed, step, task, stream);
    double u1 = 1.0 - u53(r.x, r.y);
    double u2 = u53(r.z, r.w);
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

// ----------------------------------------------------------------------------- selection
// numpy pairwise float32 sum (numpy/_core/src/umath/loops_utils.h.src pairwise_sum):
// sequential from 0 below 8 elements, 8 running partials + fixed tree above.
// Element k is produced by elem(k) (recomputed, never stored: no scratch arrays).
template <class Elem>
__device__ inline float np_pairwise_sum_f32(Elem elem, int n) {
    if (n < 8) {
        float res = 0.f;
        for (int i = 0; i < n; ++i) res += elem(i);
        return res;
    }
    float r0 = elem(0), r1 = elem(1), r2 = elem(2), r3 = elem(3);
    float r4 = elem(4), r5 = elem(5), r6 = elem(6), r7 = elem(7);
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
        r0 += elem(i); r1 += elem(i + 1); r2 += elem(i + 2); r3 += elem(i + 3);
        r4 += elem(i + 4); r5 += elem(i + 5); r6 += elem(i + 6); r7 += elem(i + 7);
    }
    float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += elem(i);
    return res;
}

// Reference action choice (ctrls/ctrl_bandit.py:435-443, ctrls/ctrl_darkroom.py:48-62):
// greedy = first argmax of the fp32 logits; sampling = scipy softmax (fp32:
// max-shift, exp, pairwise sum, divide) then numpy RandomState.choice(A, p)
// with its uniform u: cdf = cumsum(float64(p)); cdf /= cdf[-1];
// idx = searchsorted(cdf, u, 'right').  Every intermediate is recomputed
// bit-identically instead of stored, so no per-lane arrays are needed.
__device__ inline int select_from_logits(const float* logits, int A, int sample, float temp, double u) {
    if (!sample) {
        int best = 0;
        float bv = logits[0];
        for (int k = 1; k < A; ++k) {
            if (logits[k] > bv) { bv = logits[k]; best = k; }
        }
        return best;
    }
    auto xk = [&](int k) { return (temp == 1.0f) ? logits[k] : logits[k] / temp; };
    float m = -INFINITY;
    for (int k = 0; k < A; ++k) m = fmaxf(m, xk(k));
    auto ek = [&](int k) { return expf(xk(k) - m); };
    const float s = np_pairwise_sum_f32(ek, A);
    double total = 0.0;
    for (int k = 0; k < A; ++k) total += (double)(ek(k) / s);
    double c = 0.0;
    int idx = 0;
    for (int k = 0; k < A; ++k) {
        c += (double)(ek(k) / s);
        idx += (c / total <= u) ? 1 : 0;
    }
    return idx < A ? idx : A - 1;
}

// Fixed-A twin of select_from_logits: same arithmetic, every intermediate in
// registers (each exp and quotient computed once).
template <int NA>
__device__ inline int select_fixed(const float (&lg)[NA], int sample, float temp, double u) {
    if (!sample) {
        int best = 0;
        float bv = lg[0];
#pragma unroll
        for (int k = 1; k < NA; ++k)
            if (lg[k] > bv) { bv = lg[k]; best = k; }
        return best;
    }
    float xk[NA], ek[NA];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        xk[k] = (temp == 1.0f) ? lg[k] : lg[k] / temp;
        m = fmaxf(m, xk[k]);
    }
#pragma unroll
    for (int k = 0; k < NA; ++k) ek[k] = expf(xk[k] - m);
    const float s = np_pairwise_sum_f32([&](int k) { return ek[k]; }, NA);
    double total = 0.0;
#pragma unroll
    for (int k = 0; k < NA; ++k) total += (double)(ek[k] / s);
    double c = 0.0;
    int idx = 0;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        c += (double)(ek[k] / s);
        idx += (c / total <= u) ? 1 : 0;
    }
    return idx < NA ? idx : NA - 1;
}

// select_fixed split at its cdf: q[k] = c_k / total (the values select_fixed
// compares with u), so a caller that meets the same logits again selects with
// select_from_cdf alone -- bit-identical to select_fixed on those logits.
template <int NA>
__device__ inline void cdf_fixed(const float (&lg)[NA], float temp, double (&q)[NA]) {
    float xk[NA], ek[NA];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        xk[k] = (temp == 1.0f) ? lg[k] : lg[k] / temp;
        m = fmaxf(m, xk[k]);
    }
#pragma unroll
    for (int k = 0; k < NA; ++k) ek[k] = expf(xk[k] - m);
    const float s = np_pairwise_sum_f32([&](int k) { return ek[k]; }, NA);
    double total = 0.0;
#pragma unroll
    for (int k = 0; k < NA; ++k) total += (double)(ek[k] / s);
    double c = 0.0;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        c += (double)(ek[k] / s);
        q[k] = c / total;
    }
}

template <int NA>
__device__ inline int select_from_cdf(const double* q, double u) {
    int idx = 0;
#pragma unroll
    for (int k = 0; k < NA; ++k) idx += (q[k] <= u) ? 1 : 0;
    return idx < NA ? idx : NA - 1;
}

// The same selection with a fp32 fast path.  cdf_fast is the cdf in fp32 (q_k = prefix_k(e) /
// sum(e), e_k = 2^((x_k - m) log2 e) on v_exp_f32); it is within about 1e-6 (absolute) of
// cdf_fixed's fp64 values (the fp32 quotients and exponentials differ by a few ulp, and a term's
// weight e_k / sum(e) shrinks faster than its argument's rounding grows).  Where every
// |q_k - u| exceeds kCdfMargin = 2^-15 the comparisons q_k <= u therefore agree with cdf_fixed's,
// and select_fast returns select_from_cdf's index without the fp64 work; otherwise (about 5e-4 of
// the draws, NaN logits included) it runs cdf_fixed itself.  Bit-identical to select_fixed.
constexpr float kCdfMargin = 1.0f / 32768.0f;
template <int NA>
__device__ inline void cdf_fast(const float (&lg)[NA], float temp, float (&q)[NA]) {
    float xk[NA], e[NA];
    float m = -INFINITY;
    // temp is uniform: a real branch, so the IEEE divisions (a dozen instructions each, on the
    // tail's serial chain) run only when temp != 1 (the empty asm keeps the compiler from
    // computing both sides and selecting)
    if (temp == 1.0f) {
#pragma unroll
        for (int k = 0; k < NA; ++k) xk[k] = lg[k];
    } else {
        asm volatile("" ::: "memory");
#pragma unroll
        for (int k = 0; k < NA; ++k) xk[k] = lg[k] / temp;
    }
#pragma unroll
    for (int k = 0; k < NA; ++k) m = fmaxf(m, xk[k]);
#pragma unroll
    for (int k = 0; k < NA; ++k) e[k] = __builtin_amdgcn_exp2f((xk[k] - m) * 1.4426950408889634f);
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < NA; ++k) tot += e[k];
    const float r = __builtin_amdgcn_rcpf(tot);
    float c = 0.f;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        c += e[k];
        q[k] = c * r;
    }
}
template <int NA>
__device__ inline int select_fast(const float* q, const float (&lg)[NA], float temp, double u) {
    const float uf = (float)u;
    int idx = 0;
    bool safe = true;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        idx += (q[k] <= uf) ? 1 : 0;
        safe = safe && __builtin_fabsf(q[k] - uf) > kCdfMargin;  // false for NaN
    }
    if (safe) return idx < NA ? idx : NA - 1;
    double qe[NA];
    cdf_fixed<NA>(lg, temp, qe);
    return select_from_cdf<NA>(qe, u);
}
// select_fixed through the fast path (bit-identical)
template <int NA>
__device__ inline int select_fixed_fast(const float (&lg)[NA], int sample, float temp, double u) {
    if (!sample) return select_fixed<NA>(lg, 0, temp, u);
    float q[NA];
    cdf_fast<NA>(lg, temp, q);
    return select_fast<NA>(q, lg, temp, u);
}

// Every block's attention folded (ModelView::l0, one L0Off block per layer,
// derived at model creation by derive_l0_kernel): with y = LN1(h), q.k_s =
// y_s . u + (terms constant over the keys s) for u = Wk q = y G + g0, and
// sum_s P_s v_s = (sum_s P_s y_s) Wv + bv.  Used by the bandit rollout
// (dpt_decode.hip) and the MFMA window forwards (dpt_mfma_fwd.h).  All
// matrices [in][out], E x E.
// Dimensions of the generic-width training forward / backward (dpt_train.hip) and rollout (dpt_generic.hip): layers, width,
// token features, actions, sequences, tokens per sequence, wpe rows.
struct TrDims {
    int L, E, F, A, B, T, npos;
    int fwd_only;  // DPT_TRAIN_FORWARD_ONLY: inference workspace (nothing saved for a backward)
    // dropout (dpt_hip.h dpt_train_desc): element kept iff its Philox word >= drop_thr, then
    // scaled by drop_scale; drop_thr == 0: no dropout
    uint32_t drop_thr;
    float drop_scale;
    uint64_t drop_seed;
    int last_loss = 0;  // DPT_TRAIN_LAST_LOSS: the loss reads the last position only (no dropout, not forward-only)
    __host__ __device__ bool drop() const { return drop_thr != 0; }
    __host__ __device__ int R() const { return B * T; }
    __host__ __device__ int64_t layer_size() const { return 12ll * E * E + 13ll * E; }
};

// dropout factor of element e of a site (dpt_hip.h dpt_train_desc): drop_scale when the element's
// Philox word clears the threshold, else 0.  Regenerated in the backward -- no mask is stored.
__device__ inline float tr_keep(const TrDims& d, int site, int64_t e) {
    const U4 r = philox(d.drop_seed, (uint64_t)site, e >> 2, DPT_STREAM_DROPOUT);
    const int k = (int)(e & 3);
    const uint32_t w = k == 0 ? r.x : k == 1 ? r.y : k == 2 ? r.z : r.w;
    return w >= d.drop_thr ? d.drop_scale : 0.0f;
}

// dropout p -> (drop_thr, drop_scale) of TrDims (defined in dpt_abi.hip): keep iff word >= ceil(p 2^32)
void drop_params(float p, uint32_t& thr, float& scale);

// The training row kernels of dpt_train.hip as host entry points for the image front end
// (dpt_image.hip): Y = X W + bias, LayerNorm forward / input gradient / parameter gradients, the
// chunked weight gradient with its fixed-order reduction, and dX = dY W^T.  `part` is scratch of
// rows_chunks(R) * (IN + 1) * OUT floats (rows_ln_param_grad: IN = 1, OUT = E).
int64_t rows_chunks(int64_t R);
int rows_linear(const float* X, const float* W, const float* bias, int R, int IN, int OUT, float* Y, hipStream_t st);
int rows_layernorm(const float* x, const float* g, const float* b, int R, int E, float* y, float* stats,
                   hipStream_t st);
int rows_layernorm_bwd(const float* x, const float* stats, const float* g, const float* dy, int R, int E, float* dx,
                       hipStream_t st);
int rows_ln_param_grad(const float* x, const float* stats, const float* dy, int R, int E, float* part, float* dg,
                       float* db, hipStream_t st);
int rows_wgrad(const float* X, const float* dY, int R, int IN, int OUT, float* part, float* dW, float* db,
               hipStream_t st);
int rows_linear_bwd_data(const float* dY, const float* W, int R, int IN, int OUT, float* dX, hipStream_t st);
// dW (IN x OUT) | db (OUT) = nch partials of (IN + 1) * OUT floats summed in chunk order (tr_wgrad_reduce)
int rows_reduce_parts(const float* part, int nch, int IN, int OUT, float* dW, float* db, hipStream_t st);

// The env action of rollout_bandit_generic (dpt_generic.hip) when it is not the action written into the context
// (dpt_rollout_bandit_generic_env, dpt_explore.hip): the reward and arm_value_out come from it.
struct GenEnvAct {
    const int32_t* env_actions;  // (H, N) injected, clamped to [0, A); or nullptr
    int random;                  // env_actions == nullptr: 1 = min(A - 1, floor(u A)), u from DPT_STREAM_ENVACT; 0 = the selected action
    int32_t* env_actions_out;    // (N, H) the env actions taken, or nullptr
};

// shared by the interactive and the explorer/exploiter training steps (defined in dpt_interactive.hip):
// the shape checks of a chunk of N envs at window K >= min_K (fills `run` = the desc with batch N,
// window K, flags 0; messages begin with `who`), and dst += src element by element in one launch
int ia_check_shape(const dpt_train_desc* d, int32_t N, int32_t K, int32_t min_K, const char* who,
                   dpt_train_desc& run);
int ia_accumulate(float* dst, const float* src, int64_t numel, void* stream);

// The hard-target cross-entropy of one row of A fp32 logits, in fp64 per element with one rounding on
// the store: returns lse(x) - x[tg] and, with dx, stores dx = sw (softmax(x) - onehot(tg)).  tg lies
// in [0, A): the callers store their explicit zeros (no class, weight 0, rows the loss skips) themselves.
__device__ inline double ce_hard_row(const float* x, int A, int64_t tg, double sw, float* dx) {
    float mf = x[0];
    for (int k = 1; k < A; ++k) mf = fmaxf(mf, x[k]);
    const double m = (double)mf;
    double s = 0.0;
    for (int k = 0; k < A; ++k) s += exp((double)x[k] - m);
    const double lse = m + log(s);
    if (dx)
        for (int k = 0; k < A; ++k) dx[k] = (float)(sw * (exp((double)x[k] - lse) - (k == tg ? 1.0 : 0.0)));
    return lse - (double)x[tg];
}
// *acc += scale * sum_i w_i values[i], w = weights or 1 (a weight of 0 adds nothing, whatever the value):
// one workgroup, thread-strided sums, then an LDS tree -- a fixed order (defined in dpt_trainstep.hip)
void ce_finish(const double* values, const double* weights, int64_t n, double scale, double* acc, hipStream_t st);

struct L0Off {
    static constexpr int G = 0;                // Wq Wk^T: u = xn G + g0 = Wk q
    static constexpr int g0 = G + kE * kE;      // Wk bq
    static constexpr int Wvp = g0 + kE;         // Wv Wproj
    static constexpr int bvp = Wvp + kE * kE;   // bv Wproj + bproj
    static constexpr int size = bvp + kE;
};

// Tasks the K/V workspace is laid out for: N rounded up to whole tiles of the
// largest decode tile (16), so the bandit rollout's tile-interleaved y rows of a
// partial last tile stay inside their block's slot (dpt_kvcache_numel).
__host__ __device__ inline int kv_tasks(int N) { return (N + 15) & ~15; }

// ----------------------------------------------------------------------------- env arithmetic
// envs/bandit_env.py:59: means[a] + np.random.normal(0, var) == means[a] + (0.0 + var*g).
__device__ inline double gaussian_reward(double mean, double var, double g) {
    double noise = __dadd_rn(0.0, __dmul_rn(var, g));
    return __dadd_rn(mean, noise);
}

// ----------------------------------------------------------------------------- across the sources
// Every function one source defines and another calls (mostly dpt_abi.hip, the extern "C" surface),
// declared here alone: the defining source includes this header too, so a changed signature fails to
// compile there.  Default arguments live here.
// dpt_decode.hip
ModelView make_view(const float* blob, const dpt_model_desc& d);
int64_t weights_numel(const dpt_model_desc& d);
int launch_decode_step(const ModelView&, float*, int, int, int, const float*, float*, hipStream_t);
int launch_window_decode(const ModelView&, float*, int, int, const float*, const float*, const float*,
                         const float*, const float*, int, float*, hipStream_t);
int launch_rollout_bandit(const ModelView&, const dpt_bandit_rollout_args&, hipStream_t);
int launch_derive_l0(const ModelView&, float*, hipStream_t);
int64_t l0_numel(int n_layer);
int set_decode_tile(int);
int set_cache_budget(int64_t);
int set_ycache_bits(int);
// dpt_env.hip
int launch_bandit_step(const double*, int, int, const int32_t*, int, double, const double*, uint64_t, uint64_t,
                       int64_t, double*, double*, hipStream_t);
int launch_darkroom_step(const int32_t*, const int32_t*, const int32_t*, const int32_t*, int, int, int32_t*,
                         int32_t*, hipStream_t);
int launch_darkroom_opt(const int32_t*, const int32_t*, const int32_t*, int, int32_t*, hipStream_t);
int launch_select(const float*, int, int, int, float, const double*, uint64_t, uint64_t, int64_t, int32_t*,
                  hipStream_t);
int launch_draw(int, uint64_t, uint64_t, int64_t, int, uint32_t, double*, hipStream_t);
int launch_rollin_bandit(const double*, const double*, int, int, int, int, double, const double*, const double*,
                         uint64_t, int64_t, int32_t*, double*, hipStream_t);
int launch_rollin_darkroom(const int32_t*, const int32_t*, int, int, int, int, const int32_t*, const int32_t*,
                           uint64_t, int64_t, int32_t*, int32_t*, int32_t*, int32_t*, int32_t*, int32_t*,
                           hipStream_t);
int set_select_fast(int);
// dpt_fresh_linear.hip
int fresh_linear_check(const char* who, const dpt_train_desc*, const dpt_fresh_linear_args*, int32_t batch);
// dpt_policies.hip
int launch_rollout_policy(const dpt_policy_rollout_args&, hipStream_t);
int set_policy_wave(int on);
// dpt_darkroom.hip
int launch_pack_fragments(const ModelView&, float*, hipStream_t);
int64_t fragments_numel(int n_layer);
int launch_rollout_darkroom(const ModelView&, const float*, const dpt_darkroom_rollout_args&, hipStream_t);
int darkroom_max_window();
int64_t darkroom_workspace_numel(int N, int64_t window);
int set_darkroom_memo(int);
// dpt_prefill.hip
int prefill_max_window(const ModelView&);
int launch_prefill(const ModelView&, const float*, const float*, const float*, const float*, const float*,
                   const float*, int, int, int, float*, hipStream_t);
bool darkroom_episode_fits(int n_layer, int K);
int launch_darkroom_episode(const ModelView&, const float*, const dpt_darkroom_episode_args&, hipStream_t);
// dpt_stats.hip
int regret_max_steps();
int64_t regret_workspace_numel(int N, int H);
int launch_regret_moments(const double*, const double*, int, int, int, const double*, double*, double*, hipStream_t);
// dpt_train.hip; embeds / dembeds: the token embedding computed by the caller, and its gradient
int train_forward(const TrDims&, const float* blob, const float* tok, float* ws, float* preds, hipStream_t,
                  const float* embeds = nullptr);
int train_backward(const TrDims&, const float* blob, const float* tok, float* ws, const float* dpreds, float* dblob,
                   hipStream_t, float* dembeds = nullptr);
int64_t train_workspace_numel(const TrDims&);
int64_t train_blob_numel(const TrDims&);
int train_dims_check(const TrDims&);
// dpt_generic.hip; env: the env action when it is not the selected one (nullptr: it is)
int64_t gen_rollout_workspace_numel(const TrDims&, int N, int H);
int rollout_bandit_generic(const TrDims&, const float* blob, const dpt_bandit_rollout_args&, hipStream_t,
                           const GenEnvAct* env = nullptr);

}  // namespace dpt
