// The generic-width bandit rollout: the online loop (evals/eval_bandit.py:56-103: decode -> select ->
// env step -> append the transition) at ANY width, for models the fused E = 32 kernel (dpt_decode.hip)
// is not built for.  Inference, not training; it borrows the training trunk's row pieces (dpt_rows.h:
// LayerNorm of rows, the decode-sized products, the head's linear) and owns the rest: the attention
// fold, the workspace, the embed of the new token, the decode attention over the y cache and the env
// step.  Reached from dpt_rollout_bandit_generic[_env] (dpt_abi.hip) and through it from the
// interactive and explorer/exploiter steps (dpt_interactive.hip, dpt_explore.hip).
//
// Exact K/V-cache decode: the bandit's query token sits at position 0 and never changes, and the
// prediction is read at the last position, so every earlier position's keys and values stay
// valid (causal attention) and a step computes the new token only.  The cache holds each block's
// LayerNorm output y instead of K and V (the folded attention, GenFold): half the bytes.  One pass per step over all N
// tasks: embed, then per layer the training forward's row kernels (or their column-split matrix-core
// forms at the widths those are built for, dec_product) on N rows, the attention of the new token over the
// task's cache, ln_f and the head; then selection and the env step with the draws and arithmetic of the fused kernel.
// Folded attention (the fused kernels' algebra, dpt_decode.hip): with y_p = LN1(x_p) a block's keys
// and values are affine in y_p, so q . k_p = u . y_p + const (u = q W_k^T = y G + g0, G = W_q W_k^T,
// g0 = b_q W_k^T; the constant shifts every score of the row equally and cancels in the softmax) and
// sum_p P_p v_p = (sum_p P_p y_p) W_v + b_v, so c_proj takes the attention-weighted y on
// Wvp = W_v W_proj with bvp = b_v W_proj + b_proj.  The cache holds y alone: E floats per position
// and layer instead of K and V's 2E.  Per layer [G | Wvp | g0 | bvp], [in][out], fp64 sums.
#include <algorithm>

#include "dpt_rows.h"

namespace dpt {

struct GenFold {
    __host__ __device__ static int64_t size(int E) { return 2ll * E * E + 2 * E; }
};
__global__ void gen_fold_kernel(const float* __restrict__ blob, TrDims d, TrBlob b, float* __restrict__ fold) {
    const int E = d.E;
    const int64_t per = GenFold::size(E), total = (int64_t)d.L * per;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int l = (int)(i / per);
        const int64_t o = i % per;
        const TrLayer P = TrLayer::make(b.layers + l * d.layer_size(), E);
        const float* Wa = blob + P.attn_w;  // [E][3E]: columns q | k | v
        const float* ba = blob + P.attn_b;
        const float* Wp = blob + P.proj_w;  // [E][E]
        double acc = 0.0;
        if (o < (int64_t)E * E) {  // G[r][c] = sum_k Wq[r][k] Wk[c][k]
            const int r = (int)(o / E), c = (int)(o % E);
            for (int k = 0; k < E; ++k) acc += (double)Wa[(int64_t)r * 3 * E + k] * Wa[(int64_t)c * 3 * E + E + k];
        } else if (o < 2ll * E * E) {  // Wvp[r][c] = sum_k Wv[r][k] Wp[k][c]
            const int64_t oo = o - (int64_t)E * E;
            const int r = (int)(oo / E), c = (int)(oo % E);
            for (int k = 0; k < E; ++k) acc += (double)Wa[(int64_t)r * 3 * E + 2 * E + k] * Wp[(int64_t)k * E + c];
        } else if (o < 2ll * E * E + E) {  // g0[c] = sum_k bq[k] Wk[c][k]
            const int c = (int)(o - 2ll * E * E);
            for (int k = 0; k < E; ++k) acc += (double)ba[k] * Wa[(int64_t)c * 3 * E + E + k];
        } else {  // bvp[c] = sum_k bv[k] Wp[k][c] + bp[c]
            const int c = (int)(o - 2ll * E * E - E);
            for (int k = 0; k < E; ++k) acc += (double)ba[2 * E + k] * Wp[(int64_t)k * E + c];
            acc += blob[P.proj_b + c];
        }
        fold[i] = (float)acc;
    }
}

// Workspace (floats): the y cache [L][N][H][E], the folded weights, then per-step rows.
struct GenWs {
    int64_t Y, fold, x, x2, y, st, qkv, o, h, lg, tok, total;
    static GenWs make(const TrDims& d, int N, int H) {
        GenWs w;
        const int64_t E = d.E, n = N;
        WsCursor c;
        w.Y = c.take((int64_t)d.L * n * H * E);
        w.fold = c.take((int64_t)d.L * GenFold::size(d.E));
        w.x = c.take(n * E);
        w.x2 = c.take(n * E);
        w.y = c.take(n * E);
        w.st = c.take(n * 2);
        w.qkv = c.take(n * 3 * E);
        w.o = c.take(n * E);
        w.h = c.take(n * 4 * E);
        w.lg = c.take(n * d.A);
        w.tok = c.take(n * d.F);
        w.total = c.p;
        return w;
    }
};

// x[n][e] = tok[n] emb_w + emb_b + wpe[pos]: the new token of every task
__global__ void gen_embed(const float* __restrict__ tok, const float* __restrict__ blob, TrDims d, TrBlob b, int N,
                          int pos, float* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * d.E) return;
    x[i] = embed_row(tok + i / d.E * d.F, blob, d, b, pos, (int)(i % d.E));
}

// The folded attention (GenFold) of the new token, one wave per task: store the token's y row (yn) at
// position pos of the task's cache (rows [pos][E] of [N][H][E]) and attend over positions 0..pos with
// the query u -- the scores are u . y_j / sqrt(E) over the cached rows and the new position's own row
// (read from yn itself), the output is the attention-weighted y (c_proj runs on Wvp).  tr_attn_fwd's
// arithmetic for the causal row of the new token (attn_row_front, the probabilities normalised, then
// lanes over the columns with the keys in order).  LDS per wave: H + E floats.
__global__ void gen_attn_ydecode(const float* __restrict__ u, const float* __restrict__ yn, float* __restrict__ Yc,
                                 int E, int N, int H, int pos, float* __restrict__ O) {
    extern __shared__ float sm[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int task = blockIdx.x * (blockDim.x / 64) + wave;
    if (task >= N) return;
    float* pr = sm + (size_t)wave * (H + E);
    const float* row = yn + (int64_t)task * E;
    float* Y = Yc + (int64_t)task * H * E;
    for (int e = lane; e < E; e += 64) Y[(int64_t)pos * E + e] = row[e];
    const float inv = attn_row_front(
        u + (int64_t)task * E, E, pos + 1, [&](int j) { return j == pos ? row : Y + (int64_t)j * E; }, pr + H, pr);
    for (int j = lane; j <= pos; j += 64) pr[j] *= inv;
    wave_lds_sync();
    for (int e = lane; e < E; e += 64) {
        float acc = 0.f;
        for (int j = 0; j < pos; ++j) acc = fmaf(pr[j], Y[(int64_t)j * E + e], acc);
        acc = fmaf(pr[pos], row[e], acc);
        O[(int64_t)task * E + e] = acc;
    }
}

// The same for E % 4 == 0, E <= 256, with the rows read as float4, in one pass over the y cache (flash
// decoding): LPK lanes per key (a power of two >= E / 4, one float4 of the row each), 64 / LPK = KPW keys
// per wave-instruction, so every key row is one coalesced read.  Scores are 4-term partial dots summed
// over the key's lanes by xor shuffles.  Lane group kq takes keys kq, kq + KPW, ..., kU keys of the group
// per iteration (kU rows in flight per lane), and keeps its own softmax state (m, l, acc) in the exp2
// domain; the KPW groups are merged at the end by xor shuffles.  Each y row is read once, for its score
// and for the weighted sum.  A different fp32 summation order than gen_attn_ydecode (and tr_attn_fwd),
// the same softmax.  No LDS.
template <int LPK>
__global__ void gen_attn_ydecode4(const float* __restrict__ u, const float* __restrict__ yn, float* __restrict__ Yc,
                                  int E, int N, int H, int pos, float* __restrict__ O) {
    constexpr int KPW = 64 / LPK, kU = 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int task = blockIdx.x * (blockDim.x / 64) + wave;
    if (task >= N) return;
    const int E4 = E >> 2, c = lane % LPK, kq = lane / LPK;
    const bool act = c < E4;
    const floatx4* Y4 = reinterpret_cast<const floatx4*>(Yc + (int64_t)task * H * E);
    const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
    const floatx4 q = act ? reinterpret_cast<const floatx4*>(u + (int64_t)task * E)[c] : zero;
    const floatx4 yv = act ? reinterpret_cast<const floatx4*>(yn + (int64_t)task * E)[c] : zero;
    if (kq == 0 && act) reinterpret_cast<floatx4*>(Yc + (int64_t)task * H * E)[(int64_t)pos * E4 + c] = yv;
    const float scale = 1.4426950408889634f / sqrtf((float)E);  // scores in the exp2 domain
    float m = -INFINITY, l = 0.f;
    floatx4 acc = zero;
    for (int jb = 0; jb <= pos; jb += KPW * kU) {
        floatx4 v[kU];
        float sc[kU];
#pragma unroll
        for (int t = 0; t < kU; ++t) {
            const int j = jb + t * KPW + kq;
            v[t] = zero;
            if (act && j < pos) v[t] = Y4[(int64_t)j * E4 + c];
            else if (act && j == pos) v[t] = yv;
        }
        float mn = m;
#pragma unroll
        for (int t = 0; t < kU; ++t) {
            const int j = jb + t * KPW + kq;
            float d = fmaf(q[0], v[t][0], fmaf(q[1], v[t][1], fmaf(q[2], v[t][2], q[3] * v[t][3])));
#pragma unroll
            for (int x = 1; x < LPK; x <<= 1) d += __shfl_xor(d, x, 64);
            sc[t] = j <= pos ? d * scale : -INFINITY;
            mn = fmaxf(mn, sc[t]);
        }
        if (mn == -INFINITY) continue;  // no key of this group in the chunk yet
        const float corr = exp2f(m - mn);  // 0 while m = -inf
        l *= corr;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] *= corr;
#pragma unroll
        for (int t = 0; t < kU; ++t) {
            const float p = exp2f(sc[t] - mn);
            l += p;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = fmaf(p, v[t][r], acc[r]);
        }
        m = mn;
    }
    // merge the KPW groups' states (every group but kq = 0 may be empty: m = -inf, l = 0)
#pragma unroll
    for (int x = LPK; x < 64; x <<= 1) {
        const float mo = __shfl_xor(m, x, 64), lo = __shfl_xor(l, x, 64);
        floatx4 ao;
#pragma unroll
        for (int r = 0; r < 4; ++r) ao[r] = __shfl_xor(acc[r], x, 64);
        const float mm = fmaxf(m, mo);
        const float ca = m == -INFINITY ? 0.f : exp2f(m - mm), cb = mo == -INFINITY ? 0.f : exp2f(mo - mm);
        l = l * ca + lo * cb;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = acc[r] * ca + ao[r] * cb;
        m = mm;
    }
    if (kq == 0 && act) reinterpret_cast<floatx4*>(O + (int64_t)task * E)[c] = acc * (1.0f / l);
}
// the LPK it is built for: at least 4 lanes per key (16 keys per wave-instruction at the most)
using GenLpk = Widths<4, 8, 16, 32, 64>;

struct GenEnv {
    int N, H, A, sd, type, sample;
    int64_t first_task;
    double var;
    uint64_t seed, counter;
    const double* means;
    const double* uniforms;
    const double* noise;
    int32_t* actions_out;
    double* rewards_out;
    double* arm_value_out;
    float* logits_out;
    GenEnvAct env;  // all zero: the env is stepped with the selected action
};

// the token rows: the query [1_sd, 0_A, 0_sd, 0] at step 0 (eval_bandit.py: query state ones)
__global__ void gen_query_token(int N, int F, int sd, float* __restrict__ tok) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * F) return;
    tok[i] = (int)(i % F) < sd ? 1.f : 0.f;
}

// selection and env step of step h for every task (the fused kernel's draws, select_from_logits
// and reward arithmetic), the outputs, and the next token [1_sd, onehot(a), 1_sd, float(r)]
// (eval_bandit.py:83-86)
__global__ void gen_select_env(const float* __restrict__ lg, GenEnv g, int h, float* __restrict__ tok) {
    const int task = blockIdx.x * blockDim.x + threadIdx.x;
    if (task >= g.N) return;
    const int64_t gtask = g.first_task + task;
    const uint64_t ctr = g.counter + (uint64_t)h;
    double u = 0.0;
    if (g.sample) u = g.uniforms ? g.uniforms[(size_t)h * g.N + task] : philox_uniform(g.seed, ctr, gtask, DPT_STREAM_SELECT);
    const float* l = lg + (int64_t)task * g.A;
    const int a = select_from_logits(l, g.A, g.sample, 1.0f, u);
    // the arm the env is stepped with: the selected one, or a separate one (injected and clamped, or uniform
    // over the arms from its own Philox stream); `a` still goes into the records and the next token
    int ea = a;
    if (g.env.env_actions) ea = min(g.A - 1, max(0, g.env.env_actions[(size_t)h * g.N + task]));
    else if (g.env.random) ea = min(g.A - 1, (int)floor(philox_uniform(g.seed, ctr, gtask, DPT_STREAM_ENVACT) * g.A));
    const double mean = g.means[(int64_t)task * g.A + ea];
    const bool bern = (g.type & ~DPT_BANDIT_F32) == DPT_BANDIT_BERNOULLI;
    double dr;
    if (g.noise) dr = g.noise[(size_t)h * g.N + task];
    else if (bern) dr = philox_uniform(g.seed, ctr, gtask, DPT_STREAM_REWARD);
    else dr = philox_normal(g.seed, ctr, gtask, DPT_STREAM_REWARD);
    double r;
    if (bern) r = dr < mean ? 1.0 : 0.0;
    else if (g.type & DPT_BANDIT_F32)  // GPUBanditEnv's fp32 arithmetic, as bandit_step_kernel (dpt_env.hip)
        r = (double)__fadd_rn((float)mean, __fmul_rn((float)dr, (float)g.var));
    else r = gaussian_reward(mean, g.var, dr);
    const size_t o = (size_t)task * g.H + h;
    g.actions_out[o] = a;
    g.rewards_out[o] = r;
    g.arm_value_out[o] = mean;
    if (g.env.env_actions_out) g.env.env_actions_out[o] = ea;
    if (g.logits_out)
        for (int k = 0; k < g.A; ++k) g.logits_out[((size_t)h * g.N + task) * g.A + k] = l[k];
    const int F = 2 * g.sd + g.A + 1;
    float* t = tok + (int64_t)task * F;
    for (int k = 0; k < g.sd; ++k) t[k] = 1.f;
    for (int k = 0; k < g.A; ++k) t[g.sd + k] = k == a ? 1.f : 0.f;
    for (int k = 0; k < g.sd; ++k) t[g.sd + g.A + k] = 1.f;
    t[F - 1] = (float)r;
}

int64_t gen_rollout_workspace_numel(const TrDims& d, int N, int H) { return GenWs::make(d, N, H).total; }

int rollout_bandit_generic(const TrDims& d, const float* blob, const dpt_bandit_rollout_args& a, hipStream_t st,
                           const GenEnvAct* env) {
    if (int rc = train_dims_check(d)) return rc;
    if (a.A != d.A || d.F != 2 + a.A + 1 || a.H > d.npos || a.N < 1 || a.H < 1 ||
        ((a.type & ~DPT_BANDIT_F32) != DPT_BANDIT_GAUSSIAN && (a.type & ~DPT_BANDIT_F32) != DPT_BANDIT_BERNOULLI) ||
        a.kvcache == nullptr || a.means == nullptr ||
        a.actions_out == nullptr || a.rewards_out == nullptr || a.arm_value_out == nullptr) {
        set_error(DPT_EINVAL, "generic bandit rollout: A=%d (model %d), state_dim must be 1, H=%d (n_positions %d), type=%d",
                  a.A, d.A, a.H, d.npos, a.type);
        return DPT_EINVAL;
    }
    const int N = a.N, H = a.H, E = d.E, L = d.L;
    const TrBlob B = TrBlob::make(d);
    const GenWs W = GenWs::make(d, N, H);
    float* ws = a.kvcache;
    const int rows_per_block = kTrThreads / 64;
    const unsigned row_blocks = (N + rows_per_block - 1) / rows_per_block;
    // the float4 attention for E % 4 == 0 up to 256 (LPK lanes per key), else the scalar one
    using AttnKernel = void (*)(const float*, const float*, float*, int, int, int, int, float*);
    AttnKernel attn_k = gen_attn_ydecode;
    if (E % 4 == 0 && E <= 256)
        if (int rc = GenLpk::run("gen_attn_ydecode4", std::max(4, pow2_ceil(E / 4)),
                                 [&](auto lpk) { attn_k = gen_attn_ydecode4<decltype(lpk)::value>; }))
            return rc;
    // the scalar form's dynamic LDS (the float4 form: none)
    const size_t attn_lds = attn_k == gen_attn_ydecode ? sizeof(float) * rows_per_block * (size_t)(H + E) : 0;
    if (attn_lds > 160 * 1024) {
        set_error(DPT_EUNSUPPORTED, "generic bandit rollout: H=%d too long for the attention kernel", H);
        return DPT_EUNSUPPORTED;
    }
    if (attn_lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)attn_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_lds);
    GenEnv g{N, H, a.A, 1, a.type, a.sample, a.first_task, a.var, a.seed, a.counter, a.means, a.uniforms, a.noise,
             a.actions_out, a.rewards_out, a.arm_value_out, a.logits_out, env ? *env : GenEnvAct{nullptr, 0, nullptr}};
    // ln_2 on load where the column-split products have it (bit-identical to the separate LayerNorm)
    const bool ln_in = dec_ln_in(E);
    int bad = DPT_OK;  // a product with no kernel (dec_product): checked with the step's launches
    auto product = [&](int kind, const float* X, const float* Wt, const float* bias, const float* res, float* Y,
                       const float* aux = nullptr) {
        if (int rc = dec_product(E, kind, X, Wt, bias, res, N, Y, st, aux)) bad = rc;
    };
    float* x = ws + W.x;
    float* x2 = ws + W.x2;
    float* y = ws + W.y;
    float* stt = ws + W.st;
    float* qkv = ws + W.qkv;
    float* o = ws + W.o;
    float* hb = ws + W.h;
    const int64_t NE = (int64_t)N * E, cache = (int64_t)N * H * E;
    hipLaunchKernelGGL(gen_query_token, dim3(blocks_for((int64_t)N * d.F)), dim3(kTrThreads), 0, st, N, d.F, 1,
                       ws + W.tok);
    hipLaunchKernelGGL(gen_fold_kernel, dim3(blocks_for((int64_t)L * GenFold::size(E))), dim3(kTrThreads), 0, st, blob, d,
                       B, ws + W.fold);
    for (int h = 0; h < H; ++h) {
        hipLaunchKernelGGL(gen_embed, dim3(blocks_for(NE)), dim3(kTrThreads), 0, st, ws + W.tok, blob, d, B, N, h, x);
        for (int l = 0; l < L; ++l) {
            const TrLayer P = TrLayer::make(B.layers + l * d.layer_size(), E);
            layernorm(x, blob + P.ln1_g, blob + P.ln1_b, N, E, y, stt, st);
            // u = y G + g0, the folded attention over the y cache, c_proj on Wvp (GenFold)
            const float* F = ws + W.fold + l * GenFold::size(E);
            const float *G = F, *Wvp = F + (int64_t)E * E, *g0 = F + 2ll * E * E, *bvp = g0 + E;
            float* uq = qkv;
            product(kMmU, y, G, g0, nullptr, uq);
            hipLaunchKernelGGL(attn_k, dim3(row_blocks), dim3(kTrThreads), attn_lds, st, uq, y, ws + W.Y + l * cache, E,
                               N, H, h, o);
            product(kMmProj, o, Wvp, bvp, x, x2);
            if (!ln_in) layernorm(x2, blob + P.ln2_g, blob + P.ln2_b, N, E, y, stt, st);
            product(ln_in ? kMmLnFc : kMmFc, ln_in ? x2 : y, blob + P.fc_w, blob + P.fc_b, nullptr, hb,
                    ln_in ? blob + P.ln2_g : nullptr);
            product(kMmMp, hb, blob + P.mp_w, blob + P.mp_b, x2, x);
        }
        layernorm(x, blob + B.lnf_g, blob + B.lnf_b, N, E, y, stt, st);
        row_linear(y, blob + B.head_w, blob + B.head_b, N, E, d.A, ws + W.lg, st);
        hipLaunchKernelGGL(gen_select_env, dim3((N + 255) / 256), dim3(256), 0, st, ws + W.lg, g, h, ws + W.tok);
        if (bad) return bad;
        if (int rc = launched("generic bandit rollout step")) return rc;
    }
    return DPT_OK;
}

}  // namespace dpt
