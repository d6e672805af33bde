// Window prefill on gfx950: Transformer.forward (models/net.py:41-60) for
// windows of T = 1 + C <= 128 tokens, all positions at once.
//
// One workgroup per sequence; each of its NW waves owns two 16-token blocks and
// runs the transposed-dataflow MFMA forward of dpt_mfma_fwd.h: token packing
// (net.py:42-54) + embed_transition + wpe, then per GPT-2 block ln_1 -> c_attn
// -> causal attention -> c_proj -> residual -> ln_2 -> c_fc -> gelu_new ->
// mlp.c_proj -> residual, then ln_f + pred_actions for the positions asked for
// (out_mode 0: the last one, test=True; out_mode 1: positions 1..C, test=False).
// NW = 4, 8, 16 waves cover windows of 128, 256, 512 tokens (16 waves: K and V
// of 512 tokens fill 140 KB of LDS, one workgroup per CU).  Longer windows go
// to window_decode_kernel (dpt_decode.hip).
//
// The same forward inside a step loop is the in-episode DarkRoom rollout
// (rollout_darkroom_episode_kernel, below): one launch runs a whole episode per env.
#include "dpt_darkroom_env.h"
#include "dpt_mfma_fwd.h"

namespace dpt {

// Model-level parameters in LDS after the per-layer blocks (offsets in floats).
struct PfTop {
    int lnf_g, lnf_b, head_w, head_b, emb_b, emb_w, total;
    __host__ __device__ static PfTop make(int L, int F, int A) {
        PfTop t;
        int o = L * PL::size;
        t.lnf_g = o; o += kE;
        t.lnf_b = o; o += kE;
        t.head_w = o; o += A * kE;  // transposed: [a][E]
        t.head_b = o; o += (A + 3) & ~3;
        t.emb_b = o; o += kE;
        t.emb_w = o; o += F * kE;
        t.total = o;
        return t;
    }
};

struct PrefillArgs {
    const float *query, *states, *actions, *next_states, *rewards;
    int N, C, out_mode;
    float* out;
    const float* frag;
};

// Feature f of token `tok` of sequence n (net.py:42-54): token 0 =
// [query, 0_A, 0_sd, 0], token 1+j = [s_j, a_j, s'_j, r_j].
__device__ inline float token_feature(const PrefillArgs& a, int sd, int A, int n, int tok, int f) {
    if (tok == 0) return f < sd ? a.query[(size_t)n * sd + f] : 0.f;
    const size_t j = (size_t)n * a.C + (tok - 1);
    if (f < sd) return a.states[j * sd + f];
    if (f < sd + A) return a.actions[j * A + (f - sd)];
    if (f < 2 * sd + A) return a.next_states[j * sd + (f - sd - A)];
    return a.rewards[j];
}

// ----------------------------------------------------------------------------- the shared window forward
// The pieces prefill_kernel and rollout_darkroom_episode_kernel are both made of.  Force-inlined: each
// kernel is compiled as if it held them itself.  A compile-time feature / action count (kF, kA > 0; the
// episode kernel's) unrolls the loop over it; 0 leaves the loop over the model's runtime count as it is.

// the model-level parameters into LDS (PfTop); the caller's barrier follows.  (nthreads unsigned, as
// blockDim.x is: with a signed stride the compiler unrolls these loops, 600 instructions a kernel.)
__device__ __forceinline__ void load_top_params(float* P, const PfTop& pt, const ModelView& M, int F, int A, int tid,
                                                unsigned nthreads) {
    for (int i = tid; i < kE; i += nthreads) {
        P[pt.lnf_g + i] = M.lnf_g[i];
        P[pt.lnf_b + i] = M.lnf_b[i];
        P[pt.emb_b + i] = M.emb_b[i];
    }
    for (int i = tid; i < kE * A; i += nthreads) P[pt.head_w + (i % A) * kE + i / A] = M.head_w[i];
    for (int i = tid; i < A; i += nthreads) P[pt.head_b + i] = M.head_b[i];
    for (int i = tid; i < F * kE; i += nthreads) P[pt.emb_w + i] = M.emb_w[i];
}

// embed_transition of one token for the lane's 8 columns: the bias, then the F features in order
// (feat(f) = feature f of the token)
template <int kF, class Feat>
__device__ __forceinline__ void embed_acc(const float* P, const PfTop& pt, int g, int F, Feat feat, floatx4& acc0,
                                          floatx4& acc1) {
    acc0 = ld4(P + pt.emb_b + 4 * g), acc1 = ld4(P + pt.emb_b + 16 + 4 * g);
    auto one = [&](int f) {
        const float v = feat(f);
        const floatx4 w0 = ld4(P + pt.emb_w + f * kE + 4 * g), w1 = ld4(P + pt.emb_w + f * kE + 16 + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            acc0[r] = fmaf(v, w0[r], acc0[r]);
            acc1[r] = fmaf(v, w1[r], acc1[r]);
        }
    };
    if constexpr (kF > 0) {
#pragma unroll
        for (int f = 0; f < kF; ++f) one(f);
    } else {
        for (int f = 0; f < F; ++f) one(f);
    }
}

// ln_f + pred_actions of one 16-token block: emit(act, logit) per action, the logit of the lane's token
// (column lane & 15) on every lane.  ln_f / head over every column keeps the permlane reductions uniform.
template <int kA, class Emit>
__device__ __forceinline__ void head_block(const float* P, const PfTop& pt, const float (&xj)[8], int A, Emit emit) {
    const int g = lane_id() >> 4;
    float xf[8];
    ln_cols(xj, xf, P + pt.lnf_g, P + pt.lnf_b);
    auto one = [&](int act) {
        const floatx4 w0 = ld4(P + pt.head_w + act * kE + 4 * g);
        const floatx4 w1 = ld4(P + pt.head_w + act * kE + 16 + 4 * g);
        float part = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            part = fmaf(xf[r], w0[r], part);
            part = fmaf(xf[4 + r], w1[r], part);
        }
        emit(act, sum_cols(part) + P[pt.head_b + act]);
    };
    if constexpr (kA > 0) {
#pragma unroll
        for (int act = 0; act < kA; ++act) one(act);
    } else {
        for (int act = 0; act < A; ++act) one(act);
    }
}

template <int NW>
__global__ void __launch_bounds__(NW * 64, (NW + 3) / 4)
prefill_kernel(ModelView M, PrefillArgs a) {
    __shared__ KVBuf<32 * NW> S;
    extern __shared__ float P[];
    const int n = blockIdx.x;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = M.n_layer, A = M.A, sd = M.sd, F = M.F;
    const int T = a.C + 1;
    const float scale = 0.17677669529663687f;  // 1/sqrt(head_dim = 32)
    const PfTop pt = PfTop::make(L, F, A);
    const FragSrc3 split0{__builtin_amdgcn_make_buffer_rsrc((void*)a.frag, (short)0, L * Frag3::bytes, 0x00020000), 0};
    load_layer_params(P, M, tid, blockDim.x);
    load_top_params(P, pt, M, F, A, tid, blockDim.x);
    __syncthreads();

    const int nqb = (T + 15) >> 4;
    int qb[2];
    const int nb = blocks_of_wave(wave, nqb, qb);

    // embeddings
    float x[2][8];
    {
        const int lane = lane_id(), g = lane >> 4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int k = 0; k < 8; ++k) x[j][k] = 0.f;
            const int tok = qb[j] * 16 + (lane & 15);
            if (j >= nb || tok >= T) continue;
            floatx4 acc0, acc1;
            embed_acc<0>(P, pt, g, F, [&](int f) { return token_feature(a, sd, A, n, tok, f); }, acc0, acc1);
            const floatx4 p0 = ld4(M.wpe + (size_t)tok * kE + 4 * g), p1 = ld4(M.wpe + (size_t)tok * kE + 16 + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                x[j][r] = acc0[r] + p0[r];
                x[j][4 + r] = acc1[r] + p1[r];
            }
        }
    }

    // (the layer loop is not one of the shared pieces: as a force-inlined function it compiles to other code
    // in the episode kernel, which then runs a K = 100 episode 1.6 % slower, past the round-to-round spread)
    for (int layer = 0; layer < L; ++layer) {
        const float* W = P + layer * PL::size;
        const FragSrc3 fs = split0.layer(layer);
        float q[2][8];
        {
            float xn[2][8];
            DPT_BLOCKS(nb, (ln_n<NB>(x, xn, W + PL::ln1_g, W + PL::ln1_b), u_proj3_n<NB>(W, fs, xn, q, M),
                            kv_from_y<NB>(S, qb, xn, M)));
        }
        bar_lds();
        if (nb > 0) {
            float o[2][8], l[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j >= nb) break;
                float m;
                attend(S, q[j], qb[j], 0, scale, m, l[j], o[j], M);
            }
            DPT_BLOCKS(nb, attn_proj3_ol<NB>(W, fs, o, l, x, M));
        }
        bar_lds();  // every read of this layer's K/V is done
        {
            float xn[2][8];
            DPT_BLOCKS(nb, (ln_n<NB>(x, xn, W + PL::ln2_g, W + PL::ln2_b), mlp3_n<NB>(W, fs, xn, x, M.mlp_ew, M.mlp_ex)));
        }
    }

    // ln_f + pred_actions for the positions asked for
    {
        const int lane = lane_id(), g = lane >> 4, c = lane & 15;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j >= nb) break;
            const int tok = qb[j] * 16 + c;
            const bool want = a.out_mode == 0 ? tok == T - 1 : (tok >= 1 && tok < T);
            head_block<0>(P, pt, x[j], A, [&](int act, float lg) {
                if (want && g == 0) {
                    if (a.out_mode == 0) a.out[(size_t)n * A + act] = lg;
                    else a.out[((size_t)n * a.C + (tok - 1)) * A + act] = lg;
                }
            });
        }
    }
}

constexpr int kPrefillMaxT = 512;

// The K/V buffer of the geometry that runs windows of up to t tokens (128, 256 or
// 512: prefill_kernel<t / 32>'s static LDS).  Not proportional to t: Vt pads each
// of its rows by 4 floats whatever the window.
constexpr size_t prefill_kv_bytes(int t) {
    return t == 128 ? sizeof(KVBuf<128>) : t == 256 ? sizeof(KVBuf<256>) : sizeof(KVBuf<512>);
}
// the geometry (its window: 128, 256 or 512 tokens) that runs a window of T tokens
constexpr int prefill_geometry(int T) { return T <= 128 ? 128 : T <= 256 ? 256 : 512; }

// Whether a `dyn`-byte parameter block fits in LDS next to that K/V buffer: the one
// test behind both prefill_max_window (what dpt_forward_window routes by) and the
// launch, so a window promised to the prefill is never rejected by it.
constexpr bool prefill_fits(size_t dyn, int t) { return dyn + prefill_kv_bytes(t) + 64 <= 160 * 1024; }

// Largest window the prefill takes for this model (the parameter block must
// fit in LDS next to the K/V buffer); 0 if none.
int prefill_max_window(const ModelView& M) {
    const size_t dyn = sizeof(float) * (size_t)PfTop::make(M.n_layer, M.F, M.A).total;
    for (int t = kPrefillMaxT; t >= 128; t /= 2)
        if (prefill_fits(dyn, t)) return t;
    return 0;
}

// ----------------------------------------------------------------------------- the episode rollout
// The in-episode DarkRoom rollout (include/dpt_hip.h, dpt_rollout_darkroom_episode) in one launch: one
// workgroup per env runs the K steps of the episode.  Step t embeds the window W_t (T = t + 1 tokens:
// the query state s_t at position 0, then the episode's own t transitions) from the records the
// workgroup keeps in LDS, runs the shared window forward over it (prefill_kernel's, the block count
// growing with t), reads the logits of position T - 1, and one thread selects, moves and appends to the
// records (darkroom_act, dpt_darkroom_env.h).  The model's parameter block is loaded once per launch,
// not per step; the records reach global memory once, after the last step.

constexpr int kEpGx = 0, kEpGy = 1, kEpRet = 2;  // EpLds::perm's tail

struct EpisodeArgs {
    int N, K, dim, sample;
    int64_t first_task;
    uint64_t seed, counter;
    const int32_t *goal, *perm;
    const double* uniforms;
    int32_t *states, *actions, *rewards, *targets;
    float* logits;
    int32_t* returns;
    const float* frag;
};

// The episode's LDS after the parameter block (byte offsets from P + PfTop::total, 16-byte aligned
// regions): the selection uniforms, the step's logits, the permutation with the goal and the return so
// far, the env's output pointers, and the records as bytes (coordinates below dim <= 255, actions below 5,
// rewards 0 / 1): 5 K bytes of records, 8 K of uniforms.
struct EpLds {
    int u, lg, perm, out, st, act, rew, tgt, total;
    __host__ __device__ static EpLds make(int K) {
        EpLds e;
        const int k16 = (K + 15) & ~15;
        int o = 0;
        e.u = o; o += 8 * k16;
        e.lg = o; o += 32;
        e.perm = o; o += 32;  // perm (5), then goal x, goal y, return
        e.out = o; o += 48;   // the five output pointers of this env (read back after the last step)
        e.st = o; o += 2 * k16;
        e.act = o; o += k16;
        e.rew = o; o += k16;
        e.tgt = o; o += k16;
        e.total = o;
        return e;
    }
};

template <int NW>
__global__ void __launch_bounds__(NW * 64, (NW + 3) / 4)
rollout_darkroom_episode_kernel(ModelView M, EpisodeArgs a) {
    __shared__ KVBuf<32 * NW> S;
    extern __shared__ float P[];
    const int n = blockIdx.x;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = M.n_layer, K = a.K;
    const float scale = 0.17677669529663687f;  // 1/sqrt(head_dim = 32)
    const PfTop pt = PfTop::make(L, kDarkroomF, kDarkroomA);
    const EpLds el = EpLds::make(K);
    unsigned char* R = reinterpret_cast<unsigned char*>(P + pt.total);
    double* u_ep = reinterpret_cast<double*>(R + el.u);
    float* lg_s = reinterpret_cast<float*>(R + el.lg);
    int32_t* perm_s = reinterpret_cast<int32_t*>(R + el.perm);
    int32_t* env_s = perm_s + kDarkroomA;  // goal x, goal y, the return so far
    int32_t** out_s = reinterpret_cast<int32_t**>(R + el.out);
    unsigned char *st = R + el.st, *ac = R + el.act, *rw = R + el.rew, *tg = R + el.tgt;
    const FragSrc3 split0{__builtin_amdgcn_make_buffer_rsrc((void*)a.frag, (short)0, L * Frag3::bytes, 0x00020000), 0};
    load_layer_params(P, M, tid, blockDim.x);
    load_top_params(P, pt, M, kDarkroomF, kDarkroomA, tid, blockDim.x);
    // the env: permutation, goal, s_0 = (0, 0) and its expert action.  What only the selecting thread
    // or the epilogue reads (goal, return, output pointers) waits in LDS, not in registers held across
    // the step loop.
    if (tid < kDarkroomA) perm_s[tid] = a.perm ? a.perm[(size_t)n * kDarkroomA + tid] : tid;
    // the episode's selection uniforms up front, one thread per step (off the serial select chain)
    if (a.sample)
        for (int t = tid; t < K - 1; t += blockDim.x)
            u_ep[t] = a.uniforms ? a.uniforms[(size_t)t * a.N + n]
                                 : philox_uniform(a.seed, a.counter + (uint64_t)t, a.first_task + n, DPT_STREAM_SELECT);
    if (tid == 0) {
        const int gx = a.goal[2 * (size_t)n], gy = a.goal[2 * (size_t)n + 1];
        env_s[kEpGx] = gx;
        env_s[kEpGy] = gy;
        env_s[kEpRet] = 0;
        int x0, y0;
        tg[0] = (unsigned char)darkroom_reset(x0, y0, gx, gy, a.perm ? a.perm + (size_t)n * kDarkroomA : nullptr);
        st[0] = (unsigned char)x0;
        st[1] = (unsigned char)y0;
        out_s[0] = a.states + (size_t)n * 2 * K;
        out_s[1] = a.actions + (size_t)n * (K - 1);
        out_s[2] = a.rewards + (size_t)n * (K - 1);
        out_s[3] = a.targets + (size_t)n * K;
        out_s[4] = a.returns ? a.returns + n : nullptr;
    }
    __syncthreads();

    for (int t = 0; t < K; ++t) {
        // The wave's blocks of this step from copies the compiler cannot see through: the block
        // assignment changes with the window, and values derived from a hoistable wave index would be
        // kept across the whole step loop in scalar registers that spill.
        int wv = wave;
        asm volatile("" : "+s"(wv));
        const int T = t + 1;
        const int nqb = (T + 15) >> 4;
        int qb[2];
        const int nb = blocks_of_wave(wv, nqb, qb);

        // embeddings of W_t from the records: token 0 = [s_t, 0_A, 0_sd, 0], token 1 + j =
        // [s_j, onehot(a_j), s_{j+1}, r_j] (prefill_kernel's accumulation order over the 10 features)
        float x[2][8];
        {
            const int lane = lane_id(), g = lane >> 4;
            // a zero made in this step: a constant's register is hoisted out of the step loop and kept
            // (spilled) across the layers
            float zero = 0.f;
            asm volatile("" : "+v"(zero));
            const __amdgpu_buffer_rsrc_t wpe_r =
                __builtin_amdgcn_make_buffer_rsrc((void*)M.wpe, (short)0, K * kE * (int)sizeof(float), 0x00020000);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int k = 0; k < 8; ++k) x[j][k] = zero;
                const int tok = qb[j] * 16 + (lane & 15);
                if (j >= nb || tok >= T) continue;
                const int sj = tok == 0 ? T - 1 : tok - 1;
                float v[kDarkroomF];
#pragma unroll
                for (int f = 0; f < kDarkroomF; ++f) v[f] = zero;
                v[0] = (float)st[2 * sj];
                v[1] = (float)st[2 * sj + 1];
                if (tok > 0) {
                    const int aj = ac[sj];
#pragma unroll
                    for (int k = 0; k < kDarkroomA; ++k) v[2 + k] = aj == k ? 1.f : zero;
                    v[2 + kDarkroomA] = (float)st[2 * tok];
                    v[3 + kDarkroomA] = (float)st[2 * tok + 1];
                    v[4 + kDarkroomA] = (float)rw[sj];
                }
                floatx4 acc0, acc1;
                embed_acc<kDarkroomF>(P, pt, g, kDarkroomF, [&](int f) { return v[f]; }, acc0, acc1);
                // (buffer loads at a 32-bit byte offset: a 64-bit per-lane address takes a zero half, a
                // constant register that is hoisted out of the step loop and spilled across the layers)
                const int po = (tok * kE + 4 * g) * 4;
                const floatx4 p0 = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(wpe_r, po, 0, 0));
                const floatx4 p1 = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(wpe_r, po + 64, 0, 0));
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    x[j][r] = acc0[r] + p0[r];
                    x[j][4 + r] = acc1[r] + p1[r];
                }
            }
        }

        for (int layer = 0; layer < L; ++layer) {
            const float* W = P + layer * PL::size;
            const FragSrc3 fs = split0.layer(layer);
            float q[2][8];
            {
                float xn[2][8];
                DPT_BLOCKS(nb, (ln_n<NB>(x, xn, W + PL::ln1_g, W + PL::ln1_b), u_proj3_n<NB>(W, fs, xn, q, M),
                                kv_from_y<NB>(S, qb, xn, M)));
            }
            bar_lds();
            if (nb > 0) {
                float o[2][8], l[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (j >= nb) break;
                    float m;
                    attend(S, q[j], qb[j], 0, scale, m, l[j], o[j], M);
                }
                DPT_BLOCKS(nb, attn_proj3_ol<NB>(W, fs, o, l, x, M));
            }
            bar_lds();  // every read of this layer's K/V is done
            {
                // the MLP's scales through copies made in this layer: the gelu constants derived from
                // them are otherwise computed once per launch and held in four registers across the
                // attention of every layer and step (a few scalar and vector instructions per layer)
                int ew = M.mlp_ew, ex = M.mlp_ex;
                asm volatile("" : "+s"(ew), "+s"(ex));
                float xn[2][8];
                DPT_BLOCKS(nb, (ln_n<NB>(x, xn, W + PL::ln2_g, W + PL::ln2_b), mlp3_n<NB>(W, fs, xn, x, ew, ex)));
            }
        }

        // ln_f + pred_actions of position T - 1, by the wave that owns its block
        {
            const int lane = lane_id(), g = lane >> 4, c = lane & 15;
            const int qlast = (T - 1) >> 4, clast = (T - 1) & 15;
            // the logits row's offset through a zero made here: the compiler otherwise addresses the
            // stores with the zero register of x's initial value, kept (spilled) across the layers
            int z0 = 0;
            asm volatile("" : "+v"(z0));
            float* lg_out = a.logits ? a.logits + ((size_t)n * K + (T - 1)) * kDarkroomA + z0 : nullptr;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j >= nb || qb[j] != qlast) continue;  // wave-uniform
                head_block<kDarkroomA>(P, pt, x[j], kDarkroomA, [&](int act, float lg) {
                    if (g == 0 && c == clast) {
                        lg_s[act] = lg;
                        if (lg_out) lg_out[act] = lg;
                    }
                });
            }
        }
        bar_lds();
        // one thread: the act rule (darkroom_act, mdp_act_kernel's call) appended to the records.  The K-th
        // action is never drawn.
        if (tid == 0 && T < K) {
            float lg[kDarkroomA];
#pragma unroll
            for (int k = 0; k < kDarkroomA; ++k) lg[k] = lg_s[k];
            const double u = a.sample ? u_ep[T - 1] : 0.0;
            int cur_x = st[2 * (T - 1)], cur_y = st[2 * (T - 1) + 1];
            const DarkroomStep step = darkroom_act(lg, a.sample, u, a.perm ? perm_s : nullptr, a.dim, env_s[kEpGx],
                                                   env_s[kEpGy], cur_x, cur_y);
            env_s[kEpRet] += step.reward;
            ac[T - 1] = (unsigned char)step.action;
            rw[T - 1] = (unsigned char)step.reward;
            st[2 * T] = (unsigned char)cur_x;
            st[2 * T + 1] = (unsigned char)cur_y;
            tg[T] = (unsigned char)step.next_opt;
        }
        bar_lds();
    }

    // the records, once (the loop's last barrier ordered them)
    int32_t *o_st = out_s[0], *o_ac = out_s[1], *o_rw = out_s[2], *o_tg = out_s[3], *o_ret = out_s[4];
    for (int i = tid; i < 2 * K; i += blockDim.x) o_st[i] = st[i];
    for (int i = tid; i < K - 1; i += blockDim.x) {
        o_ac[i] = ac[i];
        o_rw[i] = rw[i];
    }
    for (int i = tid; i < K; i += blockDim.x) o_tg[i] = tg[i];
    if (tid == 0 && o_ret) *o_ret = env_s[kEpRet];
}

// ----------------------------------------------------------------------------- the launches
// One workgroup of NW waves per sequence / env with `dyn` bytes of dynamic LDS, on the geometry that
// runs windows of T tokens; the callers have checked prefill_fits(dyn, prefill_geometry(T)).
template <int NW>
static auto kernel_of(const PrefillArgs&) { return prefill_kernel<NW>; }
template <int NW>
static auto kernel_of(const EpisodeArgs&) { return rollout_darkroom_episode_kernel<NW>; }

template <int NW, class Args>
static int launch_nw(const char* what, const ModelView& M, const Args& a, size_t dyn, hipStream_t st) {
    const auto kernel = kernel_of<NW>(a);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)dyn);
    hipLaunchKernelGGL(kernel, dim3(a.N), dim3(NW * 64), dyn, st, M, a);
    return check_hip(hipGetLastError(), what);
}
template <class Args>
static int launch_window(const char* what, int T, const ModelView& M, const Args& a, size_t dyn, hipStream_t st) {
    if (T <= 128) return launch_nw<4>(what, M, a, dyn, st);
    if (T <= 256) return launch_nw<8>(what, M, a, dyn, st);
    return launch_nw<16>(what, M, a, dyn, st);
}

int launch_prefill(const ModelView& M, const float* frag, const float* q, const float* cs, const float* ca,
                   const float* cn, const float* cr, int N, int C, int out_mode, float* out, hipStream_t st) {
    PrefillArgs a{q, cs, ca, cn, cr, N, C, out_mode, out, frag};
    const size_t dyn = sizeof(float) * (size_t)PfTop::make(M.n_layer, M.F, M.A).total;
    if (!prefill_fits(dyn, prefill_geometry(C + 1))) {
        set_error(DPT_EUNSUPPORTED, "prefill: parameter block does not fit in LDS");
        return DPT_EUNSUPPORTED;
    }
    return launch_window("prefill_kernel launch", C + 1, M, a, dyn, st);
}

// Bytes of dynamic LDS of an episode of K steps for a model of n_layer blocks, and whether they fit
// next to the K/V buffer of the geometry K runs on (a host-only test: dpt_rollout_darkroom_episode's
// unsupported-shape check, made before any launch).
static size_t episode_dyn_bytes(int n_layer, int K) {
    return sizeof(float) * (size_t)PfTop::make(n_layer, kDarkroomF, kDarkroomA).total + (size_t)EpLds::make(K).total;
}
bool darkroom_episode_fits(int n_layer, int K) {
    if (K > kPrefillMaxT) return false;
    return prefill_fits(episode_dyn_bytes(n_layer, K), prefill_geometry(K));
}

int launch_darkroom_episode(const ModelView& M, const float* frag, const dpt_darkroom_episode_args& h,
                            hipStream_t st) {
    EpisodeArgs a{h.N,     h.K,      h.dim,     h.sample,  h.first_task, h.seed,   h.counter, h.goal, h.perm,
                  h.uniforms, h.states, h.actions, h.rewards, h.targets,    h.logits, h.returns, frag};
    const size_t dyn = episode_dyn_bytes(M.n_layer, h.K);
    if (!prefill_fits(dyn, prefill_geometry(h.K))) {
        set_error(DPT_EUNSUPPORTED, "darkroom episode: parameter block and records (%zu bytes) do not fit in LDS", dyn);
        return DPT_EUNSUPPORTED;
    }
    return launch_window("rollout_darkroom_episode_kernel launch", h.K, M, a, dyn, st);
}

}  // namespace dpt
