// The interactive (on-policy) bandit training step of train_interactive.py:92-143 (include/dpt_hip.h,
// "interactive training step"): the K - 1 sampled rollout steps through dpt_rollout_bandit_generic
// with GPUBanditEnv's fp32 reward arithmetic, the window packed from the rollout's records, the
// training forward, the cross-entropy of the LAST position against the optimal arm, and the
// backward -- one chain of launches on one stream for a chunk of envs, with no host
// synchronisation.  Nothing here allocates: every buffer is the caller's.
//
// Arithmetic: the cross-entropy is evaluated in fp64 per element from the fp32 logits and rounded
// once on the store, as ts_ce_kernel (dpt_trainstep.hip) does; the loss is summed in a fixed order
// (the sequences thread-strided in index order, then an LDS tree): repeated calls are bit-identical.
// The pack kernel copies and converts each reward to fp32 once: bit-exact.
#include "dpt_chain.h"

namespace dpt {

// ----------------------------------------------------------------------------- pack
// One thread per output float.  tokens (N, Hc + 1, A + 3): row 0 = [1, 0_A, 0, 0] (the query state
// of a bandit is 1), row 1 + j = [1, onehot(a_j), 1, float(r_j)] (models/net.py:42-54 with state 1).
// An action outside [0, A) packs an all-zero one-hot.
__global__ __launch_bounds__(kChainThreads) void ia_pack_kernel(const int32_t* __restrict__ actions,
                                                             const double* __restrict__ rewards, int N, int Hc,
                                                             int A, float* __restrict__ tokens) {
    const int F = A + 3, T = Hc + 1;
    const int64_t e = (int64_t)blockIdx.x * kChainThreads + threadIdx.x;
    if (e >= (int64_t)N * T * F) return;
    const int f = (int)(e % F);
    const int64_t row = e / F;
    const int t = (int)(row % T);
    const int64_t i = row / T;
    float val = f == 0 ? 1.f : 0.f;
    if (t > 0 && f > 0) {
        const int64_t o = i * Hc + (t - 1);
        if (f <= A) val = actions[o] == f - 1 ? 1.f : 0.f;
        else if (f == A + 1) val = 1.f;
        else val = (float)rewards[o];
    }
    tokens[e] = val;
}

// ----------------------------------------------------------------------------- last-position cross-entropy
// One thread per row (b, t) of preds.  t < T - 1: the row of dpreds is zero.  t = T - 1:
// partial[b] = lse(x) - x[target_b] and dpreds = scale (softmax(x) - onehot(target_b)).  A target
// outside [0, A) reads nothing: zero loss, zero gradient.
__global__ __launch_bounds__(kChainThreads) void ia_ce_last_kernel(const float* __restrict__ preds,
                                                                const int64_t* __restrict__ targets, int B, int T,
                                                                int A, double scale, float* __restrict__ dpreds,
                                                                double* __restrict__ partial) {
    const int64_t row = (int64_t)blockIdx.x * kChainThreads + threadIdx.x;
    if (row >= (int64_t)B * T) return;
    const int t = (int)(row % T);
    const int64_t b = row / T;
    float* dx = dpreds ? dpreds + row * A : nullptr;
    if (t != T - 1) {
        if (dx)
            for (int k = 0; k < A; ++k) dx[k] = 0.f;
        return;
    }
    const int64_t tg = targets[b];
    if (tg < 0 || tg >= A) {
        partial[b] = 0.0;
        if (dx)
            for (int k = 0; k < A; ++k) dx[k] = 0.f;
        return;
    }
    partial[b] = ce_hard_row(preds + row * A, A, tg, scale, dx);
}

// dst += src, element by element (each element has one writer: the order is fixed)
__global__ __launch_bounds__(kChainThreads) void ia_accumulate_kernel(float* __restrict__ dst,
                                                                   const float* __restrict__ src, int64_t numel) {
    const int64_t i = (int64_t)blockIdx.x * kChainThreads + threadIdx.x;
    if (i < numel) dst[i] += src[i];
}

// workspace of dpt_interactive_grad for N envs at window K (floats; every region 16-byte aligned)
struct IaWs {
    int64_t train, tokens, preds, dpreds, grad, partial, arm_value, rollout, total;
};

// `run` = the caller's desc with batch = N, window = K, flags 0
static int ia_ws(const dpt_train_desc* run, IaWs& w, int64_t* nblob_out) {
    int64_t nws = 0, nblob = 0, nroll = 0;
    if (int rc = dpt_train_workspace_numel(run, &nws)) return rc;
    if (int rc = dpt_train_blob_numel(run, &nblob)) return rc;
    const int64_t N = run->batch, K = run->window, A = run->action_dim, F = A + 3;
    if (K > 1)
        if (int rc = dpt_rollout_bandit_generic_workspace_numel(run, (int32_t)N, (int32_t)(K - 1), &nroll)) return rc;
    w.train = 0;
    w.tokens = round4(nws);
    w.preds = w.tokens + round4(N * K * F);
    w.dpreds = w.preds + round4(N * K * A);
    w.grad = w.dpreds + round4(N * K * A);
    w.partial = w.grad + round4(nblob);              // N doubles
    w.arm_value = w.partial + round4(2 * N);         // (N, K - 1) doubles, the rollout's arm_value_out
    w.rollout = w.arm_value + round4(2 * N * (K - 1));
    w.total = w.rollout + round4(nroll);
    if (nblob_out) *nblob_out = nblob;
    return DPT_OK;
}

// the bandit chains' shape checks (dpt_chain.h); also the explorer/exploiter step's (dpt_explore.hip)
int ia_check_shape(const dpt_train_desc* d, int32_t N, int32_t K, int32_t min_K, const char* who,
                   dpt_train_desc& run) {
    auto bandit = [who](const dpt_train_desc* d) -> int {
        DPT_REQUIRE(d->state_dim == 1, "%s: state_dim=%d (bandits have state_dim 1)", who, d->state_dim);
        return check_action_dim(who, d->action_dim);
    };
    return chain_check_shape(d, N, K, min_K, who, "the cached decode has no dropout masks", bandit, run);
}

int ia_accumulate(float* dst, const float* src, int64_t numel, void* stream) {
    hipLaunchKernelGGL(ia_accumulate_kernel, chain_grid(numel), dim3(kChainThreads), 0, as_stream(stream), dst, src,
                       numel);
    return launched("ia_accumulate");
}

}  // namespace dpt

using namespace dpt;

extern "C" {

int dpt_interactive_pack(const int32_t* actions, const double* rewards, int32_t N, int32_t Hc, int32_t A,
                         float* tokens, void* stream) {
    DPT_REQUIRE(tokens && (Hc == 0 || (actions && rewards)), "interactive pack: null pointer");
    DPT_REQUIRE(N >= 1 && Hc >= 0 && A >= 1, "interactive pack: N=%d Hc=%d A=%d", N, Hc, A);
    const int64_t total = (int64_t)N * (Hc + 1ll) * (A + 3);
    DPT_REQUIRE(chain_blocks(total) < (1ll << 31), "interactive pack: %lld elements", (long long)total);
    hipLaunchKernelGGL(ia_pack_kernel, chain_grid(total), dim3(kChainThreads), 0, as_stream(stream), actions, rewards,
                       N, Hc, A, tokens);
    return launched("ia_pack");
}

int dpt_train_ce_last(const float* preds, const int64_t* targets, int32_t batch, int32_t window, int32_t A,
                      double scale, float* dpreds, double* partial, double* loss_acc, void* stream) {
    DPT_REQUIRE(preds && targets && partial && loss_acc, "train ce last: null pointer");
    DPT_REQUIRE(batch >= 1 && window >= 1 && A >= 1, "train ce last: batch=%d window=%d A=%d", batch, window, A);
    if (int rc = check_action_dim("train ce last", A)) return rc;
    const int64_t rows = (int64_t)batch * window;
    DPT_REQUIRE(chain_blocks(rows) < (1ll << 31), "train ce last: %lld rows", (long long)rows);
    hipLaunchKernelGGL(ia_ce_last_kernel, chain_grid(rows), dim3(kChainThreads), 0, as_stream(stream), preds, targets,
                       batch, window, A, scale, dpreds, partial);
    ce_finish(partial, nullptr, batch, scale, loss_acc, as_stream(stream));
    return launched("ia_ce_last");
}

int dpt_interactive_workspace_numel(const dpt_train_desc* d, int32_t N, int32_t K, int64_t* numel) {
    DPT_REQUIRE(numel != nullptr, "interactive workspace: null numel");
    dpt_train_desc run;
    if (int rc = ia_check_shape(d, N, K, 1, "interactive", run)) return rc;
    IaWs w;
    if (int rc = ia_ws(&run, w, nullptr)) return rc;
    *numel = w.total;
    return DPT_OK;
}

int dpt_interactive_grad(const dpt_train_desc* d, const float* blob, const dpt_interactive_args* a, void* stream) {
    DPT_REQUIRE(d && blob && a, "interactive grad: null desc / blob / args");
    DPT_REQUIRE(a->means && a->targets && a->workspace && a->dblob && a->loss_acc, "interactive grad: null pointer");
    DPT_REQUIRE(a->K <= 1 || (a->actions_out && a->rewards_out), "interactive grad: null actions_out / rewards_out");
    dpt_train_desc run;
    if (int rc = ia_check_shape(d, a->N, a->K, 1, "interactive", run)) return rc;
    const int base = a->type & ~DPT_BANDIT_F32;
    DPT_REQUIRE(base == DPT_BANDIT_GAUSSIAN || base == DPT_BANDIT_BERNOULLI, "interactive grad: bandit type %d",
                a->type);
    if (int rc = chain_check_call("interactive grad", a->flags, DPT_INTERACTIVE_ACCUMULATE | DPT_INTERACTIVE_FULL_WIDTH,
                                  a->workspace))
        return rc;
    const bool accumulate = (a->flags & DPT_INTERACTIVE_ACCUMULATE) != 0;
    IaWs w;
    int64_t nblob = 0;
    if (int rc = ia_ws(&run, w, &nblob)) return rc;
    const int32_t N = a->N, K = a->K, A = run.action_dim;
    float* ws = a->workspace;
    const ChainBufs b{ws + w.tokens, ws + w.train, ws + w.preds, ws + w.dpreds, nblob};
    dpt_train_desc fit = run;  // the training forward / backward: the loss reads the last position only
    if (!(a->flags & DPT_INTERACTIVE_FULL_WIDTH)) fit.reserved = DPT_TRAIN_LAST_LOSS;
    double* partial = reinterpret_cast<double*>(ws + w.partial);
    if (K > 1) {
        const dpt_bandit_rollout_args r =
            chain_rollout_args(*a, A, ws + w.rollout, reinterpret_cast<double*>(ws + w.arm_value));
        if (int rc = dpt_rollout_bandit_generic(&run, blob, &r, stream)) return rc;
    }
    if (int rc = dpt_interactive_pack(a->actions_out, a->rewards_out, N, K - 1, A, b.tokens, stream)) return rc;
    auto loss = [&] {
        return dpt_train_ce_last(b.preds, a->targets, N, K, A, a->scale, b.dpreds, partial, a->loss_acc, stream);
    };
    // the chunk's gradient: dblob itself, or workspace when it is added to dblob
    return chain_fit(&fit, blob, b, accumulate ? ws + w.grad : a->dblob, accumulate ? a->dblob : nullptr, loss, stream);
}

}  // extern "C"
