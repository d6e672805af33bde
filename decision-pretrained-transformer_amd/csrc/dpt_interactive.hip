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
#include "dpt_common.h"

namespace dpt {

constexpr int kIaThreads = 256;

// ----------------------------------------------------------------------------- pack
// One thread per output float.  tokens (N, Hc + 1, A + 3): row 0 = [1, 0_A, 0, 0] (the query state
// of a bandit is 1), row 1 + j = [1, onehot(a_j), 1, float(r_j)] (models/net.py:42-54 with state 1).
// An action outside [0, A) packs an all-zero one-hot.
__global__ __launch_bounds__(kIaThreads) void ia_pack_kernel(const int32_t* __restrict__ actions,
                                                             const double* __restrict__ rewards, int N, int Hc,
                                                             int A, float* __restrict__ tokens) {
    const int F = A + 3, T = Hc + 1;
    const int64_t e = (int64_t)blockIdx.x * kIaThreads + threadIdx.x;
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
__global__ __launch_bounds__(kIaThreads) void ia_ce_last_kernel(const float* __restrict__ preds,
                                                                const int64_t* __restrict__ targets, int B, int T,
                                                                int A, double scale, float* __restrict__ dpreds,
                                                                double* __restrict__ partial) {
    const int64_t row = (int64_t)blockIdx.x * kIaThreads + threadIdx.x;
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
__global__ __launch_bounds__(kIaThreads) void ia_accumulate_kernel(float* __restrict__ dst,
                                                                   const float* __restrict__ src, int64_t numel) {
    const int64_t i = (int64_t)blockIdx.x * kIaThreads + threadIdx.x;
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

// the shape checks shared by the workspace queries and the steps of the interactive (`who` =
// "interactive", min_K 1) and the explorer/exploiter (dpt_explore.hip) training steps; fills `run`
int ia_check_shape(const dpt_train_desc* d, int32_t N, int32_t K, int32_t min_K, const char* who,
                   dpt_train_desc& run) {
    DPT_REQUIRE(d != nullptr, "%s: null desc", who);
    DPT_REQUIRE(N >= 1, "%s: N=%d", who, N);
    DPT_REQUIRE(K >= min_K, "%s: K=%d (at least %d)", who, K, min_K);
    DPT_REQUIRE(K <= d->n_positions, "%s: K=%d exceeds n_positions=%d", who, K, d->n_positions);
    DPT_REQUIRE((int64_t)N * K <= (1ll << 26), "%s: N * K = %lld rows (use smaller chunks)", who, (long long)N * K);
    DPT_REQUIRE(d->state_dim == 1, "%s: state_dim=%d (bandits have state_dim 1)", who, d->state_dim);
    if (int rc = check_action_dim(who, d->action_dim)) return rc;
    DPT_REQUIRE(d->dropout == 0.0f, "%s: dropout=%g must be 0 (the cached decode has no dropout masks)", who,
                (double)d->dropout);
    run = *d;
    run.batch = N;
    run.window = K;
    run.reserved = 0;
    return DPT_OK;
}

// dst += src over `numel` floats, one launch on `stream`
int ia_accumulate(float* dst, const float* src, int64_t numel, void* stream) {
    const int64_t blocks = (numel + kIaThreads - 1) / kIaThreads;
    hipLaunchKernelGGL(ia_accumulate_kernel, dim3((unsigned)blocks), dim3(kIaThreads), 0, as_stream(stream), dst, src,
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
    const int64_t blocks = (total + kIaThreads - 1) / kIaThreads;
    DPT_REQUIRE(blocks < (1ll << 31), "interactive pack: %lld elements", (long long)total);
    hipLaunchKernelGGL(ia_pack_kernel, dim3((unsigned)blocks), dim3(kIaThreads), 0, as_stream(stream), actions,
                       rewards, N, Hc, A, tokens);
    return launched("ia_pack");
}

int dpt_train_ce_last(const float* preds, const int64_t* targets, int32_t batch, int32_t window, int32_t A,
                      double scale, float* dpreds, double* partial, double* loss_acc, void* stream) {
    DPT_REQUIRE(preds && targets && partial && loss_acc, "train ce last: null pointer");
    DPT_REQUIRE(batch >= 1 && window >= 1 && A >= 1, "train ce last: batch=%d window=%d A=%d", batch, window, A);
    if (int rc = check_action_dim("train ce last", A)) return rc;
    const int64_t rows = (int64_t)batch * window;
    const int64_t blocks = (rows + kIaThreads - 1) / kIaThreads;
    DPT_REQUIRE(blocks < (1ll << 31), "train ce last: %lld rows", (long long)rows);
    hipLaunchKernelGGL(ia_ce_last_kernel, dim3((unsigned)blocks), dim3(kIaThreads), 0, as_stream(stream), preds,
                       targets, batch, window, A, scale, dpreds, partial);
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
    DPT_REQUIRE((a->flags & ~(DPT_INTERACTIVE_ACCUMULATE | DPT_INTERACTIVE_FULL_WIDTH)) == 0,
                "interactive grad: unknown flags 0x%x", a->flags);
    const bool accumulate = (a->flags & DPT_INTERACTIVE_ACCUMULATE) != 0;
    DPT_REQUIRE((reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0,
                "interactive grad: workspace not 16-byte aligned");
    IaWs w;
    int64_t nblob = 0;
    if (int rc = ia_ws(&run, w, &nblob)) return rc;
    const int32_t N = a->N, K = a->K, A = run.action_dim;
    float* ws = a->workspace;
    float *tokens = ws + w.tokens, *preds = ws + w.preds, *dpreds = ws + w.dpreds;
    float* grad = accumulate ? ws + w.grad : a->dblob;
    dpt_train_desc fit = run;  // the training forward / backward: the loss reads the last position only
    if (!(a->flags & DPT_INTERACTIVE_FULL_WIDTH)) fit.reserved = DPT_TRAIN_LAST_LOSS;
    double* partial = reinterpret_cast<double*>(ws + w.partial);
    if (K > 1) {
        dpt_bandit_rollout_args r{};
        r.N = N; r.H = K - 1; r.A = A; r.type = a->type | DPT_BANDIT_F32; r.sample = 1;
        r.first_task = a->first_task; r.var = a->var; r.seed = a->seed; r.counter = a->counter;
        r.means = a->means; r.uniforms = a->uniforms; r.noise = a->noise;
        r.kvcache = ws + w.rollout;
        r.actions_out = a->actions_out; r.rewards_out = a->rewards_out;
        r.arm_value_out = reinterpret_cast<double*>(ws + w.arm_value);
        r.logits_out = nullptr;
        if (int rc = dpt_rollout_bandit_generic(&run, blob, &r, stream)) return rc;
    }
    if (int rc = dpt_interactive_pack(a->actions_out, a->rewards_out, N, K - 1, A, tokens, stream)) return rc;
    if (int rc = dpt_train_forward(&fit, blob, tokens, ws + w.train, preds, stream)) return rc;
    if (int rc = dpt_train_ce_last(preds, a->targets, N, K, A, a->scale, dpreds, partial, a->loss_acc, stream))
        return rc;
    if (int rc = dpt_train_backward(&fit, blob, tokens, ws + w.train, dpreds, grad, stream)) return rc;
    if (accumulate) return ia_accumulate(a->dblob, grad, nblob, stream);
    return DPT_OK;
}

}  // extern "C"
