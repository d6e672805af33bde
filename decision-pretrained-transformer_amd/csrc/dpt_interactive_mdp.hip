// The interactive (on-policy) DarkRoom training step (include/dpt_hip.h, "interactive DarkRoom (MDP)
// training step"): for each of the K steps of a chunk of envs the window packed from the records so far,
// the model's forward over that window (in an MDP the query state changes every step and sits at position
// 0, so there is no cached decode), on a loss-bearing step the last-position cross-entropy against the
// expert action and the backward, and one act step (selection, env move, next expert action) -- one chain
// of launches on one stream, with no host synchronisation.  Nothing here allocates: every buffer is the
// caller's.
//
// Arithmetic: the pack kernel copies and converts small integers to fp32 (exact); the act step is
// dpt_select_action's rule, dpt_darkroom_step's move and dpt_darkroom_opt_action's label in one thread
// per env (bit-equal to that chain); the cross-entropy and its fixed-order sum are dpt_train_ce_last's; the
// steps' gradients are added element by element in step order.  Repeated calls are bit-identical.
#include "dpt_chain.h"
#include "dpt_darkroom_env.h"

namespace dpt {

// ----------------------------------------------------------------------------- pack
// One thread per output float.  tokens (N, t + 1, 10): row 0 = [s_t | 0_5 | 0_2 | 0], row 1 + j =
// [s_j | onehot(a_j) | s_{j+1} | r_j] (models/net.py:42-54).  An action outside [0, 5) packs zeros.
__global__ __launch_bounds__(kChainThreads) void mdp_pack_kernel(const int32_t* __restrict__ states,
                                                               const int32_t* __restrict__ actions,
                                                               const int32_t* __restrict__ rewards, int N, int K,
                                                               int t, float* __restrict__ tokens) {
    const int T = t + 1;
    const int64_t e = (int64_t)blockIdx.x * kChainThreads + threadIdx.x;
    if (e >= (int64_t)N * T * kDarkroomF) return;
    const int f = (int)(e % kDarkroomF);
    const int64_t row = e / kDarkroomF;
    const int p = (int)(row % T);
    const int64_t i = row / T;
    const int32_t* s = states + i * K * 2;
    float val = 0.f;
    if (p == 0) {
        if (f < 2) val = (float)s[2 * t + f];
    } else {
        const int j = p - 1;
        const int64_t o = i * (K - 1) + j;
        if (f < 2) val = (float)s[2 * j + f];
        else if (f < 2 + kDarkroomA) val = actions[o] == f - 2 ? 1.f : 0.f;
        else if (f < 4 + kDarkroomA) val = (float)s[2 * (j + 1) + (f - 2 - kDarkroomA)];
        else val = (float)rewards[o];
    }
    tokens[e] = val;
}

// ----------------------------------------------------------------------------- reset
// s_0 = (0, 0) and target_0 = opt_action(s_0) of every env (and its int64 copy for dpt_train_ce_last)
__global__ __launch_bounds__(kChainThreads) void mdp_reset_kernel(const int32_t* __restrict__ goal,
                                                                const int32_t* __restrict__ perm, int N, int K,
                                                                int32_t* __restrict__ states,
                                                                int32_t* __restrict__ targets,
                                                                int64_t* __restrict__ target_next) {
    const int i = blockIdx.x * kChainThreads + threadIdx.x;
    if (i >= N) return;
    int x, y;
    const int tg = darkroom_reset(x, y, goal[2 * i], goal[2 * i + 1], perm ? perm + (int64_t)i * 5 : nullptr);
    states[(int64_t)i * K * 2] = x;
    states[(int64_t)i * K * 2 + 1] = y;
    targets[(int64_t)i * K] = tg;
    target_next[i] = tg;
}

// ----------------------------------------------------------------------------- act step
// One thread per env: select_kernel's draw and rule at temp 1 (dpt_env.hip; its 5-arm path, which is
// bit-identical to select_from_logits), darkroom_step_kernel's move and darkroom_opt_kernel's label.
__global__ __launch_bounds__(kChainThreads) void mdp_act_kernel(const float* __restrict__ logits, int N, int window,
                                                              int K, int t, int dim, int sample,
                                                              const double* __restrict__ uniforms, uint64_t seed,
                                                              uint64_t counter, int64_t first_task,
                                                              const int32_t* __restrict__ goal,
                                                              const int32_t* __restrict__ perm,
                                                              int32_t* __restrict__ states,
                                                              int32_t* __restrict__ actions,
                                                              int32_t* __restrict__ rewards,
                                                              int32_t* __restrict__ targets,
                                                              int64_t* __restrict__ target_next) {
    const int i = blockIdx.x * kChainThreads + threadIdx.x;
    if (i >= N) return;
    double u = 0.0;
    if (sample) u = uniforms ? uniforms[i] : philox_uniform(seed, counter, first_task + i, DPT_STREAM_SELECT);
    const float* lp = logits + ((int64_t)i * window + (window - 1)) * kDarkroomA;
    float lg[kDarkroomA];
#pragma unroll
    for (int k = 0; k < kDarkroomA; ++k) lg[k] = lp[k];
    int32_t* s = states + (int64_t)i * K * 2;
    int x = s[2 * t], y = s[2 * t + 1];
    const DarkroomStep step = darkroom_act(lg, sample, u, perm ? perm + (int64_t)i * 5 : nullptr, dim, goal[2 * i],
                                           goal[2 * i + 1], x, y);
    s[2 * (t + 1)] = x;
    s[2 * (t + 1) + 1] = y;
    actions[(int64_t)i * (K - 1) + t] = step.action;
    rewards[(int64_t)i * (K - 1) + t] = step.reward;
    targets[(int64_t)i * K + t + 1] = step.next_opt;
    if (target_next) target_next[i] = step.next_opt;
}

// workspace of dpt_interactive_mdp_grad for N envs over K steps (floats; every region 16-byte aligned)
struct MdpWs {
    int64_t train, tokens, preds, target, dpreds, grad, gstep, partial, total;
};

static bool mdp_has_loss(int mode) { return mode == DPT_MDP_LOSS_LAST || mode == DPT_MDP_LOSS_EVERY; }

// `run` = the caller's desc with batch = N, window = K, flags 0.  The training workspace is the larger of
// the two forms the chain runs at window K (a shorter window needs no more of either).
static int mdp_ws(const dpt_train_desc* run, int mode, MdpWs& w, int64_t* nblob_out) {
    int64_t nfwd = 0, nfit = 0, nblob = 0;
    dpt_train_desc d = *run;
    d.reserved = DPT_TRAIN_FORWARD_ONLY | DPT_TRAIN_LAST_ONLY;
    if (int rc = dpt_train_workspace_numel(&d, &nfwd)) return rc;
    if (int rc = dpt_train_blob_numel(run, &nblob)) return rc;
    const bool loss = mdp_has_loss(mode);
    if (loss) {
        d.reserved = DPT_TRAIN_LAST_LOSS;
        if (int rc = dpt_train_workspace_numel(&d, &nfit)) return rc;
    }
    const int64_t N = run->batch, K = run->window;
    w.train = 0;
    w.tokens = round4(nfwd > nfit ? nfwd : nfit);
    w.preds = w.tokens + round4(N * K * kDarkroomF);
    w.target = w.preds + round4(N * K * kDarkroomA);  // N int64
    w.dpreds = w.target + round4(2 * N);
    w.grad = w.dpreds + (loss ? round4(N * K * kDarkroomA) : 0);
    w.gstep = w.grad + (loss ? round4(nblob) : 0);
    w.partial = w.gstep + (mode == DPT_MDP_LOSS_EVERY ? round4(nblob) : 0);  // N doubles
    w.total = w.partial + (loss ? round4(2 * N) : 0);
    if (nblob_out) *nblob_out = nblob;
    return DPT_OK;
}

// the shape checks shared by the workspace query and the step; fills `run`
static int mdp_check_shape(const dpt_train_desc* d, int32_t N, int32_t K, int32_t mode, dpt_train_desc& run) {
    const char* who = "interactive mdp";
    auto darkroom = [who](const dpt_train_desc* d) -> int {
        if (d->state_dim == 2 && d->action_dim == kDarkroomA) return DPT_OK;
        set_error(DPT_EUNSUPPORTED, "%s: state_dim=%d action_dim=%d (DarkRoom has state_dim 2, action_dim 5)", who,
                  d->state_dim, d->action_dim);
        return DPT_EUNSUPPORTED;
    };
    if (int rc = chain_check_shape(d, N, K, 1, who, "the fused path draws no dropout masks", darkroom, run)) return rc;
    DPT_REQUIRE(mode == DPT_MDP_LOSS_NONE || mdp_has_loss(mode), "%s: unknown loss mode %d", who, mode);
    return DPT_OK;
}

}  // namespace dpt

using namespace dpt;

extern "C" {

int dpt_mdp_pack(const int32_t* states, const int32_t* actions, const int32_t* rewards, int32_t N, int32_t K,
                 int32_t t, float* tokens, void* stream) {
    DPT_REQUIRE(states && tokens && (t == 0 || (actions && rewards)), "mdp pack: null pointer");
    DPT_REQUIRE(N >= 1 && K >= 1 && t >= 0 && t < K, "mdp pack: N=%d K=%d t=%d", N, K, t);
    const int64_t total = (int64_t)N * (t + 1ll) * kDarkroomF;
    DPT_REQUIRE(chain_blocks(total) < (1ll << 31), "mdp pack: %lld elements", (long long)total);
    hipLaunchKernelGGL(mdp_pack_kernel, chain_grid(total), dim3(kChainThreads), 0, as_stream(stream), states, actions,
                       rewards, N, K, t, tokens);
    return launched("mdp_pack");
}

int dpt_darkroom_act_step(const float* logits, int32_t N, int32_t window, int32_t K, int32_t t, int32_t dim,
                          int32_t sample, const double* uniforms, uint64_t seed, uint64_t counter,
                          int64_t first_task, const int32_t* goal, const int32_t* perm, int32_t* states,
                          int32_t* actions, int32_t* rewards, int32_t* targets, int64_t* target_next,
                          void* stream) {
    DPT_REQUIRE(logits && goal && states && actions && rewards && targets, "darkroom act step: null pointer");
    DPT_REQUIRE(N >= 1 && window >= 1 && dim >= 1, "darkroom act step: N=%d window=%d dim=%d", N, window, dim);
    DPT_REQUIRE(K >= 2 && t >= 0 && t < K - 1, "darkroom act step: K=%d t=%d (0 <= t < K - 1)", K, t);
    DPT_REQUIRE(sample == 0 || sample == 1, "darkroom act step: sample=%d", sample);
    hipLaunchKernelGGL(mdp_act_kernel, chain_grid(N), dim3(kChainThreads), 0, as_stream(stream), logits, N, window, K, t,
                       dim, sample, uniforms, seed, counter, first_task, goal, perm, states, actions, rewards, targets,
                       target_next);
    return launched("mdp_act");
}

int dpt_interactive_mdp_workspace_numel(const dpt_train_desc* d, int32_t N, int32_t K, int32_t loss_mode,
                                        int64_t* numel) {
    DPT_REQUIRE(numel != nullptr, "interactive mdp workspace: null numel");
    dpt_train_desc run;
    if (int rc = mdp_check_shape(d, N, K, loss_mode, run)) return rc;
    MdpWs w;
    if (int rc = mdp_ws(&run, loss_mode, w, nullptr)) return rc;
    *numel = w.total;
    return DPT_OK;
}

int dpt_interactive_mdp_grad(const dpt_train_desc* d, const float* blob, const dpt_interactive_mdp_args* a,
                             void* stream) {
    DPT_REQUIRE(d && blob && a, "interactive mdp grad: null desc / blob / args");
    DPT_REQUIRE(a->goal && a->states_out && a->targets_out && a->workspace, "interactive mdp grad: null pointer");
    DPT_REQUIRE(a->K <= 1 || (a->actions_out && a->rewards_out),
                "interactive mdp grad: null actions_out / rewards_out");
    dpt_train_desc run;
    if (int rc = mdp_check_shape(d, a->N, a->K, a->loss_mode, run)) return rc;
    const bool loss = mdp_has_loss(a->loss_mode), every = a->loss_mode == DPT_MDP_LOSS_EVERY;
    DPT_REQUIRE(!loss || (a->dblob && a->loss_acc), "interactive mdp grad: null dblob / loss_acc in a loss mode");
    DPT_REQUIRE(a->dim >= 1, "interactive mdp grad: dim=%d", a->dim);
    DPT_REQUIRE(a->sample == 0 || a->sample == 1, "interactive mdp grad: sample=%d", a->sample);
    if (int rc = chain_check_call("interactive mdp grad", a->flags, DPT_INTERACTIVE_ACCUMULATE, a->workspace)) return rc;
    const bool accumulate = (a->flags & DPT_INTERACTIVE_ACCUMULATE) != 0;
    MdpWs w;
    int64_t nblob = 0;
    if (int rc = mdp_ws(&run, a->loss_mode, w, &nblob)) return rc;
    const int32_t N = a->N, K = a->K;
    hipStream_t st = as_stream(stream);
    float* ws = a->workspace;
    const ChainBufs b{ws + w.tokens, ws + w.train, ws + w.preds, ws + w.dpreds, nblob};
    int64_t* target = reinterpret_cast<int64_t*>(ws + w.target);
    double* partial = reinterpret_cast<double*>(ws + w.partial);
    // the chunk's gradient: dblob itself, or workspace when it is added to dblob at the end
    float* grad = !loss ? nullptr : accumulate ? ws + w.grad : a->dblob;
    hipLaunchKernelGGL(mdp_reset_kernel, chain_grid(N), dim3(kChainThreads), 0, st, a->goal, a->perm, N, K, a->states_out,
                       a->targets_out, target);
    if (int rc = launched("mdp_reset")) return rc;
    for (int32_t t = 0; t < K; ++t) {
        dpt_train_desc step = run;
        step.window = t + 1;
        if (int rc = dpt_mdp_pack(a->states_out, a->actions_out, a->rewards_out, N, K, t, b.tokens, stream))
            return rc;
        if (loss && (every || t == K - 1)) {
            step.reserved = DPT_TRAIN_LAST_LOSS;
            const bool first = every ? t == 0 : true;  // the step whose backward writes the chunk's gradient
            auto ce = [&] {
                return dpt_train_ce_last(b.preds, target, N, t + 1, kDarkroomA, a->scale, b.dpreds, partial, a->loss_acc,
                                         stream);
            };
            if (int rc = chain_fit(&step, blob, b, first ? grad : ws + w.gstep, first ? nullptr : grad, ce, stream))
                return rc;
        } else {
            step.reserved = DPT_TRAIN_FORWARD_ONLY | DPT_TRAIN_LAST_ONLY;
            if (int rc = dpt_train_forward(&step, blob, b.tokens, b.train, b.preds, stream)) return rc;
        }
        if (t < K - 1)
            if (int rc = dpt_darkroom_act_step(b.preds, N, t + 1, K, t, a->dim, a->sample,
                                               a->uniforms ? a->uniforms + (int64_t)t * N : nullptr, a->seed,
                                               a->counter + (uint64_t)t, a->first_task, a->goal, a->perm, a->states_out,
                                               a->actions_out, a->rewards_out, a->targets_out, target, stream))
                return rc;
    }
    if (loss && accumulate) return ia_accumulate(a->dblob, grad, nblob, stream);
    return DPT_OK;
}

}  // extern "C"
