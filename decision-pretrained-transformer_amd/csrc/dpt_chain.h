// The host glue the three fused rollout-and-train chains share (dpt_interactive.hip, dpt_explore.hip,
// dpt_interactive_mdp.hip): the 1-D launch geometry of their small kernels, the shape checks of a chunk,
// the flag and alignment checks of a step, the bandit rollout's arguments, and one "fit" (forward, loss,
// backward, optional accumulate).  What needs one home is defined in dpt_interactive.hip.
#pragma once

#include "dpt_common.h"

namespace dpt {

// the chains' element-wise kernels: one thread per element, kChainThreads per workgroup
constexpr int kChainThreads = 256;
inline int64_t chain_blocks(int64_t n) { return (n + kChainThreads - 1) / kChainThreads; }
inline dim3 chain_grid(int64_t n) { return dim3((unsigned)chain_blocks(n)); }

// The shape checks shared by the workspace queries and the steps: a chunk of N envs at window K >= min_K
// of a model without dropout (`no_dropout`: why, for the message); `env_check(d)` holds the caller's
// state_dim / action_dim lines.  Fills `run` = the desc with batch N, window K, flags 0.  Messages
// begin with `who`.
template <class EnvCheck>
int chain_check_shape(const dpt_train_desc* d, int32_t N, int32_t K, int32_t min_K, const char* who,
                      const char* no_dropout, EnvCheck env_check, dpt_train_desc& run) {
    DPT_REQUIRE(d != nullptr, "%s: null desc", who);
    DPT_REQUIRE(N >= 1, "%s: N=%d", who, N);
    DPT_REQUIRE(K >= min_K, "%s: K=%d (at least %d)", who, K, min_K);
    DPT_REQUIRE(K <= d->n_positions, "%s: K=%d exceeds n_positions=%d", who, K, d->n_positions);
    DPT_REQUIRE((int64_t)N * K <= (1ll << 26), "%s: N * K = %lld rows (use smaller chunks)", who, (long long)N * K);
    if (int rc = env_check(d)) return rc;
    DPT_REQUIRE(d->dropout == 0.0f, "%s: dropout=%g must be 0 (%s)", who, (double)d->dropout, no_dropout);
    run = *d;
    run.batch = N;
    run.window = K;
    run.reserved = 0;
    return DPT_OK;
}

// a step's flags (any outside `allowed` is an error) and its workspace's alignment; `who` = "... grad"
static inline int chain_check_call(const char* who, int32_t flags, int32_t allowed, const float* workspace) {
    DPT_REQUIRE((flags & ~allowed) == 0, "%s: unknown flags 0x%x", who, flags);
    DPT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: workspace not 16-byte aligned", who);
    return DPT_OK;
}

// The K - 1 sampled fp32-reward rollout steps of a bandit chain, from dpt_interactive_args or
// dpt_explore_args (the same field names): the records go to the caller's buffers, no logits.
template <class Args>
dpt_bandit_rollout_args chain_rollout_args(const Args& a, int32_t A, float* kvcache, double* arm_value) {
    dpt_bandit_rollout_args r{};
    r.N = a.N; r.H = a.K - 1; r.A = A; r.type = a.type | DPT_BANDIT_F32; r.sample = 1;
    r.first_task = a.first_task; r.var = a.var; r.seed = a.seed; r.counter = a.counter;
    r.means = a.means; r.uniforms = a.uniforms; r.noise = a.noise;
    r.kvcache = kvcache;
    r.actions_out = a.actions_out; r.rewards_out = a.rewards_out;
    r.arm_value_out = arm_value;
    return r;
}

// the buffers one fit runs on: the packed window, the training workspace, the logits and their gradient
struct ChainBufs {
    float *tokens, *train, *preds, *dpreds;
    int64_t nblob;
};

// One fit: the training forward of `blob` under `d`, the caller's loss launch (`loss()` reads preds and
// writes dpreds), the backward into `grad`, and with `add_to` the sum add_to += grad.
template <class Loss>
int chain_fit(const dpt_train_desc* d, const float* blob, const ChainBufs& b, float* grad, float* add_to, Loss loss,
              void* stream) {
    if (int rc = dpt_train_forward(d, blob, b.tokens, b.train, b.preds, stream)) return rc;
    if (int rc = loss()) return rc;
    if (int rc = dpt_train_backward(d, blob, b.tokens, b.train, b.dpreds, grad, stream)) return rc;
    return add_to ? ia_accumulate(add_to, grad, b.nblob, stream) : DPT_OK;
}

}  // namespace dpt
