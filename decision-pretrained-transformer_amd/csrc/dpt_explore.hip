// The explorer/exploiter bandit training step of train_explorer_exploiter.py:102-192 (include/dpt_hip.h,
// "explorer/exploiter training step") for one chunk of envs: the explorer's K - 1 sampled rollout steps
// through the y-cache decode with the env stepped by a separate arm, the window packed once from the
// records, then for the exploiter and for the explorer in turn a full-width training forward, the
// cross-entropy of EVERY position and the backward, with the explorer's advantage weights taken from
// the exploiter's row losses in between -- one chain of launches on one stream, with no host
// synchronisation.  Nothing here allocates: every buffer is the caller's.
//
// Arithmetic: as dpt_interactive.hip -- fp64 per element from the fp32 logits, one rounding on the
// store; the loss is summed in a fixed order (the rows thread-strided in index order, then an LDS
// tree): repeated calls are bit-identical.  The weights are exp() of a difference of doubles.
#include <cmath>

#include "dpt_chain.h"

namespace dpt {

// ----------------------------------------------------------------------------- every-position cross-entropy
// One thread per row (b, t) of preds.  The target is tseq[b] or trow[row]; w = weights[row] or 1.
// rowloss[row] = lse(x) - x[target] (unweighted) and dpreds = scale w (softmax(x) - onehot(target)),
// stored as exact zeros when w == 0.  A target outside [0, A) reads nothing: zero loss, zero gradient.
__global__ __launch_bounds__(kChainThreads) void ex_ce_rows_kernel(const float* __restrict__ preds,
                                                                const int64_t* __restrict__ tseq,
                                                                const int32_t* __restrict__ trow,
                                                                const double* __restrict__ weights, int B, int T,
                                                                int A, double scale, double* __restrict__ rowloss,
                                                                float* __restrict__ dpreds) {
    const int64_t row = (int64_t)blockIdx.x * kChainThreads + threadIdx.x;
    if (row >= (int64_t)B * T) return;
    const int64_t tg = tseq ? tseq[row / T] : (int64_t)trow[row];
    float* dx = dpreds ? dpreds + row * A : nullptr;
    if (tg < 0 || tg >= A) {
        rowloss[row] = 0.0;
        if (dx)
            for (int k = 0; k < A; ++k) dx[k] = 0.f;
        return;
    }
    const double w = dx && weights ? weights[row] : 1.0;
    if (dx && w == 0.0) {  // the row loss alone
        for (int k = 0; k < A; ++k) dx[k] = 0.f;
        dx = nullptr;
    }
    rowloss[row] = ce_hard_row(preds + row * A, A, tg, scale * w, dx);
}

// ----------------------------------------------------------------------------- advantage weights
// One thread per (b, j): w = exp((rowloss[b][j+1] - rowloss[b][j]) inv_beta), 0 at j = T - 1.  With
// `actions` (B, T - 1) the explorer's per-row targets are written alongside: trow[b][j] = actions[b][j],
// -1 (no class) at j = T - 1.
__global__ __launch_bounds__(kChainThreads) void ex_weights_kernel(const double* __restrict__ rowloss, int B, int T,
                                                                double inv_beta, double* __restrict__ weights,
                                                                const int32_t* __restrict__ actions,
                                                                int32_t* __restrict__ trow) {
    const int64_t row = (int64_t)blockIdx.x * kChainThreads + threadIdx.x;
    if (row >= (int64_t)B * T) return;
    const int j = (int)(row % T);
    const int64_t b = row / T;
    const bool last = j == T - 1;
    weights[row] = last ? 0.0 : exp((rowloss[row + 1] - rowloss[row]) * inv_beta);
    if (trow) trow[row] = last ? -1 : actions[b * (T - 1) + j];
}

// workspace of dpt_explore_grad for N envs at window K (floats; every region 16-byte aligned)
struct ExWs {
    int64_t train, tokens, preds, dpreds, grad, rowloss, weights, trow, arm_value, rollout, total;
};

// `run` = the caller's desc with batch = N, window = K, flags 0
static int ex_ws(const dpt_train_desc* run, ExWs& w, int64_t* nblob_out) {
    int64_t nws = 0, nblob = 0, nroll = 0;
    if (int rc = dpt_train_workspace_numel(run, &nws)) return rc;
    if (int rc = dpt_train_blob_numel(run, &nblob)) return rc;
    const int64_t N = run->batch, K = run->window, A = run->action_dim, F = A + 3;
    if (int rc = dpt_rollout_bandit_generic_workspace_numel(run, (int32_t)N, (int32_t)(K - 1), &nroll)) return rc;
    w.train = 0;
    w.tokens = round4(nws);
    w.preds = w.tokens + round4(N * K * F);
    w.dpreds = w.preds + round4(N * K * A);
    w.grad = w.dpreds + round4(N * K * A);
    w.rowloss = w.grad + round4(nblob);               // (N, K) doubles
    w.weights = w.rowloss + round4(2 * N * K);        // (N, K) doubles
    w.trow = w.weights + round4(2 * N * K);           // (N, K) int32: the explorer's per-row targets
    w.arm_value = w.trow + round4(N * K);             // (N, K - 1) doubles, the rollout's arm_value_out
    w.rollout = w.arm_value + round4(2 * N * (K - 1));
    w.total = w.rollout + round4(nroll);
    if (nblob_out) *nblob_out = nblob;
    return DPT_OK;
}

// the interactive step's shape checks with K >= 2: the explorer's loss is a mean over K - 1 positions
static int ex_check_shape(const dpt_train_desc* d, int32_t N, int32_t K, dpt_train_desc& run) {
    return ia_check_shape(d, N, K, 2, "explore", run);
}

static int ex_weights(const double* rowloss, int32_t B, int32_t T, double inv_beta, double* weights,
                      const int32_t* actions, int32_t* trow, void* stream) {
    const int64_t rows = (int64_t)B * T;
    DPT_REQUIRE(chain_blocks(rows) < (1ll << 31), "explore weights: %lld rows", (long long)rows);
    hipLaunchKernelGGL(ex_weights_kernel, chain_grid(rows), dim3(kChainThreads), 0, as_stream(stream), rowloss, B, T,
                       inv_beta, weights, actions, trow);
    return launched("ex_weights");
}

}  // namespace dpt

using namespace dpt;

extern "C" {

int dpt_train_ce_rows(const float* preds, const int64_t* targets_seq, const int32_t* targets_row,
                      const double* weights, int32_t batch, int32_t window, int32_t A, double scale,
                      double* rowloss, float* dpreds, double* loss_acc, void* stream) {
    DPT_REQUIRE(preds && rowloss && loss_acc, "train ce rows: null pointer");
    DPT_REQUIRE((targets_seq != nullptr) != (targets_row != nullptr),
                "train ce rows: exactly one of targets_seq / targets_row must be given");
    DPT_REQUIRE(batch >= 1 && window >= 1 && A >= 1, "train ce rows: batch=%d window=%d A=%d", batch, window, A);
    if (int rc = check_action_dim("train ce rows", A)) return rc;
    const int64_t rows = (int64_t)batch * window;
    DPT_REQUIRE(chain_blocks(rows) < (1ll << 31), "train ce rows: %lld rows", (long long)rows);
    hipLaunchKernelGGL(ex_ce_rows_kernel, chain_grid(rows), dim3(kChainThreads), 0, as_stream(stream), preds, targets_seq,
                       targets_row, weights, batch, window, A, scale, rowloss, dpreds);
    ce_finish(rowloss, weights, rows, scale, loss_acc, as_stream(stream));
    return launched("ex_ce_rows");
}

int dpt_explore_weights(const double* rowloss, int32_t batch, int32_t window, double inv_beta, double* weights,
                        void* stream) {
    DPT_REQUIRE(rowloss && weights, "explore weights: null pointer");
    DPT_REQUIRE(batch >= 1 && window >= 1, "explore weights: batch=%d window=%d", batch, window);
    DPT_REQUIRE(std::isfinite(inv_beta), "explore weights: inv_beta=%g", inv_beta);
    return ex_weights(rowloss, batch, window, inv_beta, weights, nullptr, nullptr, stream);
}

int dpt_explore_workspace_numel(const dpt_train_desc* d, int32_t N, int32_t K, int64_t* numel) {
    DPT_REQUIRE(numel != nullptr, "explore workspace: null numel");
    dpt_train_desc run;
    if (int rc = ex_check_shape(d, N, K, run)) return rc;
    ExWs w;
    if (int rc = ex_ws(&run, w, nullptr)) return rc;
    *numel = w.total;
    return DPT_OK;
}

int dpt_explore_grad(const dpt_train_desc* d, const float* explorer_blob, const float* exploiter_blob,
                     const dpt_explore_args* a, void* stream) {
    DPT_REQUIRE(d && explorer_blob && exploiter_blob && a, "explore grad: null desc / blob / args");
    DPT_REQUIRE(explorer_blob != exploiter_blob, "explore grad: the explorer and the exploiter share one blob");
    DPT_REQUIRE(a->means && a->targets && a->workspace && a->dblob_explorer && a->dblob_exploiter &&
                    a->loss_explorer && a->loss_exploiter,
                "explore grad: null pointer");
    DPT_REQUIRE(a->dblob_explorer != a->dblob_exploiter, "explore grad: the two gradient blobs are one buffer");
    DPT_REQUIRE(a->loss_explorer != a->loss_exploiter, "explore grad: the two loss accumulators are one buffer");
    DPT_REQUIRE(a->actions_out && a->rewards_out && a->env_actions_out,
                "explore grad: null actions_out / env_actions_out / rewards_out");
    dpt_train_desc run;
    if (int rc = ex_check_shape(d, a->N, a->K, run)) return rc;
    DPT_REQUIRE(std::isfinite(a->beta) && a->beta > 0.0, "explore grad: beta=%g must be finite and > 0", a->beta);
    const int base = a->type & ~DPT_BANDIT_F32;
    DPT_REQUIRE(base == DPT_BANDIT_GAUSSIAN || base == DPT_BANDIT_BERNOULLI, "explore grad: bandit type %d", a->type);
    if (int rc = chain_check_call("explore grad", a->flags, DPT_EXPLORE_ACCUMULATE, a->workspace)) return rc;
    const bool accumulate = (a->flags & DPT_EXPLORE_ACCUMULATE) != 0;
    ExWs w;
    int64_t nblob = 0;
    if (int rc = ex_ws(&run, w, &nblob)) return rc;
    const int32_t N = a->N, K = a->K, A = run.action_dim;
    float* ws = a->workspace;
    const ChainBufs b{ws + w.tokens, ws + w.train, ws + w.preds, ws + w.dpreds, nblob};
    double* rowloss = reinterpret_cast<double*>(ws + w.rowloss);
    double* weights = reinterpret_cast<double*>(ws + w.weights);
    int32_t* trow = reinterpret_cast<int32_t*>(ws + w.trow);

    // the explorer's K - 1 steps: its action into the context, the env stepped by a separate arm
    const dpt_bandit_rollout_args r =
        chain_rollout_args(*a, A, ws + w.rollout, reinterpret_cast<double*>(ws + w.arm_value));
    if (int rc = dpt_rollout_bandit_generic_env(&run, explorer_blob, &r, a->env_actions, a->env_actions ? 0 : 1,
                                                a->env_actions_out, stream))
        return rc;
    if (int rc = dpt_interactive_pack(a->actions_out, a->rewards_out, N, K - 1, A, b.tokens, stream)) return rc;

    // each fit's gradient: its dblob itself, or workspace when it is added to the dblob
    auto fit = [&](const float* blob, float* dblob, auto loss) {
        return chain_fit(&run, blob, b, accumulate ? ws + w.grad : dblob, accumulate ? dblob : nullptr, loss, stream);
    };
    // the exploiter: row t of this one forward is its step-t last-position logits
    if (int rc = fit(exploiter_blob, a->dblob_exploiter, [&] {
            return dpt_train_ce_rows(b.preds, a->targets, nullptr, nullptr, N, K, A, a->scale_exploiter, rowloss,
                                     b.dpreds, a->loss_exploiter, stream);
        }))
        return rc;
    // the explorer: weights from the exploiter's row losses, targets = the recorded context actions
    if (int rc = ex_weights(rowloss, N, K, 1.0 / a->beta, weights, a->actions_out, trow, stream)) return rc;
    return fit(explorer_blob, a->dblob_explorer, [&] {
        return dpt_train_ce_rows(b.preds, nullptr, trow, weights, N, K, A, a->scale_explorer, rowloss, b.dpreds,
                                 a->loss_explorer, stream);
    });
}

}  // extern "C"
