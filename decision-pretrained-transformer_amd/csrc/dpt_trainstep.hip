// The training step around dpt_train_forward / dpt_train_backward (include/dpt_hip.h, "training
// step"): batch packing from a device-resident dataset, the summed cross-entropy of train.py:295-301
// with its gradient, AdamW over the whole packed blob, and the entry points that chain them on one
// stream without a host synchronisation; the fresh-task steps are the same chain with a generator
// (dpt_fresh.hip, dpt_fresh_linear.hip) in place of the pack.  Nothing here allocates: every buffer is the caller's.
//
// Arithmetic: the cross-entropy and the AdamW update are evaluated in fp64 per element from the
// fp32 inputs and rounded once on the store (both kernels are bound by their loads and stores, the
// fp64 work is free), so each stored value is the correctly rounded fp32 of the documented formula.
// The loss is summed in a fixed order (thread-strided rows, an LDS tree per sequence, the sequences
// in index order): repeated calls are bit-identical.
#include "dpt_common.h"

namespace dpt {

constexpr int kTsThreads = 256;

// ----------------------------------------------------------------------------- pack
// One thread per output float.  tokens (B, T, F): row 0 = [query | 0], row 1 + j = transition
// perm[b][j] (or j) of sample index[b] as [s | a | s' | r]; then targets (B, A).  A sample or
// permutation index outside its range reads nothing and packs zeros.
__global__ __launch_bounds__(kTsThreads) void ts_pack_kernel(dpt_train_data data, const int64_t* __restrict__ index,
                                                             const int64_t* __restrict__ perm, int B, int T, int sd,
                                                             int A, float* __restrict__ tokens,
                                                             float* __restrict__ targets) {
    const int F = 2 * sd + A + 1;
    const int64_t ntok = (int64_t)B * T * F;
    const int64_t e = (int64_t)blockIdx.x * kTsThreads + threadIdx.x;
    if (e >= ntok + (int64_t)B * A) return;
    const int64_t H = data.horizon;
    if (e >= ntok) {
        const int64_t k = e - ntok;
        const int b = (int)(k / A), a = (int)(k % A);
        const int64_t s = index[b];
        targets[k] = (s >= 0 && s < data.n) ? data.optimal_actions[s * A + a] : 0.f;
        return;
    }
    const int f = (int)(e % F);
    const int64_t row = e / F;
    const int t = (int)(row % T), b = (int)(row / T);
    const int64_t s = index[b];
    float val = 0.f;
    if (s >= 0 && s < data.n) {
        if (t == 0) {
            if (f < sd) val = data.query_states[s * sd + f];
        } else {
            const int64_t j = perm ? perm[(int64_t)b * H + (t - 1)] : (int64_t)(t - 1);
            if (j >= 0 && j < H) {
                const int64_t r = s * H + j;
                if (f < sd) val = data.context_states[r * sd + f];
                else if (f < sd + A) val = data.context_actions[r * A + (f - sd)];
                else if (f < 2 * sd + A) val = data.context_next_states[r * sd + (f - sd - A)];
                else val = data.context_rewards[r];
            }
        }
    }
    tokens[e] = val;
}

// ----------------------------------------------------------------------------- cross-entropy
// One workgroup per sequence b; its threads stride over positions 1..T-1.  Row loss =
// sum_k t_k (lse - x_k), d/dx_k = softmax_k sum(t) - t_k.  partial[b] = the sequence's loss.
__global__ __launch_bounds__(kTsThreads) void ts_ce_kernel(const float* __restrict__ preds,
                                                           const float* __restrict__ targets, int T, int A,
                                                           float* __restrict__ dpreds, double* __restrict__ partial) {
    __shared__ double red[kTsThreads];
    __shared__ double tg[kMaxA];  // the sequence's target row (the logits are re-read: no per-lane arrays)
    const int b = blockIdx.x;
    if ((int)threadIdx.x < A) tg[threadIdx.x] = (double)targets[(int64_t)b * A + threadIdx.x];
    __syncthreads();
    double tsum = 0.0;
    for (int k = 0; k < A; ++k) tsum += tg[k];
    double acc = 0.0;
    for (int t = threadIdx.x; t < T; t += kTsThreads) {
        const float* x = preds + ((int64_t)b * T + t) * A;
        float* dx = dpreds ? dpreds + ((int64_t)b * T + t) * A : nullptr;
        if (t == 0) {
            if (dx)
                for (int k = 0; k < A; ++k) dx[k] = 0.f;
            continue;
        }
        float mf = x[0];
        for (int k = 1; k < A; ++k) mf = fmaxf(mf, x[k]);
        const double m = (double)mf;
        double s = 0.0;
        for (int k = 0; k < A; ++k) s += exp((double)x[k] - m);
        const double lse = m + log(s);
        double row = 0.0;
        for (int k = 0; k < A; ++k) row += tg[k] * (lse - (double)x[k]);
        acc += row;
        if (dx)
            for (int k = 0; k < A; ++k) dx[k] = (float)(exp((double)x[k] - lse) * tsum - tg[k]);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kTsThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[b] = red[0];
}

// *acc += scale * sum_i w_i values[i] (dpt_common.h ce_finish), one workgroup: thread-strided sums, then
// the same LDS tree.  A weight or a scale of 1.0 is exact in fp64: the plain sum of ts_ce_kernel's partials.
__global__ __launch_bounds__(kTsThreads) void ce_finish_kernel(const double* __restrict__ values,
                                                               const double* __restrict__ weights, int64_t n,
                                                               double scale, double* __restrict__ acc) {
    __shared__ double red[kTsThreads];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kTsThreads) {
        const double w = weights ? weights[i] : 1.0;
        if (w != 0.0) s += w * values[i];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kTsThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *acc += scale * red[0];
}
void ce_finish(const double* values, const double* weights, int64_t n, double scale, double* acc, hipStream_t st) {
    hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(kTsThreads), 0, st, values, weights, n, scale, acc);
}

// ----------------------------------------------------------------------------- AdamW
// torch.optim.AdamW's documented update, constants folded on the host:
//   p *= 1 - lr wd;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2
//   p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
struct AdamConst {
    double decay, b1, b2, step_size, rsqrt_bc2, eps;
};

__device__ inline void adam_one(float& p, float g, float& m, float& v, const AdamConst& c) {
    const double gd = (double)g;
    const double md = c.b1 * (double)m + (1.0 - c.b1) * gd;
    const double vd = c.b2 * (double)v + (1.0 - c.b2) * gd * gd;
    const double pd = (double)p * c.decay - c.step_size * md / (sqrt(vd) * c.rsqrt_bc2 + c.eps);
    p = (float)pd;
    m = (float)md;
    v = (float)vd;
}

// n4 groups of four floats (16-byte accesses; 0 when a pointer is not 16-byte aligned), then the
// remaining numel - 4 n4 elements one per thread
__global__ __launch_bounds__(kTsThreads) void ts_adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                              float* __restrict__ m, float* __restrict__ v,
                                                              int64_t n4, int64_t numel, AdamConst c) {
    const int64_t i = (int64_t)blockIdx.x * kTsThreads + threadIdx.x;
    if (i < n4) {
        floatx4 pp = reinterpret_cast<floatx4*>(p)[i];
        const floatx4 gg = reinterpret_cast<const floatx4*>(g)[i];
        floatx4 mm = reinterpret_cast<floatx4*>(m)[i];
        floatx4 vv = reinterpret_cast<floatx4*>(v)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float a = pp[k], bm = mm[k], bv = vv[k];
            adam_one(a, gg[k], bm, bv, c);
            pp[k] = a; mm[k] = bm; vv[k] = bv;
        }
        reinterpret_cast<floatx4*>(p)[i] = pp;
        reinterpret_cast<floatx4*>(m)[i] = mm;
        reinterpret_cast<floatx4*>(v)[i] = vv;
        return;
    }
    const int64_t e = 4 * n4 + (i - n4);
    if (e < numel) adam_one(p[e], g[e], m[e], v[e], c);
}

// workspace of dpt_train_step for desc.batch sequences (floats; every region 16-byte aligned)
struct StepWs {
    int64_t train, tokens, targets, preds, dpreds, dblob, partial, total;
};

static int step_ws(const dpt_train_desc* d, StepWs& w) {
    int64_t nws = 0, nblob = 0;
    if (int rc = dpt_train_workspace_numel(d, &nws)) return rc;
    if (int rc = dpt_train_blob_numel(d, &nblob)) return rc;
    const int64_t B = d->batch, T = d->window, A = d->action_dim, F = 2 * (int64_t)d->state_dim + A + 1;
    w.train = 0;
    w.tokens = round4(nws);
    w.targets = w.tokens + round4(B * T * F);
    w.preds = w.targets + round4(B * A);
    w.dpreds = w.preds + round4(B * T * A);
    w.dblob = w.dpreds + round4(B * T * A);
    w.partial = w.dblob + round4(nblob);      // B doubles
    w.total = w.partial + round4(2 * B);
    return DPT_OK;
}

static int check_step_args(const dpt_train_desc* d, const dpt_train_data* data, const int64_t* index, int32_t batch) {
    DPT_REQUIRE(d && data && index, "null desc / data / index");
    DPT_REQUIRE(batch >= 1 && batch <= d->batch, "batch=%d outside 1..desc.batch=%d", batch, d->batch);
    DPT_REQUIRE(d->reserved == 0, "train step: desc flags must be 0 (got 0x%x)", d->reserved);
    return DPT_OK;
}

// What dpt_train_step (opt given) / dpt_train_eval_loss (opt NULL) and their fresh-task twins share: the
// workspace regions, the batch written into tokens / targets by `batch_into(run, tokens, targets)` (the
// pack from a dataset, or the generator), then forward -> cross-entropy [-> backward -> AdamW].  The
// workspace is laid out for desc.batch; a smaller batch uses a prefix of each region.
template <class Batch>
static int step_chain(const char* who, const dpt_train_desc* d, int32_t batch, const float* blob_in, float* blob,
                      float* m, float* v, const dpt_adamw_args* opt, float* ws, double* loss_acc, void* stream,
                      Batch batch_into) {
    StepWs w;
    if (int rc = step_ws(d, w)) return rc;
    int64_t nblob = 0;
    if (int rc = dpt_train_blob_numel(d, &nblob)) return rc;
    DPT_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: workspace not 16-byte aligned", who);
    dpt_train_desc run = *d;
    run.batch = batch;
    if (!opt) run.reserved = DPT_TRAIN_FORWARD_ONLY;  // every position's preds: never DPT_TRAIN_LAST_ONLY
    float *tokens = ws + w.tokens, *targets = ws + w.targets, *preds = ws + w.preds, *dpreds = ws + w.dpreds;
    double* partial = reinterpret_cast<double*>(ws + w.partial);
    if (int rc = batch_into(run, tokens, targets)) return rc;
    if (int rc = dpt_train_forward(&run, blob_in, tokens, ws + w.train, preds, stream)) return rc;
    if (int rc = dpt_train_ce_loss(preds, targets, batch, run.window, run.action_dim, opt ? dpreds : nullptr, partial,
                                   loss_acc, stream))
        return rc;
    if (!opt) return DPT_OK;
    if (int rc = dpt_train_backward(&run, blob, tokens, ws + w.train, dpreds, ws + w.dblob, stream)) return rc;
    return dpt_adamw_step(blob, ws + w.dblob, m, v, nblob, opt, stream);
}

// the checks of the fresh-task steps that precede the generator's own (dpt_fresh_batch)
static int check_fresh_args(const char* who, const dpt_train_desc* d, const dpt_fresh_args* a, int32_t batch) {
    DPT_REQUIRE(d && a, "%s: null desc / args", who);
    DPT_REQUIRE(batch >= 1 && batch <= d->batch, "%s: batch=%d outside 1..desc.batch=%d", who, batch, d->batch);
    DPT_REQUIRE(d->reserved == 0, "%s: desc flags must be 0 (got 0x%x)", who, d->reserved);
    DPT_REQUIRE((int64_t)d->window == 1 + (int64_t)a->H, "%s: desc.window=%d != 1 + H=%d", who, d->window, a->H);
    return check_action_dim(who, d->action_dim);
}

// the same for the linear bandit: every check of its generator (dpt_fresh_linear.hip), then the desc flags
static int check_fresh_linear_args(const char* who, const dpt_train_desc* d, const dpt_fresh_linear_args* a,
                                   int32_t batch) {
    if (int rc = fresh_linear_check(who, d, a, batch)) return rc;
    DPT_REQUIRE(d->reserved == 0, "%s: desc flags must be 0 (got 0x%x)", who, d->reserved);
    return DPT_OK;
}

}  // namespace dpt

using namespace dpt;

extern "C" {

int dpt_train_pack_batch(const dpt_train_desc* d, const dpt_train_data* data, const int64_t* index,
                         const int64_t* perm, int32_t batch, float* tokens, float* targets, void* stream) {
    DPT_REQUIRE(d && data && index && tokens && targets, "train pack: null pointer");
    DPT_REQUIRE(data->query_states && data->context_states && data->context_actions && data->context_next_states &&
                    data->context_rewards && data->optimal_actions,
                "train pack: null dataset array");
    DPT_REQUIRE(batch >= 1 && d->state_dim >= 1 && d->action_dim >= 1 && data->n >= 1 && data->horizon >= 0,
                "train pack: batch=%d sd=%d A=%d n=%lld horizon=%d", batch, d->state_dim, d->action_dim,
                (long long)data->n, data->horizon);
    DPT_REQUIRE((int64_t)d->window == 1 + (int64_t)data->horizon, "train pack: desc.window=%d != 1 + horizon=%d",
                d->window, data->horizon);
    const int64_t F = 2 * (int64_t)d->state_dim + d->action_dim + 1;
    const int64_t total = (int64_t)batch * d->window * F + (int64_t)batch * d->action_dim;
    DPT_REQUIRE((total + kTsThreads - 1) / kTsThreads < (1ll << 31), "train pack: %lld elements", (long long)total);
    hipLaunchKernelGGL(ts_pack_kernel, dim3((unsigned)((total + kTsThreads - 1) / kTsThreads)), dim3(kTsThreads), 0,
                       as_stream(stream), *data, index, perm, batch, d->window, d->state_dim, d->action_dim, tokens,
                       targets);
    return launched("ts_pack");
}

int dpt_train_ce_loss(const float* preds, const float* targets, int32_t batch, int32_t window, int32_t A,
                      float* dpreds, double* partial, double* loss_acc, void* stream) {
    DPT_REQUIRE(preds && targets && partial && loss_acc, "train ce: null pointer");
    DPT_REQUIRE(batch >= 1 && window >= 1 && A >= 1, "train ce: batch=%d window=%d A=%d", batch, window, A);
    if (int rc = check_action_dim("train ce", A)) return rc;
    hipLaunchKernelGGL(ts_ce_kernel, dim3(batch), dim3(kTsThreads), 0, as_stream(stream), preds, targets, window, A,
                       dpreds, partial);
    ce_finish(partial, nullptr, batch, 1.0, loss_acc, as_stream(stream));
    return launched("ts_ce");
}

int dpt_adamw_step(float* blob, const float* dblob, float* m, float* v, int64_t numel, const dpt_adamw_args* a,
                   void* stream) {
    DPT_REQUIRE(blob && dblob && m && v && a, "adamw: null pointer");
    DPT_REQUIRE(numel >= 0, "adamw: numel=%lld", (long long)numel);
    DPT_REQUIRE(a->step >= 1, "adamw: step=%lld (the first step is 1)", (long long)a->step);
    DPT_REQUIRE(a->lr >= 0.0 && a->eps >= 0.0 && a->weight_decay >= 0.0 && a->beta1 >= 0.0 && a->beta1 < 1.0 &&
                    a->beta2 >= 0.0 && a->beta2 < 1.0,
                "adamw: lr=%g betas=(%g, %g) eps=%g weight_decay=%g", a->lr, a->beta1, a->beta2, a->eps,
                a->weight_decay);
    if (numel == 0) return DPT_OK;
    const double bc1 = 1.0 - std::pow(a->beta1, (double)a->step);
    const double bc2 = 1.0 - std::pow(a->beta2, (double)a->step);
    const AdamConst c{1.0 - a->lr * a->weight_decay, a->beta1, a->beta2, a->lr / bc1, 1.0 / std::sqrt(bc2), a->eps};
    const bool aligned = ((reinterpret_cast<uintptr_t>(blob) | reinterpret_cast<uintptr_t>(dblob) |
                           reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    const int64_t n4 = aligned ? numel / 4 : 0;
    const int64_t threads = n4 + (numel - 4 * n4);
    const int64_t blocks = (threads + kTsThreads - 1) / kTsThreads;
    DPT_REQUIRE(blocks < (1ll << 31), "adamw: numel=%lld", (long long)numel);
    hipLaunchKernelGGL(ts_adamw_kernel, dim3((unsigned)blocks), dim3(kTsThreads), 0, as_stream(stream), blob, dblob,
                       m, v, n4, numel, c);
    return launched("ts_adamw");
}

int dpt_train_step_workspace_numel(const dpt_train_desc* d, int64_t* numel) {
    DPT_REQUIRE(d && numel, "train step workspace: null pointer");
    StepWs w;
    if (int rc = step_ws(d, w)) return rc;
    *numel = w.total;
    return DPT_OK;
}

int dpt_train_step(const dpt_train_desc* d, const dpt_train_data* data, const int64_t* index, const int64_t* perm,
                   int32_t batch, float* blob, float* m, float* v, const dpt_adamw_args* opt, float* ws,
                   double* loss_acc, void* stream) {
    if (int rc = check_step_args(d, data, index, batch)) return rc;
    DPT_REQUIRE(blob && m && v && opt && ws && loss_acc, "train step: null pointer");
    DPT_REQUIRE(opt->step >= 1, "train step: step=%lld (the first step is 1)", (long long)opt->step);
    if (int rc = check_action_dim("train step", d->action_dim)) return rc;
    DPT_REQUIRE((int64_t)d->window == 1 + (int64_t)data->horizon, "train step: desc.window=%d != 1 + horizon=%d",
                d->window, data->horizon);
    return step_chain("train step", d, batch, blob, blob, m, v, opt, ws, loss_acc, stream,
                      [&](const dpt_train_desc& run, float* tokens, float* targets) {
                          return dpt_train_pack_batch(&run, data, index, perm, batch, tokens, targets, stream);
                      });
}

int dpt_train_eval_loss(const dpt_train_desc* d, const dpt_train_data* data, const int64_t* index,
                        const int64_t* perm, int32_t batch, const float* blob, float* ws, double* loss_acc,
                        void* stream) {
    if (int rc = check_step_args(d, data, index, batch)) return rc;
    DPT_REQUIRE(blob && ws && loss_acc, "train eval loss: null pointer");
    if (int rc = check_action_dim("train eval loss", d->action_dim)) return rc;
    DPT_REQUIRE((int64_t)d->window == 1 + (int64_t)data->horizon, "train eval loss: desc.window=%d != 1 + horizon=%d",
                d->window, data->horizon);
    return step_chain("train eval loss", d, batch, blob, nullptr, nullptr, nullptr, nullptr, ws, loss_acc, stream,
                      [&](const dpt_train_desc& run, float* tokens, float* targets) {
                          return dpt_train_pack_batch(&run, data, index, perm, batch, tokens, targets, stream);
                      });
}

int dpt_fresh_step(const dpt_train_desc* d, const dpt_fresh_args* a, int32_t batch, float* blob, float* m, float* v,
                   const dpt_adamw_args* opt, float* ws, double* loss_acc, void* stream) {
    if (int rc = check_fresh_args("fresh step", d, a, batch)) return rc;
    DPT_REQUIRE(blob && m && v && opt && ws && loss_acc, "fresh step: null pointer");
    DPT_REQUIRE(opt->step >= 1, "fresh step: step=%lld (the first step is 1)", (long long)opt->step);
    return step_chain("fresh step", d, batch, blob, blob, m, v, opt, ws, loss_acc, stream,
                      [&](const dpt_train_desc& run, float* tokens, float* targets) {
                          return dpt_fresh_batch(&run, a, batch, tokens, targets, stream);
                      });
}

int dpt_fresh_eval_loss(const dpt_train_desc* d, const dpt_fresh_args* a, int32_t batch, const float* blob, float* ws,
                        double* loss_acc, void* stream) {
    if (int rc = check_fresh_args("fresh eval loss", d, a, batch)) return rc;
    DPT_REQUIRE(blob && ws && loss_acc, "fresh eval loss: null pointer");
    return step_chain("fresh eval loss", d, batch, blob, nullptr, nullptr, nullptr, nullptr, ws, loss_acc, stream,
                      [&](const dpt_train_desc& run, float* tokens, float* targets) {
                          return dpt_fresh_batch(&run, a, batch, tokens, targets, stream);
                      });
}

int dpt_fresh_linear_step(const dpt_train_desc* d, const dpt_fresh_linear_args* a, int32_t batch, float* blob,
                          float* m, float* v, const dpt_adamw_args* opt, float* ws, double* loss_acc, void* stream) {
    if (int rc = check_fresh_linear_args("fresh linear step", d, a, batch)) return rc;
    DPT_REQUIRE(blob && m && v && opt && ws && loss_acc, "fresh linear step: null pointer");
    DPT_REQUIRE(opt->step >= 1, "fresh linear step: step=%lld (the first step is 1)", (long long)opt->step);
    return step_chain("fresh linear step", d, batch, blob, blob, m, v, opt, ws, loss_acc, stream,
                      [&](const dpt_train_desc& run, float* tokens, float* targets) {
                          return dpt_fresh_linear_batch(&run, a, batch, tokens, targets, stream);
                      });
}

int dpt_fresh_linear_eval_loss(const dpt_train_desc* d, const dpt_fresh_linear_args* a, int32_t batch,
                               const float* blob, float* ws, double* loss_acc, void* stream) {
    if (int rc = check_fresh_linear_args("fresh linear eval loss", d, a, batch)) return rc;
    DPT_REQUIRE(blob && ws && loss_acc, "fresh linear eval loss: null pointer");
    return step_chain("fresh linear eval loss", d, batch, blob, nullptr, nullptr, nullptr, nullptr, ws, loss_acc,
                      stream, [&](const dpt_train_desc& run, float* tokens, float* targets) {
                          return dpt_fresh_linear_batch(&run, a, batch, tokens, targets, stream);
                      });
}

}  // extern "C"
