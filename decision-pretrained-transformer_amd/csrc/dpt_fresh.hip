// The fresh-task generator (include/dpt_hip.h, "fresh-task training step"): the packed tokens and targets
// of a pretraining batch drawn from Philox where the training step consumes them, instead of gathered
// from a resident dataset by ts_pack_kernel (dpt_trainstep.hip).
//
// One workgroup per sample.  The first lanes draw the task (bandit: the means, the Dirichlet / point-mass
// behaviour policy; DarkRoom: the goal and the permutation from the caller's lists, the query) and leave
// it in LDS.  Neither rollin is adaptive, so the H steps are independent: the lanes take kFreshThreads
// steps at a time, each lane computing one step with the rollin kernels' own draws and arithmetic
// (dpt_rollin.h) into an LDS record, and then stride over the chunk's floats so that consecutive lanes
// store consecutive words.  The kernels read nothing but the goal / permutation lists, write the bytes the
// pack wrote (about 1 MB at batch 64, window 501, 5 arms) and allocate nothing.
#include "dpt_common.h"
#include "dpt_fresh.h"
#include "dpt_rollin.h"

namespace dpt {

constexpr int kFreshMaxDim = 255;  // a DarkRoom coordinate is recorded in one byte

// The task's means at counters [0, A), then the behaviour policy from counter A on and the rows: the shared
// pieces of dpt_fresh.h (fresh_bandit_policy; fresh_bandit_rows, which runs rollin_bandit_arm() and
// rollin_bandit_reward() of dpt_rollin.h once per step), the same code the linear bandit's 'uniform' rollin runs.
__global__ __launch_bounds__(kFreshThreads) void fresh_bandit_kernel(int A, int H, int type, double var,
                                                                     uint64_t seed, int64_t first_task,
                                                                     float* __restrict__ tokens,
                                                                     float* __restrict__ targets,
                                                                     double* __restrict__ means_out,
                                                                     double* __restrict__ probs_out,
                                                                     int32_t* __restrict__ opt_out) {
    __shared__ double s_means[kMaxA], s_e[kMaxA], s_probs[kMaxA];
    __shared__ int s_best;
    __shared__ int s_arm[kFreshThreads];
    __shared__ float s_r[kFreshThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t task = first_task + b;
    const int F = A + 3;  // [1 | onehot(arm) | 1 | r]
    if (tid < A) s_means[tid] = philox_uniform(seed, tid, task, DPT_STREAM_TASK);
    fresh_bandit_policy(A, seed, task, A, s_e, s_probs);
    if (tid < A) {
        if (means_out) means_out[(int64_t)b * A + tid] = s_means[tid];
        if (probs_out) probs_out[(int64_t)b * A + tid] = s_probs[tid];
    }
    if (tid == 0) {
        int best = 0;
        for (int k = 1; k < A; ++k)
            if (s_means[k] > s_means[best]) best = k;
        s_best = best;
        if (opt_out) opt_out[b] = best;
    }
    __syncthreads();
    float* tok = tokens + (int64_t)b * (1 + H) * F;
    if (tid < F) tok[tid] = tid == 0 ? 1.f : 0.f;  // the query token [1 | 0 ...]
    if (tid < A) targets[(int64_t)b * A + tid] = tid == s_best ? 1.f : 0.f;
    fresh_bandit_rows(A, H, type, var, seed, task, s_means, s_probs, s_arm, s_r, tok);
}

__global__ __launch_bounds__(kFreshThreads) void fresh_darkroom_kernel(const int32_t* __restrict__ goals,
                                                                       int n_goals,
                                                                       const int32_t* __restrict__ perms,
                                                                       int n_perms, int H, int dim, uint64_t seed,
                                                                       int64_t first_task,
                                                                       float* __restrict__ tokens,
                                                                       float* __restrict__ targets,
                                                                       int32_t* __restrict__ goal_out,
                                                                       int32_t* __restrict__ perm_out,
                                                                       int32_t* __restrict__ query_out,
                                                                       int32_t* __restrict__ opt_out) {
    __shared__ int32_t s_perm[kDarkroomA];
    __shared__ int s_task[5];             // goal x, y; query x, y; the expert action at the query
    __shared__ uint32_t s_rec[kFreshThreads];  // x | y << 8 | x' << 16 | y' << 24
    __shared__ uint32_t s_ar[kFreshThreads];   // a | r << 8
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t task = first_task + b;
    constexpr int F = kDarkroomF, A = kDarkroomA;
    const int32_t* pm = perms ? s_perm : nullptr;
    if (tid < A) {
        const int pi = perms ? philox_randint(seed, 0, task, DPT_STREAM_TASK, 1, n_perms) : 0;
        const int32_t v = perms ? perms[(int64_t)pi * A + tid] : tid;
        s_perm[tid] = v;
        if (perm_out) perm_out[(int64_t)b * A + tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        const int gi = philox_randint(seed, 0, task, DPT_STREAM_TASK, 0, n_goals);
        const int gx = goals[2 * (int64_t)gi], gy = goals[2 * (int64_t)gi + 1];
        int qx, qy;
        rollin_darkroom_query(seed, H, task, dim, qx, qy);
        const int opt = darkroom_opt(qx, qy, gx, gy, pm);
        s_task[0] = gx; s_task[1] = gy; s_task[2] = qx; s_task[3] = qy; s_task[4] = opt;
        if (goal_out) { goal_out[2 * (int64_t)b] = gx; goal_out[2 * (int64_t)b + 1] = gy; }
        if (query_out) { query_out[2 * (int64_t)b] = qx; query_out[2 * (int64_t)b + 1] = qy; }
        if (opt_out) opt_out[b] = opt;
    }
    __syncthreads();
    const int gx = s_task[0], gy = s_task[1];
    float* tok = tokens + (int64_t)b * (1 + H) * F;
    if (tid < F) tok[tid] = tid < 2 ? (float)s_task[2 + tid] : 0.f;  // the query token [query | 0 ...]
    // a permutation entry outside [0, 5) finds no expert action: index 5, no class, as the pack of such a dataset
    if (tid < A) targets[(int64_t)b * A + tid] = tid == s_task[4] ? 1.f : 0.f;
    for (int h0 = 0; h0 < H; h0 += kFreshThreads) {
        const int h = h0 + tid;
        if (h < H) {
            int x, y, a;
            rollin_darkroom_draw(seed, h, task, dim, x, y, a);
            uint32_t rec = (uint32_t)x | (uint32_t)y << 8;
            const int r = rollin_darkroom_step(x, y, a, pm, dim, gx, gy);
            s_rec[tid] = rec | (uint32_t)x << 16 | (uint32_t)y << 24;
            s_ar[tid] = (uint32_t)a | (uint32_t)r << 8;
        }
        __syncthreads();
        fresh_store_rows(tok + (int64_t)(1 + h0) * F, min(kFreshThreads, H - h0), F, [&](int row, int f) {
            const uint32_t rec = s_rec[row], ar = s_ar[row];
            if (f < 2) return (float)(rec >> (8 * f) & 255u);
            if (f < 2 + A) return (int)(ar & 255u) == f - 2 ? 1.f : 0.f;
            if (f < 4 + A) return (float)(rec >> (8 * (f - A)) & 255u);
            return (float)(ar >> 8);
        });
        __syncthreads();
    }
}

}  // namespace dpt

using namespace dpt;

extern "C" int dpt_fresh_batch(const dpt_train_desc* d, const dpt_fresh_args* a, int32_t batch, float* tokens,
                               float* targets, void* stream) {
    DPT_REQUIRE(d && a && tokens && targets, "fresh batch: null pointer");
    DPT_REQUIRE(batch >= 1 && batch <= d->batch, "fresh batch: batch=%d outside 1..desc.batch=%d", batch, d->batch);
    DPT_REQUIRE(a->H >= 0 && (int64_t)d->window == 1 + (int64_t)a->H, "fresh batch: desc.window=%d != 1 + H=%d",
                d->window, a->H);
    DPT_REQUIRE(a->dim >= 1, "fresh batch: dim=%d", a->dim);
    if (a->env == DPT_FRESH_BANDIT) {
        DPT_REQUIRE(d->state_dim == 1 && d->action_dim == a->dim,
                    "fresh batch: a bandit of %d arms needs desc state_dim 1, action_dim %d (got %d, %d)", a->dim,
                    a->dim, d->state_dim, d->action_dim);
        if (int rc = check_action_dim("fresh batch", a->dim)) return rc;
        DPT_REQUIRE(a->type == DPT_BANDIT_GAUSSIAN || a->type == DPT_BANDIT_BERNOULLI, "fresh batch: bandit type=%d",
                    a->type);
        hipLaunchKernelGGL(fresh_bandit_kernel, dim3(batch), dim3(kFreshThreads), 0, as_stream(stream), a->dim, a->H,
                           a->type, a->var, a->seed, a->first_task, tokens, targets, a->means_out, a->probs_out,
                           a->opt_action_out);
        return launched("fresh_bandit");
    }
    DPT_REQUIRE(a->env == DPT_FRESH_DARKROOM, "fresh batch: env=%d", a->env);
    DPT_REQUIRE(d->state_dim == 2 && d->action_dim == kDarkroomA,
                "fresh batch: DarkRoom needs desc state_dim 2, action_dim 5 (got %d, %d)", d->state_dim,
                d->action_dim);
    DPT_REQUIRE(a->goals && a->n_goals >= 1, "fresh batch: DarkRoom needs a goal list (n_goals=%d)", a->n_goals);
    DPT_REQUIRE(a->perms ? a->n_perms >= 1 : a->n_perms == 0, "fresh batch: n_perms=%d %s a permutation list",
                a->n_perms, a->perms ? "with" : "without");
    if (a->dim > kFreshMaxDim) {
        set_error(DPT_EUNSUPPORTED, "fresh batch: dim=%d above %d", a->dim, kFreshMaxDim);
        return DPT_EUNSUPPORTED;
    }
    hipLaunchKernelGGL(fresh_darkroom_kernel, dim3(batch), dim3(kFreshThreads), 0, as_stream(stream), a->goals,
                       a->n_goals, a->perms, a->n_perms, a->H, a->dim, a->seed, a->first_task, tokens, targets,
                       a->goal_out, a->perm_out, a->query_out, a->opt_action_out);
    return launched("fresh_darkroom");
}
