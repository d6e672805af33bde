// The fresh-task generator of the linear bandit (include/dpt_hip.h, "fresh-task training step: the linear
// bandit"): the packed tokens and targets of a pretraining batch whose rollin is the reference's adaptive
// Thompson run (rollin_linear_bandit_vec: a per-arm Gaussian posterior, prior 0 / 1), or its i.i.d.
// 'uniform' rollin, drawn from Philox where the training step consumes them.
//
// One workgroup per sample.  The task (theta, then means = arms @ theta in fp64) goes to LDS.  Only the
// select -> reward -> update chain of the Thompson rollin is serial, and no draw depends on the state, so
// the steps are taken kLinChunk at a time:
//   * the normals of a chunk (A posterior draws and one reward draw per step: the log / sqrt / cospi cost)
//     are computed into one of two LDS buffers by waves 1 - 3 while wave 0 runs the chain of the chunk
//     before (the first chunk's by the whole block);
//   * wave 0 runs the chain, lane k holding arm k's posterior mean m, std s, reward sum S and count n in
//     registers: v = m + s g, the maximum by DPP inside each row of 16 lanes and one readlane per row, and
//     the arm as the first set bit of the ballot v == max (the lowest index among equal values).  Every
//     lane computes the reward and the update its arm would get (they do not depend on the arm chosen), so
//     the one fp64 division, S / n, runs beside the reduction, and lane a alone keeps its result (a
//     select).  The next step's normals are loaded a step ahead, and the posterior weight 1 - w(n) and
//     std s(n) come from a table over the count filled up front by the same operations: O(H) per task,
//     where rollout_policy_wave_kernel re-sums every arm pairwise at every step to match np.mean bit for bit;
//   * behind one barrier per chunk every lane strides over the chunk's floats so that consecutive lanes
//     store consecutive words.
// No global workspace, no allocation, no atomics; the kernels read the arm features alone.
#include "dpt_common.h"
#include "dpt_fresh.h"
#include "dpt_linucb.h"

namespace dpt {

constexpr int kLinChunk = 32;   // steps per chunk of the Thompson rollin: lane hh of wave 0 records step hh
constexpr int kLinTable = 1024; // counts 1 .. kLinTable have their posterior weight and std in LDS

// update_posterior_all (ctrl_bandit.py:218-226) with prior mean 0, prior variance 1 at count n >= 1:
// the weight on the empirical mean, 1 - w, and the posterior std
__device__ inline void lin_posterior(int n, double variance, double& omw, double& sd) {
    const double nn = (double)n;
    const double w = variance / (variance + nn * 1.0);
    omw = 1.0 - w;
    sd = sqrt(1.0 / (1.0 + nn / variance));
}

// the task of sample `b` by the whole block: theta (counters [0, d)) and means = arms @ theta into LDS, the
// label's index into *s_best, the optional outputs, the query row and the target row.  Ends behind a barrier.
__device__ inline void fresh_linear_task(int A, int d, int H, const double* __restrict__ arms, uint64_t seed,
                                         int64_t task, double* s_theta, double* s_means, int* s_best,
                                         float* __restrict__ tokens, float* __restrict__ targets,
                                         double* __restrict__ theta_out, double* __restrict__ means_out,
                                         int32_t* __restrict__ opt_out) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int F = A + 3;
    if (tid < d) {
        const double t = philox_normal(seed, tid, task, DPT_STREAM_TASK) / sqrt((double)d);
        s_theta[tid] = t;
        if (theta_out) theta_out[(int64_t)b * d + tid] = t;
    }
    __syncthreads();
    if (tid < A) {
        const double* x = arms + (int64_t)tid * d;
        double acc = x[0] * s_theta[0];  // multiply, then add, in index order
        for (int p = 1; p < d; ++p) acc = acc + x[p] * s_theta[p];
        s_means[tid] = acc;
        if (means_out) means_out[(int64_t)b * A + tid] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        int best = 0;
        for (int k = 1; k < A; ++k)
            if (s_means[k] > s_means[best]) best = k;
        *s_best = best;
        if (opt_out) opt_out[b] = best;
    }
    __syncthreads();
    float* tok = tokens + (int64_t)b * (1 + H) * F;
    if (tid < F) tok[tid] = tid == 0 ? 1.f : 0.f;  // the query token [1 | 0 ...]
    if (tid < A) targets[(int64_t)b * A + tid] = tid == *s_best ? 1.f : 0.f;
}

// x of the lane the DPP control names (every lane of a quad_perm / row_ror has a source)
template <int CTRL>
__device__ inline int lin_dpp(int x) {
    return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, true);
}

// one exchange of the row maximum
template <int CTRL>
__device__ inline double lin_max_stage(double v) {
    return fmax(v, __hiloint2double(lin_dpp<CTRL>(__double2hiint(v)), lin_dpp<CTRL>(__double2loint(v))));
}

__device__ inline double lin_readlane(double x, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), lane),
                            __builtin_amdgcn_readlane(__double2loint(x), lane));
}

// arm k's state in lane k of wave 0; nx_*: the posterior weight and std at count n + 1
struct LinArm {
    double m, s, S, nx_omw, nx_sd;
    int n;
};

// `rows` steps of the chain by wave 0 on the chunk's normals s_g (row hh: A posterior normals, the reward
// normal; row `rows` is read ahead and not used); lane hh returns step hh's arm and reward in rec_a / rec_r.
// The loop body is one basic block -- selects, a read-ahead that needs no bound, and, unless LONG, no
// slow path for counts beyond the table -- so that the scheduler interleaves the division with the reduction
// (behind any branch the compiler sinks the division to its use, after the arg-max).  LONG: H > kLinTable.
template <bool LONG>
__device__ inline void lin_chain(LinArm& st, int A, int rows, double mean_k, double var, double variance,
                                 const double* s_g, const double* s_omw, const double* s_sd, int& rec_a,
                                 float& rec_r) {
    const int tid = threadIdx.x, G = A + 1;
    const int col = min(tid, A);  // a lane without an arm reads the (finite) reward normal: 0 * g = 0
    double g = s_g[col], gr = s_g[A];
    for (int hh = 0; hh < rows; ++hh) {
        const double v = st.m + st.s * g;  // a lane without an arm: -inf + 0 * g
        // the update this lane would make were its arm the one pulled: it does not depend on the arg-max
        const double r_k = gaussian_reward(mean_k, var, gr);
        const double S_k = st.S + r_k;
        const double m_k = st.nx_omw * (S_k / (double)(st.n + 1));
        // the next step's normals, in flight during this step
        double g_next = s_g[(hh + 1) * G + col], gr_next = s_g[(hh + 1) * G + A];
        double vm = lin_max_stage<0xB1>(v);  // quad_perm [1, 0, 3, 2]
        vm = lin_max_stage<0x4E>(vm);        // quad_perm [2, 3, 0, 1]
        vm = lin_max_stage<0x124>(vm);       // row_ror:4
        vm = lin_max_stage<0x128>(vm);       // row_ror:8: every lane of a row of 16 holds the row's maximum
        const double vmax = fmax(lin_readlane(vm, 0), lin_readlane(vm, 16));  // lanes >= A hold -inf
        const unsigned long long eq = __ballot(v == vmax);
        const int a = eq ? __builtin_ctzll(eq) : 0;  // the first index of the maximum
        const float r_a = (float)lin_readlane(r_k, a);
        rec_a = tid == hh ? a : rec_a;
        rec_r = tid == hh ? r_a : rec_r;
        // lane a keeps its update, then every lane reloads the posterior at its next count (only lane a's moved)
        const bool pulled = tid == a;
        st.n = pulled ? st.n + 1 : st.n;
        st.S = pulled ? S_k : st.S;
        st.m = pulled ? m_k : st.m;
        st.s = pulled ? st.nx_sd : st.s;
        const int e = min(st.n, kLinTable - 1);  // not LONG: n <= H <= kLinTable, and count H + 1 is never used
        st.nx_omw = s_omw[e];
        st.nx_sd = s_sd[e];
        if (LONG && st.n >= kLinTable) lin_posterior(st.n + 1, variance, st.nx_omw, st.nx_sd);
        // an empty statement that needs the two normals in registers here: without it the compiler sinks
        // their loads to the top of the next iteration and the chain waits for LDS at every step
        asm volatile("" : "+v"(g_next), "+v"(gr_next));
        g = g_next;
        gr = gr_next;
    }
}

__global__ __launch_bounds__(kFreshThreads) void fresh_linear_thompson_kernel(
    int A, int d, int H, double var, const double* __restrict__ arms, uint64_t seed, int64_t first_task,
    float* __restrict__ tokens, float* __restrict__ targets, double* __restrict__ theta_out,
    double* __restrict__ means_out, int32_t* __restrict__ opt_out) {
    __shared__ double s_theta[kMaxD], s_means[kMaxA];
    __shared__ double s_g[2][(kLinChunk + 1) * (kMaxA + 1)];  // chunk c in buffer c & 1: its normals, the row read ahead
    __shared__ double s_omw[kLinTable], s_sd[kLinTable];      // entry n - 1: count n
    __shared__ int s_best;
    __shared__ int s_arm[2][kLinChunk];
    __shared__ float s_r[2][kLinChunk];
    const int tid = threadIdx.x;
    const int64_t task = first_task + blockIdx.x;
    const int F = A + 3, G = A + 1;
    const double variance = var * var;
    fresh_linear_task(A, d, H, arms, seed, task, s_theta, s_means, &s_best, tokens, targets, theta_out, means_out,
                      opt_out);
    for (int n = 1 + tid; n <= min(H, kLinTable); n += kFreshThreads) lin_posterior(n, variance, s_omw[n - 1], s_sd[n - 1]);
    // the normals of chunk c by `lanes` lanes, this one being number `lane` of them
    auto draw_chunk = [&](int c, int lane, int lanes) {
        const int h0 = c * kLinChunk, n = min(kLinChunk, H - h0) * G;
        for (int e = lane; e < n; e += lanes) {
            const int hh = e / G, j = e - hh * G;
            s_g[c & 1][e] = philox_normal(seed, (uint64_t)(h0 + hh), task,
                                          j < A ? DPT_STREAM_POLICY + j : DPT_STREAM_REWARD);
        }
    };
    const int chunks = (H + kLinChunk - 1) / kLinChunk;
    if (chunks > 0) draw_chunk(0, tid, kFreshThreads);
    __syncthreads();  // chunk 0's normals, the table and the means
    float* tok = tokens + (int64_t)blockIdx.x * (1 + H) * F;
    LinArm st{tid < A ? 0.0 : -INFINITY, tid < A ? 1.0 : 0.0, 0.0, s_omw[0], s_sd[0], 0};  // a lane without an arm never wins
    const double mean_k = tid < A ? s_means[tid] : 0.0;
    for (int c = 0; c < chunks; ++c) {
        const int rows = min(kLinChunk, H - c * kLinChunk);
        if (tid < 64) {
            int rec_a = 0;
            float rec_r = 0.f;
            if (H > kLinTable)
                lin_chain<true>(st, A, rows, mean_k, var, variance, s_g[c & 1], s_omw, s_sd, rec_a, rec_r);
            else
                lin_chain<false>(st, A, rows, mean_k, var, variance, s_g[c & 1], s_omw, s_sd, rec_a, rec_r);
            if (tid < rows) {
                s_arm[c & 1][tid] = rec_a;
                s_r[c & 1][tid] = rec_r;
            }
        } else if (c + 1 < chunks) {
            draw_chunk(c + 1, tid - 64, kFreshThreads - 64);
        }
        // One barrier per chunk.  Behind it: chunk c's records and chunk c + 1's normals are complete.  What
        // is written before the next one was last read before this one: buffer (c + 2) & 1 of s_g by the
        // chain of chunk c, and s_arm / s_r [(c + 1) & 1] by the stores of chunk c - 1, which every wave
        // finished before it entered this iteration.
        __syncthreads();
        fresh_store_bandit_rows(tok + (int64_t)(1 + c * kLinChunk) * F, rows, A, s_arm[c & 1], s_r[c & 1]);
    }
}

__global__ __launch_bounds__(kFreshThreads) void fresh_linear_uniform_kernel(
    int A, int d, int H, double var, const double* __restrict__ arms, uint64_t seed, int64_t first_task,
    float* __restrict__ tokens, float* __restrict__ targets, double* __restrict__ theta_out,
    double* __restrict__ means_out, double* __restrict__ probs_out, int32_t* __restrict__ opt_out) {
    __shared__ double s_theta[kMaxD], s_means[kMaxA], s_e[kMaxA], s_probs[kMaxA];
    __shared__ int s_best;
    __shared__ int s_arm[kFreshThreads];
    __shared__ float s_r[kFreshThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t task = first_task + b;
    fresh_linear_task(A, d, H, arms, seed, task, s_theta, s_means, &s_best, tokens, targets, theta_out, means_out,
                      opt_out);
    fresh_bandit_policy(A, seed, task, d, s_e, s_probs);  // the bandit's task counters, moved behind theta
    if (tid < A && probs_out) probs_out[(int64_t)b * A + tid] = s_probs[tid];
    fresh_bandit_rows(A, H, DPT_BANDIT_GAUSSIAN, var, seed, task, s_means, s_probs, s_arm, s_r,
                      tokens + (int64_t)b * (1 + H) * (A + 3));
}

}  // namespace dpt

using namespace dpt;

// every host check of the generator, before any launch: the step entry points (dpt_trainstep.hip) run it ahead
// of their own chain so that a bad argument is named, not a shape derived from it
int dpt::fresh_linear_check(const char* who, const dpt_train_desc* d, const dpt_fresh_linear_args* a, int32_t batch) {
    DPT_REQUIRE(d && a, "%s: null desc / args", who);
    DPT_REQUIRE(a->arms, "%s: null arms (the (dim, lin_d) fp64 arm features)", who);
    DPT_REQUIRE(batch >= 1 && batch <= d->batch, "%s: batch=%d outside 1..desc.batch=%d", who, batch, d->batch);
    DPT_REQUIRE(a->H >= 0, "%s: H=%d", who, a->H);
    DPT_REQUIRE((int64_t)d->window == 1 + (int64_t)a->H, "%s: desc.window=%d != 1 + H=%d", who, d->window, a->H);
    DPT_REQUIRE(a->dim >= 1, "%s: dim=%d arms", who, a->dim);
    DPT_REQUIRE(a->lin_d >= 1, "%s: lin_d=%d", who, a->lin_d);
    DPT_REQUIRE(d->state_dim == 1 && d->action_dim == a->dim,
                "%s: a bandit of %d arms needs desc state_dim 1, action_dim %d (got %d, %d)", who, a->dim, a->dim,
                d->state_dim, d->action_dim);
    DPT_REQUIRE(a->rollin == DPT_FRESH_LINEAR_THOMPSON || a->rollin == DPT_FRESH_LINEAR_UNIFORM, "%s: rollin=%d", who,
                a->rollin);
    DPT_REQUIRE(std::isfinite(a->var) && a->var >= 0.0, "%s: var=%g (a finite std >= 0)", who, a->var);
    DPT_REQUIRE(a->rollin != DPT_FRESH_LINEAR_THOMPSON || a->var > 0.0,
                "%s: var=0 with the Thompson rollin (the posterior divides by var^2)", who);
    if (int rc = check_action_dim(who, a->dim)) return rc;
    if (a->lin_d > kMaxD) {
        set_error(DPT_EUNSUPPORTED, "%s: lin_d=%d above %d", who, a->lin_d, kMaxD);
        return DPT_EUNSUPPORTED;
    }
    return DPT_OK;
}

extern "C" int dpt_fresh_linear_batch(const dpt_train_desc* d, const dpt_fresh_linear_args* a, int32_t batch,
                                      float* tokens, float* targets, void* stream) {
    DPT_REQUIRE(tokens && targets, "fresh linear batch: null tokens / targets");
    if (int rc = fresh_linear_check("fresh linear batch", d, a, batch)) return rc;
    if (a->rollin == DPT_FRESH_LINEAR_THOMPSON) {
        hipLaunchKernelGGL(fresh_linear_thompson_kernel, dim3(batch), dim3(kFreshThreads), 0, as_stream(stream),
                           a->dim, a->lin_d, a->H, a->var, a->arms, a->seed, a->first_task, tokens, targets,
                           a->theta_out, a->means_out, a->opt_action_out);
        return launched("fresh_linear_thompson");
    }
    hipLaunchKernelGGL(fresh_linear_uniform_kernel, dim3(batch), dim3(kFreshThreads), 0, as_stream(stream), a->dim,
                       a->lin_d, a->H, a->var, a->arms, a->seed, a->first_task, tokens, targets, a->theta_out,
                       a->means_out, a->probs_out, a->opt_action_out);
    return launched("fresh_linear_uniform");
}
