// Explore-then-exploit evaluation (include/dpt_hip.h, "explore-then-exploit evaluation"): what an
// exploiter recommends after every budget t = 0 .. H of someone's exploratory pulls, and what that
// recommendation is worth.
//
//   rc_curve_kernel     per row (task i, budget t) of logits (N, T, A): the greedy arm (first maximum),
//                       its mean, the expected mean under softmax(logits) and the optimal arm's
//                       probability.  A row sits on W = 2^ceil(log2 A) neighbouring lanes, one logit a
//                       lane, so a wave reads 64 / W whole rows as one contiguous run; the maximum, its
//                       first index and the sums are xor-butterflies over those W lanes.
//   rc_empirical_kernel EmpMeanPolicy(online=False) on every prefix of the records: one wave per task,
//                       arm a on lane a, the pulls applied in order (64 of them loaded at a time, one a
//                       lane, and handed round by lane index), the H + 1 answers stored 64 at a time.
//   dpt_exploit_eval    dpt_interactive_pack -> dpt_train_forward (forward-only, every position) ->
//                       rc_curve_kernel for one chunk of tasks: the bandit's query token is constant and
//                       sits at position 0 and attention is causal, so row t of ONE forward over the
//                       (1 + H)-token window is the model after t transitions.
//
// Arithmetic: fp64 per element from the fp32 logits, one rounding on the store.  Every reduction has a
// fixed order (the butterflies; the pulls in pull order): repeated calls are bit-identical.  Nothing
// here allocates.
#include "dpt_common.h"

namespace dpt {

constexpr int kRcThreads = 256;

// np.argmax's order on (value, index) pairs: a NaN beats every number, then the larger value, then the
// smaller index -- so the butterfly ends on the first maximum (the first NaN when there is one)
template <class V>
__device__ inline bool rc_better(V v1, int i1, V v2, int i2) {
    const bool n1 = v1 != v1, n2 = v2 != v2;
    if (n1 != n2) return n1;
    if (!n1 && v1 != v2) return v1 > v2;
    return i1 < i2;
}

template <int W, class V>
__device__ inline void rc_argmax(V& v, int& idx) {
#pragma unroll
    for (int off = W >> 1; off > 0; off >>= 1) {
        const V ov = __shfl_xor(v, off, W);
        const int oi = __shfl_xor(idx, off, W);
        if (rc_better(ov, oi, v, idx)) { v = ov; idx = oi; }
    }
}

template <int W>
__device__ inline double rc_sum(double v) {
#pragma unroll
    for (int off = W >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, W);
    return v;
}

// One row per W lanes, lane a of the group holding logit a (a < A <= W).  Lanes past A carry -inf with an
// index no valid lane has, e = 0 and mean 0; groups past the last row run the same code on those values
// and load / store nothing (no lane leaves before the shuffles).
template <int W>
__global__ __launch_bounds__(kRcThreads) void rc_curve_kernel(const float* __restrict__ logits,
                                                              const double* __restrict__ means,
                                                              const int64_t* __restrict__ targets, int64_t rows,
                                                              int T, int A, int32_t* __restrict__ greedy_arm,
                                                              double* __restrict__ greedy_value,
                                                              double* __restrict__ expected_value,
                                                              double* __restrict__ p_opt) {
    constexpr int kRows = kRcThreads / W;
    const int a = threadIdx.x % W;
    const int64_t row = (int64_t)blockIdx.x * kRows + threadIdx.x / W;
    const bool live = row < rows && a < A;
    const int64_t task = row < rows ? row / T : 0;
    float x = -INFINITY;
    double mu = 0.0;
    if (live) {
        x = logits[row * A + a];
        mu = means[task * A + a];
    }
    float best = x;
    int arm = a;
    rc_argmax<W>(best, arm);
    // softmax with the maximum subtracted (a NaN logit is the maximum: every probability is NaN, as numpy's)
    const double e = live ? exp((double)x - (double)best) : 0.0;
    const double p = e / rc_sum<W>(e);
    const double ev = rc_sum<W>(live ? p * mu : 0.0);
    const int64_t tg = p_opt && row < rows ? targets[task] : -1;
    const double po = rc_sum<W>(live && a == tg ? p : 0.0);  // at most one term
    const double gv = __shfl(mu, arm, W);
    if (row < rows && a == 0) {
        if (greedy_arm) greedy_arm[row] = arm;
        if (greedy_value) greedy_value[row] = gv;
        if (expected_value) expected_value[row] = ev;
        if (p_opt) p_opt[row] = po;
    }
}

template <int W>
static int rc_curve_launch(const float* logits, const double* means, const int64_t* targets, int64_t rows, int T,
                           int A, int32_t* greedy_arm, double* greedy_value, double* expected_value, double* p_opt,
                           hipStream_t st) {
    constexpr int kRows = kRcThreads / W;
    const int64_t blocks = (rows + kRows - 1) / kRows;
    DPT_REQUIRE(blocks < (1ll << 31), "recommend curve: %lld rows", (long long)rows);
    hipLaunchKernelGGL(rc_curve_kernel<W>, dim3((unsigned)blocks), dim3(kRcThreads), 0, st, logits, means, targets,
                       rows, T, A, greedy_arm, greedy_value, expected_value, p_opt);
    return launched("rc_curve");
}

// One wave per task.  sum / cnt of arm `lane` live in that lane; budget t's answer is taken BEFORE pull t
// is applied, so t = 0 sees an empty record (every b_mean 0: arm 0).  Chunk c loads pulls 64 c .. 64 c +
// 63 one a lane and keeps answer 64 c + j in lane j for one coalesced store.
__global__ __launch_bounds__(kWave) void rc_empirical_kernel(const int32_t* __restrict__ actions,
                                                             const double* __restrict__ rewards,
                                                             const double* __restrict__ means, int H, int A,
                                                             int32_t* __restrict__ emp_arm,
                                                             double* __restrict__ emp_value) {
    const int lane = threadIdx.x;
    const int64_t task = blockIdx.x;
    const bool live = lane < A;
    const double mu = live ? means[task * A + lane] : 0.0;
    double sum = 0.0, cnt = 0.0;
    for (int base = 0; base <= H; base += kWave) {
        int my_a = -1;
        double my_r = 0.0;
        if (base + lane < H) {
            my_a = actions[task * H + base + lane];
            my_r = rewards[task * H + base + lane];
        }
        int out_arm = 0;
        double out_val = 0.0;
        const int n = min(kWave, H + 1 - base);
        for (int j = 0; j < n; ++j) {
            double v = live ? sum / fmax(1.0, cnt) : -INFINITY;
            int arm = lane;
            rc_argmax<kWave>(v, arm);
            const double val = __shfl(mu, arm, kWave);
            if (lane == j) { out_arm = arm; out_val = val; }
            // pull base + j (past the record: my_a = -1, no lane; outside [0, A): no lane holds that arm)
            const int pa = __shfl(my_a, j, kWave);
            const double pr = __shfl(my_r, j, kWave);
            if (live && lane == pa) { sum += pr; cnt += 1.0; }
        }
        if (lane < n) {
            const int64_t o = task * (H + 1ll) + base + lane;
            if (emp_arm) emp_arm[o] = out_arm;
            if (emp_value) emp_value[o] = out_val;
        }
    }
}

// workspace of dpt_exploit_eval for N tasks at window K = H + 1 (floats; every region 16-byte aligned)
struct RcWs {
    int64_t train, tokens, preds, total;
};

static int rc_ws(const dpt_train_desc* run, RcWs& w) {
    int64_t nws = 0;
    if (int rc = dpt_train_workspace_numel(run, &nws)) return rc;
    const int64_t N = run->batch, K = run->window, A = run->action_dim;
    w.train = 0;
    w.tokens = round4(nws);
    w.preds = w.tokens + round4(N * K * (A + 3));
    w.total = w.preds + round4(N * K * A);
    return DPT_OK;
}

// the interactive step's shape checks at window H + 1; `run` = the forward-only desc of the chunk
static int rc_check_shape(const dpt_train_desc* d, int32_t N, int32_t H, dpt_train_desc& run) {
    DPT_REQUIRE(H >= 0 && H < INT32_MAX, "exploit eval: H=%d", H);
    if (int rc = ia_check_shape(d, N, H + 1, 1, "exploit eval", run)) return rc;
    run.reserved = DPT_TRAIN_FORWARD_ONLY;
    return DPT_OK;
}

}  // namespace dpt

using namespace dpt;

extern "C" {

int dpt_recommend_curve(const float* logits, const double* means, const int64_t* targets, int32_t N, int32_t T,
                        int32_t A, int32_t* greedy_arm, double* greedy_value, double* expected_value, double* p_opt,
                        void* stream) {
    DPT_REQUIRE(logits && means, "recommend curve: null logits / means");
    DPT_REQUIRE(targets || !p_opt, "recommend curve: p_opt needs targets");
    DPT_REQUIRE(N >= 1 && T >= 1 && A >= 1, "recommend curve: N=%d T=%d A=%d", N, T, A);
    if (int rc = check_action_dim("recommend curve", A)) return rc;
    const int64_t rows = (int64_t)N * T;
    hipStream_t st = as_stream(stream);
#define RC_CASE(W) \
    if (A <= W) return rc_curve_launch<W>(logits, means, targets, rows, T, A, greedy_arm, greedy_value, \
                                          expected_value, p_opt, st)
    RC_CASE(1);
    RC_CASE(2);
    RC_CASE(4);
    RC_CASE(8);
    RC_CASE(16);
    RC_CASE(32);
#undef RC_CASE
    return DPT_EINVAL;  // not reached: A <= kMaxA = 32
}

int dpt_empirical_recommend(const int32_t* actions, const double* rewards, const double* means, int32_t N,
                            int32_t H, int32_t A, int32_t* emp_arm, double* emp_value, void* stream) {
    DPT_REQUIRE(means && (H == 0 || (actions && rewards)), "empirical recommend: null pointer");
    DPT_REQUIRE(N >= 1 && H >= 0 && H < INT32_MAX && A >= 1, "empirical recommend: N=%d H=%d A=%d", N, H, A);
    if (int rc = check_action_dim("empirical recommend", A)) return rc;
    hipLaunchKernelGGL(rc_empirical_kernel, dim3((unsigned)N), dim3(kWave), 0, as_stream(stream), actions, rewards,
                       means, H, A, emp_arm, emp_value);
    return launched("rc_empirical");
}

int dpt_exploit_eval_workspace_numel(const dpt_train_desc* d, int32_t N, int32_t H, int64_t* numel) {
    DPT_REQUIRE(numel != nullptr, "exploit eval workspace: null numel");
    dpt_train_desc run;
    if (int rc = rc_check_shape(d, N, H, run)) return rc;
    RcWs w;
    if (int rc = rc_ws(&run, w)) return rc;
    *numel = w.total;
    return DPT_OK;
}

int dpt_exploit_eval(const dpt_train_desc* d, const float* blob, const dpt_exploit_eval_args* a, void* stream) {
    DPT_REQUIRE(d && blob && a, "exploit eval: null desc / blob / args");
    DPT_REQUIRE(a->means && a->workspace, "exploit eval: null means / workspace");
    DPT_REQUIRE(a->targets || !a->p_opt, "exploit eval: p_opt needs targets");
    DPT_REQUIRE(a->H <= 0 || (a->actions && a->rewards), "exploit eval: null actions / rewards");
    DPT_REQUIRE(a->flags == 0 && a->reserved == 0, "exploit eval: unknown flags 0x%x / reserved 0x%x", a->flags,
                a->reserved);
    dpt_train_desc run;
    if (int rc = rc_check_shape(d, a->N, a->H, run)) return rc;
    DPT_REQUIRE((reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0, "exploit eval: workspace not 16-byte aligned");
    RcWs w;
    if (int rc = rc_ws(&run, w)) return rc;
    const int32_t N = a->N, H = a->H, A = run.action_dim;
    float* ws = a->workspace;
    float* tokens = ws + w.tokens;
    float* preds = a->logits_out ? a->logits_out : ws + w.preds;
    if (int rc = dpt_interactive_pack(a->actions, a->rewards, N, H, A, tokens, stream)) return rc;
    // row t of this one forward: the model after t transitions
    if (int rc = dpt_train_forward(&run, blob, tokens, ws + w.train, preds, stream)) return rc;
    return dpt_recommend_curve(preds, a->means, a->targets, N, H + 1, A, a->greedy_arm, a->greedy_value,
                               a->expected_value, a->p_opt, stream);
}

}  // extern "C"
