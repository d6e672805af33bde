// The Bayes posterior of the optimal action (include/dpt_hip.h, "Bayes posterior of the optimal action"):
// the exact target of the pretraining cross-entropy, for every prefix of a context.
//
//   pb_tables_kernel   log(x_i) and log1p(-x_i) of the grid x_i = (i + 0.5) / G, once per call (Bernoulli).
//   pb_kernel<AP, LDS> the bandit grid posterior.  One 256-thread workgroup walks t = 0 .. H of one task.
//                      Thread j owns the grid points i = j, j + 256, ...: it alone writes and reads w_a(i)
//                      and C_a(i) of every arm, so the 2 A G doubles of a task need no fence: they live in
//                      LDS while 2 A G 8 B <= 128 KiB, else in the caller's workspace (one slot per
//                      workgroup, L2-resident).  Between row t and row t + 1 only the pulled arm changes:
//                      its log-likelihood, maximum, exponentials, their sum, the quotients and their
//                      mid-point scan (a wave scan per 256 points, the four wave totals through LDS, a
//                      carry across the chunks).  Then u_a = sum_i w_a(i) prod_{b != a} C_b(i) for all arms
//                      from one prefix / suffix product per grid point (AP = A rounded up to a power of
//                      two: the products stay in registers).
//   pd_kernel          the DarkRoom posterior: one wave per sample, goal k of a 64-goal chunk on lane k, the
//                      chunk's consistent goals a 64-bit mask in LDS, counts by ballot and popcount.
//   pc_kernel          the compare: one thread per row (n, t), fp64 log-softmax of the fp32 logits.
//
// Every reduction has a fixed order (the butterflies, the waves in index order, the chunks in index order,
// the pulls in pull order): repeated calls are bit-identical and a task's rows do not depend on N, on the
// slot it ran in or on how the caller chunks the tasks.  Nothing here allocates.
#include "dpt_common.h"

namespace dpt {

constexpr int kPbThreads = 256;
constexpr int kPbWaves = kPbThreads / kWave;
constexpr int64_t kPbLdsBytes = 128 * 1024;  // w and C of one task in LDS up to here (beside ~2 KiB static)
constexpr int kPbSlots = 256;                // workgroups (workspace slots) of the workspace path
constexpr int kPbMinG = 64, kPbMaxG = 8192;
constexpr int kPdMaxGoals = 1 << 18;         // 4096 chunk masks = 32 KiB of LDS

inline bool pb_in_lds(int A, int G) { return 2ll * A * G * 8 <= kPbLdsBytes; }

// the reductions' LDS: two alternating sets of wave partials (one barrier per reduction), the per-wave u
// partials and their totals, and the sufficient statistics of every arm
struct PbShared {
    double part[2][kPbWaves];
    double u[kPbWaves][kMaxA];
    double tot[kMaxA];
    double cnt[kMaxA], sum[kMaxA];
};

__device__ inline double pb_wave_sum(double v) {
#pragma unroll
    for (int off = kWave >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

__device__ inline double pb_wave_max(double v) {
#pragma unroll
    for (int off = kWave >> 1; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, kWave));
    return v;
}

// every thread calls these in the same sequence; `phase` alternates the partial set, so a set is
// rewritten only after the barrier of the reduction in between
__device__ inline double pb_block_sum(double v, PbShared& sh, int& phase) {
    v = pb_wave_sum(v);
    double* p = sh.part[phase];
    phase ^= 1;
    if ((threadIdx.x & (kWave - 1)) == 0) p[threadIdx.x / kWave] = v;
    __syncthreads();
    return ((p[0] + p[1]) + p[2]) + p[3];
}

__device__ inline double pb_block_max(double v, PbShared& sh, int& phase) {
    v = pb_wave_max(v);
    double* p = sh.part[phase];
    phase ^= 1;
    if ((threadIdx.x & (kWave - 1)) == 0) p[threadIdx.x / kWave] = v;
    __syncthreads();
    return fmax(fmax(p[0], p[1]), fmax(p[2], p[3]));
}

// the log-likelihood of grid point i in the header's operation order (-ffp-contract=off: no fused
// multiply-add, so numpy's values bit for bit up to log / log1p)
template <bool BERN>
__device__ inline double pb_loglik(int i, int G, double n, double s, double var, const double* __restrict__ tab) {
    if (BERN) return s * tab[i] + (n - s) * tab[G + i];
    const double x = ((double)i + 0.5) / (double)G;
    return -((n * x) * x - (2.0 * s) * x) / ((2.0 * var) * var);
}

// w and C of one arm with statistics (n, s): W[i], C[i] for this thread's grid points
template <bool BERN>
__device__ inline void pb_update_arm(double* __restrict__ W, double* __restrict__ C, int G, double n, double s,
                                     double var, const double* __restrict__ tab, PbShared& sh, int& phase) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    double m = -INFINITY;
    for (int i = tid; i < G; i += kPbThreads) m = fmax(m, pb_loglik<BERN>(i, G, n, s, var, tab));
    m = pb_block_max(m, sh, phase);
    double z = 0.0;
    for (int i = tid; i < G; i += kPbThreads) {
        const double e = exp(pb_loglik<BERN>(i, G, n, s, var, tab) - m);
        W[i] = e;
        z += e;
    }
    z = pb_block_sum(z, sh, phase);
    double carry = 0.0;
    for (int base = 0; base < G; base += kPbThreads) {  // uniform: every thread meets every barrier
        const int i = base + tid;
        const double v = i < G ? W[i] / z : 0.0;
        double incl = v;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const double o = __shfl_up(incl, off, kWave);
            if (lane >= off) incl += o;
        }
        double excl = __shfl_up(incl, 1, kWave);
        if (lane == 0) excl = 0.0;
        const double total = __shfl(incl, kWave - 1, kWave);
        double* p = sh.part[phase];
        phase ^= 1;
        if (lane == 0) p[wave] = total;
        __syncthreads();
        double before = carry;
        for (int k = 0; k < wave; ++k) before += p[k];
        carry += ((p[0] + p[1]) + p[2]) + p[3];
        if (i < G) {
            W[i] = v;
            C[i] = (before + excl) + v / 2.0;
        }
    }
}

// A task's W | C: arm a at [a G, (a + 1) G) of each half.
template <int AP, bool LDS, bool BERN>
__global__ __launch_bounds__(kPbThreads) void pb_kernel(const int32_t* __restrict__ actions,
                                                        const double* __restrict__ rewards, int N, int H, int A,
                                                        int G, double var, double* __restrict__ ws,
                                                        double* __restrict__ post) {
    extern __shared__ __align__(16) double pb_dyn[];
    __shared__ PbShared sh;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const double* tab = ws;  // log x | log1p(-x), 2 G doubles
    double* W = LDS ? pb_dyn : ws + 2ll * G + (int64_t)blockIdx.x * 2 * A * G;
    double* C = W + (int64_t)A * G;
    int phase = 0;
    for (int64_t task = blockIdx.x; task < N; task += gridDim.x) {
        __syncthreads();  // the previous task's last reads of sh
        if (tid < kMaxA) { sh.cnt[tid] = 0.0; sh.sum[tid] = 0.0; }
        for (int a = 0; a < A; ++a)
            pb_update_arm<BERN>(W + (int64_t)a * G, C + (int64_t)a * G, G, 0.0, 0.0, var, tab, sh, phase);
        double out = 0.0;  // post[task][t][tid] of the row before, for tid < A
        for (int t = 0; t <= H; ++t) {
            bool changed = t == 0;
            if (t > 0) {
                const int a = actions[task * H + t - 1];
                if (a >= 0 && a < A) {  // uniform
                    const double n = sh.cnt[a] + 1.0;
                    const double s = sh.sum[a] + rewards[task * H + t - 1];
                    __syncthreads();
                    if (tid == 0) { sh.cnt[a] = n; sh.sum[a] = s; }
                    pb_update_arm<BERN>(W + (int64_t)a * G, C + (int64_t)a * G, G, n, s, var, tab, sh, phase);
                    changed = true;
                }
            }
            if (changed) {
                double u[AP];
#pragma unroll
                for (int b = 0; b < AP; ++b) u[b] = 0.0;
                for (int i = tid; i < G; i += kPbThreads) {
                    double c[AP], pre[AP];
                    double p = 1.0;
#pragma unroll
                    for (int b = 0; b < AP; ++b) {
                        c[b] = b < A ? C[(int64_t)b * G + i] : 1.0;
                        pre[b] = p;
                        p = p * c[b];
                    }
                    double suf = 1.0;
#pragma unroll
                    for (int b = AP - 1; b >= 0; --b) {
                        if (b < A) u[b] += W[(int64_t)b * G + i] * (pre[b] * suf);
                        suf = suf * c[b];
                    }
                }
#pragma unroll
                for (int b = 0; b < AP; ++b) {
                    const double r = pb_wave_sum(u[b]);
                    if (lane == 0) sh.u[wave][b] = r;
                }
                __syncthreads();
                if (tid < A) sh.tot[tid] = ((sh.u[0][tid] + sh.u[1][tid]) + sh.u[2][tid]) + sh.u[3][tid];
                __syncthreads();
                if (tid < A) {
                    double total = 0.0;
                    for (int b = 0; b < A; ++b) total += sh.tot[b];
                    out = sh.tot[tid] / total;
                }
            }
            if (tid < A) post[(task * (H + 1ll) + t) * A + tid] = out;
        }
    }
}

__global__ void pb_tables_kernel(int G, double* __restrict__ tab) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G) return;
    const double x = ((double)i + 0.5) / (double)G;
    tab[i] = log(x);
    tab[G + i] = log1p(-x);
}

template <int AP>
static int pb_launch(const dpt_bandit_posterior_args& a, hipStream_t st) {
    const bool lds = pb_in_lds(a.A, a.G), bern = a.type == DPT_BANDIT_BERNOULLI;
    const int64_t dyn = lds ? 2ll * a.A * a.G * 8 : 0;
    const unsigned blocks = lds ? (unsigned)a.N : (unsigned)(a.N < kPbSlots ? a.N : kPbSlots);
    void (*kern)(const int32_t*, const double*, int, int, int, int, double, double*, double*) =
        lds ? (bern ? pb_kernel<AP, true, true> : pb_kernel<AP, true, false>)
            : (bern ? pb_kernel<AP, false, true> : pb_kernel<AP, false, false>);
    if (dyn > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)dyn);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(kPbThreads), (size_t)dyn, st, a.actions, a.rewards, a.N, a.H, a.A,
                       a.G, a.var, a.workspace, a.post);
    return launched("bandit posterior");
}

static int pb_check_shape(int32_t N, int32_t A, int32_t G) {
    DPT_REQUIRE(N >= 1 && A >= 1, "bandit posterior: N=%d A=%d", N, A);
    DPT_REQUIRE(G >= kPbMinG && G <= kPbMaxG && G % 64 == 0, "bandit posterior: G=%d is not a multiple of 64 in [%d, %d]",
                G, kPbMinG, kPbMaxG);
    return check_action_dim("bandit posterior", A);
}

// expert action at the query for goal (gx, gy), identity permutation (envs/darkroom_env.py:69-82)
__device__ inline int pd_opt(int x, int y, int gx, int gy) {
    return x < gx ? 0 : x > gx ? 1 : y < gy ? 2 : y > gy ? 3 : 4;
}

__global__ __launch_bounds__(kWave) void pd_kernel(const int32_t* __restrict__ goals, int n_goals,
                                                   const int32_t* __restrict__ query,
                                                   const int32_t* __restrict__ next_states,
                                                   const int32_t* __restrict__ rewards, int H,
                                                   double* __restrict__ post, int32_t* __restrict__ consistent) {
    extern __shared__ __align__(16) unsigned long long pd_alive[];  // one mask per 64 goals
    const int lane = threadIdx.x;
    const int64_t n = blockIdx.x;
    const int chunks = (n_goals + kWave - 1) / kWave;
    const int qx = query[2 * n], qy = query[2 * n + 1];
    for (int t = 0; t <= H; ++t) {
        int nx = 0, ny = 0, r = 0;
        if (t > 0) {
            const int64_t j = n * H + t - 1;
            nx = next_states[2 * j];
            ny = next_states[2 * j + 1];
            r = rewards[j];
        }
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
        for (int ch = 0; ch < chunks; ++ch) {
            const int k = ch * kWave + lane;
            const bool valid = k < n_goals;
            const int gx = valid ? goals[2 * k] : 0, gy = valid ? goals[2 * k + 1] : 0;
            unsigned long long m;
            if (t == 0) {
                m = __ballot(valid);
            } else {
                const bool ok = (r != 0) == (nx == gx && ny == gy);
                m = pd_alive[ch] & __ballot(valid && ok);
            }
            if (lane == 0) pd_alive[ch] = m;
            const bool mine = (m >> lane) & 1ull;
            const int act = pd_opt(qx, qy, gx, gy);
            c0 += __popcll(__ballot(mine && act == 0));
            c1 += __popcll(__ballot(mine && act == 1));
            c2 += __popcll(__ballot(mine && act == 2));
            c3 += __popcll(__ballot(mine && act == 3));
            c4 += __popcll(__ballot(mine && act == 4));
        }
        __syncthreads();  // one wave: orders lane 0's masks before the next row's reads
        const int total = c0 + c1 + c2 + c3 + c4;
        const int64_t row = n * (H + 1ll) + t;
        if (lane < 5) {
            const int c = lane == 0 ? c0 : lane == 1 ? c1 : lane == 2 ? c2 : lane == 3 ? c3 : c4;
            post[row * 5 + lane] = total > 0 ? (double)c / (double)total : 0.0;
        }
        if (consistent && lane == 0) consistent[row] = total;
    }
}

constexpr int kPcThreads = 256;

__global__ __launch_bounds__(kPcThreads) void pc_kernel(const double* __restrict__ post,
                                                        const float* __restrict__ logits,
                                                        const int64_t* __restrict__ targets, int64_t rows, int T,
                                                        int A, double* __restrict__ nll_model,
                                                        double* __restrict__ nll_bayes, double* __restrict__ kl,
                                                        double* __restrict__ entropy) {
    const int64_t row = (int64_t)blockIdx.x * kPcThreads + threadIdx.x;
    if (row >= rows) return;
    const float* x = logits + row * A;
    const double* p = post + row * A;
    float mf = x[0];
    for (int a = 1; a < A; ++a) mf = fmaxf(mf, x[a]);
    const double m = (double)mf;
    double s = 0.0;
    for (int a = 0; a < A; ++a) s += exp((double)x[a] - m);
    const double lse = m + log(s);
    double k = 0.0, h = 0.0;
    for (int a = 0; a < A; ++a) {
        const double pa = p[a];
        if (pa > 0.0) {
            const double lp = log(pa);
            k += pa * (lp - ((double)x[a] - lse));
            h += pa * lp;
        }
    }
    const int64_t tg = targets[row / T];
    const bool in = tg >= 0 && tg < A;
    if (nll_model) nll_model[row] = in ? -((double)x[tg] - lse) : NAN;
    if (nll_bayes) nll_bayes[row] = in ? -log(p[tg]) : NAN;
    if (kl) kl[row] = k;
    if (entropy) entropy[row] = -h;
}

}  // namespace dpt

using namespace dpt;

extern "C" {

int dpt_bandit_posterior_workspace_numel(int32_t N, int32_t A, int32_t G, int64_t* numel) {
    DPT_REQUIRE(numel != nullptr, "bandit posterior workspace: null numel");
    if (int rc = pb_check_shape(N, A, G)) return rc;
    const int64_t slots = pb_in_lds(A, G) ? 0 : (N < kPbSlots ? N : kPbSlots);
    *numel = 2ll * G + slots * 2 * A * G;
    return DPT_OK;
}

int dpt_bandit_posterior(const dpt_bandit_posterior_args* a, void* stream) {
    DPT_REQUIRE(a != nullptr, "bandit posterior: null args");
    DPT_REQUIRE(a->workspace && a->post, "bandit posterior: null workspace / post");
    DPT_REQUIRE(a->H >= 0 && a->H < INT32_MAX, "bandit posterior: H=%d", a->H);
    DPT_REQUIRE(a->H == 0 || (a->actions && a->rewards), "bandit posterior: null actions / rewards");
    DPT_REQUIRE(a->flags == 0, "bandit posterior: unknown flags 0x%x", a->flags);
    if (int rc = pb_check_shape(a->N, a->A, a->G)) return rc;
    if (a->type != DPT_BANDIT_GAUSSIAN && a->type != DPT_BANDIT_BERNOULLI) {
        set_error(DPT_EUNSUPPORTED, "bandit posterior: type=%d (DPT_BANDIT_GAUSSIAN or DPT_BANDIT_BERNOULLI)", a->type);
        return DPT_EUNSUPPORTED;
    }
    DPT_REQUIRE(a->type != DPT_BANDIT_GAUSSIAN || a->var > 0.0, "bandit posterior: Gaussian var=%g (the noise std) is not > 0",
                a->var);
    DPT_REQUIRE((reinterpret_cast<uintptr_t>(a->workspace) & 7) == 0, "bandit posterior: workspace not 8-byte aligned");
    hipStream_t st = as_stream(stream);
    if (a->type == DPT_BANDIT_BERNOULLI) {
        hipLaunchKernelGGL(pb_tables_kernel, dim3((unsigned)((a->G + 255) / 256)), dim3(256), 0, st, a->G, a->workspace);
        if (int rc = launched("bandit posterior tables")) return rc;
    }
#define PB_CASE(AP) \
    if (a->A <= AP) return pb_launch<AP>(*a, st)
    PB_CASE(1);
    PB_CASE(2);
    PB_CASE(4);
    PB_CASE(8);
    PB_CASE(16);
    PB_CASE(32);
#undef PB_CASE
    return DPT_EINVAL;  // not reached: A <= kMaxA = 32
}

int dpt_darkroom_posterior(const dpt_darkroom_posterior_args* a, void* stream) {
    DPT_REQUIRE(a != nullptr, "darkroom posterior: null args");
    DPT_REQUIRE(a->goals && a->query && a->post, "darkroom posterior: null goals / query / post");
    DPT_REQUIRE(a->N >= 1 && a->H >= 0 && a->H < INT32_MAX && a->n_goals >= 1 && a->dim >= 1,
                "darkroom posterior: N=%d H=%d n_goals=%d dim=%d", a->N, a->H, a->n_goals, a->dim);
    DPT_REQUIRE(a->H == 0 || (a->next_states && a->rewards), "darkroom posterior: null next_states / rewards");
    DPT_REQUIRE(a->flags == 0 && a->reserved == 0, "darkroom posterior: unknown flags 0x%x / reserved 0x%x", a->flags,
                a->reserved);
    if (a->dim > 255 || a->n_goals > kPdMaxGoals) {
        set_error(DPT_EUNSUPPORTED, "darkroom posterior: dim=%d above 255 or n_goals=%d above %d", a->dim, a->n_goals,
                  kPdMaxGoals);
        return DPT_EUNSUPPORTED;
    }
    const size_t lds = (size_t)((a->n_goals + kWave - 1) / kWave) * 8;
    hipLaunchKernelGGL(pd_kernel, dim3((unsigned)a->N), dim3(kWave), lds, as_stream(stream), a->goals, a->n_goals,
                       a->query, a->next_states, a->rewards, a->H, a->post, a->consistent);
    return launched("darkroom posterior");
}

int dpt_posterior_compare(const dpt_posterior_compare_args* a, void* stream) {
    DPT_REQUIRE(a != nullptr, "posterior compare: null args");
    DPT_REQUIRE(a->post && a->logits && a->targets, "posterior compare: null post / logits / targets");
    DPT_REQUIRE(a->N >= 1 && a->T >= 1 && a->A >= 1, "posterior compare: N=%d T=%d A=%d", a->N, a->T, a->A);
    DPT_REQUIRE(a->flags == 0, "posterior compare: unknown flags 0x%x", a->flags);
    if (int rc = check_action_dim("posterior compare", a->A)) return rc;
    const int64_t rows = (int64_t)a->N * a->T;
    const int64_t blocks = (rows + kPcThreads - 1) / kPcThreads;
    DPT_REQUIRE(blocks < (1ll << 31), "posterior compare: %lld rows", (long long)rows);
    hipLaunchKernelGGL(pc_kernel, dim3((unsigned)blocks), dim3(kPcThreads), 0, as_stream(stream), a->post, a->logits,
                       a->targets, rows, a->T, a->A, a->nll_model, a->nll_bayes, a->kl, a->entropy);
    return launched("posterior compare");
}

}  // extern "C"
