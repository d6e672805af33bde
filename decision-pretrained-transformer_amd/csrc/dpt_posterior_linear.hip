// The linear bandit's Bayes posterior of the optimal arm at lin_d = 2 (include/dpt_hip.h, "Linear bandit,
// lin_d = 2"): the posterior of theta is a 2-D Gaussian, the winner along a ray from its mean is the upper
// envelope of A straight lines alpha_a + r beta_a, and the mass of a stretch [lo, hi] of a ray is
// exp(-lo^2 / 2) - exp(-hi^2 / 2).
//
//   lp_setup_kernel  once per call: cos / sin of the G ray angles, and from the arms alone the prior in closed
//                    form (thread a: the arc that the half-circles of its A - 1 rivals leave), the list of the
//                    arms whose prior is not 0 and every arm's rank in it, all into the workspace.
//   lp_kernel        one 256-thread workgroup walks t = 0 .. H of one task.  Every thread reads the row's
//                    (uniform) action and reward and keeps the five statistics in registers: the same bits in
//                    every lane, with no barrier or LDS round trip per row to share them; thread k derives m,
//                    L and from them alpha, xl0, xl1 of kept arm k into LDS (one barrier).  Thread j owns the
//                    rays j, j + 256, ...: it walks the envelope from the winner at r = 0 (the next breakpoint
//                    is the smallest of the header's quotients over the arms of larger beta) until
//                    exp(-r^2 / 2) is 0, at O(A) per stretch where the pairwise form costs O(A^2) per ray,
//                    reading the arms' terms as LDS broadcasts and adding each stretch's mass to its own
//                    column of the dynamic LDS (kept arm k at [k 256 + j]).  Then a butterfly per kept arm,
//                    the four waves in order, the kept arms in index order.
//
// The kernel is not templated on the arm count.  A first form kept alpha, beta and u of every arm in registers,
// templated on A rounded up to a power of two as pb_kernel is: at 32 it took 256 VGPRs and 140 AGPRs (one wave
// per SIMD) and every stretch paid a 32-way select to add its mass; it measured 41.1 and 704 ms where this form
// takes 25.7 and 219 ms (1024 tasks: 10 arms, H = 200 and 20 arms, H = 1000, G = 8192), the same arithmetic in the same order.
//
// A breakpoint is the header's quotient of the two arms that meet there, so a stretch's ends are the pairwise
// form's lo and hi wherever no third arm's line passes within rounding of the same point.  Every reduction has
// a fixed order: repeated calls are bit-identical and a task's rows do not depend on N, on the workgroup it ran
// in or on how the caller chunks the tasks.  Nothing here allocates.
#include "dpt_common.h"

namespace dpt {

constexpr int kLpThreads = 256;
constexpr int kLpWaves = kLpThreads / kWave;
constexpr int kLpMinG = 64, kLpMaxG = 65536;
constexpr double kLpTwoPi = 6.283185307179586;
constexpr double kLpMinAngle = 0x1p-40;
// workspace after the 2 G table entries
constexpr int kLpPrior = 0, kLpCount = kMaxA, kLpIndex = kMaxA + 8, kLpRank = 2 * kMaxA + 8, kLpMeta = 3 * kMaxA + 8;

__global__ __launch_bounds__(kLpThreads) void lp_setup_kernel(const double* __restrict__ arms, int A, int G,
                                                              double* __restrict__ ws) {
    __shared__ double prior[kMaxA];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * kLpThreads + tid;
    if (i < G) {
        const double phi = (kLpTwoPi * ((double)i + 0.5)) / (double)G;
        ws[i] = cos(phi);
        ws[G + i] = sin(phi);
    }
    if (blockIdx.x != 0) return;
    if (tid < A) {
        const double pi = kLpTwoPi / 2.0;
        const double x0 = arms[2 * tid], x1 = arms[2 * tid + 1];
        double first = 0.0, hi = 0.0, lo = 0.0;
        bool any = false, dead = false;
        for (int b = 0; b < A; ++b) {
            if (b == tid) continue;
            const double d0 = x0 - arms[2 * b], d1 = x1 - arms[2 * b + 1];
            if (d0 == 0.0 && d1 == 0.0) {
                dead = dead || b < tid;
                continue;
            }
            const double th = atan2(d1, d0);
            if (!any) {
                any = true;
                first = th;
                continue;
            }
            double dl = th - first;
            if (dl > pi) dl = dl - kLpTwoPi;
            else if (dl <= -pi) dl = dl + kLpTwoPi;
            hi = fmax(hi, dl);
            lo = fmin(lo, dl);
        }
        const double ang = any ? (pi - hi) + lo : kLpTwoPi;
        prior[tid] = !dead && ang >= kLpMinAngle ? ang / kLpTwoPi : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double* meta = ws + 2ll * G;
        int K = 0;
        for (int a = 0; a < kMaxA; ++a) {
            const bool keep = a < A && prior[a] > 0.0;
            meta[kLpPrior + a] = a < A ? prior[a] : 0.0;
            meta[kLpRank + a] = keep ? (double)K : -1.0;
            if (keep) meta[kLpIndex + K++] = (double)a;
        }
        for (int k = K; k < kMaxA; ++k) meta[kLpIndex + k] = -1.0;
        meta[kLpCount] = (double)K;
    }
}

struct LpShared {
    double x[2 * kMaxA];    // every arm
    double xk[2 * kMaxA];   // the kept arms, in index order
    double prior[kMaxA];
    int rank[kMaxA];        // of every arm among the kept ones, or -1
    double alpha[kMaxA], xl0[kMaxA], xl1[kMaxA];  // of the kept arms, this row
    double u[kLpWaves][kMaxA];
    double tot[kMaxA];
};

__device__ inline double lp_wave_sum(double v) {
#pragma unroll
    for (int off = kWave >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

__global__ __launch_bounds__(kLpThreads) void lp_kernel(const double* __restrict__ arms,
                                                        const int32_t* __restrict__ actions,
                                                        const double* __restrict__ rewards, int N, int H, int A,
                                                        int G, double var, const double* __restrict__ ws,
                                                        double* __restrict__ post) {
    extern __shared__ __align__(16) double lp_u[];  // u of kept arm k over this thread's rays at [k 256 + tid]
    __shared__ LpShared sh;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const double* meta = ws + 2ll * G;
    const int K = (int)meta[kLpCount];  // uniform, 1 .. A
    if (tid < kMaxA) {
        const int src = (int)meta[kLpIndex + tid];
        sh.prior[tid] = meta[kLpPrior + tid];
        sh.rank[tid] = (int)meta[kLpRank + tid];
        sh.x[2 * tid] = tid < A ? arms[2 * tid] : 0.0;
        sh.x[2 * tid + 1] = tid < A ? arms[2 * tid + 1] : 0.0;
        sh.xk[2 * tid] = src >= 0 ? arms[2 * src] : 0.0;
        sh.xk[2 * tid + 1] = src >= 0 ? arms[2 * src + 1] : 0.0;
    }
    __syncthreads();
    const double v2 = var * var;
    for (int64_t task = blockIdx.x; task < N; task += gridDim.x) {
        double sxx = 0.0, sxy = 0.0, syy = 0.0, b0 = 0.0, b1 = 0.0;
        double out = tid < A ? sh.prior[tid] : 0.0;  // post[task][t][tid] of the row before
        for (int t = 0; t <= H; ++t) {
            bool changed = false;
            if (t > 0) {
                const int a = actions[task * H + t - 1];
                if (a >= 0 && a < A) {  // uniform
                    const double r = rewards[task * H + t - 1];
                    const double x0 = sh.x[2 * a], x1 = sh.x[2 * a + 1];
                    sxx += (x0 * x0) / v2;
                    sxy += (x0 * x1) / v2;
                    syy += (x1 * x1) / v2;
                    b0 += (r * x0) / v2;
                    b1 += (r * x1) / v2;
                    changed = true;
                }
            }
            if (changed) {
                if (tid < K) {
                    const double l00 = 2.0 + sxx, l01 = sxy, l11 = 2.0 + syy;
                    const double det = l00 * l11 - l01 * l01;
                    const double S00 = l11 / det, S01 = -(l01 / det), S11 = l00 / det;
                    const double m0 = S00 * b0 + S01 * b1, m1 = S01 * b0 + S11 * b1;
                    const double L00 = sqrt(S00);
                    const double L10 = S01 / L00, L11 = 1.0 / sqrt(l11);
                    const double x0 = sh.xk[2 * tid], x1 = sh.xk[2 * tid + 1];
                    sh.alpha[tid] = x0 * m0 + x1 * m1;
                    sh.xl0[tid] = x0 * L00 + x1 * L10;
                    sh.xl1[tid] = x1 * L11;
                }
                for (int k = 0; k < K; ++k) lp_u[k * kLpThreads + tid] = 0.0;
                __syncthreads();
                for (int i = tid; i < G; i += kLpThreads) {
                    const double c = ws[i], s = ws[G + i];
                    // the winner at r = 0: the largest alpha, then the largest beta, then the lowest index
                    int cur = 0;
                    double ac = sh.alpha[0], bc = sh.xl0[0] * c + sh.xl1[0] * s;
                    for (int k = 1; k < K; ++k) {
                        const double a = sh.alpha[k], b = sh.xl0[k] * c + sh.xl1[k] * s;
                        if (a > ac || (a == ac && b > bc)) {
                            cur = k;
                            ac = a;
                            bc = b;
                        }
                    }
                    double lo = 0.0, elo = 1.0;
                    while (true) {
                        double hi = INFINITY, an = 0.0, bn = 0.0;
                        int nxt = -1;
                        for (int k = 0; k < K; ++k) {
                            const double b = sh.xl0[k] * c + sh.xl1[k] * s;
                            if (b > bc) {
                                const double a = sh.alpha[k];
                                const double q = (ac - a) / (b - bc);
                                if (q < hi) {
                                    hi = q;
                                    nxt = k;
                                    an = a;
                                    bn = b;
                                }
                            }
                        }
                        if (nxt < 0) {  // the steepest line: it holds the rest of the ray
                            lp_u[cur * kLpThreads + tid] += elo;
                            break;
                        }
                        if (hi > lo) {
                            const double ehi = exp(-(hi * hi) / 2.0);
                            lp_u[cur * kLpThreads + tid] += elo - ehi;
                            lo = hi;
                            elo = ehi;
                            if (ehi == 0.0) break;
                        }
                        cur = nxt;
                        ac = an;
                        bc = bn;
                    }
                }
                for (int k = 0; k < K; ++k) {
                    const double r = lp_wave_sum(lp_u[k * kLpThreads + tid]);
                    if (lane == 0) sh.u[wave][k] = r;
                }
                __syncthreads();
                if (tid < K) sh.tot[tid] = ((sh.u[0][tid] + sh.u[1][tid]) + sh.u[2][tid]) + sh.u[3][tid];
                __syncthreads();
                if (tid < A) {
                    double total = 0.0;
                    for (int k = 0; k < K; ++k) total += sh.tot[k];
                    const int k = sh.rank[tid];
                    out = k >= 0 ? sh.tot[k] / total : 0.0;
                }
            }
            if (tid < A) post[(task * (H + 1ll) + t) * A + tid] = out;
        }
        __syncthreads();  // this task's last reads of sh.tot before the next one's writes
    }
}

static int lp_check_shape(int32_t N, int32_t A, int32_t lin_d, int32_t G) {
    DPT_REQUIRE(N >= 1 && A >= 1 && lin_d >= 1 && G >= 1, "linear posterior: N=%d A=%d lin_d=%d G=%d", N, A, lin_d, G);
    if (lin_d != 2) {
        set_error(DPT_EUNSUPPORTED, "linear posterior: lin_d=%d (P(arm optimal) is a lin_d-dimensional integral; "
                  "only lin_d = 2 has the ray form)", lin_d);
        return DPT_EUNSUPPORTED;
    }
    if (G < kLpMinG || G > kLpMaxG || G % 64 != 0) {
        set_error(DPT_EUNSUPPORTED, "linear posterior: G=%d is not a multiple of 64 in [%d, %d]", G, kLpMinG, kLpMaxG);
        return DPT_EUNSUPPORTED;
    }
    return check_action_dim("linear posterior", A);
}

static int lp_launch(const dpt_linear_posterior_args& a, hipStream_t st) {
    const size_t dyn = (size_t)a.A * kLpThreads * 8;  // with the static part above 64 KiB from 31 arms on
    if (dyn + sizeof(LpShared) > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lp_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)dyn);
    hipLaunchKernelGGL(lp_kernel, dim3((unsigned)a.N), dim3(kLpThreads), dyn, st, a.arms, a.actions, a.rewards, a.N,
                       a.H, a.A, a.G, a.var, a.workspace, a.post);
    return launched("linear posterior");
}

}  // namespace dpt

using namespace dpt;

extern "C" {

int dpt_linear_posterior_workspace_numel(int32_t N, int32_t A, int32_t lin_d, int32_t G, int64_t* numel) {
    DPT_REQUIRE(numel != nullptr, "linear posterior workspace: null numel");
    if (int rc = lp_check_shape(N, A, lin_d, G)) return rc;
    *numel = 2ll * G + kLpMeta;
    return DPT_OK;
}

int dpt_linear_posterior(const dpt_linear_posterior_args* a, void* stream) {
    DPT_REQUIRE(a != nullptr, "linear posterior: null args");
    DPT_REQUIRE(a->arms && a->workspace && a->post, "linear posterior: null arms / workspace / post");
    DPT_REQUIRE(a->H >= 0 && a->H < INT32_MAX, "linear posterior: H=%d", a->H);
    DPT_REQUIRE(a->H == 0 || (a->actions && a->rewards), "linear posterior: null actions / rewards");
    DPT_REQUIRE(a->flags == 0, "linear posterior: unknown flags 0x%x", a->flags);
    DPT_REQUIRE(a->var > 0.0, "linear posterior: var=%g (the noise std) is not > 0", a->var);
    if (int rc = lp_check_shape(a->N, a->A, a->lin_d, a->G)) return rc;
    DPT_REQUIRE((reinterpret_cast<uintptr_t>(a->workspace) & 7) == 0, "linear posterior: workspace not 8-byte aligned");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(lp_setup_kernel, dim3((unsigned)(a->G / kLpThreads + 1)), dim3(kLpThreads), 0, st, a->arms, a->A,
                       a->G, a->workspace);
    if (int rc = launched("linear posterior setup")) return rc;
    return lp_launch(*a, st);
}

}  // extern "C"
