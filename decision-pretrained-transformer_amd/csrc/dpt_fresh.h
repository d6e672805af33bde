// What the fresh-task generators share (dpt_fresh.hip: bandit, DarkRoom; dpt_fresh_linear.hip: the linear
// bandit): the block size, the coalesced row store, and the bandit's Dirichlet / point-mass behaviour
// policy with its i.i.d. rollin rows -- one copy, so the linear bandit's 'uniform' rollin is
// fresh_bandit_kernel's on other task counters.
#pragma once

#include "dpt_common.h"
#include "dpt_rollin.h"

namespace dpt {

constexpr int kFreshThreads = 256;

// the rows 1 + h0 .. 1 + h0 + rows - 1 of one sample, F floats each, element (row, f) = val(row, f)
template <class Val>
__device__ inline void fresh_store_rows(float* __restrict__ dst, int rows, int F, Val val) {
    const int n = rows * F;
    for (int e = threadIdx.x; e < n; e += kFreshThreads) {
        const int row = e / F;
        dst[e] = val(row, e - row * F);
    }
}

// rows of a bandit sample from the chunk's arms and rewards: [1 | onehot(arm) | 1 | r]
__device__ inline void fresh_store_bandit_rows(float* __restrict__ dst, int rows, int A, const int* s_arm,
                                               const float* s_r) {
    fresh_store_rows(dst, rows, A + 3, [&](int row, int f) {
        return f == 0 || f == A + 1 ? 1.f : f == A + 2 ? s_r[row] : (s_arm[row] == f - 1 ? 1.f : 0.f);
    });
}

// The behaviour policy of a bandit task into s_probs (LDS, A entries; s_e: A entries of scratch), by the
// whole block: probs = (1 - cov) e / sum(e) + cov onehot(rand), e_k = -log(1 - uniform) at task counter
// c0 + k (the Gamma(1) variates of Dirichlet(1_A)), and at counter c0 + A word 0 -> the index into the
// 11-point cov grid, word 1 -> the point-mass arm.  Ends behind a barrier: every lane may read s_probs.
__device__ inline void fresh_bandit_policy(int A, uint64_t seed, int64_t task, int c0, double* s_e, double* s_probs) {
    const int tid = threadIdx.x;
    if (tid < A) s_e[tid] = -log(1.0 - philox_uniform(seed, c0 + tid, task, DPT_STREAM_TASK));  // Gamma(1) = Exp(1)
    __syncthreads();
    if (tid < A) {
        double total = 0.0;  // every lane sums in index order: one value
        for (int k = 0; k < A; ++k) total += s_e[k];
        // the grid point index / 10 is the correctly rounded decimal: the double that 0.1, 0.2, ... name
        const double cov = (double)philox_randint(seed, c0 + A, task, DPT_STREAM_TASK, 0, 11) / 10.0;
        const int rand_index = philox_randint(seed, c0 + A, task, DPT_STREAM_TASK, 1, A);
        s_probs[tid] = (1.0 - cov) * (s_e[tid] / total) + cov * (tid == rand_index ? 1.0 : 0.0);
    }
    __syncthreads();
}

// The H i.i.d. rollin rows of a bandit sample (rows 1 .. H of tok) under s_means / s_probs: the lanes take
// kFreshThreads steps at a time, each lane one step with the rollin kernel's draws and arithmetic
// (dpt_rollin.h), then stride over the chunk's floats.  s_arm / s_r: kFreshThreads entries of LDS.
__device__ inline void fresh_bandit_rows(int A, int H, int type, double var, uint64_t seed, int64_t task,
                                         const double* s_means, const double* s_probs, int* s_arm, float* s_r,
                                         float* __restrict__ tok) {
    const int tid = threadIdx.x, F = A + 3;
    for (int h0 = 0; h0 < H; h0 += kFreshThreads) {
        const int h = h0 + tid;
        if (h < H) {
            const double u = philox_uniform(seed, h, task, DPT_STREAM_ROLLIN);
            const int a = rollin_bandit_arm(s_probs, A, u);
            s_arm[tid] = a;
            s_r[tid] = (float)rollin_bandit_reward(type, s_means[a], var, false, 0.0, seed, h, task);
        }
        __syncthreads();
        fresh_store_bandit_rows(tok + (int64_t)(1 + h0) * F, min(kFreshThreads, H - h0), A, s_arm, s_r);
        __syncthreads();
    }
}

}  // namespace dpt
