// The per-step draws and arithmetic of the i.i.d. rollins (collect_data.py:23-53, :83-111, :189-218),
// shared by the rollin kernels (dpt_env.hip: a dataset's records) and the fresh-task generator
// (dpt_fresh.hip: the packed tokens of a training batch): one copy of the arm choice, of the reward
// and of the DarkRoom step and query draws, so the two write the same values for the same
// (seed, task, step).
#pragma once

#include "dpt_common.h"
#include "dpt_darkroom_env.h"

namespace dpt {

// word `word` of the block as an integer in [0, n)
__device__ inline int philox_randint(uint64_t seed, uint64_t step, int64_t task, uint32_t stream, int word, int n) {
    U4 r = philox(seed, step, task, stream);
    const uint32_t w = word == 0 ? r.x : word == 1 ? r.y : word == 2 ? r.z : r.w;
    return (int)(((uint64_t)w * (uint64_t)n) >> 32);  // multiply-shift, bias < n / 2^32
}

// arm ~ choice(A, p) from the uniform u (numpy legacy cdf / searchsorted 'right' semantics): the number
// of k with cumsum(p)[k] / sum(p) <= u, clamped to A - 1
__device__ inline int rollin_bandit_arm(const double* p, int A, double u) {
    double total = 0.0;
    for (int k = 0; k < A; ++k) total += p[k];
    double c = 0.0;
    int a = 0;
    for (int k = 0; k < A; ++k) {
        c += p[k];
        a += (c / total <= u) ? 1 : 0;
    }
    return a < A ? a : A - 1;
}

// the reward of step h at the chosen arm's mean: Bernoulli(mean) from a uniform, or mean + (0.0 + var g);
// noise: the injected uniform / normal (`injected`), else Philox(seed, (h, task, DPT_STREAM_REWARD))
__device__ inline double rollin_bandit_reward(int type, double mean, double var, bool injected, double noise,
                                              uint64_t seed, int h, int64_t task) {
    if (type == DPT_BANDIT_BERNOULLI) {
        const double ur = injected ? noise : philox_uniform(seed, h, task, DPT_STREAM_REWARD);
        return (ur < mean) ? 1.0 : 0.0;
    }
    const double g = injected ? noise : philox_normal(seed, h, task, DPT_STREAM_REWARD);
    return gaussian_reward(mean, var, g);
}

// step h of the 'uniform' DarkRoom rollin: s ~ U{0..dim-1}^2 and a ~ U{0..4}, words 0 / 1 / 2 of
// Philox(seed, (h, task, DPT_STREAM_ROLLIN))
__device__ inline void rollin_darkroom_draw(uint64_t seed, int h, int64_t task, int dim, int& x, int& y, int& a) {
    x = philox_randint(seed, h, task, DPT_STREAM_ROLLIN, 0, dim);
    y = philox_randint(seed, h, task, DPT_STREAM_ROLLIN, 1, dim);
    a = philox_randint(seed, h, task, DPT_STREAM_ROLLIN, 2, 5);
}

// the query state of a task ~ U{0..dim-1}^2: words 0 / 1 at counter H (the step after the rollin's last)
__device__ inline void rollin_darkroom_query(uint64_t seed, int H, int64_t task, int dim, int& qx, int& qy) {
    qx = philox_randint(seed, H, task, DPT_STREAM_ROLLIN, 0, dim);
    qy = philox_randint(seed, H, task, DPT_STREAM_ROLLIN, 1, dim);
}

// one rollin transition from (x, y) under action a (perm: the task's action permutation or nullptr):
// moves (x, y) in place and returns the reward at the goal
__device__ inline int rollin_darkroom_step(int& x, int& y, int a, const int32_t* perm, int dim, int gx, int gy) {
    darkroom_move(x, y, perm ? perm[a] : a, dim);
    return (x == gx && y == gy) ? 1 : 0;
}

}  // namespace dpt
