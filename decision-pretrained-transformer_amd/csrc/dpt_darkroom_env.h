// DarkRoom env arithmetic shared by the per-step / rollin kernels (dpt_env.hip), the interactive MDP
// training step (dpt_interactive_mdp.hip) and the episode rollout (dpt_prefill.hip): one copy of the
// move, of the expert action, and of the reset and act rules built on them.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

#include "dpt_common.h"

namespace dpt {

// DarkRoom: 5 actions, tokens [s (2) | onehot(a) (5) | s' (2) | r]
constexpr int kDarkroomA = 5, kDarkroomF = 10;

// envs/darkroom_env.py:37-55: env action a (after any permutation) -> move -> clip
__device__ inline void darkroom_move(int& x, int& y, int a, int dim) {
    x += (a == 0) - (a == 1);
    y += (a == 2) - (a == 3);
    x = min(max(x, 0), dim - 1);
    y = min(max(y, 0), dim - 1);
}

// envs/darkroom_env.py:69-82 (+ :105-111: index of the expert action inside this task's perm (5) or nullptr)
__device__ inline int darkroom_opt(int x, int y, int gx, int gy, const int32_t* perm) {
    int a = x < gx ? 0 : x > gx ? 1 : y < gy ? 2 : y > gy ? 3 : 4;
    if (perm) {
        int k = 0;
        while (k < 5 && perm[k] != a) ++k;
        a = k;
    }
    return a;
}

// The reset rule of an episode: s_0 = (0, 0); returns target_0, the expert action there.
__device__ inline int darkroom_reset(int& x, int& y, int gx, int gy, const int32_t* perm) {
    x = 0;
    y = 0;
    return darkroom_opt(0, 0, gx, gy, perm);
}

// What one act step appends to an episode's records.
struct DarkroomStep {
    int action, reward, next_opt;
};

// The act rule of one env: dpt_select_action's rule at temperature 1 over the 5 logits (its 5-arm path,
// bit-identical to select_from_logits; `u` is read only when `sample`), the permuted move of (x, y) in
// place, the reward at the goal and the expert action at the new state.
__device__ inline DarkroomStep darkroom_act(const float (&lg)[kDarkroomA], int sample, double u,
                                            const int32_t* perm, int dim, int gx, int gy, int& x, int& y) {
    DarkroomStep s;
    s.action = select_fixed_fast<kDarkroomA>(lg, sample, 1.0f, u);
    darkroom_move(x, y, perm ? perm[s.action] : s.action, dim);
    s.reward = (x == gx && y == gy) ? 1 : 0;
    s.next_opt = darkroom_opt(x, y, gx, gy, perm);
    return s;
}

}  // namespace dpt
