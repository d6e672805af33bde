// DarkRoom env arithmetic shared by the per-step / rollin kernels (dpt_env.hip) and the interactive
// MDP training step (dpt_interactive_mdp.hip): one copy of the move and of the expert action.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace dpt {

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

}  // namespace dpt
