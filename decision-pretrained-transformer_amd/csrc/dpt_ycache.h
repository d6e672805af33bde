// The bandit rollout's packed y cache (rollout_bandit_kernel, dpt_decode.hip): blocks >= 1
// cache the normalised row yhat_p = (h_p - mean_p) rstd_p of ln_1 (its g and b are folded into
// the derived weights, derive_l0_kernel) as signed 24-bit fixed point, 96 B per row.
//
// Format: q = rint(yhat 2^20) clamped to +-(2^23 - 1).  |yhat_i| <= sqrt(E - 1) = 5.57 < 8 for
// every model, so one scale serves all of them and the clamp is never reached by a LayerNorm
// output; the absolute error is at most 2^-21.
//
// A lane owns four consecutive dims, 12 B: two dwords with the four high halves (q >> 8, 16
// bits each) and one dword with the four low bytes.  Unpacking element i is one byte permute
// (v_perm_b32) that builds q << 8 and one v_cvt_f32_i32: the float is yhat 2^28 exactly (24
// significant bits), and the 2^-28 goes into the score scale and the output normalisation.
//
// Layout of one tile's rows of one block: [8-position group][task in tile][8 rows x 96 B], so
// a wave's load of 8 positions of its task is one 768-B run aligned to 128 B, and the tile's
// waves read adjacent runs.  The last group, when max_pos is no multiple of 8, holds only
// max_pos % 8 rows per task, so a tile's rows take max_pos x tile x 96 B and stay inside its
// fp32-sized slot at every horizon.
//
// Plain C++ apart from the device fast paths: tests/test_ycache_pack_host.py compiles it
// with the host compiler.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DPT_YQ_HD __host__ __device__
#else
#define DPT_YQ_HD
#endif

namespace dpt {

constexpr int kYqFrac = 20;                   // fraction bits of the stored value
constexpr int kYqMax = (1 << 23) - 1;         // clamp of the 24-bit value
constexpr int kYqRowBytes = 96;               // one packed row (32 dims)
constexpr int kYqGroupBytes = 8 * kYqRowBytes;  // 8 positions of one task
constexpr float kYqScale = 1048576.0f;        // 2^kYqFrac
constexpr float kYqUnscale = 1.0f / 268435456.0f;  // 2^-(kYqFrac + 8): unpacked floats are yhat 2^28

struct YqLane {
    uint32_t h01, h23, lo;  // high halves of elements 0|1 and 2|3, the four low bytes
};

// q = rint(y 2^20), round-half-even, saturating (a NaN clamps to the negative end)
DPT_YQ_HD inline int32_t yq_quant(float y) {
    float s = y * kYqScale;
    s = fminf(fmaxf(s, -(float)kYqMax), (float)kYqMax);
    return (int32_t)rintf(s);
}

DPT_YQ_HD inline YqLane yq_pack(int32_t q0, int32_t q1, int32_t q2, int32_t q3) {
    YqLane p;
    p.h01 = (((uint32_t)q0 >> 8) & 0xffffu) | (((uint32_t)q1 >> 8) << 16);
    p.h23 = (((uint32_t)q2 >> 8) & 0xffffu) | (((uint32_t)q3 >> 8) << 16);
    p.lo = ((uint32_t)q0 & 0xffu) | (((uint32_t)q1 & 0xffu) << 8) | (((uint32_t)q2 & 0xffu) << 16) |
           ((uint32_t)q3 << 24);
    return p;
}

// element i (0..3) of a lane as q << 8
template <int I>
DPT_YQ_HD inline int32_t yq_unpack_q8(const YqLane& p) {
    const uint32_t h = I < 2 ? p.h01 : p.h23;
#if defined(__HIP_DEVICE_COMPILE__)
    // bytes of the result, low to high: 0x00, lo.b[I], h.b[2 (I & 1)], h.b[2 (I & 1) + 1]
    constexpr uint32_t sel = (I & 1 ? 0x07060000u : 0x05040000u) | ((uint32_t)I << 8) | 0x0cu;
    return (int32_t)__builtin_amdgcn_perm(h, p.lo, sel);
#else
    const uint32_t hi = (I & 1) ? (h & 0xffff0000u) : (h << 16);
    return (int32_t)(hi | (((p.lo >> (8 * I)) & 0xffu) << 8));
#endif
}

// element i as yhat 2^28 (exact: 24 significant bits)
template <int I>
DPT_YQ_HD inline float yq_unpack_f28(const YqLane& p) {
    return (float)yq_unpack_q8<I>(p);
}

// the value a stored element stands for
template <int I>
DPT_YQ_HD inline float yq_value(const YqLane& p) {
    return yq_unpack_f28<I>(p) * kYqUnscale;
}

// Byte offset of the packed row of position p of task t (of a tile of `tile` tasks) from the
// start of the tile's rows of one block; max_pos is the rollout's horizon.
DPT_YQ_HD inline int64_t yq_row_offset(int p, int t, int tile, int max_pos) {
    const int grp = p >> 3, row = p & 7;
    const int rows = grp < (max_pos >> 3) ? 8 : (max_pos & 7);  // rows per task in this group
    return (int64_t)grp * tile * kYqGroupBytes + (t * rows + row) * kYqRowBytes;
}

}  // namespace dpt
