// The conv encoder of the image front end as device functions of one workgroup of kImgThreads threads,
// shared by img_enc_fwd / img_enc_bwd (dpt_image.hip) and the act step's fused front (dpt_imageact.hip):
// one copy of the arithmetic, so every caller produces the same bits for the same image and weights.
#pragma once

#include "dpt_common.h"

namespace dpt {

constexpr int kImgThreads = 256;
constexpr int kImgSize = 25, kImgPix = 3 * kImgSize * kImgSize;  // 1875 floats per image
constexpr int kC1 = 12, kA1 = kC1 * kC1;   // conv1 output 16 x 12 x 12
constexpr int kC2 = 10, kA2 = kC2 * kC2;   // conv2 output 16 x 10 x 10
constexpr int kCh = 16, kEnc = 8, kFlat = kCh * kA2;  // 1600
// LDS channel stride of the conv1 activations: the four k-groups of an MFMA operand read channels 4
// apart, 4 * 148 = 16 (mod 32) banks apart (144 would put all four on the same banks); the 4 pad
// floats per channel are zero (the weight gradient's padded columns read up to 2 past a channel)
constexpr int kA1S = 148;

// front blob offsets (dpt_hip.h order); F = 8 + sd + A + 1
struct ImgBlob {
    int64_t c1w, c1b, c2w, c2b, fcw, fcb, embw, embb, lng, lnb, total;
    __host__ __device__ static ImgBlob make(int F, int E) {
        ImgBlob b;
        int64_t p = 0;
        b.c1w = p; p += 432;
        b.c1b = p; p += 16;
        b.c2w = p; p += 2304;
        b.c2b = p; p += 16;
        b.fcw = p; p += (int64_t)kFlat * kEnc;
        b.fcb = p; p += kEnc;
        b.embw = p; p += (int64_t)F * E;
        b.embb = p; p += E;
        b.lng = p; p += E;
        b.lnb = p; p += E;
        b.total = p;
        return b;
    }
};

__device__ inline float img_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the forward encoder's LDS (34.6 KB): staged weights, one image and its two activation maps
struct ImgEncLds {
    float w1[448];            // conv1_w | conv1_b
    float w2t[144 * kCh];     // conv2_w as [k = ci 9 + ky 3 + kx][co]: a B operand read is 16 contiguous floats
    float b2[kCh];
    float img[kImgPix + 1];
    float a1[kCh * kA1S];
    float a2[kFlat];
    float red[kImgThreads / 64][kEnc];
};

// a1[co][y][x] = relu(b[co] + sum_{ci, ky, kx} img[ci][2y + ky][2x + kx] w[co][ci][ky][kx]) into LDS (channel
// stride kA1S); w1 = conv1_w then conv1_b (448 floats, LDS)
__device__ inline void img_conv1(const float* __restrict__ w1, const float* __restrict__ img, float* __restrict__ a1) {
    for (int o = threadIdx.x; o < kCh * kA1; o += kImgThreads) {
        const int co = o / kA1, p = o % kA1, y = p / kC1, x = p % kC1;
        const float* w = w1 + co * 27;
        const float* in = img + (2 * y) * kImgSize + 2 * x;
        float acc = w1[432 + co];
#pragma unroll
        for (int ci = 0; ci < 3; ++ci)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
                    acc = fmaf(in[ci * kImgSize * kImgSize + ky * kImgSize + kx], w[ci * 9 + ky * 3 + kx], acc);
        a1[co * kA1S + p] = acc > 0.f ? acc : 0.f;
    }
}

// the conv weights into LDS, once per workgroup (a barrier must follow before they are read)
__device__ inline void img_stage_weights(const float* __restrict__ blob, const ImgBlob& B, ImgEncLds& s) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 448; i += kImgThreads) s.w1[i] = blob[B.c1w + i];
    for (int i = tid; i < 2304; i += kImgThreads) s.w2t[(i % 144) * kCh + i / 144] = blob[B.c2w + i];
    if (tid < kCh) s.b2[tid] = blob[B.c2b + tid];
}

// conv2 on the matrix cores: z2[p][co] = sum_k a1patch[p][k] w2[k][co], k = (ci, ky, kx); lane (i16, kq)
// holds the k run kq 36 .. kq 36 + 35 = channels 4 kq .. 4 kq + 3 (A and B read the same k).  Then bias,
// ReLU and (drop) the encoder's dropout of image `row` into s.a2.
__device__ inline void img_conv2(ImgEncLds& s, const TrDims& dd, bool drop, int64_t row) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i16 = lane & 15, kq = lane >> 4;
    for (int mt = wave; mt < 7; mt += kImgThreads / 64) {
        const int p = min(16 * mt + i16, kA2 - 1);  // positions past 99 compute a copy that is never stored
        const float* ap = s.a1 + (4 * kq) * kA1S + (p / kC2) * kC1 + p % kC2;
        const float* bp = s.w2t + (36 * kq) * kCh + i16;
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 36; ++t)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[(t / 9) * kA1S + ((t % 9) / 3) * kC1 + t % 3], bp[t * kCh],
                                                       acc, 0, 0, 0);
        // C layout: lane (co = i16, kq) holds positions 16 mt + 4 kq + r
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int pp = 16 * mt + 4 * kq + r;
            if (pp >= kA2) continue;
            float v = acc[r] + s.b2[i16];
            v = v > 0.f ? v : 0.f;
            if (drop) v *= tr_keep(dd, DPT_SITE_IMAGE_ENC, row * kFlat + i16 * kA2 + pp);
            s.a2[i16 * kA2 + pp] = v;
        }
    }
}

// the 1600 -> 8 product: thread-strided partial sums over s.a2, a wave tree, one partial per wave into
// s.red (a barrier must follow; img_enc_out then sums the waves in order).  a2row, when given, receives
// the activations (the backward's copy).
__device__ inline void img_fc(const float* __restrict__ blob, const ImgBlob& B, ImgEncLds& s, float* __restrict__ a2row) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float acc[kEnc];
#pragma unroll
    for (int j = 0; j < kEnc; ++j) acc[j] = 0.f;
    for (int i = tid; i < kFlat; i += kImgThreads) {
        const float v = s.a2[i];
        if (a2row) a2row[i] = v;
        const floatx4* w = reinterpret_cast<const floatx4*>(blob + B.fcw + (int64_t)i * kEnc);
        const floatx4 wa = w[0], wb = w[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[j] = fmaf(v, wa[j], acc[j]);
            acc[4 + j] = fmaf(v, wb[j], acc[4 + j]);
        }
    }
#pragma unroll
    for (int j = 0; j < kEnc; ++j) acc[j] = img_wave_sum(acc[j]);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kEnc; ++j) s.red[wave][j] = acc[j];
    }
}

// encoder output f (0..7) after img_fc and a barrier: the waves' partials in order, bias, ReLU
__device__ inline float img_enc_out(const float* __restrict__ blob, const ImgBlob& B, const ImgEncLds& s, int f) {
    const float v = ((s.red[0][f] + s.red[1][f]) + (s.red[2][f] + s.red[3][f])) + blob[B.fcb + f];
    return v > 0.f ? v : 0.f;
}

}  // namespace dpt
