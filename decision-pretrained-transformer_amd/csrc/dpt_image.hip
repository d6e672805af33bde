// The image front end of the image-conditioned DPT (models/net.py:63-132 ImageTransformer;
// include/dpt_hip.h "image-conditioned DPT"): per token an image (3, 25, 25) -> Conv2d(3,16,k3,s2) ->
// ReLU -> Conv2d(16,16,k3,s1) -> ReLU -> Dropout -> flatten (c, y, x) -> Linear(1600, 8) -> ReLU, then
// [enc | state | action | reward] -> embed_transition -> embed_ln, forward and backward, all fp32.
//
//   img_enc_fwd : one launch for the whole encoder.  A workgroup takes kImgTileF images in turn; the
//                 image, the conv1 activations (16 x 12 x 12) and the conv2 activations (16 x 10 x 10)
//                 stay in LDS, the conv weights are staged once per workgroup.  conv2 (230 k of the
//                 305 k multiply-adds of an image) is an implicit GEMM on v_mfma_f32_16x16x4_f32:
//                 positions (100, in 7 tiles of 16) x K = (ci, ky, kx) = 144 x 16 output channels;
//                 conv1 (27 taps) and the 1600 -> 8 product run on the VALU.  Its stages are the device
//                 functions of dpt_image_enc.h, which the act step's fused front (dpt_imageact.hip)
//                 calls too: one copy of the encoder's arithmetic.
//   img_enc_bwd : conv1 recomputed from the image, dz2 from the fc gradient, then conv2's weight
//                 gradient (co x (ci, ky, kx) over the positions) and data gradient ((y, x) x ci over
//                 (co, ky, kx)) on the same MFMA form, conv1's weight gradient on the VALU.  The
//                 weight and bias gradients accumulate over the workgroup's kImgTileB images in
//                 registers and leave as one partial per workgroup, summed in workgroup order by
//                 tr_wgrad_reduce: bit-identical across calls, no float atomics.
//
// The rest (embed_transition, embed_ln, the fc weight gradient) are the training row kernels of
// dpt_train.hip (rows_* in dpt_common.h; dpt_generic.hip's rollout drives the same kernels through
// dpt_rows.h).  A ReLU's gradient is taken where the saved activation is > 0 (torch's convention at 0).  The encoder dropout's mask is regenerated in the backward from the
// desc (site DPT_SITE_IMAGE_ENC), never stored; the workspace keeps the DROPPED conv2 activations,
// which are the fc product's input and are > 0 exactly where the ReLU passed and the mask kept.
#include <algorithm>

#include "dpt_image_enc.h"

namespace dpt {

constexpr int kImgTileF = 4;   // images per workgroup, forward
constexpr int kImgTileB = 8;   // images per workgroup, backward (one partial each)
constexpr int kDzW = 14, kDzS = kDzW * kDzW;  // dz2 with a zero border of 2: the data gradient reads (y - ky, x - kx)
constexpr int kConvPart = 432 + 16 + 2304 + 16;  // one backward partial: conv1_w, conv1_b, conv2_w, conv2_b (blob order)

struct ImgDims {
    int rows, G, F, E, fwd_only;  // G = sd + A + 1 caller features per row, F = 8 + G
    TrDims drop;                  // drop_thr / drop_scale / drop_seed only
};

// workspace (floats, every array 16-byte aligned): what the forward keeps, then the backward's scratch
struct ImgWs {
    int64_t tok, h, st, a2, dh, dtok, de, part, total;
    static int64_t bwd_groups(int rows) { return ((int64_t)rows + kImgTileB - 1) / kImgTileB; }
    static ImgWs make(const ImgDims& d) {
        ImgWs w;
        const int64_t R = d.rows, E = d.E, F = d.F;
        int64_t p = 0;
        w.tok = p; p += round4(R * F);   // [enc | feats], enc after its ReLU
        w.h = p; p += round4(R * E);     // embed_transition's output (embed_ln's input)
        w.st = p; p += round4(R * 2);    // embed_ln's (mean, rstd)
        if (d.fwd_only) {
            w.a2 = w.dh = w.dtok = w.de = w.part = w.total = p;
            return w;
        }
        w.a2 = p; p += R * kFlat;           // conv2 activations after ReLU and dropout
        w.dh = p; p += round4(R * E);
        w.dtok = p; p += round4(R * F);
        w.de = p; p += R * kEnc;            // dL/d(fc pre-activation)
        const int64_t nch = rows_chunks(R);
        int64_t part = std::max<int64_t>(nch * (F + 1) * E, nch * 2 * E);
        part = std::max<int64_t>(part, nch * (kFlat + 1) * kEnc);
        part = std::max<int64_t>(part, bwd_groups(d.rows) * kConvPart);
        w.part = p; p += round4(part);
        w.total = p;
        return w;
    }
};

// ------------------------------------------------------------------------------ encoder forward
// grid = ceil(rows / kImgTileF).  Writes tok[row] = [relu(fc) | feats[row]] and, when a2out is given
// (a backward will follow), the dropped conv2 activations a2out[row][1600].
__global__ __launch_bounds__(kImgThreads) void img_enc_fwd(const float* __restrict__ blob,
                                                           const float* __restrict__ images,
                                                           const float* __restrict__ feats, ImgDims d,
                                                           float* __restrict__ a2out, float* __restrict__ tok) {
    __shared__ ImgEncLds s;
    const ImgBlob B = ImgBlob::make(d.F, d.E);
    const int tid = threadIdx.x;
    img_stage_weights(blob, B, s);
    const bool drop = d.drop.drop();
    const int row0 = blockIdx.x * kImgTileF;
    for (int im = 0; im < kImgTileF; ++im) {
        const int row = row0 + im;
        if (row >= d.rows) break;  // uniform over the workgroup
        __syncthreads();           // the staged weights; the previous image's readers are done
        for (int i = tid; i < kImgPix; i += kImgThreads) s.img[i] = images[(int64_t)row * kImgPix + i];
        __syncthreads();
        img_conv1(s.w1, s.img, s.a1);
        __syncthreads();
        img_conv2(s, d.drop, drop, row);
        __syncthreads();
        img_fc(blob, B, s, a2out ? a2out + (int64_t)row * kFlat : nullptr);
        __syncthreads();
        for (int f = tid; f < d.F; f += kImgThreads)
            tok[(int64_t)row * d.F + f] = f < kEnc ? img_enc_out(blob, B, s, f) : feats[(int64_t)row * d.G + (f - kEnc)];
    }
}

// de[row][j] = dtok[row][j] where the encoder's output ReLU passed (tok[row][j] > 0), else 0
__global__ void img_enc_relu_bwd(const float* __restrict__ tok, const float* __restrict__ dtok, int rows, int F,
                                 float* __restrict__ de) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * kEnc) return;
    const int64_t o = (i / kEnc) * F + i % kEnc;
    de[i] = tok[o] > 0.f ? dtok[o] : 0.f;
}

// ------------------------------------------------------------------------------ encoder backward
// grid = ceil(rows / kImgTileB); part[g] = this workgroup's conv1_w | conv1_b | conv2_w | conv2_b gradient
__global__ __launch_bounds__(kImgThreads) void img_enc_bwd(const float* __restrict__ blob,
                                                           const float* __restrict__ images,
                                                           const float* __restrict__ a2d,
                                                           const float* __restrict__ de, ImgDims d,
                                                           float* __restrict__ part) {
    __shared__ float w1[448];
    __shared__ float w2d[144 * kCh];   // conv2_w as [co 9 + ky 3 + kx][ci]: the data gradient's B operand
    __shared__ float img[kImgPix + 1];
    __shared__ float a1[kCh * kA1S];
    __shared__ float dz[kCh * kDzS];   // dL/dz2 (conv2 pre-activation), zero border of 2
    __shared__ float dz1[kCh * kA1];   // dL/dz1 (conv1 pre-activation)
    const ImgBlob B = ImgBlob::make(d.F, d.E);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i16 = lane & 15, kq = lane >> 4;
    for (int i = tid; i < 448; i += kImgThreads) w1[i] = blob[B.c1w + i];
    for (int i = tid; i < 2304; i += kImgThreads) {
        const int co = i / 144, ci = (i % 144) / 9, t = i % 9;
        w2d[(co * 9 + t) * kCh + ci] = blob[B.c2w + i];
    }
    for (int i = tid; i < kCh * kA1S; i += kImgThreads) a1[i] = 0.f;  // the pad floats stay zero
    for (int i = tid; i < kCh * kDzS; i += kImgThreads) dz[i] = 0.f;  // the border stays zero
    const bool drop = d.drop.drop();
    // accumulators over the workgroup's images: conv2_w tiles nt = wave, wave + 4, wave + 8 (co x 16
    // columns of (ci, ky, kx)); thread t's two VALU outputs t and t + 256 of [conv1_w | conv1_b | conv2_b]
    floatx4 accw[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) accw[t] = floatx4{0.f, 0.f, 0.f, 0.f};
    float accv[2] = {0.f, 0.f};
    const int row0 = blockIdx.x * kImgTileB;
    for (int im = 0; im < kImgTileB; ++im) {
        const int row = row0 + im;
        if (row >= d.rows) break;  // uniform over the workgroup
        __syncthreads();
        for (int i = tid; i < kImgPix; i += kImgThreads) img[i] = images[(int64_t)row * kImgPix + i];
        // dz2 = (de . fc_w^T) keep where the dropped activation is > 0
        float g[kEnc];
#pragma unroll
        for (int j = 0; j < kEnc; ++j) g[j] = de[(int64_t)row * kEnc + j];
        for (int i = tid; i < kFlat; i += kImgThreads) {
            const floatx4* w = reinterpret_cast<const floatx4*>(blob + B.fcw + (int64_t)i * kEnc);
            const floatx4 wa = w[0], wb = w[1];
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) v = fmaf(g[j], wa[j], v);
#pragma unroll
            for (int j = 0; j < 4; ++j) v = fmaf(g[4 + j], wb[j], v);
            if (drop) v *= tr_keep(d.drop, DPT_SITE_IMAGE_ENC, (int64_t)row * kFlat + i);
            const int c = i / kA2, p = i % kA2;
            dz[c * kDzS + (p / kC2 + 2) * kDzW + p % kC2 + 2] = a2d[(int64_t)row * kFlat + i] > 0.f ? v : 0.f;
        }
        __syncthreads();
        img_conv1(w1, img, a1);
        __syncthreads();
        // conv2 weight gradient: dW[co][n] += sum_p dz2[co][p] a1patch[p][n], n = (ci, ky, kx).  The
        // positions run as 10 rows x 12 columns (3 k-steps of 4 per row): columns 10, 11 meet dz's zero border
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int nt = wave + 4 * t;
            if (nt < 9) {
                const int n = 16 * nt + i16;
                const float* ap = dz + i16 * kDzS + 2 * kDzW + 2 + kq;
                const float* bp = a1 + (n / 9) * kA1S + ((n % 9) / 3) * kC1 + n % 3 + kq;
#pragma unroll
                for (int s = 0; s < 30; ++s)
                    accw[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[(s / 3) * kDzW + 4 * (s % 3)],
                                                                   bp[(s / 3) * kC1 + 4 * (s % 3)], accw[t], 0, 0, 0);
            }
        }
        // conv2 data gradient: da1[q][ci] = sum_{co, ky, kx} dz2[co][qy - ky][qx - kx] w2[co][ci][ky][kx] over
        // the 144 conv1 positions q (9 tiles); lane (i16, kq) holds the k run of channels co = 4 kq .. 4 kq + 3
        for (int mt = wave; mt < 9; mt += kImgThreads / 64) {
            const int q = 16 * mt + i16;
            const float* ap = dz + (4 * kq) * kDzS + (q / kC1 + 2) * kDzW + q % kC1 + 2;
            const float* bp = w2d + (36 * kq) * kCh + i16;
            floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 36; ++s)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[(s / 9) * kDzS - ((s % 9) / 3) * kDzW - s % 3], bp[s * kCh],
                                                           acc, 0, 0, 0);
            // C layout: lane (ci = i16, kq) holds positions 16 mt + 4 kq + r
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qq = 16 * mt + 4 * kq + r;
                dz1[i16 * kA1 + qq] = a1[i16 * kA1S + qq] > 0.f ? acc[r] : 0.f;
            }
        }
        __syncthreads();
        // conv1 weight gradient and the two bias gradients on the VALU
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int o = tid + kImgThreads * t;
            float acc = accv[t];
            if (o < 432) {
                const int co = o / 27, ci = (o % 27) / 9, ky = (o % 9) / 3, kx = o % 3;
                const float* in = img + ci * kImgSize * kImgSize + ky * kImgSize + kx;
                const float* gz = dz1 + co * kA1;
                for (int y = 0; y < kC1; ++y)
#pragma unroll
                    for (int x = 0; x < kC1; ++x) acc = fmaf(gz[y * kC1 + x], in[2 * y * kImgSize + 2 * x], acc);
            } else if (o < 448) {
                const float* gz = dz1 + (o - 432) * kA1;
                for (int p = 0; p < kA1; ++p) acc += gz[p];
            } else if (o < 464) {
                const float* gz = dz + (o - 448) * kDzS + 2 * kDzW + 2;
                for (int y = 0; y < kC2; ++y)
#pragma unroll
                    for (int x = 0; x < kC2; ++x) acc += gz[y * kDzW + x];
            }
            accv[t] = acc;
        }
    }
    float* pc = part + (int64_t)blockIdx.x * kConvPart;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int nt = wave + 4 * t;
        if (nt < 9) {  // C layout: lane (n = 16 nt + i16, kq) holds co = 4 kq + r
#pragma unroll
            for (int r = 0; r < 4; ++r) pc[448 + (4 * kq + r) * 144 + 16 * nt + i16] = accw[t][r];
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int o = tid + kImgThreads * t;
        if (o < 448) pc[o] = accv[t];
        else if (o < 464) pc[448 + 2304 + (o - 448)] = accv[t];
    }
}

// ------------------------------------------------------------------------------ host side
static int img_dims(const dpt_image_desc* d, ImgDims& o) {
    DPT_REQUIRE(d != nullptr, "image front: null desc");
    if (d->image_size != kImgSize) {
        set_error(DPT_EUNSUPPORTED, "image front: image_size=%d (only %d is built)", d->image_size, kImgSize);
        return DPT_EUNSUPPORTED;
    }
    DPT_REQUIRE(d->rows >= 1 && d->rows <= (1 << 26), "image front: rows=%d", d->rows);
    DPT_REQUIRE(d->n_embd >= 1 && d->n_embd <= 1024, "image front: n_embd=%d", d->n_embd);
    DPT_REQUIRE(d->state_dim >= 0 && d->state_dim <= 4096, "image front: state_dim=%d", d->state_dim);
    DPT_REQUIRE(d->action_dim >= 1 && d->action_dim <= 4096, "image front: action_dim=%d", d->action_dim);
    DPT_REQUIRE(d->dropout >= 0.0f && d->dropout < 1.0f, "image front: dropout %g outside [0, 1)", (double)d->dropout);
    DPT_REQUIRE(d->reserved == 0, "image front: reserved=%d must be 0", d->reserved);
    DPT_REQUIRE((d->flags & ~DPT_TRAIN_FORWARD_ONLY) == 0, "image front: unknown flags 0x%x", d->flags);
    o.rows = d->rows;
    o.G = d->state_dim + d->action_dim + 1;
    o.F = kEnc + o.G;
    o.E = d->n_embd;
    o.fwd_only = (d->flags & DPT_TRAIN_FORWARD_ONLY) ? 1 : 0;
    o.drop = TrDims{};
    o.drop.drop_seed = d->dropout_seed;
    drop_params(d->dropout, o.drop.drop_thr, o.drop.drop_scale);
    return DPT_OK;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace dpt

using namespace dpt;

extern "C" {

int dpt_image_front_blob_numel(const dpt_image_desc* d, int64_t* numel) {
    ImgDims t;
    if (int rc = img_dims(d, t)) return rc;
    DPT_REQUIRE(numel != nullptr, "image front: null numel");
    *numel = ImgBlob::make(t.F, t.E).total;
    return DPT_OK;
}

int dpt_image_front_workspace_numel(const dpt_image_desc* d, int64_t* numel) {
    ImgDims t;
    if (int rc = img_dims(d, t)) return rc;
    DPT_REQUIRE(numel != nullptr, "image front: null numel");
    *numel = ImgWs::make(t).total;
    return DPT_OK;
}

int dpt_image_front_forward(const dpt_image_desc* d, const float* blob, const float* images, const float* feats,
                            float* ws, float* embeds, void* stream) {
    ImgDims t;
    if (int rc = img_dims(d, t)) return rc;
    DPT_REQUIRE(blob && images && feats && ws && embeds, "image front forward: null pointer");
    DPT_REQUIRE(aligned16(ws), "image front forward: workspace not 16-byte aligned");
    DPT_REQUIRE(aligned16(blob), "image front forward: front blob not 16-byte aligned");
    const ImgBlob B = ImgBlob::make(t.F, t.E);
    const ImgWs W = ImgWs::make(t);
    hipStream_t st = as_stream(stream);
    const unsigned groups = (unsigned)(((int64_t)t.rows + kImgTileF - 1) / kImgTileF);
    hipLaunchKernelGGL(img_enc_fwd, dim3(groups), dim3(kImgThreads), 0, st, blob, images, feats, t,
                       t.fwd_only ? (float*)nullptr : ws + W.a2, ws + W.tok);
    if (int rc = launched("img_enc_fwd")) return rc;
    if (int rc = rows_linear(ws + W.tok, blob + B.embw, blob + B.embb, t.rows, t.F, t.E, ws + W.h, st)) return rc;
    return rows_layernorm(ws + W.h, blob + B.lng, blob + B.lnb, t.rows, t.E, embeds, ws + W.st, st);
}

int dpt_image_front_backward(const dpt_image_desc* d, const float* blob, const float* images, const float* feats,
                             float* ws, const float* dembeds, float* dblob, void* stream) {
    ImgDims t;
    if (int rc = img_dims(d, t)) return rc;
    DPT_REQUIRE(blob && images && feats && ws && dembeds && dblob, "image front backward: null pointer");
    DPT_REQUIRE(!t.fwd_only, "image front backward: the description is forward-only (DPT_TRAIN_FORWARD_ONLY)");
    DPT_REQUIRE(aligned16(ws), "image front backward: workspace not 16-byte aligned");
    DPT_REQUIRE(aligned16(blob), "image front backward: front blob not 16-byte aligned");
    const ImgBlob B = ImgBlob::make(t.F, t.E);
    const ImgWs W = ImgWs::make(t);
    hipStream_t st = as_stream(stream);
    const int R = t.rows, E = t.E, F = t.F;
    float* part = ws + W.part;
    // embed_ln, then embed_transition
    if (int rc = rows_ln_param_grad(ws + W.h, ws + W.st, dembeds, R, E, part, dblob + B.lng, dblob + B.lnb, st)) return rc;
    if (int rc = rows_layernorm_bwd(ws + W.h, ws + W.st, blob + B.lng, dembeds, R, E, ws + W.dh, st)) return rc;
    if (int rc = rows_wgrad(ws + W.tok, ws + W.dh, R, F, E, part, dblob + B.embw, dblob + B.embb, st)) return rc;
    if (int rc = rows_linear_bwd_data(ws + W.dh, blob + B.embw, R, F, E, ws + W.dtok, st)) return rc;
    // the encoder's output ReLU, then the fc weight gradient over the dropped conv2 activations
    const int64_t ne = (int64_t)R * kEnc;
    hipLaunchKernelGGL(img_enc_relu_bwd, dim3((unsigned)((ne + kImgThreads - 1) / kImgThreads)), dim3(kImgThreads), 0, st,
                       ws + W.tok, ws + W.dtok, R, F, ws + W.de);
    if (int rc = launched("img_enc_relu_bwd")) return rc;
    if (int rc = rows_wgrad(ws + W.a2, ws + W.de, R, kFlat, kEnc, part, dblob + B.fcw, dblob + B.fcb, st)) return rc;
    // the convolutions: one partial per workgroup, then the fixed-order sum.  The 2768 floats of a partial
    // are the blob's first four arrays in order, reduced as a (172 + 1) x 16 product: conv2_b is its bias row
    const int groups = (int)ImgWs::bwd_groups(R);
    hipLaunchKernelGGL(img_enc_bwd, dim3(groups), dim3(kImgThreads), 0, st, blob, images, ws + W.a2, ws + W.de, t, part);
    if (int rc = launched("img_enc_bwd")) return rc;
    static_assert(kConvPart == 173 * 16, "conv partial = 173 rows of 16");
    return rows_reduce_parts(part, groups, 172, 16, dblob + B.c1w, dblob + B.c2b, st);
}

}  // extern "C"
