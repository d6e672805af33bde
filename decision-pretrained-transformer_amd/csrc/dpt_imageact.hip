// Deployment of the image-conditioned DPT (include/dpt_hip.h, "image act step"): the reference's
// MiniworldTransformerController.act (ctrls/ctrl_miniworld.py:68-113) without its per-step waste.
//
//   dpt_image_obs_tables     : host, double precision.  skimage's anti-aliased resize to 25 x 25 restated as
//                              two banded 25 x n_in tables R = Z G (Gaussian blur with mirrored edges,
//                              then the order-1 zoom at half-pixel centres).
//   obs_preprocess_kernel    : one workgroup per raw uint8 frame: the column pass into LDS, the row
//                              pass, the division by 255 and the ImageNet normalisation, all in
//                              fp64 with one rounding on the store.  A channel at a time, so the fp64
//                              intermediate is 25 x in_w doubles (25.6 KB at the widest frame).
//   act_front_kernel         : one workgroup per env does the whole per-step front: the same resize
//                              (obs_resize, shared with the kernel above) straight into the encoder's LDS
//                              image and into obs_out, conv1 / conv2 (MFMA implicit GEMM) / the 1600 -> 8
//                              product through the device functions of img_enc_fwd (dpt_image_enc.h),
//                              embed_transition on [enc | angle | 0_A | 0] in tr_linear's order, embed_ln
//                              in tr_layernorm_rows' / tr_layernorm's order, and the row into position 0
//                              of the env's sequence.  img_enc_fwd takes four images per workgroup in
//                              turn, the wrong shape for 20..100 rows on 256 CUs; here every env has its
//                              own workgroup.
//   LDS of act_front_kernel  : the encoder's 34.6 KB + 25.6 KB fp64 intermediate = 60.2 KB
//                              (under the 64 KB a workgroup may take; one or two workgroups per CU is
//                              all a grid of B <= a few hundred needs).  The raw frame (up to 48 KB) is
//                              NOT staged: the column pass reads it from global memory, each byte by the
//                              few output rows whose band covers it, which the L1/L2 serve.  After the
//                              resize the intermediate's space holds the token row and the pre-LayerNorm row.
//
// The context rows are encoded once per episode by dpt_image_front_forward and scattered into rows
// 1..C of embeds; the step then runs dpt_train_forward_embeds (forward-only, last position only).
#include <algorithm>
#include <cmath>
#include <vector>

#include "dpt_image_enc.h"

namespace dpt {

constexpr int kObsOut = DPT_OBS_OUT, kObsArea = kObsOut * kObsOut;
constexpr int kObsTmp = kObsOut * DPT_OBS_MAX_SIDE;  // doubles: one channel's column pass at the widest frame
constexpr int kActRowFloats = 2 * kObsTmp;           // floats the intermediate's space holds afterwards (6400)
static_assert(kObsOut == kImgSize, "the resize feeds the 25 x 25 encoder");

// train.py:224-228: the ImageNet statistics of dataset.image_transform (as dpt_image_normalize)
__device__ inline double obs_mean(int c) { return c == 0 ? 0.485 : c == 1 ? 0.456 : 0.406; }
__device__ inline double obs_std(int c) { return c == 0 ? 0.229 : c == 1 ? 0.224 : 0.225; }

struct alignas(16) ObsLds {
    double tmp[kObsTmp];  // tmp[oy][x] of the channel in flight
};
constexpr int kObsTaps = 8;  // taps a round: the loads of a round are in flight together

// The band of output o over an axis of n_in samples, clamped to the axis: the table lives in device
// memory the host cannot check, and a wrong one must not read outside the frame.
__device__ inline void obs_band(const int32_t* __restrict__ first, const int32_t* __restrict__ count, int o, int n_in,
                                int& lo, int& cnt) {
    lo = min(max(first[o], 0), n_in - 1);
    cnt = min(min(max(count[o], 0), DPT_OBS_BAND), n_in - lo);
}

// One frame (in_h, in_w, 3) uint8 -> (3, 25, 25) normalised fp32 into out_g (global) and, when given,
// out_lds.  Both passes run on the integer samples (R is linear: one IEEE division by 255 per output
// instead of one per sample, and at the identity tables of 25 x 25 the quotient is float64(x) / 255 to
// the bit).  Ends with a barrier.
__device__ inline void obs_resize(const uint8_t* __restrict__ frame, int in_h, int in_w,
                                  const dpt_obs_tables* __restrict__ tab, ObsLds& s, float* __restrict__ out_lds,
                                  float* __restrict__ out_g) {
    const int tid = threadIdx.x;
    for (int c = 0; c < 3; ++c) {
        // column pass: tmp[oy][x] = sum_k wy[oy][k] frame[lo + k][x][c]
        for (int i = tid; i < kObsOut * in_w; i += kImgThreads) {
            const int oy = i / in_w, x = i % in_w;
            int lo, cnt;
            obs_band(tab->first_y, tab->count_y, oy, in_h, lo, cnt);
            const uint8_t* p = frame + ((int64_t)lo * in_w + x) * 3 + c;
            const double* w = tab->wy[oy];
            double acc = 0.0;
            // kObsTaps taps a round, so that their byte loads are in flight together: a tap past the band
            // re-reads the band's last sample with the table's zero weight (fma(0, v, acc) = acc exactly)
            for (int k0 = 0; k0 < cnt; k0 += kObsTaps) {
                uint8_t px[kObsTaps];
#pragma unroll
                for (int j = 0; j < kObsTaps; ++j) px[j] = p[(int64_t)min(k0 + j, cnt - 1) * in_w * 3];
#pragma unroll
                for (int j = 0; j < kObsTaps; ++j) acc = fma(w[min(k0 + j, DPT_OBS_BAND - 1)], (double)px[j], acc);
            }
            s.tmp[i] = acc;
        }
        __syncthreads();
        // row pass and normalisation: one rounding, on the store
        for (int i = tid; i < kObsArea; i += kImgThreads) {
            const int oy = i / kObsOut, ox = i % kObsOut;
            int lo, cnt;
            obs_band(tab->first_x, tab->count_x, ox, in_w, lo, cnt);
            const double* t = s.tmp + oy * in_w + lo;
            const double* w = tab->wx[ox];
            double acc = 0.0;
            for (int k0 = 0; k0 < cnt; k0 += kObsTaps) {
#pragma unroll
                for (int j = 0; j < kObsTaps; ++j)
                    acc = fma(w[min(k0 + j, DPT_OBS_BAND - 1)], t[min(k0 + j, cnt - 1)], acc);
            }
            const float v = (float)((acc / 255.0 - obs_mean(c)) / obs_std(c));
            if (out_lds) out_lds[c * kObsArea + i] = v;
            out_g[c * kObsArea + i] = v;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kImgThreads) void obs_preprocess_kernel(const uint8_t* __restrict__ frames, int in_h,
                                                                     int in_w, const dpt_obs_tables* __restrict__ tab,
                                                                     float* __restrict__ out) {
    __shared__ ObsLds s;
    const int64_t n = blockIdx.x;
    obs_resize(frames + n * in_h * in_w * 3, in_h, in_w, tab, s, nullptr, out + n * kImgPix);
}

struct ActDims {
    int B, T, sd, A, F, E, in_h, in_w;  // T = 1 + C tokens per sequence, F = 8 + sd + A + 1
};

// grid = B.  embeds[b][0] = embed_ln(embed_transition([enc(resize(frame b)) | query_states[b] | 0_A | 0]))
__global__ __launch_bounds__(kImgThreads) void act_front_kernel(const float* __restrict__ blob,
                                                                const uint8_t* __restrict__ frames,
                                                                const dpt_obs_tables* __restrict__ tab,
                                                                const float* __restrict__ query_states, ActDims d,
                                                                float* __restrict__ obs_out, float* __restrict__ embeds) {
    __shared__ ImgEncLds s;
    __shared__ ObsLds o;
    const ImgBlob B = ImgBlob::make(d.F, d.E);
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t b = blockIdx.x;
    const int E = d.E, F = d.F;
    img_stage_weights(blob, B, s);
    __syncthreads();
    obs_resize(frames + b * d.in_h * d.in_w * 3, d.in_h, d.in_w, tab, o, s.img, obs_out + b * kImgPix);
    img_conv1(s.w1, s.img, s.a1);
    __syncthreads();
    const TrDims nodrop{};
    img_conv2(s, nodrop, false, 0);
    __syncthreads();
    img_fc(blob, B, s, nullptr);
    __syncthreads();
    // the fp64 intermediate is done with: its space holds the pre-LayerNorm row h[E] (16-byte aligned)
    // and the token row tok[F] (the host checks round4(E) + F <= kActRowFloats)
    float* h = reinterpret_cast<float*>(o.tmp);
    float* tok = h + ((E + 3) & ~3);
    for (int f = tid; f < F; f += kImgThreads)
        tok[f] = f < kEnc ? img_enc_out(blob, B, s, f) : f - kEnc < d.sd ? query_states[b * d.sd + (f - kEnc)] : 0.f;
    __syncthreads();
    // embed_transition, tr_linear's order
    for (int e = tid; e < E; e += kImgThreads) {
        float acc = blob[B.embb + e];
        for (int f = 0; f < F; ++f) acc = fmaf(tok[f], blob[B.embw + (int64_t)f * E + e], acc);
        h[e] = acc;
    }
    __syncthreads();
    if (tid >= 64) return;  // embed_ln on one wave, in the order rows_layernorm takes for this E
    const float* g = blob + B.lng;
    const float* bb = blob + B.lnb;
    float* y = embeds + b * d.T * E;
    if (E % 4 == 0 && E <= 256) {  // tr_layernorm_rows: a float4 per lane, an xor tree over the row's lanes
        int lpr = 1;
        while (lpr < E / 4) lpr <<= 1;
        const bool act = lane < (E >> 2);
        const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
        const floatx4 v = act ? reinterpret_cast<const floatx4*>(h)[lane] : zero;
        float sum = (v[0] + v[1]) + (v[2] + v[3]);
        for (int k = 1; k < lpr; k <<= 1) sum += __shfl_xor(sum, k, 64);
        const float mean = sum / E;
        const floatx4 dv = act ? v - mean : zero;
        float q = (dv[0] * dv[0] + dv[1] * dv[1]) + (dv[2] * dv[2] + dv[3] * dv[3]);
        for (int k = 1; k < lpr; k <<= 1) q += __shfl_xor(q, k, 64);
        const float rstd = 1.0f / sqrtf(q / E + 1e-5f);
        if (act) {
            floatx4 out;
#pragma unroll
            for (int r = 0; r < 4; ++r) out[r] = dv[r] * rstd * g[4 * lane + r] + bb[4 * lane + r];
            reinterpret_cast<floatx4*>(y)[lane] = out;
        }
    } else {  // tr_layernorm: lane-strided sums, a full-wave tree
        float sum = 0.f;
        for (int e = lane; e < E; e += 64) sum += h[e];
        const float mean = img_wave_sum(sum) / E;
        float q = 0.f;
        for (int e = lane; e < E; e += 64) q += (h[e] - mean) * (h[e] - mean);
        const float rstd = 1.0f / sqrtf(img_wave_sum(q) / E + 1e-5f);
        for (int e = lane; e < E; e += 64) y[e] = (h[e] - mean) * rstd * g[e] + bb[e];
    }
}

// embeds[b][1 + j][:] = ctx[b C + j][:]
__global__ void act_scatter_context(const float* __restrict__ ctx, int64_t n, int C, int E, float* __restrict__ embeds) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t per = (int64_t)C * E, b = i / per;
    embeds[(b * (C + 1) + 1) * E + i % per] = ctx[i];
}

// logits[b][:] = preds[b][T - 1][:]
__global__ void act_last_logits(const float* __restrict__ preds, int B, int T, int A, float* __restrict__ logits) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * A) return;
    logits[i] = preds[((i / A) * T + T - 1) * A + i % A];
}

// ------------------------------------------------------------------------------ host side
static bool act_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int obs_sides(const char* who, int32_t in_h, int32_t in_w) {
    if (in_h < DPT_OBS_MIN_SIDE || in_h > DPT_OBS_MAX_SIDE || in_w < DPT_OBS_MIN_SIDE || in_w > DPT_OBS_MAX_SIDE) {
        set_error(DPT_EUNSUPPORTED, "%s: frame %d x %d (sides %d..%d are built)", who, in_h, in_w, DPT_OBS_MIN_SIDE,
                  DPT_OBS_MAX_SIDE);
        return DPT_EUNSUPPORTED;
    }
    return DPT_OK;
}

// one axis: R = Z G as banded rows
static int obs_axis(int n_in, int32_t* first, int32_t* count, double (*w)[DPT_OBS_BAND]) {
    const int n = n_in;
    const double f = (double)n / kObsOut;
    const double sigma = std::max(0.0, (f - 1.0) / 2.0);
    const int r = (int)(4.0 * sigma + 0.5);
    auto mirror = [n](int j) {  // reflect about the edge samples, not repeating them
        const int period = 2 * (n - 1);
        j = j < 0 ? -j : j;
        j %= period;
        return j > n - 1 ? period - j : j;
    };
    std::vector<double> G((size_t)n * n, 0.0), R((size_t)kObsOut * n, 0.0);
    if (sigma > 0.0) {
        std::vector<double> k(2 * r + 1);
        double sum = 0.0;
        for (int t = -r; t <= r; ++t) sum += k[t + r] = std::exp(-0.5 / (sigma * sigma) * t * t);
        for (int i = 0; i < n; ++i)
            for (int t = -r; t <= r; ++t) G[(size_t)i * n + mirror(i + t)] += k[t + r] / sum;
    } else {
        for (int i = 0; i < n; ++i) G[(size_t)i * n + i] = 1.0;
    }
    for (int o = 0; o < kObsOut; ++o) {
        double x = std::fabs((o + 0.5) * f - 0.5);
        if (x > n - 1) x = 2.0 * (n - 1) - x;
        const int i0 = (int)std::floor(x);
        const double t = x - i0;
        double* row = &R[(size_t)o * n];
        for (int j = 0; j < n; ++j) {
            double v = (1.0 - t) * G[(size_t)i0 * n + j];
            if (t > 0.0 && i0 + 1 < n) v += t * G[(size_t)(i0 + 1) * n + j];
            row[j] = v;
        }
        int lo = 0, hi = n - 1;
        while (lo < hi && row[lo] == 0.0) ++lo;
        while (hi > lo && row[hi] == 0.0) --hi;
        if (hi - lo + 1 > DPT_OBS_BAND) {
            set_error(DPT_EUNSUPPORTED, "obs tables: a band of %d weights at side %d (at most %d)", hi - lo + 1, n,
                      DPT_OBS_BAND);
            return DPT_EUNSUPPORTED;
        }
        first[o] = lo;
        count[o] = hi - lo + 1;
        for (int k = 0; k < DPT_OBS_BAND; ++k) w[o][k] = k <= hi - lo ? row[lo + k] : 0.0;
    }
    return DPT_OK;
}

struct ActWs {
    int64_t front, ctx, trunk, preds, total;
};

static dpt_train_desc act_train_desc(const dpt_image_act_desc* d, int32_t C) {
    dpt_train_desc t{};
    t.n_layer = d->n_layer;
    t.n_embd = d->n_embd;
    t.state_dim = d->state_dim;
    t.action_dim = d->action_dim;
    t.n_positions = d->n_positions;
    t.batch = d->batch;
    t.window = 1 + C;
    t.reserved = DPT_TRAIN_FORWARD_ONLY | DPT_TRAIN_LAST_ONLY;
    return t;
}

static dpt_image_desc act_front_desc(const dpt_image_act_desc* d, int32_t C) {
    dpt_image_desc f{};
    f.image_size = d->image_size;
    f.rows = d->batch * C;
    f.state_dim = d->state_dim;
    f.action_dim = d->action_dim;
    f.n_embd = d->n_embd;
    f.flags = DPT_TRAIN_FORWARD_ONLY;
    return f;
}

// every check of the description the three entry points share, then the workspace layout for max_context
static int act_check(const char* who, const dpt_image_act_desc* d, ActWs& w) {
    DPT_REQUIRE(d != nullptr, "%s: null desc", who);
    if (d->image_size != kImgSize) {
        set_error(DPT_EUNSUPPORTED, "%s: image_size=%d (only %d is built)", who, d->image_size, kImgSize);
        return DPT_EUNSUPPORTED;
    }
    if (int rc = obs_sides(who, d->in_h, d->in_w)) return rc;
    DPT_REQUIRE(d->batch >= 1, "%s: batch=%d", who, d->batch);
    DPT_REQUIRE(d->max_context >= 0, "%s: max_context=%d", who, d->max_context);
    DPT_REQUIRE(d->n_positions >= 1 && (int64_t)1 + d->max_context <= d->n_positions,
                "%s: window 1 + %d above n_positions=%d", who, d->max_context, d->n_positions);
    DPT_REQUIRE((int64_t)d->batch * (1 + (int64_t)d->max_context) <= (1 << 26), "%s: batch=%d max_context=%d", who,
                d->batch, d->max_context);
    DPT_REQUIRE(d->dropout == 0.0f, "%s: dropout=%g (the act step is inference: dropout must be 0)", who,
                (double)d->dropout);
    DPT_REQUIRE(d->reserved == 0, "%s: reserved=%d must be 0", who, d->reserved);
    DPT_REQUIRE(d->n_embd >= 1 && d->state_dim >= 0 && d->action_dim >= 1, "%s: n_embd=%d sd=%d A=%d", who, d->n_embd,
                d->state_dim, d->action_dim);
    const int64_t F = (int64_t)kEnc + d->state_dim + d->action_dim + 1;
    if (round4(d->n_embd) + F > kActRowFloats) {
        set_error(DPT_EUNSUPPORTED, "%s: token of %lld features at n_embd=%d does not fit the front kernel's row space",
                  who, (long long)F, d->n_embd);
        return DPT_EUNSUPPORTED;
    }
    const int32_t C = d->max_context;
    const int64_t B = d->batch, E = d->n_embd;
    int64_t nfront = 0, ntrunk = 0;
    if (C > 0) {
        const dpt_image_desc fd = act_front_desc(d, C);
        if (int rc = dpt_image_front_workspace_numel(&fd, &nfront)) return rc;
    }
    const dpt_train_desc td = act_train_desc(d, C);
    if (int rc = dpt_train_workspace_numel(&td, &ntrunk)) return rc;
    int64_t p = 0;
    w.front = p; p += round4(nfront);
    w.ctx = p; p += round4(B * C * E);
    w.trunk = p; p += round4(ntrunk);
    w.preds = p; p += round4(B * (1 + C) * d->action_dim);
    w.total = p;
    return DPT_OK;
}

static int act_check_context(const char* who, const dpt_image_act_desc* d, int32_t C) {
    DPT_REQUIRE(C >= 0, "%s: C=%d", who, C);
    DPT_REQUIRE((int64_t)1 + C <= d->n_positions, "%s: window 1 + %d above n_positions=%d", who, C, d->n_positions);
    DPT_REQUIRE(C <= d->max_context, "%s: C=%d above desc.max_context=%d", who, C, d->max_context);
    return DPT_OK;
}

}  // namespace dpt

using namespace dpt;

extern "C" {

int dpt_image_obs_tables(int32_t in_h, int32_t in_w, dpt_obs_tables* t) {
    DPT_REQUIRE(t != nullptr, "obs tables: null output");
    if (int rc = obs_sides("obs tables", in_h, in_w)) return rc;
    t->in_h = in_h;
    t->in_w = in_w;
    if (int rc = obs_axis(in_h, t->first_y, t->count_y, t->wy)) return rc;
    return obs_axis(in_w, t->first_x, t->count_x, t->wx);
}

int dpt_image_obs_preprocess(const uint8_t* frames, int64_t n, int32_t in_h, int32_t in_w,
                             const dpt_obs_tables* tables, float* out, void* stream) {
    DPT_REQUIRE(frames && tables && out, "obs preprocess: null pointer");
    DPT_REQUIRE(n >= 0 && n < (1ll << 31), "obs preprocess: n=%lld", (long long)n);
    if (int rc = obs_sides("obs preprocess", in_h, in_w)) return rc;
    if (n == 0) return DPT_OK;
    hipLaunchKernelGGL(obs_preprocess_kernel, dim3((unsigned)n), dim3(kImgThreads), 0, as_stream(stream), frames, in_h,
                       in_w, tables, out);
    return launched("obs_preprocess");
}

int dpt_image_act_workspace_numel(const dpt_image_act_desc* d, int64_t* numel) {
    ActWs w;
    if (int rc = act_check("image act workspace", d, w)) return rc;
    DPT_REQUIRE(numel != nullptr, "image act workspace: null numel");
    *numel = w.total;
    return DPT_OK;
}

int dpt_image_act_set_context(const dpt_image_act_desc* d, int32_t C, const float* front, const float* images,
                              const float* feats, float* ws, float* embeds, void* stream) {
    const char* who = "image act context";
    ActWs w;
    if (int rc = act_check(who, d, w)) return rc;
    if (int rc = act_check_context(who, d, C)) return rc;
    DPT_REQUIRE(front && ws && embeds && (C == 0 || (images && feats)), "%s: null pointer", who);
    DPT_REQUIRE(act_aligned16(ws) && act_aligned16(front) && act_aligned16(embeds),
                "%s: workspace, front blob or embeds not 16-byte aligned", who);
    if (C == 0) return DPT_OK;
    const dpt_image_desc fd = act_front_desc(d, C);
    if (int rc = dpt_image_front_forward(&fd, front, images, feats, ws + w.front, ws + w.ctx, stream)) return rc;
    const int64_t n = (int64_t)d->batch * C * d->n_embd;
    hipLaunchKernelGGL(act_scatter_context, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream),
                       ws + w.ctx, n, C, d->n_embd, embeds);
    return launched("act_scatter_context");
}

int dpt_image_act_step(const dpt_image_act_desc* d, int32_t C, const float* trunk, const float* front,
                       const uint8_t* frames, const dpt_obs_tables* tables, const float* query_states, float* ws,
                       float* embeds, float* obs_out, float* logits, void* stream) {
    const char* who = "image act step";
    ActWs w;
    if (int rc = act_check(who, d, w)) return rc;
    if (int rc = act_check_context(who, d, C)) return rc;
    DPT_REQUIRE(trunk && front && frames && tables && ws && embeds && obs_out && logits &&
                    (query_states || d->state_dim == 0),
                "%s: null pointer", who);
    DPT_REQUIRE(act_aligned16(ws) && act_aligned16(front) && act_aligned16(embeds),
                "%s: workspace, front blob or embeds not 16-byte aligned", who);
    DPT_REQUIRE(trunk != front, "%s: the trunk blob and the front blob are one buffer", who);
    const dpt_train_desc td = act_train_desc(d, C);
    int64_t ntrunk = 0;
    if (int rc = dpt_train_workspace_numel(&td, &ntrunk)) return rc;  // the trunk's own checks, before the launch
    ActDims a;
    a.B = d->batch;
    a.T = 1 + C;
    a.sd = d->state_dim;
    a.A = d->action_dim;
    a.F = kEnc + d->state_dim + d->action_dim + 1;
    a.E = d->n_embd;
    a.in_h = d->in_h;
    a.in_w = d->in_w;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(act_front_kernel, dim3((unsigned)a.B), dim3(kImgThreads), 0, st, front, frames, tables,
                       query_states, a, obs_out, embeds);
    if (int rc = launched("act_front")) return rc;
    if (int rc = dpt_train_forward_embeds(&td, trunk, embeds, ws + w.trunk, ws + w.preds, stream)) return rc;
    const int64_t n = (int64_t)a.B * a.A;
    hipLaunchKernelGGL(act_last_logits, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ws + w.preds, a.B, a.T,
                       a.A, logits);
    return launched("act_last_logits");
}

}  // extern "C"
