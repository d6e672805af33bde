// The training step of the image-conditioned DPT (include/dpt_hip.h, "image training step"): the
// reference's image normalisation on the device, batch packing from a device-resident image set, and
// the entry points that chain pack -> image front end -> trunk on embeds -> cross-entropy -> the two
// backwards -> AdamW on the trunk blob and on the front blob, on one stream without a host
// synchronisation.  Nothing here allocates: every buffer is the caller's.
//
// Both kernels only move data (the normalisation adds one subtraction and one division per element):
// they are bound by their loads and stores.  The normalisation is bit-equal to dataset.image_transform
// followed by .float(): the subtraction and the IEEE division run in the input's dtype with the
// constants rounded to that dtype (no contraction: -ffp-contract=off), then one rounding to fp32.
#include "dpt_common.h"

namespace dpt {

constexpr int kIsThreads = 256;
constexpr int kIsSize = 25, kIsArea = kIsSize * kIsSize, kIsPix = 3 * kIsArea;  // 1875 floats = 7500 B an image

// train.py:224-228: the ImageNet statistics of dataset.image_transform
__device__ inline double is_mean(int c) { return c == 0 ? 0.485 : c == 1 ? 0.456 : 0.406; }
__device__ inline double is_std(int c) { return c == 0 ? 0.229 : c == 1 ? 0.224 : 0.225; }

// ----------------------------------------------------------------------------- normalise
// One thread per pixel: its three channels are contiguous in the HWC input and 625 floats apart in the
// CHW output, so a wave reads 192 contiguous values and writes three runs of 64.  Scalar accesses:
// correct at every alignment of `raw` and `out`.
template <typename T>
__global__ __launch_bounds__(kIsThreads) void is_normalize_kernel(const T* __restrict__ raw, int64_t npix,
                                                                  float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kIsThreads + threadIdx.x;
    if (i >= npix) return;
    const int64_t img = i / kIsArea;
    const int p = (int)(i % kIsArea);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const T x = raw[3 * i + c];
        out[img * kIsPix + c * kIsArea + p] = (float)((x - (T)is_mean(c)) / (T)is_std(c));
    }
}

// ----------------------------------------------------------------------------- pack
// One workgroup per sequence row (b, t): its image (1875 floats), its features [state | action |
// reward] and, at t = 0, the sequence's target row.  Row 0 = the query ([query_state | 0_A | 0]), row
// 1 + j = transition perm[b][j] (or j) of sample index[b].  A sample or permutation index outside its
// range reads nothing and packs zeros.  An image is 7500 B: source and destination are 16-byte
// aligned only at every fourth image, so the copy takes 16-byte accesses where both sides reach a
// 16-byte boundary after the same 0..3 leading floats, and single floats otherwise.
__global__ __launch_bounds__(kIsThreads) void is_pack_kernel(dpt_image_data data, const int64_t* __restrict__ index,
                                                             const int64_t* __restrict__ perm, int T, int sd, int A,
                                                             float* __restrict__ images, float* __restrict__ feats,
                                                             float* __restrict__ targets) {
    const int64_t row = blockIdx.x;
    const int t = (int)(row % T);
    const int64_t b = row / T;
    const int tid = threadIdx.x;
    const int64_t H = data.horizon;
    const int64_t s = index[b];
    const bool sample = s >= 0 && s < data.n;
    int64_t j = 0;
    if (t > 0) j = perm ? perm[b * H + (t - 1)] : (int64_t)(t - 1);
    const bool live = sample && (t == 0 || (j >= 0 && j < H));
    const int64_t r = s * H + j;  // the context transition; read only when live and t > 0

    if (t == 0)
        for (int a = tid; a < A; a += kIsThreads) targets[b * A + a] = sample ? data.optimal_actions[s * A + a] : 0.f;

    const int G = sd + A + 1;
    for (int f = tid; f < G; f += kIsThreads) {
        float v = 0.f;
        if (live) {
            if (t == 0) {
                if (f < sd) v = data.query_states[s * sd + f];
            } else if (f < sd) {
                v = data.context_states[r * sd + f];
            } else if (f < sd + A) {
                v = data.context_actions[r * A + (f - sd)];
            } else {
                v = data.context_rewards[r];
            }
        }
        feats[row * G + f] = v;
    }

    float* dst = images + row * kIsPix;
    if (!live) {
        for (int i = tid; i < kIsPix; i += kIsThreads) dst[i] = 0.f;
        return;
    }
    const float* src = t == 0 ? data.query_images + s * kIsPix : data.context_images + r * kIsPix;
    const int head = (int)(((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) >> 2);  // floats up to dst's boundary
    if (((reinterpret_cast<uintptr_t>(src) + 4 * head) & 15) != 0) {                      // uniform over the workgroup
        for (int i = tid; i < kIsPix; i += kIsThreads) dst[i] = src[i];
        return;
    }
    const int n4 = (kIsPix - head) / 4;
    const floatx4* s4 = reinterpret_cast<const floatx4*>(src + head);
    floatx4* d4 = reinterpret_cast<floatx4*>(dst + head);
    for (int i = tid; i < n4; i += kIsThreads) d4[i] = s4[i];
    const int rest = kIsPix - head - 4 * n4;  // 0..3 trailing floats
    if (tid < head) dst[tid] = src[tid];
    else if (tid < head + rest) dst[4 * n4 + tid] = src[4 * n4 + tid];
}

// workspace of dpt_image_train_step for desc.batch sequences (floats; every region 16-byte aligned)
struct ImageStepWs {
    int64_t images, feats, targets, embeds, dembeds, preds, dpreds, front, trunk, dfront, dtrunk, partial, total;
    int64_t nfront, ntrunk;  // the two blobs' floats
};

static dpt_image_desc image_desc_of(const dpt_train_desc* d, int32_t batch, int32_t image_size, int32_t flags) {
    dpt_image_desc f{};
    f.image_size = image_size;
    f.rows = batch * d->window;
    f.state_dim = d->state_dim;
    f.action_dim = d->action_dim;
    f.n_embd = d->n_embd;
    f.flags = flags;
    f.dropout = d->dropout;
    f.reserved = 0;
    f.dropout_seed = d->dropout_seed;
    return f;
}

static int image_step_ws(const dpt_train_desc* d, ImageStepWs& w) {
    DPT_REQUIRE(d->batch >= 1 && d->window >= 1 && (int64_t)d->batch * d->window <= (1 << 26),
                "image train step: batch=%d window=%d", d->batch, d->window);
    const dpt_image_desc f = image_desc_of(d, d->batch, kIsSize, 0);
    int64_t nfws = 0, ntws = 0;
    if (int rc = dpt_image_front_workspace_numel(&f, &nfws)) return rc;
    if (int rc = dpt_image_front_blob_numel(&f, &w.nfront)) return rc;
    if (int rc = dpt_train_workspace_numel(d, &ntws)) return rc;
    if (int rc = dpt_train_blob_numel(d, &w.ntrunk)) return rc;
    const int64_t R = (int64_t)d->batch * d->window, B = d->batch, A = d->action_dim, E = d->n_embd;
    const int64_t G = (int64_t)d->state_dim + A + 1;
    int64_t p = 0;
    w.images = p; p += round4(R * kIsPix);
    w.feats = p; p += round4(R * G);
    w.targets = p; p += round4(B * A);
    w.embeds = p; p += round4(R * E);
    w.dembeds = p; p += round4(R * E);
    w.preds = p; p += round4(R * A);
    w.dpreds = p; p += round4(R * A);
    w.front = p; p += round4(nfws);
    w.trunk = p; p += round4(ntws);
    w.dfront = p; p += round4(w.nfront);
    w.dtrunk = p; p += round4(w.ntrunk);
    w.partial = p; p += round4(2 * B);  // B doubles
    w.total = p;
    return DPT_OK;
}

static int check_image_data(const char* who, const dpt_train_desc* d, const dpt_image_data* data) {
    DPT_REQUIRE(data->query_states && data->context_states && data->context_actions && data->context_rewards &&
                    data->optimal_actions && data->query_images && data->context_images,
                "%s: null dataset array", who);
    DPT_REQUIRE(data->n >= 1 && data->horizon >= 0, "%s: n=%lld horizon=%d", who, (long long)data->n, data->horizon);
    DPT_REQUIRE((int64_t)d->window == 1 + (int64_t)data->horizon, "%s: desc.window=%d != 1 + horizon=%d", who,
                d->window, data->horizon);
    if (data->image_size != kIsSize) {
        set_error(DPT_EUNSUPPORTED, "%s: image_size=%d (only %d is built)", who, data->image_size, kIsSize);
        return DPT_EUNSUPPORTED;
    }
    return DPT_OK;
}

// the checks the step and the eval loss share, in the header's order
static int check_image_step(const char* who, const dpt_train_desc* d, const dpt_image_data* data,
                            const int64_t* index, int32_t batch) {
    DPT_REQUIRE(d && data && index, "%s: null desc / data / index", who);
    DPT_REQUIRE(batch >= 1 && batch <= d->batch, "%s: batch=%d outside 1..desc.batch=%d", who, batch, d->batch);
    DPT_REQUIRE(d->reserved == 0, "%s: desc flags must be 0 (got 0x%x)", who, d->reserved);
    if (int rc = check_image_data(who, d, data)) return rc;
    return check_action_dim(who, d->action_dim);
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace dpt

using namespace dpt;

extern "C" {

int dpt_image_normalize(const void* raw, int32_t dtype, int64_t n_images, float* out, void* stream) {
    DPT_REQUIRE(raw && out, "image normalize: null pointer");
    DPT_REQUIRE(dtype == 0 || dtype == 1, "image normalize: dtype=%d (0: float64, 1: float32)", dtype);
    DPT_REQUIRE(n_images >= 0, "image normalize: n_images=%lld", (long long)n_images);
    if (n_images == 0) return DPT_OK;
    const int64_t npix = n_images * kIsArea;
    const int64_t blocks = (npix + kIsThreads - 1) / kIsThreads;
    DPT_REQUIRE(blocks < (1ll << 31), "image normalize: n_images=%lld", (long long)n_images);
    if (dtype == 0)
        hipLaunchKernelGGL(is_normalize_kernel<double>, dim3((unsigned)blocks), dim3(kIsThreads), 0, as_stream(stream),
                           static_cast<const double*>(raw), npix, out);
    else
        hipLaunchKernelGGL(is_normalize_kernel<float>, dim3((unsigned)blocks), dim3(kIsThreads), 0, as_stream(stream),
                           static_cast<const float*>(raw), npix, out);
    return launched("is_normalize");
}

int dpt_image_pack_batch(const dpt_train_desc* d, const dpt_image_data* data, const int64_t* index,
                         const int64_t* perm, int32_t batch, float* images, float* feats, float* targets,
                         void* stream) {
    DPT_REQUIRE(d && data && index && images && feats && targets, "image pack: null pointer");
    DPT_REQUIRE(batch >= 1 && d->state_dim >= 0 && d->action_dim >= 1 && d->window >= 1,
                "image pack: batch=%d sd=%d A=%d window=%d", batch, d->state_dim, d->action_dim, d->window);
    if (int rc = check_image_data("image pack", d, data)) return rc;
    const int64_t rows = (int64_t)batch * d->window;
    DPT_REQUIRE(rows < (1ll << 31), "image pack: %lld rows", (long long)rows);
    hipLaunchKernelGGL(is_pack_kernel, dim3((unsigned)rows), dim3(kIsThreads), 0, as_stream(stream), *data, index, perm,
                       d->window, d->state_dim, d->action_dim, images, feats, targets);
    return launched("is_pack");
}

int dpt_image_train_step_workspace_numel(const dpt_train_desc* d, int64_t* numel) {
    DPT_REQUIRE(d && numel, "image train step workspace: null pointer");
    ImageStepWs w;
    if (int rc = image_step_ws(d, w)) return rc;
    *numel = w.total;
    return DPT_OK;
}

int dpt_image_train_step(const dpt_train_desc* d, const dpt_image_data* data, const int64_t* index,
                         const int64_t* perm, int32_t batch, float* trunk, float* trunk_m, float* trunk_v,
                         float* front, float* front_m, float* front_v, const dpt_adamw_args* opt, float* ws,
                         double* loss_acc, void* stream) {
    const char* who = "image train step";
    if (int rc = check_image_step(who, d, data, index, batch)) return rc;
    DPT_REQUIRE(trunk && trunk_m && trunk_v && front && front_m && front_v && opt && ws && loss_acc,
                "%s: null pointer", who);
    DPT_REQUIRE(opt->step >= 1, "%s: step=%lld (the first step is 1)", who, (long long)opt->step);
    DPT_REQUIRE(aligned16(ws), "%s: workspace not 16-byte aligned", who);
    DPT_REQUIRE(trunk != front, "%s: the trunk blob and the front blob are one buffer", who);
    DPT_REQUIRE(aligned16(front), "%s: front blob not 16-byte aligned", who);
    ImageStepWs w;
    if (int rc = image_step_ws(d, w)) return rc;  // laid out for desc.batch; a smaller batch uses a prefix of each region
    dpt_train_desc run = *d;
    run.batch = batch;
    const dpt_image_desc fd = image_desc_of(&run, batch, data->image_size, 0);
    float *images = ws + w.images, *feats = ws + w.feats, *targets = ws + w.targets, *embeds = ws + w.embeds;
    float *dembeds = ws + w.dembeds, *preds = ws + w.preds, *dpreds = ws + w.dpreds;
    double* partial = reinterpret_cast<double*>(ws + w.partial);
    if (int rc = dpt_image_pack_batch(&run, data, index, perm, batch, images, feats, targets, stream)) return rc;
    if (int rc = dpt_image_front_forward(&fd, front, images, feats, ws + w.front, embeds, stream)) return rc;
    if (int rc = dpt_train_forward_embeds(&run, trunk, embeds, ws + w.trunk, preds, stream)) return rc;
    if (int rc = dpt_train_ce_loss(preds, targets, batch, run.window, run.action_dim, dpreds, partial, loss_acc,
                                   stream))
        return rc;
    if (int rc = dpt_train_backward_embeds(&run, trunk, ws + w.trunk, dpreds, ws + w.dtrunk, dembeds, stream))
        return rc;
    if (int rc = dpt_image_front_backward(&fd, front, images, feats, ws + w.front, dembeds, ws + w.dfront, stream))
        return rc;
    if (int rc = dpt_adamw_step(trunk, ws + w.dtrunk, trunk_m, trunk_v, w.ntrunk, opt, stream)) return rc;
    return dpt_adamw_step(front, ws + w.dfront, front_m, front_v, w.nfront, opt, stream);
}

int dpt_image_train_eval_loss(const dpt_train_desc* d, const dpt_image_data* data, const int64_t* index,
                              const int64_t* perm, int32_t batch, const float* trunk, const float* front, float* ws,
                              double* loss_acc, void* stream) {
    const char* who = "image train eval loss";
    if (int rc = check_image_step(who, d, data, index, batch)) return rc;
    DPT_REQUIRE(trunk && front && ws && loss_acc, "%s: null pointer", who);
    DPT_REQUIRE(aligned16(ws), "%s: workspace not 16-byte aligned", who);
    DPT_REQUIRE(trunk != front, "%s: the trunk blob and the front blob are one buffer", who);
    DPT_REQUIRE(aligned16(front), "%s: front blob not 16-byte aligned", who);
    ImageStepWs w;
    if (int rc = image_step_ws(d, w)) return rc;
    dpt_train_desc run = *d;
    run.batch = batch;
    run.reserved = DPT_TRAIN_FORWARD_ONLY;  // every position's preds: never DPT_TRAIN_LAST_ONLY
    const dpt_image_desc fd = image_desc_of(&run, batch, data->image_size, DPT_TRAIN_FORWARD_ONLY);
    float *images = ws + w.images, *feats = ws + w.feats, *targets = ws + w.targets, *embeds = ws + w.embeds;
    float* preds = ws + w.preds;
    double* partial = reinterpret_cast<double*>(ws + w.partial);
    if (int rc = dpt_image_pack_batch(&run, data, index, perm, batch, images, feats, targets, stream)) return rc;
    if (int rc = dpt_image_front_forward(&fd, front, images, feats, ws + w.front, embeds, stream)) return rc;
    if (int rc = dpt_train_forward_embeds(&run, trunk, embeds, ws + w.trunk, preds, stream)) return rc;
    return dpt_train_ce_loss(preds, targets, batch, run.window, run.action_dim, nullptr, partial, loss_acc, stream);
}

}  // extern "C"
