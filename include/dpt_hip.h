/*
 * dpt_hip.h — C ABI of libdpt_hip.so, the MI355X (gfx950) implementation of the
 * DPT data-generation, training-step (offline, interactive and explorer/exploiter) and
 * in-context-evaluation hot paths.
 *
 * Reference: titanium-47/decision-pretrained-transformer (pure Python).  The
 * reference has no FFI; its "plugin API" is three duck-typed Python protocols
 * (Env, Controller, model.forward).  Every entry point below names the reference
 * interface it replaces (path:line relative to the reference root).  The Python
 * shims in decision-pretrained-transformer_amd/ (envs/, ctrls/, evals/, models/)
 * keep the reference names and call these through ctypes.
 *
 * Conventions
 *  - Every pointer argument is a DEVICE pointer unless the name ends in _host.
 *    The caller (torch) allocates every tensor; the library allocates only the
 *    weight blob owned by an opaque dpt_model handle.
 *  - Workspaces and outputs need no initialisation, and no result depends on
 *    what they held before the call: every word a kernel reads from them was
 *    written earlier in the same call (or by the documented earlier call, as
 *    the forward's workspace handed to its backward), and every documented
 *    output element is written.  A workspace may be reused across calls, also
 *    with other shapes, without being cleared (tests/test_gpu_dirty_buffers.py
 *    fills them with NaN and 3.39e38 patterns before every call).
 *  - All launches are asynchronous on the given stream (hipStream_t passed as
 *    void* so this header needs no HIP include; NULL = default stream).  No
 *    entry point that takes a stream synchronises the host or touches another
 *    stream: every launch, memset and copy of a call is ordered on that one
 *    stream (tests/test_gpu_side_stream.py).  dpt_model_create takes none and
 *    synchronises the device.
 *  - Return 0 (DPT_OK) or a negative DPT_E* code; dpt_last_error() returns a
 *    thread-local message for the last failing call on this thread.
 *  - Layouts are C-contiguous, row-major.  fp64 for everything the reference
 *    keeps in numpy float64 (means, rewards, arm values, uniforms, normals),
 *    fp32 for the model (the reference converts contexts with .float()).
 *  - Randomness: when an optional uniforms/normals pointer is NULL the library
 *    draws from Philox4x32-10 keyed by `seed` with counter
 *    (step, global task id, stream, 0); results therefore do not depend on how
 *    tasks are sharded over GPUs.  Passing explicit draws reproduces a
 *    reference run draw-for-draw (tests/golden).
 */
#ifndef DPT_HIP_H
#define DPT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 7 (round 6): dpt_policy_workspace_numel returns 0 and dpt_policy_rollout_args.workspace may be
 * NULL (each task's context lives in LDS); DPT_TUNE_POLICY_WAVE accepts only 1 */
/* 8: the training step (dpt_train_pack_batch, dpt_train_ce_loss, dpt_adamw_step, dpt_train_step,
 * dpt_train_eval_loss); added since without a bump (additions only): the interactive training step
 * (dpt_interactive_pack, dpt_train_ce_last, dpt_interactive_workspace_numel, dpt_interactive_grad)
 * and DPT_BANDIT_F32 in dpt_rollout_bandit_generic; the explorer/exploiter training step
 * (dpt_rollout_bandit_generic_env, DPT_STREAM_ENVACT, dpt_train_ce_rows, dpt_explore_weights,
 * dpt_explore_workspace_numel, dpt_explore_grad); the tuning key DPT_TUNE_YCACHE_BITS (dpt_rollout_bandit
 * caches its rows as 24-bit fixed point by default; no struct or signature changed); the image-conditioned
 * DPT (dpt_image_front_*, dpt_train_*_embeds) and its training step (dpt_image_normalize,
 * dpt_image_pack_batch, dpt_image_train_step_workspace_numel, dpt_image_train_step,
 * dpt_image_train_eval_loss); its act step (dpt_image_obs_tables, dpt_image_obs_preprocess,
 * dpt_image_act_workspace_numel, dpt_image_act_set_context, dpt_image_act_step); the explore-then-exploit
 * evaluation (dpt_recommend_curve, dpt_empirical_recommend, dpt_exploit_eval_workspace_numel,
 * dpt_exploit_eval); the interactive DarkRoom training step (dpt_mdp_pack, dpt_darkroom_act_step,
 * dpt_interactive_mdp_workspace_numel, dpt_interactive_mdp_grad); the in-episode DarkRoom rollout in one
 * launch (dpt_rollout_darkroom_episode); the fresh-task generator and its training step (DPT_STREAM_TASK,
 * dpt_fresh_args, dpt_fresh_batch, dpt_fresh_step, dpt_fresh_eval_loss) and its linear-bandit twin
 * (dpt_fresh_linear_args, dpt_fresh_linear_batch, dpt_fresh_linear_step, dpt_fresh_linear_eval_loss); the
 * Bayes posterior of the optimal action (dpt_bandit_posterior_workspace_numel, dpt_bandit_posterior,
 * dpt_darkroom_posterior, dpt_posterior_compare) and its linear-bandit twin at lin_d = 2
 * (dpt_linear_posterior_workspace_numel, dpt_linear_posterior) */
#define DPT_ABI_VERSION 8

/* error codes (mapped to the reference's Python exceptions by dpt_hip/_lib.py) */
#define DPT_OK 0
#define DPT_EINVAL (-1)          /* bad shape / argument        -> ValueError            */
#define DPT_EEPISODE_ENDED (-2)  /* step past horizon           -> ValueError("Episode has already ended")
                                    envs/bandit_env.py:67-68, envs/darkroom_env.py:58-59 */
#define DPT_EHIP (-3)            /* HIP runtime error           -> RuntimeError          */
#define DPT_ENOMEM (-4)          /* device allocation failed    -> MemoryError           */
#define DPT_EUNSUPPORTED (-5)    /* configuration not built     -> NotImplementedError
                                    (envs/bandit_env.py:16,63 unknown bandit type)      */

/* bandit reward type, envs/bandit_env.py:57-63 / envs/gpu_bandit_env.py:57-62 */
#define DPT_BANDIT_GAUSSIAN 0
#define DPT_BANDIT_BERNOULLI 1
/* OR-ed into `type`: fp32 arithmetic, r = float(m) + float(g) * float(var) (two
 * roundings), the torch semantics of GPUBanditEnv.transit (gpu_bandit_env.py:58-59) */
#define DPT_BANDIT_F32 16

/* Philox stream ids (counter word 2) */
#define DPT_STREAM_SELECT 0
#define DPT_STREAM_REWARD 1
#define DPT_STREAM_ROLLIN 2
#define DPT_STREAM_DROPOUT 3 /* training dropout masks: counter (site, element / 4), word element % 4 */
#define DPT_STREAM_ENVACT 4  /* the env action of dpt_rollout_bandit_generic_env when it is drawn apart from the context action */
/* the task draws of the fresh-task generator (dpt_fresh_batch), per task at counters:
 *   bandit, A arms:  k in [0, A): means[k] = the 53-bit uniform;  A + k: e_k = -log(1 - uniform), the
 *                    Gamma(1) variates of Dirichlet(1_A);  2 A: word 0 -> index into the 11-point cov
 *                    grid, word 1 -> the point-mass arm (multiply-shift, as every integer draw)
 *   DarkRoom:        0: word 0 -> index into the goal list, word 1 -> index into the permutation list
 *   linear bandit (dpt_fresh_linear_batch), A arms, d features:  p in [0, d): theta[p] = the normal / sqrt(d);
 *                    'uniform' rollin only, the bandit's policy draws moved behind theta:  d + k: e_k;
 *                    d + A: word 0 -> index into the cov grid, word 1 -> the point-mass arm */
#define DPT_STREAM_TASK 5
#define DPT_STREAM_POLICY 16/* + arm index: baseline-policy draws (Thompson posterior samples) */

int dpt_abi_version(void);
const char* dpt_last_error(void);
/* Process-wide tuning knobs (no effect on results beyond fp32 summation order):
 * DPT_TUNE_DECODE_TILE = tasks per workgroup of the decode kernels, 8 (default:
 * two workgroups per CU) or 16.
 * DPT_TUNE_PREFILL = 1 (default): dpt_forward_window runs windows of up to
 * dpt_prefill_max_window() tokens as one MFMA prefill; 0: always position by
 * position through the K/V workspace.
 * DPT_TUNE_DARKROOM_MEMO = 1 (default): dpt_rollout_darkroom runs one window
 * forward per distinct query state per episode (the window is fixed within an
 * episode, so a repeated state's logits are the same pure function of the same
 * inputs: results are bit-identical); 0: one forward per step.
 * DPT_TUNE_CACHE_BUDGET = bytes of the 256 MiB Infinity Cache that
 * dpt_rollout_bandit may fill with the cached rows of its earliest positions
 * (stored and streamed with the default cache policy, so they stay resident and
 * are re-read on-die every step; later positions stream non-temporally and do
 * not displace them).  0: every row non-temporal.  Cache policy only: results
 * are bit-identical for any value.
 * DPT_TUNE_BLOCK0_MFMA = 0 (the only value): dpt_rollout_bandit computes block
 * 0's attention with one wave per task on the vector ALUs; any other value
 * returns DPT_EUNSUPPORTED (the matrix-core form for tiles of 8 five-arm tasks
 * was retired: equal speed at config 2, slower at 20 arms).
 * DPT_TUNE_SELECT_FAST = 1 (default): dpt_select_action decides 5- and 20-arm
 * samples on the fp32 cdf when the uniform is more than 2^-15 from every cdf
 * edge and runs the exact fp64 cdf otherwise (the rollouts always do); 0: the
 * fp64 cdf for every sample.  Bit-identical either way.
 * DPT_TUNE_POLICY_WAVE = 1 (the only value): dpt_rollout_policy runs one 64-lane
 * workgroup per task with the task's context in LDS (the per-arm pairwise sums
 * split over lanes in numpy's order); 0 returns DPT_EUNSUPPORTED since round 6
 * (the lane-per-task kernel was retired).
 * DPT_TUNE_YCACHE_BITS = 24 (default): dpt_rollout_bandit caches the normalised
 * ln_1 rows of blocks >= 1 as signed 24-bit fixed point (96 B per position,
 * absolute error <= 2^-21, below the kernel's fp32 summation noise; ln_1's g and b
 * are folded into the derived weights); 32: as fp32 rows (128 B), the comparison
 * path.  The workspace size (dpt_kvcache_numel) is the same for both.  */
#define DPT_TUNE_DECODE_TILE 1
#define DPT_TUNE_PREFILL 2
#define DPT_TUNE_DARKROOM_MEMO 3
#define DPT_TUNE_CACHE_BUDGET 4
#define DPT_TUNE_BLOCK0_MFMA 5
#define DPT_TUNE_SELECT_FAST 6
#define DPT_TUNE_POLICY_WAVE 7
#define DPT_TUNE_YCACHE_BITS 8
int dpt_tuning_set(int32_t key, int64_t value);
/* number of visible gfx950 devices (0 on a CPU-only host; never faults) */
int dpt_device_count(int* count_out_host);

/* ------------------------------------------------------------------ model
 * Replaces models/net.py:9-60 `Transformer` (+ transformers.GPT2Model with
 * n_head forced to 1, net.py:29).  The dpt_model handle and every entry point
 * that takes it (dpt_forward_window, dpt_decode_step, dpt_rollout_bandit,
 * dpt_rollout_darkroom) are built for n_embd == 32 (the reference default,
 * common_args.py:31); n_layer is free.  Any other width runs through the
 * width-generic dpt_train_forward / dpt_train_backward below (same blob layout),
 * which Transformer.forward uses for inference at such widths as well.
 *
 * Packed fp32 weight blob, in this order (all matrices stored [in][out]):
 *   emb_w [F][E]  emb_b [E]                 F = 2*state_dim + action_dim + 1
 *   wpe   [n_positions][E]                  n_positions = 4*(1+horizon) (net.py:26)
 *   per layer l < n_layer:
 *     ln1_g[E] ln1_b[E] attn_w[E][3E] attn_b[3E] proj_w[E][E] proj_b[E]
 *     ln2_g[E] ln2_b[E] fc_w[E][4E] fc_b[4E] mp_w[4E][E] mp_b[E]
 *   lnf_g[E] lnf_b[E]
 *   head_w[E][A]  head_b[A]
 * Conv1D weights are already [in][out]; nn.Linear weights (embed_transition,
 * pred_actions) are transposed by the packer.
 */
typedef struct dpt_model dpt_model;

typedef struct dpt_model_desc {
    int32_t n_layer;
    int32_t n_embd;      /* must be 32 for this handle (other widths: dpt_train_*) */
    int32_t state_dim;
    int32_t action_dim;  /* 1..32 */
    int32_t n_positions; /* rows of wpe */
    int32_t reserved[3];
} dpt_model_desc;

/* number of floats in the packed blob for `desc` */
int dpt_weights_numel(const dpt_model_desc* desc_host, int64_t* numel_out_host);
/* copies `packed` (device, dpt_weights_numel floats) into a blob owned by the handle */
int dpt_model_create(const dpt_model_desc* desc_host, const float* packed, dpt_model** out_host);
int dpt_model_free(dpt_model* model);

/* Full-window forward, replaces Transformer.forward (models/net.py:41-60)
 * including the token packing (net.py:42-54):
 *   token 0 = [query, 0_A, 0_sd, 0], token 1+j = [s_j, a_j, s'_j, r_j].
 * query (N,sd); states/next_states (N,C,sd); actions (N,C,A); rewards (N,C).
 * C may be 0 (the context pointers may then be NULL).  T = C+1 <= n_positions.
 * out_mode 0: out (N,A) = preds[:, -1]  (test=True)
 * out_mode 1: out (N,C,A) = preds[:, 1:] (test=False)                       */
int dpt_forward_window(const dpt_model* model, const float* query, const float* states,
                       const float* actions, const float* next_states, const float* rewards,
                       int32_t N, int32_t C, int32_t out_mode, float* out, float* workspace,
                       void* stream);
/* Windows of T = C + 1 <= dpt_prefill_max_window(model) tokens (512 for the
 * reference models) run as one MFMA prefill (all positions at once, one
 * workgroup per sequence) and `workspace` may be NULL.  Longer windows are
 * evaluated causally, position by position, through a K/V cache in
 * `workspace` (dpt_kvcache_numel(model, N, C + 1) floats); both are the full
 * causal forward (each row attends to rows <= itself).                        */
int dpt_prefill_max_window(const dpt_model* model, int32_t* tokens_out_host);

/* ------------------------------------------------------------------ KV-cache decode
 * Exact incremental form of the growing-window forward used by the bandit
 * online loop (evals/eval_bandit.py:70-89): the query token is identical at
 * every step, so positions 0..h-1 are unchanged between steps h-1 and h and
 * their keys/values can be cached.  dpt_kvcache_numel sizes the buffer for
 * [2][n_layer][N'][max_pos][E] floats, N' = N rounded up to a multiple of 16.
 * Only dpt_rollout_bandit lays it out with the padded N' stride (whole decode
 * tiles; its own per-position records); dpt_decode_step and the
 * long-window dpt_forward_window use [2][n_layer][N][max_pos][E] (V half at
 * n_layer*N*max_pos*E) and simply leave the padding unused.                   */
int dpt_kvcache_numel(const dpt_model* model, int32_t N, int32_t max_pos, int64_t* numel_out_host);
/* one decode position for all N tasks: token (N,F) packed features of position
 * `pos` (pos 0 is the query token), appends K/V at `pos`, logits (N,A) of it.  */
int dpt_decode_step(const dpt_model* model, float* kvcache, int32_t N, int32_t max_pos,
                    int32_t pos, const float* token, float* logits, void* stream);

/* ------------------------------------------------------------------ action selection
 * Replaces ctrls/ctrl_bandit.py:435-443 and ctrls/ctrl_darkroom.py:48-62:
 * sample=1: p = softmax_fp32(logits/temp) (scipy.special.softmax semantics,
 *   pairwise fp32 sum), i = #{k : cdf64_k <= u} with cdf64 = cumsum(fp64(p)) /
 *   cdf[-1] — numpy legacy RandomState.choice(A, p=p) given its uniform u.
 * sample=0: first argmax (np.argmax).
 * uniforms (N) or NULL -> Philox(seed, (counter, first_task+i, DPT_STREAM_SELECT)). */
int dpt_select_action(const float* logits, int32_t N, int32_t A, int32_t sample, float temp,
                      const double* uniforms, uint64_t seed, uint64_t counter, int64_t first_task,
                      int32_t* action_out, void* stream);

/* ------------------------------------------------------------------ environments
 * BanditEnvVec.step / GPUBanditEnv.transit (envs/bandit_env.py:56-74,
 * envs/gpu_bandit_env.py:53-74):
 *   gaussian : r = means[a] + (0.0 + var*g)   fp64, no contraction (bit-exact to numpy)
 *   bernoulli: r = (u < means[a]) ? 1 : 0      (torch.bernoulli)
 * arm_value_out (optional) = means[a]  (get_arm_value, envs/bandit_env.py:151-153).
 * noise (N) or NULL -> Philox(seed, (counter, first_task+i, DPT_STREAM_REWARD)).   */
int dpt_bandit_step(const double* means, int32_t N, int32_t A, const int32_t* action,
                    int32_t type, double var, const double* noise, uint64_t seed,
                    uint64_t counter, int64_t first_task, double* reward_out,
                    double* arm_value_out, void* stream);

/* DarkroomEnv(.Permuted).transit (envs/darkroom_env.py:37-55, :100-103): int32
 * states (N,2), action index (N), goal (N,2), perm (N,5) or NULL.  Bit-exact.   */
int dpt_darkroom_step(const int32_t* state, const int32_t* action, const int32_t* goal,
                      const int32_t* perm, int32_t N, int32_t dim, int32_t* next_state,
                      int32_t* reward, void* stream);
/* DarkroomEnv.opt_action (envs/darkroom_env.py:69-82, permuted :105-111) */
int dpt_darkroom_opt_action(const int32_t* state, const int32_t* goal, const int32_t* perm,
                            int32_t N, int32_t* action_out, void* stream);

/* Materialise the Philox draws the library would use: kind 0 = uniform [0,1),
 * kind 1 = standard normal; out[i] for global task first_task+i at `counter`. */
int dpt_draw(int32_t kind, uint64_t seed, uint64_t counter, int64_t first_task, int32_t N,
             uint32_t stream_id, double* out, void* stream);

/* ------------------------------------------------------------------ data generation
 * collect_data.py:23-53 rollin_bandit (+ generate_bandit_histories :158-182,
 * :221-225): for every task i and step h, i.i.d. arm ~ choice(A, probs[i])
 * (cdf/searchsorted semantics on the given fp64 behaviour policy, which the
 * host draws as (1-cov)*Dirichlet(1) + cov*e_rand, collect_data.py:30-36) and
 * r = means[i][arm] + (0.0 + var*g) (or Bernoulli).  uniforms/noise (H,N) or
 * NULL -> Philox streams DPT_STREAM_ROLLIN / DPT_STREAM_REWARD.
 * Outputs actions (N,H) int32, rewards (N,H) fp64.                         */
int dpt_rollin_bandit(const double* means, const double* probs, int32_t N, int32_t A, int32_t H,
                      int32_t type, double var, const double* uniforms, const double* noise,
                      uint64_t seed, int64_t first_task, int32_t* actions_out, double* rewards_out,
                      void* stream);

/* collect_data.py:83-111 rollin_mdp + :189-218: mode 0 'uniform' (i.i.d. state
 * ~ U{0..dim-1}^2 and action ~ U{0..4} per step; states_in (N,H,2) /
 * actions_in (N,H) inject them), mode 1 'expert' (greedy walk from (0,0)).
 * Outputs (N,H,2)/(N,H) int32; query_out (N,2) ~ U and opt_action_out (N) =
 * its expert label (optional).                                              */
int dpt_rollin_darkroom(const int32_t* goal, const int32_t* perm, int32_t N, int32_t H, int32_t dim,
                        int32_t mode, const int32_t* states_in, const int32_t* actions_in,
                        uint64_t seed, int64_t first_task, int32_t* states_out,
                        int32_t* actions_out, int32_t* next_states_out, int32_t* rewards_out,
                        int32_t* query_out, int32_t* opt_action_out, void* stream);

/* ------------------------------------------------------------------ fused rollouts
 * The whole online loop on device, one launch: replaces
 * evals/eval_bandit.py:56-103 (and the identical evals/eval_linear_bandit.py:54-97)
 * with BanditTransformerController (ctrls/ctrl_bandit.py:383-444) in the loop.
 * For h in [0,H): decode position h (query token at h=0, else transition h-1),
 * select a_h, step the env, append [1, onehot(a_h), 1, float(r_h)].           */
typedef struct dpt_bandit_rollout_args {
    int32_t N;            /* tasks on this device                         */
    int32_t H;            /* horizon (steps = positions)                  */
    int32_t A;            /* arms == model action_dim                     */
    int32_t type;         /* DPT_BANDIT_*                                 */
    int32_t sample;       /* 1: softmax sampling (eval online), 0: argmax */
    int32_t reserved0;
    int64_t first_task;   /* global id of task 0 (Philox counter)         */
    double var;           /* reward noise std (the reference's `var`)     */
    uint64_t seed;
    const double* means;  /* (N, A)                                       */
    const double* uniforms; /* (H, N) or NULL                             */
    const double* noise;    /* (H, N) or NULL (normals, or bernoulli uniforms) */
    float* kvcache;         /* dpt_kvcache_numel(model, N, H) floats: blocks
                             * 1..L-1 keep their ln_1 outputs y (tile-
                             * interleaved rows); block 0 is recomputed from
                             * the tokens, so its K slot holds the 16-B token
                             * records and its V slot the per-step draws     */
    int32_t* actions_out;   /* (N, H)                                       */
    double* rewards_out;    /* (N, H)                                       */
    double* arm_value_out;  /* (N, H)  = cum_means.T                         */
    float* logits_out;      /* (H, N, A) or NULL                             */
    uint64_t counter;       /* Philox counter of step 0: step h draws at
                             * counter + h, as the per-step path's selects
                             * (dpt_select_action) numbered from `counter` */
} dpt_bandit_rollout_args;

int dpt_rollout_bandit(const dpt_model* model, const dpt_bandit_rollout_args* args_host,
                       void* stream);

/* The classical comparison policies of the same online loop, fused with the env
 * (one lane per task, all H steps): replaces deploy_online_vec with
 *   DPT_POLICY_OPT      OptPolicy            ctrls/ctrl_bandit.py:22-38
 *   DPT_POLICY_EMP      EmpMeanPolicy        :57-118  (online flag: play unseen arms first)
 *   DPT_POLICY_UCB      UCBPolicy(c)         :318-380
 *   DPT_POLICY_THOMPSON ThompsonSampling     :122-251 (std, prior_mean, prior_var; sample 0 = 100-draw vote)
 *   DPT_POLICY_LCB      PessMeanPolicy(c)    :255-314
 *   DPT_POLICY_LINUCB   LinUCBPolicy(c)      :447-528 (arms (A, lin_d), lin_d <= 8)
 * Per-arm statistics are recomputed each step from the per-arm reward lists in
 * numpy's fp64 pairwise-summation order, as the reference does, so action
 * indices match it bit for bit given the same draws (LinUCB: numpy's BLAS/LAPACK
 * rounding order restated at every lin_d, csrc/dpt_linucb.h).  policy_noise:
 * Thompson (H,N,A) posterior normals (sample = 1) or (H,100,N,A) for the 100-draw vote
 * (sample = 0); LinUCB (N) uniforms for the empty-context arm.  */
#define DPT_POLICY_OPT 0
#define DPT_POLICY_EMP 1
#define DPT_POLICY_UCB 2
#define DPT_POLICY_THOMPSON 3
#define DPT_POLICY_LCB 4
#define DPT_POLICY_LINUCB 5

typedef struct dpt_policy_rollout_args {
    int32_t N, H, A, policy;
    int32_t online, type, sample, lin_d;
    int64_t first_task;
    double var;          /* env reward noise std */
    double c;            /* UCB / LCB / LinUCB constant */
    double ts_std, ts_prior_mean, ts_prior_var;
    uint64_t seed;
    const double* means;        /* (N, A) */
    const double* arms;         /* (A, lin_d) or NULL */
    const double* noise;        /* (H, N) or NULL */
    const double* policy_noise; /* see above, or NULL */
    double* workspace;          /* unused since round 6 (may be NULL): dpt_policy_workspace_numel = 0 */
    int32_t* actions_out;       /* (N, H) */
    double* rewards_out;        /* (N, H) */
    double* arm_value_out;      /* (N, H) */
    /* optional prefix context (set_batch_numpy_vec): C transitions per task,
     * replayed into the statistics before step 0 (offline eval: C = h, H = 1) */
    int32_t C;
    int32_t step0;              /* Philox step counter of step 0: step h draws at step0 + h, so a
                                 * per-step call (H = 1, step0 = h) draws what the fused launch
                                 * (step0 = 0) draws at step h */
    const int32_t* ctx_actions; /* (N, C) arm indices.  Precondition: every value in [0, A).  They are
                                 * device memory, so dpt_rollout_policy cannot check them; a value
                                 * outside the range indexes the kernel's LDS tables out of range */
    const double* ctx_rewards;  /* (N, C) */
} dpt_policy_rollout_args;

int dpt_policy_workspace_numel(int32_t N, int32_t A, int32_t H, int64_t* numel_out_host);
int dpt_rollout_policy(const dpt_policy_rollout_args* args_host, void* stream);

/* DarkRoom in-context online evaluation, one launch: replaces
 * evals/eval_darkroom.py:20-84 deploy_online_vec with
 * DarkroomTransformerController (ctrls/ctrl_darkroom.py:23-66) and
 * DarkroomEnvVec.deploy_eval (envs/darkroom_env.py:151-175).  Episode e runs
 * `horizon` steps from (0,0); its context is episodes max(0,e-R)..e-1 in order
 * (R = ctx_episodes = H / horizon, shift-append :75-82), and every step is a
 * full forward over the window [query = current state, context...] with the
 * prediction at the last position.  Action a_t = select(logits, u_t) with
 * u_t = uniforms[(e*horizon+t)*N + i] or Philox(seed, counter + e*horizon + t,
 * first_task + i, DPT_STREAM_SELECT) -- the same draws as dpt_select_action.
 * Requires sd = 2, A = 5, 1 + R*horizon <= 512 and dim <= 255 (else
 * DPT_EUNSUPPORTED: use dpt_forward_window per step).  Windows of up to 128
 * tokens run 4 waves per task (two tasks per CU), up to 256 8 waves, up to
 * 512 16 waves (one task per CU; these need the workspace).                 */
typedef struct dpt_darkroom_rollout_args {
    int32_t N, Heps, horizon, ctx_episodes;
    int32_t dim, sample;
    int64_t first_task;
    uint64_t seed, counter;
    float temp;                 /* softmax temperature (1.0 in the reference) */
    int32_t reserved0;
    const int32_t* goals;       /* (N, 2) */
    const int32_t* perms;       /* (N, 5) action permutation or NULL */
    const double* uniforms;     /* (Heps*horizon, N) or NULL */
    int32_t* returns_out;       /* (N, Heps) sum of rewards per episode */
    int32_t* actions_out;       /* (N, Heps*horizon) or NULL */
    float* logits_out;          /* (Heps*horizon, N, 5) or NULL */
    int32_t* forwards_out;      /* (N, Heps) window forwards run per task and episode, or NULL */
    float* workspace;           /* dpt_darkroom_workspace_numel_window(N, 1 + R*horizon) floats
                                 * (dpt_darkroom_workspace_numel(N): enough for any window), or
                                 * NULL (windows up to 256 only): the context
                                 * tokens' layer-0 inputs, queries and attention partials, fixed
                                 * within an episode, are kept there instead of recomputed every
                                 * step (or kept in LDS: the partials) */
} dpt_darkroom_rollout_args;

int dpt_darkroom_workspace_numel(int32_t N, int64_t* numel_out_host);
int dpt_darkroom_workspace_numel_window(int32_t N, int32_t window, int64_t* numel_out_host);

int dpt_rollout_darkroom(const dpt_model* model, const dpt_darkroom_rollout_args* args_host,
                         void* stream);

/* Regret statistics of the online bandit eval: replaces evals/eval_bandit.py:169-178
 * (diff = opt - lnr per step, cumsum over steps, mean and scipy.stats.sem over
 * tasks) on device, in scipy's two-pass form so that ranks can all-reduce between
 * the passes.  With diff[t][h] = opt[t] - arm_value[t][h] and cr[t][h] its cumsum
 * over h, out (2, H) fp64 is
 *   DPT_REGRET_SUMS:    (sum_t diff[.][h], sum_t cr[.][h])                 (mean unused)
 *   DPT_REGRET_CENTRED: (sum_t (diff - mean[0][h])^2, sum_t (cr - mean[1][h])^2)
 * for a caller-supplied mean (2, H).  Fixed reduction order (deterministic).
 * arm_value (N, H) fp64 (dpt_rollout_bandit's arm_value_out), opt (N) fp64,
 * H <= dpt_regret_max_steps(), workspace dpt_regret_workspace_numel(N, H) doubles. */
#define DPT_REGRET_SUMS 0
#define DPT_REGRET_CENTRED 1
int dpt_regret_max_steps(int32_t* steps_out_host);
int dpt_regret_workspace_numel(int32_t N, int32_t H, int64_t* numel_out_host);
int dpt_regret_moments(const double* arm_value, const double* opt, int32_t N, int32_t H, int32_t mode,
                       const double* mean, double* workspace, double* out, void* stream);

/* ------------------------------------------------------------------ training
 * Replaces the autograd of Transformer.forward with test=False (models/net.py:41-60: preds at
 * positions 1..T-1) inside train.py:286-331 (CrossEntropyLoss(sum) over preds[:, 1:], AdamW).
 * Any n_embd (FF = 4 n_embd, one head as net.py:29 forces), fp32.  The weights are a packed
 * blob in the dpt_weights_numel layout with this desc's width (dpt_train_blob_numel floats);
 * tokens (batch, window, 2 sd + A + 1) are the packed sequences of net.py:42-54.
 * dpt_train_forward writes preds (batch, window, A) at EVERY position (position 0 included) and
 * keeps in `workspace` what the backward needs; dpt_train_backward takes dL/dpreds (batch,
 * window, A) -- zero at positions the loss does not use -- and writes every parameter's
 * gradient into dblob (same layout; wpe rows >= window are zero).  Reductions over the
 * batch * window rows run in a fixed order: the gradients are deterministic.               */
typedef struct dpt_train_desc {
    int32_t n_layer, n_embd, state_dim, action_dim, n_positions;
    int32_t batch, window;        /* sequences and tokens per sequence (1 + context length) */
    int32_t reserved;             /* flags: DPT_TRAIN_FORWARD_ONLY [| DPT_TRAIN_LAST_ONLY], DPT_TRAIN_LAST_LOSS, or 0 */
    float dropout;                /* GPT2Config embd/attn/resid_pdrop (net.py:30-32), 0 <= p < 1 */
    int32_t reserved2;            /* 0 */
    uint64_t dropout_seed;        /* Philox key of this forward's masks (a fresh one per step) */
} dpt_train_desc;
/* Dropout (GPT2Model in training mode, p = dropout > 0): element e of a site is kept iff
 * word_e >= thr, thr = min(ceil(p 2^32), 2^32 - 1), word_e = component e % 4 of
 * Philox(dropout_seed, (site, e / 4, DPT_STREAM_DROPOUT)), and kept elements are scaled by
 * float(1 / (1 - p)).  Sites: 0 = the embedding sum x0 (B, T, E); per layer l, 1 + 3 l = the
 * attention probabilities (B, T, T) [element (b t + i) T + j], 2 + 3 l = c_proj's output,
 * 3 + 3 l = mlp.c_proj's output (B, T, E), each dropped before its residual add.  The backward
 * regenerates the same masks from the desc: pass the forward's desc unchanged.  p > 0 runs the
 * row kernels (no matrix-core forms).                                                       */
/* Inference through the training forward (no backward will follow): the workspace holds one
 * layer's activations and no attention probabilities or backward scratch
 * (dpt_train_workspace_numel sizes it by the flag); dpt_train_backward rejects the desc. */
#define DPT_TRAIN_FORWARD_ONLY 1
/* with DPT_TRAIN_FORWARD_ONLY and no dropout: preds only at the last position of each sequence
 * (models/net.py:56-58 test mode reads preds[:, -1]); the last block runs for that position alone
 * (its keys and values still cover the window) and the other rows of preds are left unwritten */
#define DPT_TRAIN_LAST_ONLY 2
/* a TRAINING forward (no DPT_TRAIN_FORWARD_ONLY, no dropout) whose loss reads the last position of each
 * sequence alone (dpt_train_ce_last): the last block's c_proj, ln_2, MLP, then ln_f and the head run
 * for `batch` rows instead of batch * window, in the forward (which saves those rows, the last block's
 * full q/k/v and the last query's probabilities) and in the backward (one query row per sequence: dq for
 * that row, dK / dV for every position; from c_attn down the full-width path).  Only preds[:, window-1]
 * is written, and dpt_train_backward reads only dpreds[:, window-1]: every row it skips contributes
 * exact zeros to the full backward, so the gradient is the same up to fp32 summation order.  Pass the
 * same desc to the backward.  window 1 (and action_dim > 3 n_embd) runs the full path. */
#define DPT_TRAIN_LAST_LOSS 4
int dpt_train_blob_numel(const dpt_train_desc* desc_host, int64_t* numel_out_host);
int dpt_train_workspace_numel(const dpt_train_desc* desc_host, int64_t* numel_out_host);
int dpt_train_forward(const dpt_train_desc* desc_host, const float* blob, const float* tokens, float* workspace,
                      float* preds, void* stream);
int dpt_train_backward(const dpt_train_desc* desc_host, const float* blob, const float* tokens, float* workspace,
                       const float* dpreds, float* dblob, void* stream);

/* The bandit online loop (evals/eval_bandit.py:56-103, as dpt_rollout_bandit) for models of ANY
 * width (state_dim 1, blob in the dpt_train_desc layout; desc batch / window unused, set 1, and
 * dropout 0): an exact K/V-cache decode, one step for all N tasks at a time (the training
 * forward's row kernels, or their matrix-core forms at widths 16 / 32 / 64, on N rows; the new
 * token's attention over the task's cache), then the fused kernel's selection, draws and env
 * step.  The cache holds each block's LayerNorm output y (the folded attention: u = y W_q W_k^T
 * scores the cached rows, c_proj runs on W_v W_proj), read once per step by a flash-decoding pass.
 * args->kvcache = dpt_rollout_bandit_generic_workspace_numel floats (the y cache
 * [n_layer][N][H][n_embd], the folded weights, per-step rows); the other fields as for
 * dpt_rollout_bandit.  args->type may carry DPT_BANDIT_F32: Gaussian rewards are then
 * float(mean) + float(g) * float(var) (two fp32 roundings, stored as double), GPUBanditEnv's
 * arithmetic as in dpt_bandit_step; Bernoulli rewards and every other output are unchanged.
 * Replaces the per-step path (Transformer.forward over the whole window every step) at widths
 * the fused kernel is not built for.                                                        */
int dpt_rollout_bandit_generic_workspace_numel(const dpt_train_desc* desc_host, int32_t N, int32_t H,
                                               int64_t* numel_out_host);
int dpt_rollout_bandit_generic(const dpt_train_desc* desc_host, const float* blob,
                               const dpt_bandit_rollout_args* args_host, void* stream);

/* ------------------------------------------------------------------ training step
 * One step of train.py:286-310 (and one batch of its test loss, :265-278) as a chain of launches
 * on one stream with no host synchronisation: pack the batch from a device-resident dataset, the
 * training forward, CrossEntropyLoss(reduction='sum') over positions 1..T-1 and its gradient, the
 * backward, and AdamW over the whole packed blob.  Host-side checks (null pointers, step < 1,
 * numel < 0, action_dim > 32 -> DPT_EUNSUPPORTED, desc.window != 1 + horizon) fail before any
 * launch.  The library allocates nothing: the weights, the optimizer state, the workspace and the
 * loss accumulator are the caller's.                                                        */

/* The whole training set on the device in fp32 (dataset.py:54-61, `Dataset.dataset`). */
typedef struct dpt_train_data {
    int64_t n;                        /* samples */
    int32_t horizon;                  /* context transitions per sample */
    int32_t reserved;                 /* 0 */
    const float* query_states;        /* (n, sd) */
    const float* context_states;      /* (n, horizon, sd) */
    const float* context_actions;     /* (n, horizon, A) */
    const float* context_next_states; /* (n, horizon, sd) */
    const float* context_rewards;     /* (n, horizon) */
    const float* optimal_actions;     /* (n, A) */
} dpt_train_data;

/* torch.optim.AdamW's documented update with the state of step `step` (the first step is 1):
 *   p *= 1 - lr weight_decay;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2
 *   p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * An entry whose gradient is exactly zero (and whose state is zero: the wpe rows past the window)
 * only decays.  Evaluated in fp64 from the fp32 inputs, stored rounded to fp32. */
typedef struct dpt_adamw_args {
    double lr, beta1, beta2, eps, weight_decay;
    int64_t step;
} dpt_adamw_args;

/* tokens (batch, 1 + horizon, 2 sd + A + 1) = the packed sequences of models/net.py:42-54 for the
 * samples index[b] (int64, any order, repeats allowed), context transition j of sequence b taken
 * from perm[b][j] when perm (batch, horizon) int64 is given (dataset.py:84-89), and targets
 * (batch, A) = optimal_actions[index].  Copies only: bit-exact.  desc: state_dim, action_dim and
 * window (= 1 + data->horizon) are read.  An index outside [0, n) or a perm entry outside
 * [0, horizon) reads nothing and packs zeros. */
int dpt_train_pack_batch(const dpt_train_desc* desc_host, const dpt_train_data* data_host, const int64_t* index,
                         const int64_t* perm, int32_t batch, float* tokens, float* targets, void* stream);
/* train.py:295-301: *loss_acc += sum over b and positions t in 1..window-1 of
 * -sum_k targets[b][k] log_softmax(preds[b][t])[k] (probability targets, not only one-hot), and
 * dpreds (batch, window, A) = softmax(preds) sum_k targets[b][k] - targets[b], zero at position 0
 * (dpreds NULL: the loss alone).  A <= 32.  partial: `batch` doubles of scratch (the per-sequence
 * losses); the sum runs in a fixed order, so repeated calls are bit-identical. */
int dpt_train_ce_loss(const float* preds, const float* targets, int32_t batch, int32_t window, int32_t A,
                      float* dpreds, double* partial, double* loss_acc, void* stream);
/* one launch over blob / dblob / m / v of `numel` floats each (any numel) */
int dpt_adamw_step(float* blob, const float* dblob, float* m, float* v, int64_t numel,
                   const dpt_adamw_args* args_host, void* stream);
/* workspace floats of dpt_train_step / dpt_train_eval_loss for desc.batch sequences: the training
 * workspace, tokens, targets, preds, dpreds, dblob and the per-sequence losses */
int dpt_train_step_workspace_numel(const dpt_train_desc* desc_host, int64_t* numel_out_host);
/* pack -> dpt_train_forward -> cross-entropy -> dpt_train_backward -> AdamW for the `batch` <=
 * desc.batch samples of index (a smaller last batch reuses the workspace sized for desc.batch).
 * desc flags 0; dropout through desc.dropout / desc.dropout_seed.  blob, m, v: dpt_train_blob_numel
 * floats, updated in place; workspace 16-byte aligned; *loss_acc += the batch's summed loss. */
int dpt_train_step(const dpt_train_desc* desc_host, const dpt_train_data* data_host, const int64_t* index,
                   const int64_t* perm, int32_t batch, float* blob, float* m, float* v,
                   const dpt_adamw_args* args_host, float* workspace, double* loss_acc, void* stream);
/* the test loss of train.py:265-278: pack -> forward only (every position, DPT_TRAIN_FORWARD_ONLY) ->
 * cross-entropy without a gradient.  desc.dropout stays active (the reference's test loss runs in
 * training mode).  Same workspace as dpt_train_step. */
int dpt_train_eval_loss(const dpt_train_desc* desc_host, const dpt_train_data* data_host, const int64_t* index,
                        const int64_t* perm, int32_t batch, const float* blob, float* workspace,
                        double* loss_acc, void* stream);

/* ------------------------------------------------------------------ fresh-task training step
 * The pretraining step on tasks nobody stored: the batch dpt_train_pack_batch would gather from a
 * dataset is generated where it is consumed.  Sample b is global task first_task + b, and everything
 * about it -- the task, the behaviour policy, the H i.i.d. rollin steps with their reward noise, the
 * query state and the optimal-action label -- is a function of (seed, first_task + b) alone: not of
 * `batch`, of how a run is cut into steps, or of the device.  One workgroup per sample, one launch.
 *
 * Bandit (env DPT_FRESH_BANDIT, desc.state_dim 1, dim = desc.action_dim = A <= 32; envs/bandit_env.py:10-18,
 * collect_data.py:30-36): means[k] ~ U[0, 1) (Beta(1, 1): both reward types), the behaviour policy
 * probs = (1 - cov) p + cov e_rand with p = e / sum(e) ~ Dirichlet(1_A) in fp64, cov = index / 10 from
 * the 11-point grid and rand uniform over the arms (draws: DPT_STREAM_TASK above).  Row 1 + h of the
 * sample = [1 | onehot(arm_h) | 1 | float(r_h)] with arm_h and r_h the values dpt_rollin_bandit gives for
 * (means, probs, seed, first_task + b) at step h (DPT_STREAM_ROLLIN / DPT_STREAM_REWARD at counter h);
 * row 0 = [1 | 0 ...]; target = the one-hot of the first argmax of means.
 * DarkRoom (env DPT_FRESH_DARKROOM, desc.state_dim 2, desc.action_dim 5, dim <= 255;
 * collect_data.py:189-218 with rollin_type 'uniform'): the goal is an entry of the caller's list goals
 * (n_goals, 2) int32 -- a held-out split is respected by passing the train or the test list -- and the
 * action permutation an entry of perms (n_perms, 5) int32 when perms is given.  Row 1 + h =
 * [s | onehot(a) | s' | r], row 0 = [query | 0 ...] and the target = the one-hot of the expert action at
 * the query: the values dpt_rollin_darkroom (mode 0) gives for (goal, perm, seed, first_task + b).
 * Optional outputs (NULL: not written): means_out / probs_out (batch, A) fp64 (bandit); goal_out
 * (batch, 2), perm_out (batch, 5; identity without a list), query_out (batch, 2) (DarkRoom);
 * opt_action_out (batch) int32: the label's index (both).                                    */
#define DPT_FRESH_BANDIT 0
#define DPT_FRESH_DARKROOM 1
typedef struct dpt_fresh_args {
    int32_t env;            /* DPT_FRESH_BANDIT / DPT_FRESH_DARKROOM                            */
    int32_t type;           /* bandit: DPT_BANDIT_GAUSSIAN / DPT_BANDIT_BERNOULLI               */
    int32_t dim;            /* bandit: arms; DarkRoom: side of the room                         */
    int32_t H;              /* rollin steps: desc.window = 1 + H                                */
    int32_t n_goals;        /* DarkRoom: entries of goals, >= 1                                 */
    int32_t n_perms;        /* DarkRoom: entries of perms (0 with perms NULL)                   */
    double var;             /* bandit: reward noise std                                         */
    uint64_t seed;          /* Philox key                                                       */
    int64_t first_task;     /* global index of sample 0                                         */
    const int32_t* goals;   /* (n_goals, 2) or NULL (bandit)                                    */
    const int32_t* perms;   /* (n_perms, 5) or NULL                                             */
    double* means_out;
    double* probs_out;
    int32_t* goal_out;
    int32_t* perm_out;
    int32_t* query_out;
    int32_t* opt_action_out;
} dpt_fresh_args;
/* the generator alone: tokens (batch, 1 + H, 2 sd + A + 1) and targets (batch, A) fp32, what
 * dpt_train_pack_batch writes for a dataset holding these samples.  Host-side checks (null pointers,
 * batch outside 1..desc.batch, desc.window != 1 + H, H < 0, the desc's state_dim / action_dim against the
 * env, n_goals < 1, dim < 1; action_dim > 32 and dim > 255 -> DPT_EUNSUPPORTED) fail before the launch. */
int dpt_fresh_batch(const dpt_train_desc* desc_host, const dpt_fresh_args* args_host, int32_t batch, float* tokens,
                    float* targets, void* stream);
/* dpt_train_step with the generator in place of the pack: generator -> dpt_train_forward ->
 * cross-entropy -> dpt_train_backward -> AdamW, the same launches after the batch with the same
 * arguments, on the dpt_train_step_workspace_numel workspace.  desc flags 0; dropout through
 * desc.dropout / desc.dropout_seed. */
int dpt_fresh_step(const dpt_train_desc* desc_host, const dpt_fresh_args* args_host, int32_t batch, float* blob,
                   float* m, float* v, const dpt_adamw_args* adamw_host, float* workspace, double* loss_acc,
                   void* stream);
/* dpt_train_eval_loss on generated samples: forward only, desc.dropout active, the loss alone. */
int dpt_fresh_eval_loss(const dpt_train_desc* desc_host, const dpt_fresh_args* args_host, int32_t batch,
                        const float* blob, float* workspace, double* loss_acc, void* stream);

/* ------------------------------------------------------------------ fresh-task training step: the linear bandit
 * The same for the linear bandit (envs/bandit_env.py LinearBanditEnv; collect_data.py
 * generate_linear_bandit_histories): desc.state_dim 1, dim = desc.action_dim = A <= 32 arms with the caller's
 * features arms (A, lin_d) fp64 on the device, lin_d <= 8.  Task first_task + b:
 *   theta[p] = normal(seed, (p, task, DPT_STREAM_TASK)) / sqrt((double)lin_d)
 *   means[k] = ((arms[k][0] theta[0]) + arms[k][1] theta[1]) + ...   (fp64, multiply then add, index order)
 * the label = the one-hot of the first argmax of means, row 0 = [1 | 0 ...] and row 1 + h =
 * [1 | onehot(a_h) | 1 | float(r_h)] with r_h = means[a_h] + (0.0 + var normal(seed, (h, task,
 * DPT_STREAM_REWARD))), the rewards of a Gaussian bandit.
 * rollin DPT_FRESH_LINEAR_THOMPSON (collect_data.py rollin_linear_bandit_vec: ThompsonSamplingPolicy(std=var,
 * sample=True, prior_mean=0, prior_var=1); adaptive): per arm the count n_k, the reward sum S_k (added in time
 * order), the posterior mean m_k and std s_k, 0 and 1 before any pull.  At step h
 *   v_k = m_k + s_k normal(seed, (h, task, DPT_STREAM_POLICY + k)),  a_h = the first index of max v,
 * and then for a = a_h, variance = var var:  n_a += 1;  S_a += r_h;  w = variance / (variance + n_a 1.0);
 *   m_a = (1.0 - w) (S_a / n_a);  s_a = sqrt(1.0 / (1.0 + n_a / variance))
 * -- update_posterior_all with the running sum over the count where the reference takes np.mean.  The
 * keying is dpt_rollout_policy's at counter 0: that kernel (DPT_POLICY_THOMPSON, sample 1, ts_std var, prior
 * 0 / 1) on means_out sees the same normals, and gives the same rows wherever the two means leave the argmax
 * alone.  O(H) per task.  var > 0.
 * rollin DPT_FRESH_LINEAR_UNIFORM (data_type 'uniform'; i.i.d. steps): dpt_fresh_batch's bandit behaviour
 * policy and steps (DPT_STREAM_ROLLIN / DPT_STREAM_REWARD at counter h), its policy draws at the task
 * counters above.
 * Optional outputs (NULL: not written): theta_out (batch, lin_d), means_out (batch, A), probs_out (batch, A;
 * uniform rollin only) fp64, opt_action_out (batch) int32.                                        */
#define DPT_FRESH_LINEAR_THOMPSON 0
#define DPT_FRESH_LINEAR_UNIFORM 1
typedef struct dpt_fresh_linear_args {
    int32_t rollin;         /* DPT_FRESH_LINEAR_THOMPSON / DPT_FRESH_LINEAR_UNIFORM             */
    int32_t dim;            /* arms A                                                           */
    int32_t lin_d;          /* features per arm                                                 */
    int32_t H;              /* rollin steps: desc.window = 1 + H                                */
    double var;             /* reward noise std (and the Thompson policy's std)                 */
    uint64_t seed;          /* Philox key                                                       */
    int64_t first_task;     /* global index of sample 0                                         */
    const double* arms;     /* (dim, lin_d) fp64, device                                        */
    double* theta_out;
    double* means_out;
    double* probs_out;
    int32_t* opt_action_out;
} dpt_fresh_linear_args;
/* the generator alone, as dpt_fresh_batch.  Host-side checks fail before the launch: DPT_EINVAL for a null
 * desc / args / tokens / targets / arms, batch outside 1..desc.batch, desc.window != 1 + H, H < 0, state_dim
 * != 1, action_dim != dim, dim < 1, lin_d < 1, an unknown rollin, var < 0 or not finite, var == 0 with the
 * Thompson rollin; DPT_EUNSUPPORTED for dim > 32 or lin_d > 8. */
int dpt_fresh_linear_batch(const dpt_train_desc* desc_host, const dpt_fresh_linear_args* args_host, int32_t batch,
                           float* tokens, float* targets, void* stream);
/* dpt_fresh_step / dpt_fresh_eval_loss with this generator: the same chain, workspace and checks. */
int dpt_fresh_linear_step(const dpt_train_desc* desc_host, const dpt_fresh_linear_args* args_host, int32_t batch,
                          float* blob, float* m, float* v, const dpt_adamw_args* adamw_host, float* workspace,
                          double* loss_acc, void* stream);
int dpt_fresh_linear_eval_loss(const dpt_train_desc* desc_host, const dpt_fresh_linear_args* args_host,
                               int32_t batch, const float* blob, float* workspace, double* loss_acc, void* stream);

/* ------------------------------------------------------------------ interactive training step
 * One episode of train_interactive.py:92-143 (the on-policy variant: sample fresh bandits, roll the
 * model out for K steps with sampling, one CrossEntropyLoss() on the LAST step's logits against the
 * optimal arm, one AdamW step) without the reference's K whole-window autograd forwards: the K - 1
 * steps whose records reach the loss run through dpt_rollout_bandit_generic (exact y-cache decode,
 * straight from the training blob), the window is packed from the rollout's records, and one
 * training forward / backward at window K gives the gradient.  The reference's K-th action and
 * reward never reach the loss and are not drawn.  ABI 8, additive.                            */

/* tokens (N, Hc + 1, A + 3) from rollout records actions (N, Hc) int32 / rewards (N, Hc) fp64:
 * row 0 = [1, 0_A, 0, 0], row 1 + j = [1, onehot(a_j), 1, float(r_j)] (models/net.py:42-54 with
 * the bandit's state 1).  Hc = 0 (the query row alone; actions / rewards may be NULL) is legal.
 * Copies and one double-to-float conversion: bit-exact.  An action outside [0, A) packs zeros. */
int dpt_interactive_pack(const int32_t* actions, const double* rewards, int32_t N, int32_t Hc, int32_t A,
                         float* tokens, void* stream);
/* CrossEntropyLoss at the last position against class indices targets (batch) int64:
 *   *loss_acc += scale * sum_b (lse(preds[b][window-1]) - preds[b][window-1][targets[b]])
 *   dpreds (batch, window, A) = scale * (softmax - onehot) at the last position, exactly zero at
 *   every other one (dpreds NULL: the loss alone).
 * scale = 1 / (envs of the whole step), so the chunks of a step add up to CrossEntropyLoss()'s mean.
 * fp64 per element, one rounding on the store; partial: `batch` doubles of scratch; the sum runs in
 * a fixed order, so repeated calls are bit-identical.  A <= 32.  A target outside [0, A) adds
 * nothing to the loss or the gradient. */
int dpt_train_ce_last(const float* preds, const int64_t* targets, int32_t batch, int32_t window, int32_t A,
                      double scale, float* dpreds, double* partial, double* loss_acc, void* stream);

/* dpt_interactive_args.flags */
#define DPT_INTERACTIVE_ACCUMULATE 1 /* dblob += the chunk's gradient (default: dblob = it)             */
#define DPT_INTERACTIVE_FULL_WIDTH 2 /* the last block at full width (no DPT_TRAIN_LAST_LOSS): the same
                                      * gradient up to fp32 summation order, slower; kept for A/B runs  */
typedef struct dpt_interactive_args {
    int32_t N;              /* envs of this chunk                                            */
    int32_t K;              /* window: K - 1 rolled-out steps, then the query of step K - 1  */
    int32_t type;           /* DPT_BANDIT_GAUSSIAN / DPT_BANDIT_BERNOULLI (DPT_BANDIT_F32 is added:
                             * GPUBanditEnv's reward arithmetic)                             */
    int32_t flags;          /* DPT_INTERACTIVE_* or 0                                        */
    int64_t first_task;     /* global id of env 0 of the chunk (Philox counter)              */
    double var;             /* reward noise std                                              */
    double scale;           /* 1 / (envs of the whole step)                                  */
    uint64_t seed;
    uint64_t counter;       /* Philox counter of step 0                                      */
    const double* means;    /* (N, A)                                                        */
    const int64_t* targets; /* (N) optimal arm (GPUBanditEnv.opt_a_index)                    */
    const double* uniforms; /* (K - 1, N) or NULL -> Philox, as dpt_rollout_bandit_generic   */
    const double* noise;    /* (K - 1, N) or NULL                                            */
    int32_t* actions_out;   /* (N, K - 1) the rollout's records, always written              */
    double* rewards_out;    /* (N, K - 1)                                                    */
    float* workspace;       /* dpt_interactive_workspace_numel floats, 16-byte aligned       */
    float* dblob;           /* dpt_train_blob_numel floats                                   */
    double* loss_acc;       /* += scale * the chunk's summed loss                            */
} dpt_interactive_args;

/* floats of workspace for a chunk of N envs at window K: the training workspace, tokens, preds,
 * dpreds, a gradient blob, the per-env losses, and (K > 1) the rollout's workspace and arm values */
int dpt_interactive_workspace_numel(const dpt_train_desc* desc_host, int32_t N, int32_t K, int64_t* numel_out_host);
/* The gradient of one chunk, chained on one stream with no host synchronisation and no allocation:
 * dpt_rollout_bandit_generic for K - 1 sampled steps from `blob` (skipped when K = 1) ->
 * dpt_interactive_pack -> dpt_train_forward at window K (DPT_TRAIN_LAST_LOSS: the loss reads the last
 * position only) -> dpt_train_ce_last -> dpt_train_backward (-> dblob += with
 * DPT_INTERACTIVE_ACCUMULATE, element-wise, in a fixed order).  desc: the model's n_layer,
 * n_embd, state_dim, action_dim, n_positions (batch / window / flags are ignored: N and K rule).
 * Host checks fail before any launch: null pointers, N < 1, K < 1, K > n_positions, state_dim != 1,
 * action_dim > 32 (DPT_EUNSUPPORTED), dropout != 0, a workspace that is not 16-byte aligned. */
int dpt_interactive_grad(const dpt_train_desc* desc_host, const float* blob, const dpt_interactive_args* args_host,
                         void* stream);

/* ------------------------------------------------------------------ interactive DarkRoom (MDP) training step
 * The on-policy episode of train_interactive.py:92-143 for the DarkRoom MDP (the reference runs it for
 * bandits only, :54-55).  N envs with goals (N, 2) in [0, dim), state_dim 2, action_dim 5, s_0 = (0, 0).
 * For t = 0 .. K - 1:
 *   W_t (N, t + 1, 10) fp32: row 0 = [s_t | 0_5 | 0_2 | 0], row 1 + j = [s_j | onehot(a_j) | s_{j+1} | r_j]
 *     for j < t in time order (models/net.py:42-54 on the transitions so far; small integers: exact);
 *   logits_t (N, 5) = the model's last position on W_t; target_t = opt_action(s_t)
 *     (envs/darkroom_env.py:69-82, permuted :105-111);
 *   for t < K - 1: a_t = dpt_select_action's rule on logits_t (sampled at temp 1 with uniforms[t][i] or
 *     Philox(seed, (counter + t, first_task + i, DPT_STREAM_SELECT)); greedy: first argmax), then
 *     (s_{t+1}, r_t) = dpt_darkroom_step(s_t, a_t).  The K-th action is never drawn.
 * The actions are data: no gradient flows through the selection.  In an MDP the query state changes every
 * step and sits at position 0, so no cached decode exists: every step is a forward over its whole window.
 * ABI 8, additive.                                                                               */

/* tokens (N, t + 1, 10) = W_t from the records states (N, K, 2), actions (N, K - 1), rewards (N, K - 1)
 * int32, 0 <= t < K (t = 0 reads no action or reward: both may be NULL when K = 1).  One thread per
 * output float, copies and int -> float conversions only: bit-exact.  An action outside [0, 5) packs a
 * zero one-hot. */
int dpt_mdp_pack(const int32_t* states, const int32_t* actions, const int32_t* rewards, int32_t N, int32_t K,
                 int32_t t, float* tokens, void* stream);
/* Step t < K - 1 of the episode for N envs in one launch, one thread per env: reads the env's
 * last-position row of logits (N, window, 5) (row stride window * 5), selects a_t (sample 1: the step's
 * uniforms (N) or NULL -> Philox(seed, (counter, first_task + i, DPT_STREAM_SELECT)); sample 0: first
 * argmax), moves from states[i][t], and writes actions[i][t], rewards[i][t], states[i][t + 1] and
 * targets[i][t + 1] = opt_action(s_{t+1}) (also into target_next (N) int64 when given:
 * dpt_train_ce_last's class indices of the next step).  Bit-equal to dpt_select_action (temp 1) ->
 * dpt_darkroom_step -> dpt_darkroom_opt_action. */
int dpt_darkroom_act_step(const float* logits, int32_t N, int32_t window, int32_t K, int32_t t, int32_t dim,
                          int32_t sample, const double* uniforms, uint64_t seed, uint64_t counter,
                          int64_t first_task, const int32_t* goal, const int32_t* perm, int32_t* states,
                          int32_t* actions, int32_t* rewards, int32_t* targets, int64_t* target_next,
                          void* stream);

/* dpt_interactive_mdp_args.loss_mode; N below = the envs of the whole step, not of a chunk */
#define DPT_MDP_LOSS_NONE 0  /* the rollout alone (evaluation): dblob and loss_acc may be NULL            */
#define DPT_MDP_LOSS_LAST 1  /* (1 / N) sum_i CE(logits_{K-1,i}, target_{K-1,i}): train_interactive.py:134-135 */
#define DPT_MDP_LOSS_EVERY 2 /* (1 / (N K)) sum_t sum_i CE(logits_{t,i}, target_{t,i}): on-policy imitation of
                              * the optimal action at every visited state                               */
typedef struct dpt_interactive_mdp_args {
    int32_t N;              /* envs of this chunk                                            */
    int32_t K;              /* steps: K forwards at windows 1 .. K, K - 1 transitions        */
    int32_t dim;            /* room side, >= 1                                               */
    int32_t loss_mode;      /* DPT_MDP_LOSS_*                                                */
    int32_t flags;          /* DPT_INTERACTIVE_ACCUMULATE or 0                               */
    int32_t sample;         /* 1: sampled actions (temp 1), 0: greedy                        */
    int64_t first_task;     /* global id of env 0 of the chunk (Philox counter)              */
    double scale;           /* LAST: 1 / (envs of the whole step); EVERY: 1 / (envs * K)     */
    uint64_t seed;
    uint64_t counter;       /* Philox counter of step 0                                      */
    const int32_t* goal;    /* (N, 2) in [0, dim)                                            */
    const int32_t* perm;    /* (N, 5) as dpt_darkroom_step takes it, or NULL                 */
    const double* uniforms; /* (K - 1, N) or NULL -> Philox                                  */
    int32_t* states_out;    /* (N, K, 2) s_0 .. s_{K-1}, always written                      */
    int32_t* actions_out;   /* (N, K - 1)                                                    */
    int32_t* rewards_out;   /* (N, K - 1)                                                    */
    int32_t* targets_out;   /* (N, K) opt_action(s_t)                                        */
    float* workspace;       /* dpt_interactive_mdp_workspace_numel floats, 16-byte aligned   */
    float* dblob;           /* dpt_train_blob_numel floats (NULL with DPT_MDP_LOSS_NONE)     */
    double* loss_acc;       /* += scale * the chunk's summed loss (NULL with LOSS_NONE)      */
} dpt_interactive_mdp_args;

/* floats of workspace for a chunk of N envs over K steps in `loss_mode`: the training workspace at window
 * K (it serves every shorter window), tokens, logits, the int64 targets of the current step and, in a loss
 * mode, dpreds, the chunk's gradient blob, the per-env losses and (EVERY) one step's gradient blob */
int dpt_interactive_mdp_workspace_numel(const dpt_train_desc* desc_host, int32_t N, int32_t K, int32_t loss_mode,
                                        int64_t* numel_out_host);
/* One chunk of envs, one chain of launches on one stream: no host synchronisation, no allocation, no side
 * streams, no graph capture.  For t = 0 .. K - 1: dpt_mdp_pack -> dpt_train_forward at window t + 1 (a
 * loss-bearing step -- every step in EVERY, step K - 1 in LAST: a training forward with
 * DPT_TRAIN_LAST_LOSS, dpt_train_ce_last against target_t with `scale`, dpt_train_backward, and the
 * step's gradient added into the chunk's element-wise in step order; otherwise DPT_TRAIN_FORWARD_ONLY |
 * DPT_TRAIN_LAST_ONLY) -> dpt_darkroom_act_step for t < K - 1.  With DPT_INTERACTIVE_ACCUMULATE the
 * chunk's gradient is added to dblob, otherwise it replaces it (apply dpt_adamw_step after the last
 * chunk).  desc: the model's n_layer, n_embd, state_dim, action_dim, n_positions (batch / window / flags
 * are ignored).  Host checks fail before any launch: null pointers, N < 1, K < 1, K > n_positions, N * K
 * above 2^26 rows, state_dim != 2 or action_dim != 5 (DPT_EUNSUPPORTED), dim < 1, dropout != 0, an unknown
 * loss mode or flags, a workspace that is not 16-byte aligned, dblob or loss_acc NULL in a loss mode. */
int dpt_interactive_mdp_grad(const dpt_train_desc* desc_host, const float* blob,
                             const dpt_interactive_mdp_args* args_host, void* stream);

/* ------------------------------------------------------------------ in-episode DarkRoom rollout, one launch
 * The episode of the section above without a loss, for a width-32 dpt_model: one workgroup per env runs
 * all K steps in one kernel.  The model's parameters are loaded into LDS once per launch, the episode's
 * records live in LDS, and each step's window W_t is embedded from them and run through the MFMA forward
 * of dpt_forward_window's prefill; the logits of position t select a_t by dpt_select_action's rule at
 * temp 1 (uniforms[t][i], or Philox(seed, (counter + t, first_task + i, DPT_STREAM_SELECT)); greedy: the
 * first argmax), then dpt_darkroom_step's move and dpt_darkroom_opt_action's label.  The records are
 * those of dpt_interactive_mdp_grad; the logits are the prefill's (fp32, within the reference logit
 * bound of the float64 forward), not the training forward's, so a draw whose uniform lies within that
 * bound of a cdf edge may fall differently in the two.  No workspace, no allocation, no host
 * synchronisation.  ABI 8, additive. */
typedef struct dpt_darkroom_episode_args {
    int32_t N;              /* envs                                                          */
    int32_t K;              /* steps: K forwards at windows 1 .. K, K - 1 transitions        */
    int32_t dim;            /* room side, 1 .. 255                                           */
    int32_t sample;         /* nonzero: sampled actions (temp 1), 0: greedy                  */
    int64_t first_task;     /* global id of env 0 (Philox counter)                           */
    uint64_t seed;
    uint64_t counter;       /* Philox counter of step 0                                      */
    const int32_t* goal;    /* (N, 2) in [0, dim)                                            */
    const int32_t* perm;    /* (N, 5) as dpt_darkroom_step takes it, or NULL                 */
    const double* uniforms; /* (K - 1, N) or NULL -> Philox                                  */
    int32_t* states;        /* (N, K, 2) s_0 .. s_{K-1}                                      */
    int32_t* actions;       /* (N, K - 1) (may be NULL when K = 1)                           */
    int32_t* rewards;       /* (N, K - 1) (may be NULL when K = 1)                           */
    int32_t* targets;       /* (N, K) opt_action(s_t)                                        */
    float* logits;          /* (N, K, 5) the logits every step selected from, or NULL        */
    int32_t* returns;       /* (N) the sum of the K - 1 rewards, or NULL                     */
} dpt_darkroom_episode_args;

/* Host checks fail before any launch.  DPT_EINVAL: null model, args, goal, states or targets; N < 1;
 * K < 1; K > n_positions; dim < 1 or dim > 255; actions or rewards NULL while K > 1.  DPT_EUNSUPPORTED:
 * state_dim != 2 or action_dim != 5; n_embd != 32; K above dpt_forward_window's prefill limit for the model
 * (512 tokens at most), or a model so deep that its parameter block and the episode's records do not fit
 * in LDS next to the keys and values of K tokens. */
int dpt_rollout_darkroom_episode(const dpt_model* model, const dpt_darkroom_episode_args* args_host, void* stream);

/* ------------------------------------------------------------------ explorer/exploiter training step
 * One episode of train_explorer_exploiter.py:102-192 for two models of one config.  The explorer's
 * sampled action goes into the context while the env is stepped with a uniformly random arm; the
 * exploiter's per-step loss l_t = CE(last-position logits, optimal arm) gives the advantages
 * adv[:, t-1] = l_t - l_{t-1}; the exploiter takes the mean CE over all N K positions of the final
 * K-token window, the explorer the mean over N (K-1) of exp(adv / beta) CE(logits_j, context action j).
 * Nothing the exploiter produces reaches the context, attention is causal and the query token sits at
 * position 0, so its step-t logits are row t of ONE forward over the final window -- the forward its
 * update needs anyway -- and only the explorer is decoded step by step (K - 1 steps of the y-cache
 * rollout; the K-th action and reward reach neither loss and are not drawn).  ABI 8, additive.   */

/* dpt_rollout_bandit_generic with the env action apart from the context action: the selected action
 * still goes to actions_out and into the next token, while the reward and arm_value_out come from
 *   env_actions (H, N) int32 (laid out like uniforms) when given -- device memory, so a value outside
 *     [0, A) cannot be rejected on the host and is CLAMPED into [0, A) -- or
 *   min(A - 1, floor(u A)), u = Philox(seed, (counter + h, first_task + i, DPT_STREAM_ENVACT)) when
 *     env_actions is NULL and random_env = 1.
 * env_actions NULL and random_env 0: the selected action, every output bit-identical to
 * dpt_rollout_bandit_generic.  env_actions_out (N, H) or NULL: the env actions taken.            */
int dpt_rollout_bandit_generic_env(const dpt_train_desc* desc_host, const float* blob,
                                   const dpt_bandit_rollout_args* args_host, const int32_t* env_actions,
                                   int32_t random_env, int32_t* env_actions_out, void* stream);

/* Cross-entropy with class targets at EVERY position of preds (batch, window, A).  Exactly one of
 * targets_seq (batch) int64 (one class per sequence, broadcast over its positions) and targets_row
 * (batch, window) int32 is non-NULL; weights (batch, window) double or NULL (all ones).
 *   rowloss (batch, window) double = lse(x) - x[target], unweighted
 *   dpreds = scale * w * (softmax - onehot), exactly 0 where w == 0 (dpreds NULL: no gradient)
 *   *loss_acc += scale * sum_rows w * rowloss
 * fp64 per element from the fp32 logits, one rounding on the store; the sum runs in a fixed order
 * (rows thread-strided in index order, then an LDS tree), so repeated calls are bit-identical.
 * A <= 32.  A target outside [0, A): zero rowloss, zero loss, zero gradient for that row.          */
int dpt_train_ce_rows(const float* preds, const int64_t* targets_seq, const int32_t* targets_row,
                      const double* weights, int32_t batch, int32_t window, int32_t A, double scale,
                      double* rowloss, float* dpreds, double* loss_acc, void* stream);
/* The explorer's advantage weights from the exploiter's row losses, in double:
 *   w[b][j] = exp((rowloss[b][j+1] - rowloss[b][j]) * inv_beta) for j < window - 1, w[b][window-1] = 0 */
int dpt_explore_weights(const double* rowloss, int32_t batch, int32_t window, double inv_beta, double* weights,
                        void* stream);

#define DPT_EXPLORE_ACCUMULATE 1 /* both dblobs += the chunk's gradients (default: = them) */
typedef struct dpt_explore_args {
    int32_t N;                 /* envs of this chunk                                              */
    int32_t K;                 /* window >= 2: K - 1 rolled-out steps                             */
    int32_t type;              /* DPT_BANDIT_GAUSSIAN / DPT_BANDIT_BERNOULLI (DPT_BANDIT_F32 is added) */
    int32_t flags;             /* DPT_EXPLORE_ACCUMULATE or 0                                     */
    int64_t first_task;        /* global id of env 0 of the chunk (Philox counter)                */
    double var;                /* reward noise std                                                */
    double beta;               /* advantage temperature, finite and > 0                           */
    double scale_exploiter;    /* 1 / (envs of the whole step * K)                                */
    double scale_explorer;     /* 1 / (envs of the whole step * (K - 1))                          */
    uint64_t seed;
    uint64_t counter;          /* Philox counter of step 0                                        */
    const double* means;       /* (N, A)                                                          */
    const int64_t* targets;    /* (N) optimal arm (GPUBanditEnv.opt_a_index)                      */
    const double* uniforms;    /* (K - 1, N) the explorer's selection uniforms, or NULL -> Philox */
    const double* noise;       /* (K - 1, N) or NULL                                              */
    const int32_t* env_actions; /* (K - 1, N) the arms the env is stepped with (clamped to [0, A)), or
                                 * NULL -> uniform over the arms from DPT_STREAM_ENVACT            */
    int32_t* actions_out;      /* (N, K - 1) the context actions (the explorer's), always written */
    int32_t* env_actions_out;  /* (N, K - 1) the env actions taken, always written                */
    double* rewards_out;       /* (N, K - 1)                                                      */
    float* workspace;          /* dpt_explore_workspace_numel floats, 16-byte aligned             */
    float* dblob_explorer;     /* dpt_train_blob_numel floats each, distinct                      */
    float* dblob_exploiter;
    double* loss_explorer;     /* += scale_explorer * sum w CE(explorer rows, context actions)    */
    double* loss_exploiter;    /* += scale_exploiter * sum CE(exploiter rows, targets)            */
} dpt_explore_args;

/* floats of workspace for a chunk of N envs at window K: ONE training workspace, token buffer and
 * preds / dpreds pair shared by the two models (the exploiter's pass ends on the stream before the
 * explorer's begins), a gradient blob, and on top of that the row losses, the weights, the row
 * targets, the rollout's workspace and its arm values */
int dpt_explore_workspace_numel(const dpt_train_desc* desc_host, int32_t N, int32_t K, int64_t* numel_out_host);
/* The gradients of one chunk for both models, one chain of launches on one stream with no host
 * synchronisation and no allocation: the explorer's rollout for K - 1 sampled steps (env stepped
 * apart) -> dpt_interactive_pack -> exploiter dpt_train_forward (full width) -> dpt_train_ce_rows
 * against targets -> exploiter dpt_train_backward -> dpt_explore_weights -> explorer forward ->
 * dpt_train_ce_rows with the weights against the recorded context actions (position K - 1 has
 * weight 0) -> explorer backward.  The advantages use exploiter_blob as passed (apply AdamW to
 * both models after the last chunk: dpt_adamw_step).  Host checks fail before any launch:
 * everything dpt_interactive_grad checks, K < 2, beta not finite or <= 0, null or equal blobs,
 * null or equal gradient blobs. */
int dpt_explore_grad(const dpt_train_desc* desc_host, const float* explorer_blob, const float* exploiter_blob,
                     const dpt_explore_args* args_host, void* stream);

/* ------------------------------------------------------------------ explore-then-exploit evaluation
 * What the explorer/exploiter step trains for, measured: after a budget of t = 0 .. H exploratory pulls
 * the exploiter recommends an arm from those t transitions, and the report is the simple regret
 * mu* - mu[recommended] as a curve over t.  As in the training step, the exploiter's logits after t
 * transitions are row t of ONE forward over the final (1 + H)-token window (constant query token at
 * position 0, causal attention): the whole curve of N tasks is one pack, one forward-only training
 * forward at every position and one reduction, where the reference's surface (Transformer.forward in
 * test mode, the last position of a growing window) needs H + 1 forwards.  ABI 8, additive.
 *
 * dpt_recommend_curve, per row (i, t) of logits (N, T, A) fp32, means (N, A) fp64, targets (N) int64
 * (the optimal arm), all arithmetic in fp64 from the fp32 logits with one rounding on the store:
 *   greedy_arm     (N, T) int32  first index of the maximum logit (np.argmax: the first NaN when there
 *                                is one); always in [0, A)
 *   greedy_value   (N, T) fp64   means[i][greedy_arm]
 *   expected_value (N, T) fp64   sum_a p_a means[i][a], p = softmax(logits[i][t]) with the maximum
 *                                subtracted: the value of SAMPLING the recommendation
 *   p_opt          (N, T) fp64   p[targets[i]], 0 for a target outside [0, A)
 * Any output may be NULL (targets may be NULL when p_opt is).  The value arrays are laid out like
 * arm_value_out of the rollouts, so dpt_regret_moments(value, opt, N, T, ...) gives the moments of the
 * simple regret opt - value over tasks.  One launch; A <= 32 (else DPT_EUNSUPPORTED); fixed reduction
 * order (deterministic).                                                                            */
int dpt_recommend_curve(const float* logits, const double* means, const int64_t* targets, int32_t N, int32_t T,
                        int32_t A, int32_t* greedy_arm, double* greedy_value, double* expected_value, double* p_opt,
                        void* stream);
/* ctrls/ctrl_bandit.py:91-117, EmpMeanPolicy(online=False), on every prefix of the records actions (N, H)
 * int32 / rewards (N, H) fp64.  For t = 0 .. H: sum[a] and cnt[a] accumulate over the pulls j < t IN
 * PULL ORDER in fp64, b_mean = sum / max(1, cnt), emp_arm (N, H + 1) int32 = the first index of its
 * maximum (arm 0 at t = 0), emp_value (N, H + 1) fp64 = means[i][emp_arm].  An action outside [0, A)
 * adds to no arm (dpt_interactive_pack packs zeros for it).  H = 0 (actions / rewards may be NULL) is
 * legal; either output may be NULL.  A <= 32.                                                        */
int dpt_empirical_recommend(const int32_t* actions, const double* rewards, const double* means, int32_t N,
                            int32_t H, int32_t A, int32_t* emp_arm, double* emp_value, void* stream);

typedef struct dpt_exploit_eval_args {
    int32_t N;                 /* tasks of this chunk                                              */
    int32_t H;                 /* recorded pulls per task (>= 0): budgets 0 .. H                   */
    int32_t flags;             /* 0                                                                */
    int32_t reserved;          /* 0                                                                */
    const int32_t* actions;    /* (N, H) the context actions of the records (NULL when H = 0)      */
    const double* rewards;     /* (N, H)                                                           */
    const double* means;       /* (N, A)                                                           */
    const int64_t* targets;    /* (N) optimal arm (may be NULL when p_opt is)                      */
    float* workspace;          /* dpt_exploit_eval_workspace_numel floats, 16-byte aligned         */
    float* logits_out;         /* (N, H + 1, A) the exploiter's logits after every budget, or NULL */
    int32_t* greedy_arm;       /* (N, H + 1) each, or NULL: as dpt_recommend_curve                 */
    double* greedy_value;
    double* expected_value;
    double* p_opt;
} dpt_exploit_eval_args;

/* floats of workspace for a chunk of N tasks with H pulls: the forward-only training workspace at
 * window H + 1, the tokens and the logits */
int dpt_exploit_eval_workspace_numel(const dpt_train_desc* desc_host, int32_t N, int32_t H, int64_t* numel_out_host);
/* One chunk of tasks, chained on one stream with no host synchronisation and no allocation, straight
 * from a packed blob (a module's or a trainer's master blob): dpt_interactive_pack -> dpt_train_forward
 * (DPT_TRAIN_FORWARD_ONLY, every position, window H + 1) -> dpt_recommend_curve.  desc: the model's
 * n_layer, n_embd, state_dim, action_dim, n_positions (batch / window / flags are ignored: N and H
 * rule).  Host checks fail before any launch: null pointers, N < 1, H < 0, 1 + H > n_positions,
 * state_dim != 1, action_dim > 32 (DPT_EUNSUPPORTED), dropout != 0, non-zero flags / reserved, a
 * workspace that is not 16-byte aligned. */
int dpt_exploit_eval(const dpt_train_desc* desc_host, const float* blob, const dpt_exploit_eval_args* args_host,
                     void* stream);

/* ------------------------------------------------------------------ Bayes posterior of the optimal action
 * The minimiser of the pretraining cross-entropy is the posterior of the optimal action given the context;
 * for the two task families the fresh-task generator draws from it is computable, and these entry points
 * compute it for EVERY prefix t = 0 .. H of a context (row t: the first t transitions), where the model's
 * logits after t transitions already live.  ABI 8, additive.  tests/posterior_oracle.py restates the
 * definitions in numpy.
 *
 * Bandit grid posterior (prior means ~ U[0,1]^A, i.i.d. rollin, `var` the reward std as everywhere here).
 *   inputs   actions (N, H) int32, rewards (N, H) fp64, A <= 32, type DPT_BANDIT_GAUSSIAN / _BERNOULLI,
 *            var (Gaussian: > 0), G
 *   grid     G a multiple of 64 in [64, 8192]; x_i = (i + 0.5) / G
 *   row t    n_a = the number of pulls j < t with actions[j] == a, s_a = the sum of their rewards IN PULL
 *            ORDER in fp64; an action outside [0, A) adds to no arm
 *   log-likelihood, in exactly this operation order (no fused multiply-add):
 *            Gaussian   l_a(i) = -((n_a * x_i) * x_i - (2 * s_a) * x_i) / ((2 * var) * var)
 *            Bernoulli  l_a(i) = s_a * log(x_i) + (n_a - s_a) * log1p(-x_i)
 *   weights  w_a(i) = exp(l_a(i) - max_i l_a) / sum_i exp(l_a(i) - max_i l_a)
 *   mid-point CDF        C_a(i) = sum_{j<i} w_a(j) + w_a(i) / 2
 *   unnormalised         u_a = sum_i w_a(i) * prod_{b != a} C_b(i)
 *   output   post[n][t][a] = u_a / sum_b u_b, (N, H + 1, A) fp64; 1 for A == 1
 * The reduction order is fixed: repeated calls are bit-identical, and a task's rows do not depend on N or
 * on how the caller chunks the tasks.
 *
 * DarkRoom posterior (the goal uniform over a list, reward 1 iff the next state is the goal).
 *   inputs   goals (n_goals, 2) int32: the prior, with multiplicity; query (N, 2), next_states (N, H, 2),
 *            rewards (N, H), all int32
 *   goal k is consistent with the first t transitions iff for every j < t
 *            (rewards[j] != 0) == (next_states[j] == goals[k])
 *   post[n][t][a] = #{consistent k whose expert action at the query (identity permutation:
 *            dpt_darkroom_opt_action with perm NULL) is a} / #{consistent k}, one fp64 division of exact
 *            integers, (N, H + 1, 5) fp64; a row with no consistent goal is all zeros
 *   consistent (N, H + 1) int32, optional: the number of consistent k
 * Action-permutation lists make the permutation latent too and are not covered.
 *
 * Compare: post (N, T, A) fp64, logits (N, T, A) fp32, targets (N) int64 in [0, A) (a target outside:
 * NaN in both nll outputs).  All arithmetic in fp64, logq = log_softmax(logits) with the maximum
 * subtracted; each output (N, T) fp64 and each may be NULL:
 *   nll_model = -logq[target]            nll_bayes = -log post[target]   (+inf where it is 0)
 *   kl        = sum_{a: post_a > 0} post_a (log post_a - logq_a)
 *   entropy   = -sum_{a: post_a > 0} post_a log post_a
 * so E[nll_model] - E[nll_bayes] = E[kl] when post is the posterior of the target.                        */
typedef struct dpt_bandit_posterior_args {
    int32_t N;                 /* tasks                                                             */
    int32_t H;                 /* recorded pulls per task (>= 0): rows 0 .. H                       */
    int32_t A;                 /* arms, <= 32                                                       */
    int32_t type;              /* DPT_BANDIT_GAUSSIAN / DPT_BANDIT_BERNOULLI                        */
    int32_t G;                 /* grid points: a multiple of 64 in [64, 8192]                       */
    int32_t flags;             /* 0                                                                 */
    double var;                /* reward std (Gaussian: > 0; Bernoulli: ignored)                    */
    const int32_t* actions;    /* (N, H) (NULL when H = 0)                                          */
    const double* rewards;     /* (N, H)                                                            */
    double* workspace;         /* dpt_bandit_posterior_workspace_numel doubles                      */
    double* post;              /* (N, H + 1, A)                                                     */
} dpt_bandit_posterior_args;

/* doubles of workspace for N tasks: the grid's log tables (2 G) and, where the 2 A G doubles of a task's
 * weights and CDFs do not fit in LDS (2 A G 8 B above 128 KiB), one such slot per resident workgroup */
int dpt_bandit_posterior_workspace_numel(int32_t N, int32_t A, int32_t G, int64_t* numel_out_host);
/* One launch (two for Bernoulli: the log tables first), no host synchronisation, no allocation.  Host
 * checks fail before any launch.  DPT_EINVAL: null args / workspace / post, null actions or rewards while
 * H > 0, N < 1, H < 0, A < 1, a G that is not a multiple of 64 in [64, 8192], a Gaussian var <= 0,
 * non-zero flags.  DPT_EUNSUPPORTED: A > 32, an unknown type. */
int dpt_bandit_posterior(const dpt_bandit_posterior_args* args_host, void* stream);

typedef struct dpt_darkroom_posterior_args {
    int32_t N;                 /* samples                                                           */
    int32_t H;                 /* transitions per sample (>= 0): rows 0 .. H                        */
    int32_t dim;               /* room side, <= 255                                                 */
    int32_t n_goals;           /* rows of goals, 1 .. 2^18                                          */
    int32_t flags;             /* 0                                                                 */
    int32_t reserved;          /* 0                                                                 */
    const int32_t* goals;      /* (n_goals, 2) the prior, with multiplicity                         */
    const int32_t* query;      /* (N, 2)                                                            */
    const int32_t* next_states;/* (N, H, 2) (NULL when H = 0)                                       */
    const int32_t* rewards;    /* (N, H)                                                            */
    double* post;              /* (N, H + 1, 5)                                                     */
    int32_t* consistent;       /* (N, H + 1), or NULL                                               */
} dpt_darkroom_posterior_args;

/* One launch, one wave per sample.  DPT_EINVAL: null args / goals / query / post, null next_states or
 * rewards while H > 0, N < 1, H < 0, n_goals < 1, dim < 1, non-zero flags / reserved.  DPT_EUNSUPPORTED:
 * dim > 255, n_goals > 2^18. */
int dpt_darkroom_posterior(const dpt_darkroom_posterior_args* args_host, void* stream);

typedef struct dpt_posterior_compare_args {
    int32_t N;                 /* tasks                                                             */
    int32_t T;                 /* rows per task (>= 1)                                              */
    int32_t A;                 /* actions, <= 32                                                    */
    int32_t flags;             /* 0                                                                 */
    const double* post;        /* (N, T, A)                                                         */
    const float* logits;       /* (N, T, A)                                                         */
    const int64_t* targets;    /* (N)                                                               */
    double* nll_model;         /* (N, T) each, or NULL                                              */
    double* nll_bayes;
    double* kl;
    double* entropy;
} dpt_posterior_compare_args;

/* One launch, one thread per row.  DPT_EINVAL: null args / post / logits / targets, N < 1, T < 1, A < 1,
 * non-zero flags.  DPT_EUNSUPPORTED: A > 32. */
int dpt_posterior_compare(const dpt_posterior_compare_args* args_host, void* stream);

/* ------------------------------------------------------------------ Linear bandit, lin_d = 2
 * The posterior of the optimal arm of the linear bandit (reward = x_a . theta + var * normal) for arms in the
 * plane, on every prefix of a record.  The posterior of theta is a 2-D Gaussian N(m, S), the regions where an
 * arm is optimal are wedges through theta = 0, and along a ray from m the winner is the upper envelope of A
 * straight lines: a 1-D angular quadrature of positive terms.  ABI 8, additive.
 * tests/linear_posterior_oracle.py restates the definition in numpy.
 *   inputs   arms X (A, 2) fp64, actions (N, H) int32, rewards (N, H) fp64, var > 0 (the noise std), G
 *   prior    theta ~ N(0, I / 2) (sample_linear's normal / sqrt(lin_d)): precision 2 I
 *   grid     G a multiple of 64 in [64, 65536]; phi_i = (6.283185307179586 * (i + 0.5)) / G,
 *            omega_i = (cos phi_i, sin phi_i)
 * All arithmetic in fp64, no fused multiply-add, every expression in the order written here.
 *   statistics of row t, over the pulls j < t IN PULL ORDER with x = X[actions[j]], r = rewards[j],
 *            v2 = var * var (an action outside [0, A) adds nothing):
 *              sxx += (x0 * x0) / v2   sxy += (x0 * x1) / v2   syy += (x1 * x1) / v2
 *              b0  += (r * x0) / v2    b1  += (r * x1) / v2
 *   moments    l00 = 2 + sxx   l01 = sxy   l11 = 2 + syy   det = l00 * l11 - l01 * l01
 *              S00 = l11 / det   S01 = -(l01 / det)   S11 = l00 / det
 *              m0 = S00 * b0 + S01 * b1   m1 = S01 * b0 + S11 * b1
 *              L00 = sqrt(S00)   L10 = S01 / L00   L11 = 1 / sqrt(l11)        (S = L L^T, L lower)
 *   per arm    alpha_a = x0 * m0 + x1 * m1   xl0_a = x0 * L00 + x1 * L10   xl1_a = x1 * L11
 *              beta_a(i) = xl0_a * cos phi_i + xl1_a * sin phi_i
 *   ray i      arm a holds the radii [lo, hi] of theta = m + r L omega_i:
 *              lo = max(0, max over b with beta_a > beta_b of (alpha_b - alpha_a) / (beta_a - beta_b))
 *              hi = min over b with beta_a < beta_b of (alpha_a - alpha_b) / (beta_b - beta_a), +inf if none
 *              empty if hi <= lo, or if some b has beta_b == beta_a and either alpha_b > alpha_a or
 *              alpha_b == alpha_a with b < a (ties to the lower index, as np.argmax)
 *              mass_a(i) = exp(-(lo * lo) / 2) - exp(-(hi * hi) / 2)
 *   output     u_a = sum_i mass_a(i), post[n][t][a] = u_a / sum_b u_b, (N, H + 1, A) fp64
 * Rows before the first valid pull (m = 0 exactly: the rule would only count grid directions, an O(1 / G)
 * error) are the prior in closed form, computed once per call from the arms alone:
 *   prior_a = angle of {psi : a = argmax_b x_b . (cos psi, sin psi), ties to the lower index} / 6.283185307179586
 *            the set is the intersection over b != a of the open half-circles centred at theta_b =
 *            atan2(x_a1 - x_b1, x_a0 - x_b0) (an identical arm b: empty if b < a, else no constraint); with
 *            delta_b = theta_b - theta_first wrapped into (-pi, pi] its angle is
 *            (pi - max(0, max_b delta_b)) + min(0, min_b delta_b); below 2^-40 it counts as 0; A == 1: 1
 * An arm whose prior is 0 is optimal on a null set only (strictly inside the hull of the arms, a copy of a
 * lower arm, or inside an edge of the hull, where the sign of hi - lo would be rounding noise on every ray): it
 * is dropped -- every row of it is exactly 0 and it bounds no other arm on any ray.  Its pulls still count in
 * the statistics.
 * The reduction order is fixed (a thread's rays in index order, a butterfly per wave, the waves in order, the
 * kept arms in index order): repeated calls are bit-identical and a task's rows do not depend on N or on how
 * the caller chunks the tasks.
 * Known limit: a row whose posterior mean lies within about 1 / G posterior standard deviations of theta = 0
 * has the prior rows' sharp transitions; for t >= 1 that is an event of probability about 1 / G^2.        */
typedef struct dpt_linear_posterior_args {
    int32_t N;                 /* tasks                                                             */
    int32_t H;                 /* recorded pulls per task (>= 0): rows 0 .. H                       */
    int32_t A;                 /* arms, <= 32                                                       */
    int32_t lin_d;             /* 2                                                                 */
    int32_t G;                 /* rays: a multiple of 64 in [64, 65536]                             */
    int32_t flags;             /* 0                                                                 */
    double var;                /* reward std, > 0                                                   */
    const double* arms;        /* (A, 2)                                                            */
    const int32_t* actions;    /* (N, H) (NULL when H = 0)                                          */
    const double* rewards;     /* (N, H)                                                            */
    double* workspace;         /* dpt_linear_posterior_workspace_numel doubles                      */
    double* post;              /* (N, H + 1, A)                                                     */
} dpt_linear_posterior_args;

/* doubles of workspace: the rays' cos | sin tables (2 G), then the prior (32), the kept arms' count (1, then
 * 7 of padding), their indices (32) and the rank of every arm among them (32); the same for every N */
int dpt_linear_posterior_workspace_numel(int32_t N, int32_t A, int32_t lin_d, int32_t G, int64_t* numel_out_host);
/* Two launches (the tables and the prior, then the rows), no host synchronisation, no allocation.  Host
 * checks fail before any launch.  DPT_EINVAL: null args / arms / workspace / post, null actions or rewards
 * while H > 0, N < 1, H < 0, A < 1, lin_d < 1, G < 1, var <= 0, non-zero flags, a workspace that is not
 * 8-byte aligned.  DPT_EUNSUPPORTED: lin_d != 2, A > 32, a G that is not a multiple of 64 in [64, 65536]. */
int dpt_linear_posterior(const dpt_linear_posterior_args* args_host, void* stream);

/* ------------------------------------------------------------------ image-conditioned DPT (ImageTransformer)
 * models/net.py:63-132: per token an image (3, 25, 25) goes through Conv2d(3,16,k3,s2) -> ReLU ->
 * Conv2d(16,16,k3,s1) -> ReLU -> Dropout(p) -> flatten (c, y, x) -> Linear(1600, 8) -> ReLU; the token
 * [enc(8) | state | action | reward] goes through embed_transition and embed_ln (eps 1e-5), and the
 * result enters the GPT-2 trunk as its input embedding.
 *
 * The trunk with the token embedding skipped: dpt_train_forward_embeds / dpt_train_backward_embeds are
 * dpt_train_forward / dpt_train_backward with x0 = drop_site0(embeds + wpe[t]) (embeds (batch, window,
 * n_embd)), every flag and dropout included.  Blob and workspace keep the dpt_train_desc layout; the
 * emb_w / emb_b region is not read and its gradient is written as exact zeros.  The backward writes
 * dembeds (batch, window, n_embd) = dL/dx0 after the site-0 mask, position 0 included. */
int dpt_train_forward_embeds(const dpt_train_desc* desc_host, const float* blob, const float* embeds,
                             float* workspace, float* preds, void* stream);
int dpt_train_backward_embeds(const dpt_train_desc* desc_host, const float* blob, float* workspace,
                              const float* dpreds, float* dblob, float* dembeds, void* stream);

/* The front end.  Front blob (floats, in this order):
 *   conv1_w[16][3][3][3] conv1_b[16] conv2_w[16][16][3][3] conv2_b[16]   (torch's layout)
 *   fc_w[1600][8] fc_b[8] emb_w[8 + sd + A + 1][E] emb_b[E]              (nn.Linear stored [in][out])
 *   embln_g[E] embln_b[E]
 * The encoder's dropout is Philox site DPT_SITE_IMAGE_ENC, element row 1600 + c 100 + y 10 + x, with the
 * keep rule and scale of dpt_train_desc; the backward regenerates the mask from the desc.  Weight and
 * bias gradients are reduced in a fixed order: repeated calls are bit-identical. */
#define DPT_SITE_IMAGE_ENC 1048576 /* 1 << 20: clear of the trunk's sites 1 + 3 l .. 3 + 3 l */
typedef struct dpt_image_desc {
    int32_t image_size;           /* 25: the only size built; anything else is rejected before a launch */
    int32_t rows;                 /* images = batch * window */
    int32_t state_dim, action_dim, n_embd;
    int32_t flags;                /* DPT_TRAIN_FORWARD_ONLY or 0 */
    float dropout;                /* the encoder's nn.Dropout, same p as the trunk */
    int32_t reserved;             /* 0 */
    uint64_t dropout_seed;        /* the same seed as the step's dpt_train_desc */
} dpt_image_desc;
int dpt_image_front_blob_numel(const dpt_image_desc* desc_host, int64_t* numel_out_host);
/* floats; with DPT_TRAIN_FORWARD_ONLY only the token rows, the pre-LayerNorm rows and their statistics */
int dpt_image_front_workspace_numel(const dpt_image_desc* desc_host, int64_t* numel_out_host);
/* images (rows, 3, 25, 25) normalised fp32; feats (rows, sd + A + 1) = [state | action | reward];
 * embeds (rows, E) = embed_ln(embed_transition([enc | feats])).  Keeps in `workspace` what the backward
 * needs (the dropped conv2 activations, the token rows, the pre-LayerNorm rows and statistics). */
int dpt_image_front_forward(const dpt_image_desc* desc_host, const float* front_blob, const float* images,
                            const float* feats, float* workspace, float* embeds, void* stream);
/* dfront_blob (front blob layout) from dembeds (rows, E); pass the forward's desc, images, feats and
 * workspace unchanged.  Host checks fail before any launch: null pointers, rows < 1, image_size != 25
 * (DPT_EUNSUPPORTED), n_embd < 1, state_dim < 0, action_dim < 1, dropout outside [0, 1), reserved != 0,
 * unknown flags, a workspace that is not 16-byte aligned, a backward on a DPT_TRAIN_FORWARD_ONLY desc. */
int dpt_image_front_backward(const dpt_image_desc* desc_host, const float* front_blob, const float* images,
                             const float* feats, float* workspace, const float* dembeds, float* dfront_blob,
                             void* stream);

/* ------------------------------------------------------------------ image training step
 * One step of train.py:286-310 on the miniworld branch (and one batch of its test loss) for the
 * image-conditioned DPT, as a chain of launches on one stream with no host synchronisation, no
 * allocation, no side stream and no graph capture: pack the batch from a device-resident image set,
 * dpt_image_front_forward, dpt_train_forward_embeds, dpt_train_ce_loss, dpt_train_backward_embeds,
 * dpt_image_front_backward, then dpt_adamw_step on the trunk blob and on the front blob. */

/* raw (n_images, 25, 25, 3) HWC in [0, 1] of float64 (dtype 0) or float32 (dtype 1), as the collected
 * .npy stacks and query_image hold it -> out (n_images, 3, 25, 25) fp32 = (x - mean_c) / std_c with the
 * ImageNet statistics of dataset.image_transform.  The subtraction and the IEEE division run in the
 * input's dtype (the constants rounded to float32 first for float32 input) and the result is rounded to
 * fp32 once: bit-equal to image_transform(x).float().  raw and out may sit at any element alignment.
 * Fails before a launch on null pointers, an unknown dtype code or n_images < 0; n_images 0 launches
 * nothing. */
int dpt_image_normalize(const void* raw, int32_t dtype, int64_t n_images, float* out, void* stream);

/* The whole image training set on the device in fp32 (dataset.py `ImageDataset`, images normalised). */
typedef struct dpt_image_data {
    int64_t n;                     /* samples */
    int32_t horizon;               /* context transitions per sample */
    int32_t image_size;            /* 25: the only size built */
    const float* query_states;     /* (n, sd) */
    const float* context_states;   /* (n, horizon, sd) */
    const float* context_actions;  /* (n, horizon, A) */
    const float* context_rewards;  /* (n, horizon) */
    const float* optimal_actions;  /* (n, A) */
    const float* query_images;     /* (n, 3, 25, 25) normalised */
    const float* context_images;   /* (n, horizon, 3, 25, 25) normalised */
} dpt_image_data;

/* images (batch, 1 + horizon, 3, 25, 25), feats (batch, 1 + horizon, sd + A + 1) and targets (batch, A)
 * for the samples index[b] (int64, any order, repeats allowed): row 0 of a sequence is the query (its
 * image query_images[index[b]], its features [query_state | 0_A | 0]), row 1 + j the context transition
 * perm[b][j] (j when perm is NULL) with its image and [state | action | reward]: the images and feats
 * models/net.py:90-123 builds from ImageDataset's items.  Copies only: bit-exact.  An index outside
 * [0, n) or a perm entry outside [0, horizon) reads nothing and packs zeros.  An image is 7500 bytes, so
 * images start at every 4-byte alignment: the copy is correct at each and takes 16-byte accesses only
 * where source and destination allow it.  desc: state_dim, action_dim and window (= 1 + horizon). */
int dpt_image_pack_batch(const dpt_train_desc* desc_host, const dpt_image_data* data_host, const int64_t* index,
                         const int64_t* perm, int32_t batch, float* images, float* feats, float* targets,
                         void* stream);

/* workspace floats of dpt_image_train_step / dpt_image_train_eval_loss for desc.batch sequences: the
 * image and feature batch, targets, embeds, dembeds, preds, dpreds, the front and trunk workspaces,
 * both gradient blobs and the per-sequence losses (every region rounded up to 4 floats) */
int dpt_image_train_step_workspace_numel(const dpt_train_desc* desc_host, int64_t* numel_out_host);
/* One step for the `batch` <= desc.batch samples of index (a smaller last batch reuses the workspace
 * sized for desc.batch).  trunk_blob keeps the dpt_train_desc layout (its emb_w / emb_b region is never
 * read, gets an exactly zero gradient and so stays zero), front_blob the front blob layout; each has its
 * own m and v, all updated in place with the same args (AdamW is element-wise: two launches give the
 * bits one would).  The dpt_image_desc is derived from desc: rows = batch * window, the same dropout and
 * dropout_seed, so the encoder's masks and the trunk's come from one seed.  *loss_acc += the batch's
 * summed loss over positions 1..window-1.  Host checks fail before any launch: null pointers, batch < 1
 * or > desc.batch, desc flags != 0, desc.window != 1 + data->horizon, image_size != 25
 * (DPT_EUNSUPPORTED), action_dim > 32 (DPT_EUNSUPPORTED), step < 1, a workspace or front blob that is
 * not 16-byte aligned, equal trunk and front blobs. */
int dpt_image_train_step(const dpt_train_desc* desc_host, const dpt_image_data* data_host, const int64_t* index,
                         const int64_t* perm, int32_t batch, float* trunk_blob, float* trunk_m, float* trunk_v,
                         float* front_blob, float* front_m, float* front_v, const dpt_adamw_args* args_host,
                         float* workspace, double* loss_acc, void* stream);
/* the test loss: pack -> both forwards with DPT_TRAIN_FORWARD_ONLY (every position) -> cross-entropy
 * without a gradient.  desc.dropout stays active (the reference's test loss runs in training mode).
 * Same workspace and host checks as dpt_image_train_step. */
int dpt_image_train_eval_loss(const dpt_train_desc* desc_host, const dpt_image_data* data_host,
                              const int64_t* index, const int64_t* perm, int32_t batch, const float* trunk_blob,
                              const float* front_blob, float* workspace, double* loss_acc, void* stream);

/* ------------------------------------------------------------------ image act step (deployment)
 * ctrls/ctrl_miniworld.py MiniworldTransformerController.act for B envs: the raw uint8 frame of each env is
 * resized to 25 x 25 and normalised on the device, encoded, embedded and written into position 0 of
 * that env's sequence; the context rows (fixed for an episode) are encoded once per episode.  ABI 8,
 * additive.  The library still owns no memory. */

/* skimage.transform.resize(frame_uint8, (25, 25, 3), anti_aliasing=True) (scikit-image 0.21) restated as a
 * fixed separable linear map: frame / 255 -> ndimage.gaussian_filter(sigma = max(0, (n_in / 25 - 1) / 2)
 * per axis, mode 'mirror', truncate 4) -> ndimage.zoom(order 1, mode 'mirror', grid_mode) -> clip (never
 * acts: every weight is >= 0 and every row sums to 1).  R = Z G (25 x n_in) per axis, kept as banded
 * rows: output o reads inputs first[o] .. first[o] + count[o] - 1 with weights w[o][0 .. count[o] - 1]
 * (the rest of the row is 0: the kernels take eight taps a round and rely on it).  count <= DPT_OBS_BAND for every side in DPT_OBS_MIN_SIDE..DPT_OBS_MAX_SIDE. */
#define DPT_OBS_OUT 25
#define DPT_OBS_BAND 24
#define DPT_OBS_MIN_SIDE 25
#define DPT_OBS_MAX_SIDE 128
typedef struct dpt_obs_tables {
    int32_t in_h, in_w;
    int32_t first_y[DPT_OBS_OUT], count_y[DPT_OBS_OUT];
    int32_t first_x[DPT_OBS_OUT], count_x[DPT_OBS_OUT];
    double wy[DPT_OBS_OUT][DPT_OBS_BAND];
    double wx[DPT_OBS_OUT][DPT_OBS_BAND];
} dpt_obs_tables;
/* Host only, double precision, no device work: fills *tables_out_host for frames of in_h x in_w.  The
 * caller uploads the struct once.  A side outside 25..128 is DPT_EUNSUPPORTED. */
int dpt_image_obs_tables(int32_t in_h, int32_t in_w, dpt_obs_tables* tables_out_host);
/* frames (n, in_h, in_w, 3) uint8 HWC, tables: the struct on the DEVICE -> out (n, 3, 25, 25) fp32 =
 * float32(((R_y (x / 255) R_x^T) - mean_c) / std_c) with dpt_image_normalize's ImageNet statistics;
 * accumulated in fp64 (the column pass, then the row pass, on the integer samples; then one IEEE division
 * by 255, the subtraction and the division by std), rounded once on the store.  At 25 x 25 the tables are the identity and the result is bit-equal to dpt_image_normalize of
 * float64(x) / 255.  One workgroup per frame.  A table the kernel reads is clamped to the frame, so a
 * wrong one gives wrong values, never an access outside the frame.  Fails before a launch on null
 * pointers, n < 0 and sides outside 25..128 (DPT_EUNSUPPORTED); n = 0 launches nothing. */
int dpt_image_obs_preprocess(const uint8_t* frames, int64_t n, int32_t in_h, int32_t in_w,
                             const dpt_obs_tables* tables_device, float* out, void* stream);

typedef struct dpt_image_act_desc {
    int32_t n_layer, n_embd, state_dim, action_dim, n_positions;
    int32_t batch;       /* B envs */
    int32_t max_context; /* the largest C the workspace is sized for */
    int32_t image_size;  /* 25 */
    int32_t in_h, in_w;  /* raw frame sides, 25..128 each */
    float dropout;       /* must be 0: the act step is inference */
    int32_t reserved;    /* 0 */
} dpt_image_act_desc;
/* floats: the front workspace and the embedded rows of batch * max_context context images, then the
 * trunk's forward-only workspace at window 1 + max_context */
int dpt_image_act_workspace_numel(const dpt_image_act_desc* desc_host, int64_t* numel_out_host);
/* Once per episode: the batch * C context rows (images (B, C, 3, 25, 25) normalised, feats (B, C, sd + A
 * + 1) = [state | action | reward]) through dpt_image_front_forward (DPT_TRAIN_FORWARD_ONLY) into rows
 * 1..C of each sequence of embeds (B, 1 + C, E).  C = 0 is valid and launches nothing (images and feats
 * may then be NULL). */
int dpt_image_act_set_context(const dpt_image_act_desc* desc_host, int32_t C, const float* front_blob,
                              const float* images, const float* feats, float* workspace, float* embeds,
                              void* stream);
/* One step, one chain on one stream with no host synchronisation and no allocation.  A fused front
 * kernel, one workgroup per env: frames (B, in_h, in_w, 3) uint8 -> resize and normalise (arithmetic
 * identical to dpt_image_obs_preprocess) -> obs_out (B, 3, 25, 25) -> conv1, conv2 (MFMA implicit GEMM),
 * the 1600 -> 8 product (the device functions of dpt_image_front_forward's encoder: the same arithmetic
 * order) -> embed_transition on [enc | query_states[b] | 0_A | 0] -> embed_ln -> embeds[b][0] (bit-equal
 * to dpt_image_front_forward on (obs_out, feats) with 16-byte aligned embeds).  Then
 * dpt_train_forward_embeds (DPT_TRAIN_FORWARD_ONLY | DPT_TRAIN_LAST_ONLY) at window 1 + C -> logits (B, A).
 * Rows 1..C of embeds (dpt_image_act_set_context) are read, never written; no context image is read.
 * Choose the action with dpt_select_action.  Host checks of the three entry points fail before any
 * launch: null pointers, batch < 1, C < 0, C > max_context, 1 + C > n_positions, frame sides outside
 * 25..128 (DPT_EUNSUPPORTED), image_size != 25 (DPT_EUNSUPPORTED), 8 + sd + A + 1 + n_embd above 6400
 * (DPT_EUNSUPPORTED), dropout != 0, reserved != 0, a workspace, front blob or embeds that is not 16-byte
 * aligned. */
int dpt_image_act_step(const dpt_image_act_desc* desc_host, int32_t C, const float* trunk_blob,
                       const float* front_blob, const uint8_t* frames, const dpt_obs_tables* tables_device,
                       const float* query_states, float* workspace, float* embeds, float* obs_out, float* logits,
                       void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DPT_HIP_H */
