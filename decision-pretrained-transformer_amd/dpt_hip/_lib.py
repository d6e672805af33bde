"""ctypes binding of libdpt_hip.so (include/dpt_hip.h).

The library is built in-tree (``make -C csrc`` / ``__graft_entry__.build()``)
and loaded from this directory.  There is no fallback: a missing or stale
library raises ImportError/OSError at first use, so nothing silently runs on
the CPU.  Return codes are mapped to the reference's Python exceptions
(envs/bandit_env.py:16,63,67-68; envs/darkroom_env.py:39,58-59).
"""
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# DPT_HIP_LIB: another build's file name in this directory (A/B runs of kernel variants)
LIB_PATH = os.path.join(_HERE, os.environ.get("DPT_HIP_LIB", "libdpt_hip.so"))
ABI_VERSION = 8

DPT_OK = 0
DPT_EINVAL = -1
DPT_EEPISODE_ENDED = -2
DPT_EHIP = -3
DPT_ENOMEM = -4
DPT_EUNSUPPORTED = -5

BANDIT_GAUSSIAN = 0
BANDIT_BERNOULLI = 1
BANDIT_F32 = 16
STREAM_SELECT = 0
STREAM_REWARD = 1
STREAM_ROLLIN = 2
STREAM_DROPOUT = 3  # training dropout masks (dpt_train_desc)
STREAM_ENVACT = 4  # the env action drawn apart from the context action (dpt_rollout_bandit_generic_env)
STREAM_TASK = 5  # the task draws of the fresh-task generator (dpt_fresh_batch)
STREAM_POLICY = 16  # + arm index (baseline-policy draws)

_c_void_p = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_u32 = ctypes.c_uint32
_u64 = ctypes.c_uint64
_f32 = ctypes.c_float
_f64 = ctypes.c_double


class ModelDesc(ctypes.Structure):
    _fields_ = [("n_layer", _i32), ("n_embd", _i32), ("state_dim", _i32), ("action_dim", _i32),
                ("n_positions", _i32), ("reserved", _i32 * 3)]


class BanditRolloutArgs(ctypes.Structure):
    _fields_ = [("N", _i32), ("H", _i32), ("A", _i32), ("type", _i32), ("sample", _i32),
                ("reserved0", _i32), ("first_task", _i64), ("var", _f64), ("seed", _u64),
                ("means", _c_void_p), ("uniforms", _c_void_p), ("noise", _c_void_p),
                ("kvcache", _c_void_p), ("actions_out", _c_void_p), ("rewards_out", _c_void_p),
                ("arm_value_out", _c_void_p), ("logits_out", _c_void_p), ("counter", _u64)]


# name -> (restype, argtypes); mirrors include/dpt_hip.h exactly
SIGNATURES = {
    "dpt_abi_version": (_i32, []),
    "dpt_last_error": (ctypes.c_char_p, []),
    "dpt_device_count": (_i32, [ctypes.POINTER(_i32)]),
    "dpt_weights_numel": (_i32, [ctypes.POINTER(ModelDesc), ctypes.POINTER(_i64)]),
    "dpt_model_create": (_i32, [ctypes.POINTER(ModelDesc), _c_void_p, ctypes.POINTER(_c_void_p)]),
    "dpt_model_free": (_i32, [_c_void_p]),
    "dpt_forward_window": (_i32, [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                  _i32, _i32, _i32, _c_void_p, _c_void_p, _c_void_p]),
    "dpt_kvcache_numel": (_i32, [_c_void_p, _i32, _i32, ctypes.POINTER(_i64)]),
    "dpt_decode_step": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p, _c_void_p, _c_void_p]),
    "dpt_select_action": (_i32, [_c_void_p, _i32, _i32, _i32, _f32, _c_void_p, _u64, _u64, _i64,
                                 _c_void_p, _c_void_p]),
    "dpt_bandit_step": (_i32, [_c_void_p, _i32, _i32, _c_void_p, _i32, _f64, _c_void_p, _u64, _u64, _i64,
                               _c_void_p, _c_void_p, _c_void_p]),
    "dpt_darkroom_step": (_i32, [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _c_void_p,
                                 _c_void_p, _c_void_p]),
    "dpt_darkroom_opt_action": (_i32, [_c_void_p, _c_void_p, _c_void_p, _i32, _c_void_p, _c_void_p]),
    "dpt_draw": (_i32, [_i32, _u64, _u64, _i64, _i32, _u32, _c_void_p, _c_void_p]),
    "dpt_rollout_bandit": (_i32, [_c_void_p, ctypes.POINTER(BanditRolloutArgs), _c_void_p]),
    "dpt_rollin_bandit": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _f64, _c_void_p, _c_void_p, _u64,
                                 _i64, _c_void_p, _c_void_p, _c_void_p]),
    "dpt_rollin_darkroom": (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _c_void_p, _c_void_p, _u64, _i64,
                                   _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p]),
}

_lock = threading.Lock()
_lib = None


def load():
    """Load and type the library once; raises if it is missing or the ABI differs."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is not built (run `make -C csrc` or __graft_entry__.build()); "
                              "the DPT hot path has no CPU fallback")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            # (tests/test_abi.py requires every header symbol; an older build loaded for an A/B may
            # lack newer entry points, which then fail when called)
            fn = getattr(lib, name, None)
            if fn is None:
                continue
            fn.restype = res
            fn.argtypes = args
        v = lib.dpt_abi_version()
        if v != ABI_VERSION:
            raise ImportError(f"libdpt_hip ABI {v} != bindings ABI {ABI_VERSION}")
        _lib = lib
        return lib


class EpisodeEndedError(ValueError):
    pass


def check(rc):
    """Map a DPT_E* code to the reference's exception types."""
    if rc == DPT_OK:
        return
    msg = load().dpt_last_error().decode(errors="replace")
    if rc == DPT_EEPISODE_ENDED:
        raise EpisodeEndedError("Episode has already ended")
    if rc == DPT_EINVAL:
        raise ValueError(msg)
    if rc == DPT_EUNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == DPT_ENOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def call(name, *args):
    check(getattr(load(), name)(*args))


POLICY_OPT, POLICY_EMP, POLICY_UCB, POLICY_THOMPSON, POLICY_LCB, POLICY_LINUCB = range(6)


class PolicyRolloutArgs(ctypes.Structure):
    _fields_ = [("N", _i32), ("H", _i32), ("A", _i32), ("policy", _i32), ("online", _i32), ("type", _i32),
                ("sample", _i32), ("lin_d", _i32), ("first_task", _i64), ("var", _f64), ("c", _f64),
                ("ts_std", _f64), ("ts_prior_mean", _f64), ("ts_prior_var", _f64), ("seed", _u64),
                ("means", _c_void_p), ("arms", _c_void_p), ("noise", _c_void_p), ("policy_noise", _c_void_p),
                ("workspace", _c_void_p), ("actions_out", _c_void_p), ("rewards_out", _c_void_p),
                ("arm_value_out", _c_void_p), ("C", _i32), ("step0", _i32), ("ctx_actions", _c_void_p),
                ("ctx_rewards", _c_void_p)]


SIGNATURES.update({
    "dpt_policy_workspace_numel": (_i32, [_i32, _i32, _i32, ctypes.POINTER(_i64)]),
    "dpt_rollout_policy": (_i32, [ctypes.POINTER(PolicyRolloutArgs), _c_void_p]),
})

TUNE_DECODE_TILE = 1
TUNE_PREFILL = 2
TUNE_DARKROOM_MEMO = 3
TUNE_CACHE_BUDGET = 4
TUNE_BLOCK0_MFMA = 5
TUNE_SELECT_FAST = 6
TUNE_POLICY_WAVE = 7
TUNE_YCACHE_BITS = 8
SIGNATURES["dpt_tuning_set"] = (_i32, [_i32, _i64])


class DarkroomRolloutArgs(ctypes.Structure):
    _fields_ = [("N", _i32), ("Heps", _i32), ("horizon", _i32), ("ctx_episodes", _i32), ("dim", _i32),
                ("sample", _i32), ("first_task", _i64), ("seed", _u64), ("counter", _u64), ("temp", _f32),
                ("reserved0", _i32), ("goals", _c_void_p), ("perms", _c_void_p), ("uniforms", _c_void_p),
                ("returns_out", _c_void_p), ("actions_out", _c_void_p), ("logits_out", _c_void_p),
                ("forwards_out", _c_void_p), ("workspace", _c_void_p)]


SIGNATURES["dpt_prefill_max_window"] = (_i32, [_c_void_p, ctypes.POINTER(_i32)])
SIGNATURES["dpt_rollout_darkroom"] = (_i32, [_c_void_p, ctypes.POINTER(DarkroomRolloutArgs), _c_void_p])

REGRET_SUMS = 0
REGRET_CENTRED = 1
SIGNATURES["dpt_regret_max_steps"] = (_i32, [ctypes.POINTER(_i32)])
SIGNATURES["dpt_regret_workspace_numel"] = (_i32, [_i32, _i32, ctypes.POINTER(_i64)])
SIGNATURES["dpt_regret_moments"] = (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p, _c_void_p,
                                           _c_void_p, _c_void_p])
SIGNATURES["dpt_darkroom_workspace_numel"] = (_i32, [_i32, ctypes.POINTER(_i64)])
SIGNATURES["dpt_darkroom_workspace_numel_window"] = (_i32, [_i32, _i32, ctypes.POINTER(_i64)])


class TrainDesc(ctypes.Structure):
    _fields_ = [("n_layer", _i32), ("n_embd", _i32), ("state_dim", _i32), ("action_dim", _i32),
                ("n_positions", _i32), ("batch", _i32), ("window", _i32), ("reserved", _i32),
                ("dropout", ctypes.c_float), ("reserved2", _i32), ("dropout_seed", ctypes.c_uint64)]


TRAIN_FORWARD_ONLY = 1  # dpt_train_desc.reserved flag (DPT_TRAIN_FORWARD_ONLY)
TRAIN_LAST_ONLY = 2  # with it: preds at the last position only (DPT_TRAIN_LAST_ONLY)
TRAIN_LAST_LOSS = 4  # training forward / backward whose loss reads the last position only (DPT_TRAIN_LAST_LOSS)


SIGNATURES["dpt_train_blob_numel"] = (_i32, [ctypes.POINTER(TrainDesc), ctypes.POINTER(_i64)])
SIGNATURES["dpt_train_workspace_numel"] = (_i32, [ctypes.POINTER(TrainDesc), ctypes.POINTER(_i64)])
SIGNATURES["dpt_train_forward"] = (_i32, [ctypes.POINTER(TrainDesc), _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                          _c_void_p])
SIGNATURES["dpt_train_backward"] = (_i32, [ctypes.POINTER(TrainDesc), _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                           _c_void_p, _c_void_p])
SIGNATURES["dpt_rollout_bandit_generic_workspace_numel"] = (_i32, [ctypes.POINTER(TrainDesc), _i32, _i32,
                                                                   ctypes.POINTER(_i64)])
SIGNATURES["dpt_rollout_bandit_generic"] = (_i32, [ctypes.POINTER(TrainDesc), _c_void_p,
                                                   ctypes.POINTER(BanditRolloutArgs), _c_void_p])


class TrainData(ctypes.Structure):
    """dpt_train_data: the fp32 training set on the device (dataset.py's ``Dataset.dataset``)."""
    _fields_ = [("n", _i64), ("horizon", _i32), ("reserved", _i32), ("query_states", _c_void_p),
                ("context_states", _c_void_p), ("context_actions", _c_void_p), ("context_next_states", _c_void_p),
                ("context_rewards", _c_void_p), ("optimal_actions", _c_void_p)]


class AdamWArgs(ctypes.Structure):
    _fields_ = [("lr", _f64), ("beta1", _f64), ("beta2", _f64), ("eps", _f64), ("weight_decay", _f64),
                ("step", _i64)]


_train_desc_p = ctypes.POINTER(TrainDesc)
_train_data_p = ctypes.POINTER(TrainData)
SIGNATURES["dpt_train_pack_batch"] = (_i32, [_train_desc_p, _train_data_p, _c_void_p, _c_void_p, _i32, _c_void_p,
                                             _c_void_p, _c_void_p])
SIGNATURES["dpt_train_ce_loss"] = (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p, _c_void_p, _c_void_p,
                                          _c_void_p])
SIGNATURES["dpt_adamw_step"] = (_i32, [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, ctypes.POINTER(AdamWArgs),
                                       _c_void_p])
SIGNATURES["dpt_train_step_workspace_numel"] = (_i32, [_train_desc_p, ctypes.POINTER(_i64)])
SIGNATURES["dpt_train_step"] = (_i32, [_train_desc_p, _train_data_p, _c_void_p, _c_void_p, _i32, _c_void_p,
                                       _c_void_p, _c_void_p, ctypes.POINTER(AdamWArgs), _c_void_p, _c_void_p,
                                       _c_void_p])
SIGNATURES["dpt_train_eval_loss"] = (_i32, [_train_desc_p, _train_data_p, _c_void_p, _c_void_p, _i32, _c_void_p,
                                            _c_void_p, _c_void_p, _c_void_p])


FRESH_BANDIT = 0  # dpt_fresh_args.env
FRESH_DARKROOM = 1


class FreshArgs(ctypes.Structure):
    """dpt_fresh_args: the fresh-task generator's samples first_task .. first_task + batch - 1."""
    _fields_ = [("env", _i32), ("type", _i32), ("dim", _i32), ("H", _i32), ("n_goals", _i32), ("n_perms", _i32),
                ("var", _f64), ("seed", _u64), ("first_task", _i64), ("goals", _c_void_p), ("perms", _c_void_p),
                ("means_out", _c_void_p), ("probs_out", _c_void_p), ("goal_out", _c_void_p), ("perm_out", _c_void_p),
                ("query_out", _c_void_p), ("opt_action_out", _c_void_p)]


_fresh_args_p = ctypes.POINTER(FreshArgs)
SIGNATURES["dpt_fresh_batch"] = (_i32, [_train_desc_p, _fresh_args_p, _i32, _c_void_p, _c_void_p, _c_void_p])
SIGNATURES["dpt_fresh_step"] = (_i32, [_train_desc_p, _fresh_args_p, _i32, _c_void_p, _c_void_p, _c_void_p,
                                       ctypes.POINTER(AdamWArgs), _c_void_p, _c_void_p, _c_void_p])
SIGNATURES["dpt_fresh_eval_loss"] = (_i32, [_train_desc_p, _fresh_args_p, _i32, _c_void_p, _c_void_p, _c_void_p,
                                            _c_void_p])


FRESH_LINEAR_THOMPSON = 0  # dpt_fresh_linear_args.rollin
FRESH_LINEAR_UNIFORM = 1
FRESH_LINEAR_CHUNK = 32  # kLinChunk of csrc/dpt_fresh_linear.hip: the Thompson rollin's steps per chunk
FRESH_LINEAR_MAX_D = 8   # kMaxD


class FreshLinearArgs(ctypes.Structure):
    """dpt_fresh_linear_args: the linear bandit's fresh-task samples first_task .. first_task + batch - 1."""
    _fields_ = [("rollin", _i32), ("dim", _i32), ("lin_d", _i32), ("H", _i32), ("var", _f64), ("seed", _u64),
                ("first_task", _i64), ("arms", _c_void_p), ("theta_out", _c_void_p), ("means_out", _c_void_p),
                ("probs_out", _c_void_p), ("opt_action_out", _c_void_p)]


_fresh_linear_args_p = ctypes.POINTER(FreshLinearArgs)
SIGNATURES["dpt_fresh_linear_batch"] = (_i32, [_train_desc_p, _fresh_linear_args_p, _i32, _c_void_p, _c_void_p,
                                               _c_void_p])
SIGNATURES["dpt_fresh_linear_step"] = (_i32, [_train_desc_p, _fresh_linear_args_p, _i32, _c_void_p, _c_void_p,
                                              _c_void_p, ctypes.POINTER(AdamWArgs), _c_void_p, _c_void_p, _c_void_p])
SIGNATURES["dpt_fresh_linear_eval_loss"] = (_i32, [_train_desc_p, _fresh_linear_args_p, _i32, _c_void_p, _c_void_p,
                                                   _c_void_p, _c_void_p])


INTERACTIVE_ACCUMULATE = 1  # dpt_interactive_args.flags: dblob += the chunk's gradient
INTERACTIVE_FULL_WIDTH = 2  # the last block at full width (no DPT_TRAIN_LAST_LOSS); for A/B runs


class InteractiveArgs(ctypes.Structure):
    """dpt_interactive_args: one chunk of an interactive (on-policy) bandit training step."""
    _fields_ = [("N", _i32), ("K", _i32), ("type", _i32), ("flags", _i32), ("first_task", _i64),
                ("var", _f64), ("scale", _f64), ("seed", _u64), ("counter", _u64), ("means", _c_void_p),
                ("targets", _c_void_p), ("uniforms", _c_void_p), ("noise", _c_void_p), ("actions_out", _c_void_p),
                ("rewards_out", _c_void_p), ("workspace", _c_void_p), ("dblob", _c_void_p), ("loss_acc", _c_void_p)]


SIGNATURES["dpt_interactive_pack"] = (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p, _c_void_p])
SIGNATURES["dpt_train_ce_last"] = (_i32, [_c_void_p, _c_void_p, _i32, _i32, _i32, _f64, _c_void_p, _c_void_p,
                                          _c_void_p, _c_void_p])
SIGNATURES["dpt_interactive_workspace_numel"] = (_i32, [_train_desc_p, _i32, _i32, ctypes.POINTER(_i64)])
SIGNATURES["dpt_interactive_grad"] = (_i32, [_train_desc_p, _c_void_p, ctypes.POINTER(InteractiveArgs), _c_void_p])


MDP_LOSS_NONE = 0  # dpt_interactive_mdp_args.loss_mode: the rollout alone (evaluation)
MDP_LOSS_LAST = 1  # mean CE of the last step's logits against its expert action (train_interactive.py:134-135)
MDP_LOSS_EVERY = 2  # mean CE over every step's logits against the expert action at the visited state


class InteractiveMDPArgs(ctypes.Structure):
    """dpt_interactive_mdp_args: one chunk of an interactive (on-policy) DarkRoom training step."""
    _fields_ = [("N", _i32), ("K", _i32), ("dim", _i32), ("loss_mode", _i32), ("flags", _i32), ("sample", _i32),
                ("first_task", _i64), ("scale", _f64), ("seed", _u64), ("counter", _u64), ("goal", _c_void_p),
                ("perm", _c_void_p), ("uniforms", _c_void_p), ("states_out", _c_void_p), ("actions_out", _c_void_p),
                ("rewards_out", _c_void_p), ("targets_out", _c_void_p), ("workspace", _c_void_p),
                ("dblob", _c_void_p), ("loss_acc", _c_void_p)]


SIGNATURES["dpt_mdp_pack"] = (_i32, [_c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p, _c_void_p])
SIGNATURES["dpt_darkroom_act_step"] = (_i32, [_c_void_p, _i32, _i32, _i32, _i32, _i32, _i32, _c_void_p, _u64, _u64,
                                              _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                              _c_void_p, _c_void_p])
SIGNATURES["dpt_interactive_mdp_workspace_numel"] = (_i32, [_train_desc_p, _i32, _i32, _i32, ctypes.POINTER(_i64)])
SIGNATURES["dpt_interactive_mdp_grad"] = (_i32, [_train_desc_p, _c_void_p, ctypes.POINTER(InteractiveMDPArgs),
                                                 _c_void_p])


class DarkroomEpisodeArgs(ctypes.Structure):
    """dpt_darkroom_episode_args: the in-episode DarkRoom rollout of N envs over K steps in one launch."""
    _fields_ = [("N", _i32), ("K", _i32), ("dim", _i32), ("sample", _i32), ("first_task", _i64), ("seed", _u64),
                ("counter", _u64), ("goal", _c_void_p), ("perm", _c_void_p), ("uniforms", _c_void_p),
                ("states", _c_void_p), ("actions", _c_void_p), ("rewards", _c_void_p), ("targets", _c_void_p),
                ("logits", _c_void_p), ("returns", _c_void_p)]


SIGNATURES["dpt_rollout_darkroom_episode"] = (_i32, [_c_void_p, ctypes.POINTER(DarkroomEpisodeArgs), _c_void_p])


EXPLORE_ACCUMULATE = 1  # dpt_explore_args.flags: both dblobs += the chunk's gradients


class ExploreArgs(ctypes.Structure):
    """dpt_explore_args: one chunk of an explorer/exploiter bandit training step."""
    _fields_ = [("N", _i32), ("K", _i32), ("type", _i32), ("flags", _i32), ("first_task", _i64),
                ("var", _f64), ("beta", _f64), ("scale_exploiter", _f64), ("scale_explorer", _f64),
                ("seed", _u64), ("counter", _u64), ("means", _c_void_p), ("targets", _c_void_p),
                ("uniforms", _c_void_p), ("noise", _c_void_p), ("env_actions", _c_void_p),
                ("actions_out", _c_void_p), ("env_actions_out", _c_void_p), ("rewards_out", _c_void_p),
                ("workspace", _c_void_p), ("dblob_explorer", _c_void_p), ("dblob_exploiter", _c_void_p),
                ("loss_explorer", _c_void_p), ("loss_exploiter", _c_void_p)]


SIGNATURES["dpt_rollout_bandit_generic_env"] = (_i32, [_train_desc_p, _c_void_p, ctypes.POINTER(BanditRolloutArgs),
                                                       _c_void_p, _i32, _c_void_p, _c_void_p])
SIGNATURES["dpt_train_ce_rows"] = (_i32, [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32, _f64,
                                          _c_void_p, _c_void_p, _c_void_p, _c_void_p])
SIGNATURES["dpt_explore_weights"] = (_i32, [_c_void_p, _i32, _i32, _f64, _c_void_p, _c_void_p])
SIGNATURES["dpt_explore_workspace_numel"] = (_i32, [_train_desc_p, _i32, _i32, ctypes.POINTER(_i64)])
SIGNATURES["dpt_explore_grad"] = (_i32, [_train_desc_p, _c_void_p, _c_void_p, ctypes.POINTER(ExploreArgs), _c_void_p])


class ExploitEvalArgs(ctypes.Structure):
    """dpt_exploit_eval_args: one chunk of the explore-then-exploit evaluation."""
    _fields_ = [("N", _i32), ("H", _i32), ("flags", _i32), ("reserved", _i32), ("actions", _c_void_p),
                ("rewards", _c_void_p), ("means", _c_void_p), ("targets", _c_void_p), ("workspace", _c_void_p),
                ("logits_out", _c_void_p), ("greedy_arm", _c_void_p), ("greedy_value", _c_void_p),
                ("expected_value", _c_void_p), ("p_opt", _c_void_p)]


SIGNATURES["dpt_recommend_curve"] = (_i32, [_c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p, _c_void_p,
                                            _c_void_p, _c_void_p, _c_void_p])
SIGNATURES["dpt_empirical_recommend"] = (_i32, [_c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32, _c_void_p,
                                                _c_void_p, _c_void_p])
SIGNATURES["dpt_exploit_eval_workspace_numel"] = (_i32, [_train_desc_p, _i32, _i32, ctypes.POINTER(_i64)])
SIGNATURES["dpt_exploit_eval"] = (_i32, [_train_desc_p, _c_void_p, ctypes.POINTER(ExploitEvalArgs), _c_void_p])


POSTERIOR_MIN_GRID, POSTERIOR_MAX_GRID = 64, 8192  # dpt_bandit_posterior_args.G: a multiple of 64 in this range


class BanditPosteriorArgs(ctypes.Structure):
    """dpt_bandit_posterior_args: the grid posterior of the optimal arm on every prefix of N records."""
    _fields_ = [("N", _i32), ("H", _i32), ("A", _i32), ("type", _i32), ("G", _i32), ("flags", _i32), ("var", _f64),
                ("actions", _c_void_p), ("rewards", _c_void_p), ("workspace", _c_void_p), ("post", _c_void_p)]


class DarkroomPosteriorArgs(ctypes.Structure):
    """dpt_darkroom_posterior_args: the posterior of the expert action on every prefix of N DarkRoom samples."""
    _fields_ = [("N", _i32), ("H", _i32), ("dim", _i32), ("n_goals", _i32), ("flags", _i32), ("reserved", _i32),
                ("goals", _c_void_p), ("query", _c_void_p), ("next_states", _c_void_p), ("rewards", _c_void_p),
                ("post", _c_void_p), ("consistent", _c_void_p)]


class PosteriorCompareArgs(ctypes.Structure):
    """dpt_posterior_compare_args: a posterior against a model's logits, row by row."""
    _fields_ = [("N", _i32), ("T", _i32), ("A", _i32), ("flags", _i32), ("post", _c_void_p), ("logits", _c_void_p),
                ("targets", _c_void_p), ("nll_model", _c_void_p), ("nll_bayes", _c_void_p), ("kl", _c_void_p),
                ("entropy", _c_void_p)]


SIGNATURES["dpt_bandit_posterior_workspace_numel"] = (_i32, [_i32, _i32, _i32, ctypes.POINTER(_i64)])
SIGNATURES["dpt_bandit_posterior"] = (_i32, [ctypes.POINTER(BanditPosteriorArgs), _c_void_p])
SIGNATURES["dpt_darkroom_posterior"] = (_i32, [ctypes.POINTER(DarkroomPosteriorArgs), _c_void_p])
SIGNATURES["dpt_posterior_compare"] = (_i32, [ctypes.POINTER(PosteriorCompareArgs), _c_void_p])


LINEAR_POSTERIOR_MIN_GRID, LINEAR_POSTERIOR_MAX_GRID = 64, 65536  # dpt_linear_posterior_args.G: a multiple of 64


class LinearPosteriorArgs(ctypes.Structure):
    """dpt_linear_posterior_args: the posterior of the optimal arm of the lin_d = 2 linear bandit on every prefix."""
    _fields_ = [("N", _i32), ("H", _i32), ("A", _i32), ("lin_d", _i32), ("G", _i32), ("flags", _i32), ("var", _f64),
                ("arms", _c_void_p), ("actions", _c_void_p), ("rewards", _c_void_p), ("workspace", _c_void_p),
                ("post", _c_void_p)]


SIGNATURES["dpt_linear_posterior_workspace_numel"] = (_i32, [_i32, _i32, _i32, _i32, ctypes.POINTER(_i64)])
SIGNATURES["dpt_linear_posterior"] = (_i32, [ctypes.POINTER(LinearPosteriorArgs), _c_void_p])


SITE_IMAGE_ENC = 1 << 20  # Philox site of the image encoder's dropout (DPT_SITE_IMAGE_ENC)


class ImageDesc(ctypes.Structure):
    """dpt_image_desc: the image front end of ImageTransformer (encoder, embed_transition, embed_ln)."""
    _fields_ = [("image_size", _i32), ("rows", _i32), ("state_dim", _i32), ("action_dim", _i32), ("n_embd", _i32),
                ("flags", _i32), ("dropout", ctypes.c_float), ("reserved", _i32), ("dropout_seed", ctypes.c_uint64)]


_image_desc_p = ctypes.POINTER(ImageDesc)
SIGNATURES["dpt_image_front_blob_numel"] = (_i32, [_image_desc_p, ctypes.POINTER(_i64)])
SIGNATURES["dpt_image_front_workspace_numel"] = (_i32, [_image_desc_p, ctypes.POINTER(_i64)])
SIGNATURES["dpt_image_front_forward"] = (_i32, [_image_desc_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                                _c_void_p])
SIGNATURES["dpt_image_front_backward"] = (_i32, [_image_desc_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                                 _c_void_p, _c_void_p])
SIGNATURES["dpt_train_forward_embeds"] = (_i32, [_train_desc_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p])
SIGNATURES["dpt_train_backward_embeds"] = (_i32, [_train_desc_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                                  _c_void_p, _c_void_p])


IMAGE_RAW_DTYPES = {"float64": 0, "float32": 1}  # dpt_image_normalize's dtype codes


class ImageData(ctypes.Structure):
    """dpt_image_data: the fp32 image training set on the device (dataset.py's ``ImageDataset``)."""
    _fields_ = [("n", _i64), ("horizon", _i32), ("image_size", _i32), ("query_states", _c_void_p),
                ("context_states", _c_void_p), ("context_actions", _c_void_p), ("context_rewards", _c_void_p),
                ("optimal_actions", _c_void_p), ("query_images", _c_void_p), ("context_images", _c_void_p)]


_image_data_p = ctypes.POINTER(ImageData)
SIGNATURES["dpt_image_normalize"] = (_i32, [_c_void_p, _i32, _i64, _c_void_p, _c_void_p])
SIGNATURES["dpt_image_pack_batch"] = (_i32, [_train_desc_p, _image_data_p, _c_void_p, _c_void_p, _i32, _c_void_p,
                                             _c_void_p, _c_void_p, _c_void_p])
SIGNATURES["dpt_image_train_step_workspace_numel"] = (_i32, [_train_desc_p, ctypes.POINTER(_i64)])
SIGNATURES["dpt_image_train_step"] = (_i32, [_train_desc_p, _image_data_p, _c_void_p, _c_void_p, _i32, _c_void_p,
                                             _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                             ctypes.POINTER(AdamWArgs), _c_void_p, _c_void_p, _c_void_p])
SIGNATURES["dpt_image_train_eval_loss"] = (_i32, [_train_desc_p, _image_data_p, _c_void_p, _c_void_p, _i32, _c_void_p,
                                                  _c_void_p, _c_void_p, _c_void_p, _c_void_p])


OBS_OUT = 25  # the resize's output side (DPT_OBS_OUT)
OBS_BAND = 24  # weights kept per banded table row (DPT_OBS_BAND)
OBS_MIN_SIDE, OBS_MAX_SIDE = 25, 128  # raw frame sides the resize is built for


class ObsTables(ctypes.Structure):
    """dpt_obs_tables: the anti-aliased resize to 25 x 25 as two banded tables (filled on the host,
    uploaded once)."""
    _fields_ = [("in_h", _i32), ("in_w", _i32), ("first_y", _i32 * OBS_OUT), ("count_y", _i32 * OBS_OUT),
                ("first_x", _i32 * OBS_OUT), ("count_x", _i32 * OBS_OUT), ("wy", (_f64 * OBS_BAND) * OBS_OUT),
                ("wx", (_f64 * OBS_BAND) * OBS_OUT)]


class ImageActDesc(ctypes.Structure):
    """dpt_image_act_desc: the act step of the image-conditioned DPT for ``batch`` envs."""
    _fields_ = [("n_layer", _i32), ("n_embd", _i32), ("state_dim", _i32), ("action_dim", _i32),
                ("n_positions", _i32), ("batch", _i32), ("max_context", _i32), ("image_size", _i32),
                ("in_h", _i32), ("in_w", _i32), ("dropout", ctypes.c_float), ("reserved", _i32)]


_act_desc_p = ctypes.POINTER(ImageActDesc)
SIGNATURES["dpt_image_obs_tables"] = (_i32, [_i32, _i32, ctypes.POINTER(ObsTables)])
SIGNATURES["dpt_image_obs_preprocess"] = (_i32, [_c_void_p, _i64, _i32, _i32, _c_void_p, _c_void_p, _c_void_p])
SIGNATURES["dpt_image_act_workspace_numel"] = (_i32, [_act_desc_p, ctypes.POINTER(_i64)])
SIGNATURES["dpt_image_act_set_context"] = (_i32, [_act_desc_p, _i32, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                                  _c_void_p, _c_void_p])
SIGNATURES["dpt_image_act_step"] = (_i32, [_act_desc_p, _i32, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p,
                                           _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p])
