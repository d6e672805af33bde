"""Device runtime of the MI355X DPT hot path: torch tensors in, libdpt_hip.so kernels out.

PyTorch-ROCm is plumbing here (device memory, the current HIP stream); every
computation below is a hand-written gfx950 kernel behind the C ABI in
include/dpt_hip.h.  There is deliberately no CPU implementation: calling any
of these without a GPU raises.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import (BANDIT_BERNOULLI, BANDIT_F32, BANDIT_GAUSSIAN, STREAM_REWARD, STREAM_ROLLIN,  # noqa: F401
                   STREAM_SELECT, EpisodeEndedError)

E = 32


def device():
    """The device the hot path runs on (``cuda`` == HIP on ROCm)."""
    if not torch.cuda.is_available():
        raise RuntimeError("the DPT HIP path needs a ROCm GPU (torch.cuda.is_available() is False)")
    _lib.load()
    return torch.device("cuda", torch.cuda.current_device())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(x, dtype, dev=None):
    dev = dev or device()
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device=dev)


def next_seed():
    """64-bit Philox key drawn from numpy's global RNG (so ``np.random.seed`` governs
    the run, as it does in the reference: eval.py:64-71, collect_data.py:352)."""
    return int(np.random.randint(0, 2 ** 62, dtype=np.int64))


# ----------------------------------------------------------------------------- weights

def layer_param_names(i):
    p = f"transformer.h.{i}."
    return [p + n for n in ("ln_1.weight", "ln_1.bias", "attn.c_attn.weight", "attn.c_attn.bias",
                            "attn.c_proj.weight", "attn.c_proj.bias", "ln_2.weight", "ln_2.bias",
                            "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")]


def pack_weights(sd, n_layer):
    """Flatten a reference ``Transformer.state_dict()`` into the dpt_hip.h blob order.

    nn.Linear weights (embed_transition, pred_actions) are stored [out][in] by
    torch and transposed here; GPT-2 Conv1D weights are already [in][out].
    """
    def t(k):
        v = sd[k]
        return v.detach().to("cpu", torch.float32) if isinstance(v, torch.Tensor) else torch.as_tensor(v, dtype=torch.float32)

    parts = [t("embed_transition.weight").t(), t("embed_transition.bias"), t("transformer.wpe.weight")]
    for i in range(n_layer):
        parts += [t(k) for k in layer_param_names(i)]
    parts += [t("transformer.ln_f.weight"), t("transformer.ln_f.bias"),
              t("pred_actions.weight").t(), t("pred_actions.bias")]
    return torch.cat([p.contiguous().reshape(-1) for p in parts])


# the image front end's parameters in front-blob order (dpt_hip.h dpt_image_desc); the two nn.Linear
# weights are stored [in][out] in the blob
FRONT_KEYS = ("image_encoder.0.weight", "image_encoder.0.bias", "image_encoder.2.weight", "image_encoder.2.bias",
              "image_encoder.6.weight", "image_encoder.6.bias", "embed_transition.weight", "embed_transition.bias",
              "embed_ln.weight", "embed_ln.bias")
_FRONT_LINEAR = ("image_encoder.6.weight", "embed_transition.weight")


def pack_front(sd):
    """Flatten the front-end entries of an ``ImageTransformer.state_dict()`` (or any mapping with
    those keys) into the front blob, on the device of its tensors."""
    def t(k):
        v = sd[k]
        v = v.detach() if isinstance(v, torch.Tensor) else torch.as_tensor(v)
        v = v.to(torch.float32)
        return v.t() if k in _FRONT_LINEAR else v

    return torch.cat([t(k).contiguous().reshape(-1) for k in FRONT_KEYS])


def unpack_front(blob, state_dim, action_dim, n_embd):
    """The inverse of ``pack_front``: {key: tensor shaped like the module's parameter} (views of
    ``blob``; the two nn.Linear weights come back transposed to torch's [out][in])."""
    F = 8 + state_dim + action_dim + 1
    shapes = {"image_encoder.0.weight": (16, 3, 3, 3), "image_encoder.0.bias": (16,),
              "image_encoder.2.weight": (16, 16, 3, 3), "image_encoder.2.bias": (16,),
              "image_encoder.6.weight": (8, 1600), "image_encoder.6.bias": (8,),
              "embed_transition.weight": (n_embd, F), "embed_transition.bias": (n_embd,),
              "embed_ln.weight": (n_embd,), "embed_ln.bias": (n_embd,)}
    out, off = {}, 0
    for k in FRONT_KEYS:
        sh = shapes[k]
        n = int(np.prod(sh))
        flat = blob[off:off + n]
        out[k] = flat.view(sh[1], sh[0]).t() if k in _FRONT_LINEAR else flat.view(sh)
        off += n
    if off != blob.numel():
        raise ValueError(f"front blob {blob.numel()} != parameters {off}")
    return out


class DeviceModel:
    """Owns one ``dpt_model`` handle (the packed fp32 weights on the GPU)."""

    def __init__(self, state_dict, n_layer, state_dim, action_dim, n_positions, n_embd=E):
        self.desc = _lib.ModelDesc(n_layer, n_embd, state_dim, action_dim, n_positions)
        numel = ctypes.c_int64()
        _lib.call("dpt_weights_numel", ctypes.byref(self.desc), ctypes.byref(numel))
        blob = pack_weights(state_dict, n_layer)
        if blob.numel() != numel.value:
            raise ValueError(f"packed weights {blob.numel()} != expected {numel.value}")
        dev = device()
        blob_d = blob.to(dev)
        h = ctypes.c_void_p()
        _lib.call("dpt_model_create", ctypes.byref(self.desc), _p(blob_d), ctypes.byref(h))
        torch.cuda.current_stream().synchronize()
        self._h = h
        self.n_layer, self.state_dim, self.action_dim = n_layer, state_dim, action_dim
        self.n_positions = n_positions
        self.F = 2 * state_dim + action_dim + 1

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.load().dpt_model_free(h)
            except Exception:
                pass
            self._h = None

    @property
    def handle(self):
        return self._h

    def kv_numel(self, N, max_pos):
        n = ctypes.c_int64()
        _lib.call("dpt_kvcache_numel", self._h, int(N), int(max_pos), ctypes.byref(n))
        return n.value

    def forward_window(self, query, cs=None, ca=None, cn=None, cr=None, out_mode=0):
        """Transformer.forward (models/net.py:41-60) on device. Returns (N,A) or (N,C,A)."""
        dev = device()
        q = _dev(query, torch.float32, dev)
        N = q.shape[0]
        C = 0 if cs is None else int(cs.shape[1])
        if C:
            cs_, ca_, cn_ = (_dev(x, torch.float32, dev) for x in (cs, ca, cn))
            cr_ = _dev(cr, torch.float32, dev).reshape(N, C)
        else:
            cs_ = ca_ = cn_ = cr_ = None
        out = torch.empty((N, self.action_dim) if out_mode == 0 else (N, C, self.action_dim),
                          dtype=torch.float32, device=dev)
        if N == 0 or (out_mode == 1 and C == 0):  # empty batch / no context rows: nothing to run
            return out
        ws = (None if C + 1 <= self.prefill_max_window()
              else torch.empty(self.kv_numel(N, C + 1), dtype=torch.float32, device=dev))
        _lib.call("dpt_forward_window", self._h, _p(q), _p(cs_), _p(ca_), _p(cn_), _p(cr_), N, C,
                  int(out_mode), _p(out), _p(ws), _stream())
        return out

    def prefill_max_window(self):
        """Longest window dpt_forward_window runs as one MFMA prefill (0 when switched off)."""
        n = ctypes.c_int32()
        _lib.call("dpt_prefill_max_window", self._h, ctypes.byref(n))
        return n.value

    def decode_step(self, kv, max_pos, pos, token):
        token = _dev(token, torch.float32)
        N = token.shape[0]
        logits = torch.empty((N, self.action_dim), dtype=torch.float32, device=token.device)
        _lib.call("dpt_decode_step", self._h, _p(kv), N, int(max_pos), int(pos), _p(token), _p(logits),
                  _stream())
        return logits

    def rollout_bandit(self, means, H, var, sample=True, bandit_type=BANDIT_GAUSSIAN, seed=0,
                       first_task=0, uniforms=None, noise=None, want_logits=False, counter=0, kvcache=None):
        """Fused online bandit rollout (evals/eval_bandit.py:56-103) on device.

        Step h draws at Philox counter ``counter + h`` (global task id first_task + i),
        the counters the per-step path's selects would consume from ``counter`` on.
        ``kvcache``, optional: the caller's fp32 device workspace (at least ``kv_numel(N, H)``
        elements, e.g. a view into a larger allocation); by default one is allocated.

        Returns dict of device tensors: actions (N,H) int32, rewards (N,H) f64,
        arm_value (N,H) f64 (= cum_means.T), logits (H,N,A) f32 if requested.
        """
        dev = device()
        means_d = _dev(means, torch.float64, dev)
        N, A = means_d.shape
        H = int(H)
        out = dict(actions=torch.empty((N, H), dtype=torch.int32, device=dev),
                   rewards=torch.empty((N, H), dtype=torch.float64, device=dev),
                   arm_value=torch.empty((N, H), dtype=torch.float64, device=dev))
        out["logits"] = (torch.empty((H, N, A), dtype=torch.float32, device=dev) if want_logits else None)
        if N == 0 or H == 0:  # no tasks or no steps: empty curves, nothing to run
            return out
        if kvcache is None:
            kv = torch.empty(self.kv_numel(N, H), dtype=torch.float32, device=dev)
        else:
            kv = kvcache
            if not (kv.is_cuda and kv.dtype == torch.float32 and kv.is_contiguous()
                    and kv.numel() >= self.kv_numel(N, H)):
                raise ValueError(f"kvcache must be a contiguous fp32 device tensor of >= {self.kv_numel(N, H)} elements")
        u_d = None if uniforms is None else _dev(uniforms, torch.float64, dev)
        g_d = None if noise is None else _dev(noise, torch.float64, dev)
        args = _lib.BanditRolloutArgs(
            N, H, A, int(bandit_type), int(bool(sample)), 0, int(first_task), float(var), int(seed) & (2 ** 64 - 1),
            _p(means_d).value, None if u_d is None else _p(u_d).value, None if g_d is None else _p(g_d).value,
            _p(kv).value, _p(out["actions"]).value, _p(out["rewards"]).value, _p(out["arm_value"]).value,
            None if out["logits"] is None else _p(out["logits"]).value, int(counter) & (2 ** 64 - 1))
        _lib.call("dpt_rollout_bandit", self._h, ctypes.byref(args), _stream())
        out["_keep"] = (kv, means_d, u_d, g_d)
        return out

    def rollout_darkroom(self, goals, Heps, horizon, ctx_episodes, dim=10, perms=None, sample=True, temp=1.0,
                         seed=0, counter=0, first_task=0, uniforms=None, want_actions=False, want_logits=False,
                         want_forwards=False):
        """Fused DarkRoom online evaluation (evals/eval_darkroom.py:20-84) on device.

        Returns dict of device tensors: returns (N, Heps) int32, actions (N, Heps*horizon)
        int32, logits (Heps*horizon, N, 5) f32 and forwards (N, Heps) int32 (window
        forwards run per task and episode: one per distinct state per episode under
        set_darkroom_memo) if requested.  Raises
        NotImplementedError outside sd=2 / A=5 / window <= darkroom_max_window() (use the
        per-step path).
        """
        dev = device()
        goals_d = _dev(goals, torch.int32, dev).contiguous()
        N = goals_d.shape[0]
        steps = int(Heps) * int(horizon)
        perms_d = None if perms is None else _dev(perms, torch.int32, dev).contiguous()
        u_d = None if uniforms is None else _dev(uniforms, torch.float64, dev).contiguous()
        out = dict(returns=torch.empty((N, int(Heps)), dtype=torch.int32, device=dev))
        out["actions"] = torch.empty((N, steps), dtype=torch.int32, device=dev) if want_actions else None
        out["logits"] = torch.empty((steps, N, 5), dtype=torch.float32, device=dev) if want_logits else None
        out["forwards"] = torch.empty((N, int(Heps)), dtype=torch.int32, device=dev) if want_forwards else None
        if N == 0 or steps == 0:  # no tasks or no steps: empty returns, nothing to run
            for k in ("returns", "forwards"):
                if out[k] is not None:
                    out[k].zero_()
            return out
        n_ws = ctypes.c_int64()
        _lib.call("dpt_darkroom_workspace_numel_window", N, 1 + int(ctx_episodes) * int(horizon), ctypes.byref(n_ws))
        ws = torch.empty(n_ws.value, dtype=torch.float32, device=dev) if _darkroom_ws else None
        args = _lib.DarkroomRolloutArgs(
            N, int(Heps), int(horizon), int(ctx_episodes), int(dim), int(bool(sample)), int(first_task),
            int(seed) & (2 ** 64 - 1), int(counter), float(temp), 0, _p(goals_d).value,
            None if perms_d is None else _p(perms_d).value, None if u_d is None else _p(u_d).value,
            _p(out["returns"]).value, None if out["actions"] is None else _p(out["actions"]).value,
            None if out["logits"] is None else _p(out["logits"]).value,
            None if out["forwards"] is None else _p(out["forwards"]).value,
            None if ws is None else _p(ws).value)
        _lib.call("dpt_rollout_darkroom", self._h, ctypes.byref(args), _stream())
        out["_keep"] = (goals_d, perms_d, u_d, ws)
        return out


# ----------------------------------------------------------------------------- element-wise ops

def select_action(logits, sample, temp=1.0, uniforms=None, seed=0, counter=0, first_task=0):
    logits = _dev(logits, torch.float32)
    N, A = logits.shape
    u = None if uniforms is None else _dev(uniforms, torch.float64, logits.device)
    out = torch.empty(N, dtype=torch.int32, device=logits.device)
    _lib.call("dpt_select_action", _p(logits), N, A, int(bool(sample)), float(temp), _p(u), int(seed),
              int(counter), int(first_task), _p(out), _stream())
    return out


def bandit_step(means, action, var, bandit_type=BANDIT_GAUSSIAN, noise=None, seed=0, counter=0,
                first_task=0):
    means = _dev(means, torch.float64)
    N, A = means.shape
    a = _dev(action, torch.int32, means.device)
    g = None if noise is None else _dev(noise, torch.float64, means.device)
    r = torch.empty(N, dtype=torch.float64, device=means.device)
    v = torch.empty(N, dtype=torch.float64, device=means.device)
    _lib.call("dpt_bandit_step", _p(means), N, A, _p(a), int(bandit_type), float(var), _p(g), int(seed),
              int(counter), int(first_task), _p(r), _p(v), _stream())
    return r, v


def darkroom_step(state, action, goal, perm=None, dim=10):
    s = _dev(state, torch.int32)
    N = s.shape[0]
    a = _dev(action, torch.int32, s.device)
    g = _dev(goal, torch.int32, s.device)
    pm = None if perm is None else _dev(perm, torch.int32, s.device)
    ns = torch.empty_like(s)
    r = torch.empty(N, dtype=torch.int32, device=s.device)
    _lib.call("dpt_darkroom_step", _p(s), _p(a), _p(g), _p(pm), N, int(dim), _p(ns), _p(r), _stream())
    return ns, r


def darkroom_opt_action(state, goal, perm=None):
    s = _dev(state, torch.int32)
    g = _dev(goal, torch.int32, s.device)
    pm = None if perm is None else _dev(perm, torch.int32, s.device)
    out = torch.empty(s.shape[0], dtype=torch.int32, device=s.device)
    _lib.call("dpt_darkroom_opt_action", _p(s), _p(g), _p(pm), s.shape[0], _p(out), _stream())
    return out


def draw(kind, seed, counter, first_task, N, stream_id):
    """The Philox draws the kernels use (kind 0 uniform, 1 normal) -> (N,) float64 device tensor."""
    out = torch.empty(int(N), dtype=torch.float64, device=device())
    _lib.call("dpt_draw", int(kind), int(seed), int(counter), int(first_task), int(N), int(stream_id),
              _p(out), _stream())
    return out


# ----------------------------------------------------------------------------- data generation

def rollin_bandit(means, probs, H, var, bandit_type=BANDIT_GAUSSIAN, uniforms=None, noise=None, seed=0,
                  first_task=0):
    """collect_data.py:23-53 for all tasks at once -> (actions (N,H) int32, rewards (N,H) f64) on device."""
    means = _dev(means, torch.float64)
    N, A = means.shape
    probs = _dev(probs, torch.float64, means.device)
    u = None if uniforms is None else _dev(uniforms, torch.float64, means.device)
    g = None if noise is None else _dev(noise, torch.float64, means.device)
    acts = torch.empty((N, int(H)), dtype=torch.int32, device=means.device)
    rews = torch.empty((N, int(H)), dtype=torch.float64, device=means.device)
    _lib.call("dpt_rollin_bandit", _p(means), _p(probs), N, A, int(H), int(bandit_type), float(var), _p(u), _p(g),
              int(seed), int(first_task), _p(acts), _p(rews), _stream())
    return acts, rews


def rollin_darkroom(goals, H, dim=10, perm=None, mode=0, states=None, actions=None, seed=0, first_task=0):
    """collect_data.py:83-111 (+ query / expert label, :199-201) for all tasks at once (device tensors)."""
    goals = _dev(goals, torch.int32)
    N = goals.shape[0]
    dev = goals.device
    pm = None if perm is None else _dev(perm, torch.int32, dev)
    si = None if states is None else _dev(states, torch.int32, dev)
    ai = None if actions is None else _dev(actions, torch.int32, dev)
    out = dict(states=torch.empty((N, int(H), 2), dtype=torch.int32, device=dev),
               actions=torch.empty((N, int(H)), dtype=torch.int32, device=dev),
               next_states=torch.empty((N, int(H), 2), dtype=torch.int32, device=dev),
               rewards=torch.empty((N, int(H)), dtype=torch.int32, device=dev),
               query=torch.empty((N, 2), dtype=torch.int32, device=dev),
               opt_action=torch.empty(N, dtype=torch.int32, device=dev))
    _lib.call("dpt_rollin_darkroom", _p(goals), _p(pm), N, int(H), int(dim), int(mode), _p(si), _p(ai), int(seed),
              int(first_task), _p(out["states"]), _p(out["actions"]), _p(out["next_states"]), _p(out["rewards"]),
              _p(out["query"]), _p(out["opt_action"]), _stream())
    return out


# ----------------------------------------------------------------------------- fresh-task generator

class FreshEnv:
    """What the fresh-task generators (dpt_fresh_batch, dpt_fresh_linear_batch) draw their samples from:
    ``FreshEnv.bandit(A, H, var, "uniform" | "bernoulli")``, ``FreshEnv.darkroom(dim, H, goals, perms=None)``
    with ``goals`` (G, 2) the list the task's goal is drawn from (a held-out split: the train list or the test
    list) and ``perms`` (P, 5) an optional list of action permutations, or ``FreshEnv.linear_bandit(arms, H,
    var, "thompson" | "uniform")`` with ``arms`` (A, d) the arm features.  The lists are int32 and the arms
    float64 device tensors, kept here.  ``kind`` is FRESH_BANDIT, FRESH_DARKROOM or ``FreshEnv.LINEAR``, which
    has entry points and an args struct of its own (``calls``, ``args``)."""
    LINEAR = 2  # not a dpt_fresh_args.env: the linear bandit's generator is dpt_fresh_linear_batch

    def __init__(self, kind, dim, H, var=0.0, bandit_type=BANDIT_GAUSSIAN, goals=None, perms=None, arms=None,
                 rollin=_lib.FRESH_LINEAR_THOMPSON):
        self.kind, self.dim, self.H, self.var, self.type = int(kind), int(dim), int(H), float(var), int(bandit_type)
        self.goals = self.perms = self.arms = None
        self.rollin = int(rollin)
        if kind == _lib.FRESH_DARKROOM:
            self.goals = _dev(goals, torch.int32).reshape(-1, 2)
            self.perms = None if perms is None else _dev(perms, torch.int32, self.goals.device).reshape(-1, 5)
        if kind == self.LINEAR:
            self.arms = _dev(arms, torch.float64)
            if self.arms.dim() != 2 or self.arms.shape[0] != self.dim:
                raise ValueError(f"arms {tuple(self.arms.shape)}: expected (A, d)")
            self.lin_d = int(self.arms.shape[1])
        self.state_dim, self.action_dim = (2, 5) if kind == _lib.FRESH_DARKROOM else (1, self.dim)
        stem = "dpt_fresh_linear_" if kind == self.LINEAR else "dpt_fresh_"
        self.calls = {k: stem + k for k in ("batch", "step", "eval_loss")}  # the C entry point of each use

    @classmethod
    def bandit(cls, A, H, var, bandit_type="uniform"):
        code = {"uniform": BANDIT_GAUSSIAN, "bernoulli": BANDIT_BERNOULLI}.get(bandit_type, bandit_type)
        return cls(_lib.FRESH_BANDIT, A, H, var, code)

    @classmethod
    def darkroom(cls, dim, H, goals, perms=None):
        return cls(_lib.FRESH_DARKROOM, dim, H, goals=goals, perms=perms)

    @classmethod
    def linear_bandit(cls, arms, H, var, rollin="thompson"):
        """``arms`` (A, d): collect_data.py's are ``RandomState(1234).normal(size=(A, d)) / sqrt(d)``.  ``rollin``:
        "thompson", the adaptive run of rollin_linear_bandit_vec (posterior prior 0 / 1, std ``var`` > 0), or
        "uniform", the bandit's i.i.d. behaviour policy (collect_data.py's data_type 'uniform')."""
        codes = {"thompson": _lib.FRESH_LINEAR_THOMPSON, "uniform": _lib.FRESH_LINEAR_UNIFORM}
        if rollin not in codes:
            raise ValueError(f"rollin {rollin!r}: 'thompson' or 'uniform'")
        arms = arms if isinstance(arms, torch.Tensor) else np.asarray(arms, np.float64)
        return cls(cls.LINEAR, arms.shape[0], H, var, arms=arms, rollin=codes[rollin])

    def args(self, seed, first_task, outs=None):
        """dpt_fresh_args (the linear bandit: dpt_fresh_linear_args) for the samples from ``first_task`` on;
        ``outs``: the optional outputs by name."""
        o = outs or {}
        ptr = lambda *ts: (None if t is None else t.data_ptr() for t in ts)  # noqa: E731
        if self.kind == self.LINEAR:
            return _lib.FreshLinearArgs(self.rollin, self.dim, self.lin_d, self.H, self.var,
                                        int(seed) & (2 ** 64 - 1), int(first_task),
                                        *ptr(self.arms, o.get("theta"), o.get("means"), o.get("probs"),
                                             o.get("opt_action")))
        return _lib.FreshArgs(
            self.kind, self.type, self.dim, self.H, 0 if self.goals is None else int(self.goals.shape[0]),
            0 if self.perms is None else int(self.perms.shape[0]), self.var, int(seed) & (2 ** 64 - 1),
            int(first_task), *ptr(self.goals, self.perms, o.get("means"), o.get("probs"), o.get("goal"),
                                  o.get("perm"), o.get("query"), o.get("opt_action")))


def fresh_batch(env, seed, first_task, n, outputs=True):
    """The generator alone (dpt_fresh_batch / dpt_fresh_linear_batch): samples ``first_task`` ..
    ``first_task + n - 1`` of ``env`` (a ``FreshEnv``) under the Philox key ``seed``, each a function of (seed,
    its global index) alone.  Returns a dict of device tensors: ``tokens`` (n, 1 + H, 2 sd + A + 1) and
    ``targets`` (n, A) fp32 -- what the training step packs from a dataset of these samples -- and, with
    ``outputs``, ``opt_action`` (n) int32 and the task itself: ``means`` / ``probs`` (n, A) float64 for a
    bandit, ``goal`` (n, 2), ``perm`` (n, 5) and ``query`` (n, 2) int32 for DarkRoom, ``theta`` (n, d), ``means``
    (n, A) and, under the uniform rollin, ``probs`` (n, A) float64 for the linear bandit."""
    dev, n = device(), int(n)
    sd, A, T = env.state_dim, env.action_dim, 1 + env.H
    out = dict(tokens=torch.empty((n, T, 2 * sd + A + 1), dtype=torch.float32, device=dev),
               targets=torch.empty((n, A), dtype=torch.float32, device=dev))
    if outputs:
        out["opt_action"] = torch.empty(n, dtype=torch.int32, device=dev)
        if env.kind == _lib.FRESH_BANDIT:
            out.update(means=torch.empty((n, A), dtype=torch.float64, device=dev),
                       probs=torch.empty((n, A), dtype=torch.float64, device=dev))
        elif env.kind == FreshEnv.LINEAR:
            out.update(theta=torch.empty((n, env.lin_d), dtype=torch.float64, device=dev),
                       means=torch.empty((n, A), dtype=torch.float64, device=dev))
            if env.rollin == _lib.FRESH_LINEAR_UNIFORM:
                out["probs"] = torch.empty((n, A), dtype=torch.float64, device=dev)
        else:
            out.update(goal=torch.empty((n, 2), dtype=torch.int32, device=dev),
                       perm=torch.empty((n, 5), dtype=torch.int32, device=dev),
                       query=torch.empty((n, 2), dtype=torch.int32, device=dev))
    d = _lib.TrainDesc(1, E, sd, A, T, n, T, 0, 0.0, 0, 0)  # the generator reads state_dim, action_dim, batch, window
    args = env.args(seed, first_task, out)
    _lib.call(env.calls["batch"], ctypes.byref(d), ctypes.byref(args), n, _p(out["tokens"]), _p(out["targets"]),
              _stream())
    return out


# ----------------------------------------------------------------------------- in-episode DarkRoom rollout

def rollout_darkroom_episode(model, goals, K, dim, sample=True, perm=None, uniforms=None, seed=None, first_task=0,
                             logits=False):
    """The in-episode DarkRoom rollout in one launch (dpt_rollout_darkroom_episode): every env runs its K
    steps from s_0 = (0, 0) in one workgroup, the context being the episode's own transitions and the
    query state sitting at position 0.  ``model``: a width-32 ``models.net.Transformer`` with state_dim 2
    and action_dim 5 (its ``device_model()`` runs).  ``goals`` (N, 2) in [0, dim), ``perm`` (N, 5) the
    action permutations dpt_darkroom_step takes, ``uniforms`` (K - 1, N) inject the selection uniforms;
    otherwise Philox keyed by ``seed`` (default ``next_seed()``) and the env's global index
    ``first_task + i``.  Returns (records, returns[, logits]): the records dict of
    ``dpt_hip.train.rollout_darkroom_interactive`` (int32 device tensors states (N, K, 2), actions
    (N, K - 1), rewards (N, K - 1), targets (N, K)), the per-env return (N) int64, and with ``logits`` the
    (N, K, 5) fp32 logits every step selected from.  Raises NotImplementedError for other widths and for K
    above the model's prefill window (use ``rollout_darkroom_interactive``)."""
    from .train import _mdp_check_model, _mdp_episode
    who = "rollout_darkroom_episode"
    _mdp_check_model(model, who)
    if model.dropout > 0 and model.training:
        raise ValueError(f"{who}: the model is in training mode with dropout > 0 (call model.eval(): the rollout's "
                         f"forwards have no dropout masks)")
    dm = model.device_model()  # NotImplementedError at other widths
    dev, K = device(), int(K)
    g, pm, u, seed = _mdp_episode(goals, K, perm, uniforms, seed, dev)
    N = int(g.shape[0])
    rec = dict(states=torch.empty((N, K, 2), dtype=torch.int32, device=dev),
               actions=torch.empty((N, K - 1), dtype=torch.int32, device=dev),
               rewards=torch.empty((N, K - 1), dtype=torch.int32, device=dev),
               targets=torch.empty((N, K), dtype=torch.int32, device=dev))
    ret = torch.empty(N, dtype=torch.int32, device=dev)
    lg = torch.empty((N, K, 5), dtype=torch.float32, device=dev) if logits else None

    def ptr(t):
        return None if t is None else t.data_ptr()

    args = _lib.DarkroomEpisodeArgs(
        N, K, int(dim), int(bool(sample)), int(first_task), seed, 0, ptr(g), ptr(pm), ptr(u), ptr(rec["states"]),
        ptr(rec["actions"]) if K > 1 else None, ptr(rec["rewards"]) if K > 1 else None, ptr(rec["targets"]), ptr(lg),
        ptr(ret))
    _lib.call("dpt_rollout_darkroom_episode", dm.handle, ctypes.byref(args), _stream())
    out = (rec, ret.to(torch.int64))
    return out + (lg,) if logits else out


# ----------------------------------------------------------------------------- classical baselines

from ._lib import (POLICY_EMP, POLICY_LCB, POLICY_LINUCB, POLICY_OPT, POLICY_THOMPSON,  # noqa: E402,F401
                   POLICY_UCB)


def rollout_policy(policy, means, H, var, bandit_type=BANDIT_GAUSSIAN, online=True, sample=True, c=1.0,
                   ts_std=0.1, ts_prior_mean=0.5, ts_prior_var=1 / 12.0, arms=None, seed=0, first_task=0,
                   noise=None, policy_noise=None, ctx_actions=None, ctx_rewards=None, counter=0):
    """Fused classical-policy rollout (dpt_rollout_policy); optional prefix context (N, C).
    ``counter``: the Philox step counter of step 0 (step h draws at counter + h).
    ``ctx_actions`` must lie in [0, A): the kernel indexes its LDS tables by them unchecked.  A host
    array is checked here (ValueError); a device tensor is the caller's to keep in range."""
    if ctx_actions is not None and not isinstance(ctx_actions, torch.Tensor):
        ca = np.asarray(ctx_actions)
        n_arms = int(means.shape[1]) if isinstance(means, torch.Tensor) else int(np.asarray(means).shape[1])
        if ca.size and (ca.min() < 0 or ca.max() >= n_arms):
            raise ValueError(f"ctx_actions holds arm indices in [{ca.min()}, {ca.max()}]; the {n_arms} arms are "
                             f"0..{n_arms - 1}")
    dev = device()
    means_d = _dev(means, torch.float64, dev)
    N, A = means_d.shape
    H = int(H)
    C = 0 if ctx_actions is None else int(np.asarray(ctx_actions).shape[1]) if not isinstance(
        ctx_actions, torch.Tensor) else int(ctx_actions.shape[1])
    keep = [means_d]

    def opt(x, dt):
        if x is None:
            return None
        t = _dev(x, dt, dev)
        keep.append(t)
        return _p(t).value

    if policy_noise is not None:
        # the kernel indexes the injected draws by the policy's own layout (dpt_policies.hip):
        # Thompson (H, N, A) when sampling, (H, 100, N, A) for the 100-draw vote; LinUCB (N,)
        # uniforms for an empty context's random arm; no other policy reads them
        got = int(policy_noise.numel() if isinstance(policy_noise, torch.Tensor) else np.asarray(policy_noise).size)
        if int(policy) == POLICY_THOMPSON:
            want = H * N * A if sample else H * 100 * N * A
            if got != want:
                raise ValueError(f"policy_noise has {got} draws; Thompson (sample={bool(sample)}) reads {want}")
        elif int(policy) == POLICY_LINUCB and got < N:  # only step 0's row (N,) is read
            raise ValueError(f"policy_noise has {got} draws; LinUCB reads the first {N}")
    n = ctypes.c_int64()
    _lib.call("dpt_policy_workspace_numel", N, A, C + H, ctypes.byref(n))  # 0: contexts live in LDS
    ws = torch.empty(max(n.value, 1), dtype=torch.float64, device=dev)
    out = dict(actions=torch.empty((N, H), dtype=torch.int32, device=dev),
               rewards=torch.empty((N, H), dtype=torch.float64, device=dev),
               arm_value=torch.empty((N, H), dtype=torch.float64, device=dev))
    d = 0 if arms is None else int(np.asarray(arms).shape[1])
    args = _lib.PolicyRolloutArgs(
        N, H, A, int(policy), int(bool(online)), int(bandit_type), int(bool(sample)), d, int(first_task), float(var),
        float(c), float(ts_std), float(ts_prior_mean), float(ts_prior_var), int(seed) & (2 ** 64 - 1),
        _p(means_d).value, opt(arms, torch.float64), opt(noise, torch.float64), opt(policy_noise, torch.float64),
        _p(ws).value, _p(out["actions"]).value, _p(out["rewards"]).value, _p(out["arm_value"]).value, C, int(counter),
        opt(ctx_actions, torch.int32), opt(ctx_rewards, torch.float64))
    _lib.call("dpt_rollout_policy", ctypes.byref(args), _stream())
    out["_keep"] = (keep, ws)
    return out


def regret_moments(arm_value, opt, mode=_lib.REGRET_SUMS, mean=None):
    """One pass of the device regret statistics (evals/eval_bandit.py:169-178, scipy's two-pass
    form): arm_value (N, H) fp64, opt (N,) fp64 -> (2, H) fp64 sums over tasks of
    (diff, cumsum(diff)) for REGRET_SUMS, or of their squared deviations from ``mean`` (2, H)
    for REGRET_CENTRED."""
    dev = device()
    av = _dev(arm_value, torch.float64, dev)
    op = _dev(opt, torch.float64, dev).reshape(-1)
    N, H = av.shape
    if op.shape[0] != N:
        raise ValueError(f"opt has {op.shape[0]} tasks, arm_value {N}")
    n = ctypes.c_int64()
    _lib.call("dpt_regret_workspace_numel", N, H, ctypes.byref(n))
    ws = torch.empty(n.value, dtype=torch.float64, device=dev)
    out = torch.empty((2, H), dtype=torch.float64, device=dev)
    mn = None if mean is None else _dev(mean, torch.float64, dev)
    _lib.call("dpt_regret_moments", _p(av), _p(op), N, H, int(mode), _p(mn), _p(ws), _p(out), _stream())
    return out


def regret_max_steps():
    n = ctypes.c_int32()
    _lib.call("dpt_regret_max_steps", ctypes.byref(n))
    return n.value


# ----------------------------------------------------------------------------- explore-then-exploit evaluation

def recommend_curve(logits, means, targets=None):
    """dpt_recommend_curve: logits (N, T, A) fp32 (row t = the recommender after t transitions), means
    (N, A), targets (N) the optimal arms (default: ``means.argmax(1)``) -> dict of device tensors
    greedy_arm (N, T) int32, greedy_value / expected_value / p_opt (N, T) float64."""
    dev = device()
    lg = _dev(logits, torch.float32, dev)
    means_d = _dev(means, torch.float64, dev)
    if lg.dim() != 3 or means_d.dim() != 2 or tuple(means_d.shape) != (lg.shape[0], lg.shape[2]):
        raise ValueError(f"logits {tuple(lg.shape)} / means {tuple(means_d.shape)} are not (N, T, A) / (N, A)")
    N, T, A = (int(x) for x in lg.shape)
    tg = means_d.argmax(dim=1) if targets is None else _dev(targets, torch.int64, dev).reshape(-1)
    if tg.numel() != N:
        raise ValueError(f"targets {tg.numel()} != tasks {N}")
    out = dict(greedy_arm=torch.empty((N, T), dtype=torch.int32, device=dev),
               **{k: torch.empty((N, T), dtype=torch.float64, device=dev)
                  for k in ("greedy_value", "expected_value", "p_opt")})
    _lib.call("dpt_recommend_curve", _p(lg), _p(means_d), _p(tg), N, T, A, _p(out["greedy_arm"]),
              _p(out["greedy_value"]), _p(out["expected_value"]), _p(out["p_opt"]), _stream())
    out["_keep"] = (lg, means_d, tg)
    return out


def empirical_recommend(actions, rewards, means):
    """dpt_empirical_recommend: EmpMeanPolicy(online=False) on every prefix of the records actions (N, H)
    int32 / rewards (N, H) -> dict of device tensors emp_arm (N, H + 1) int32, emp_value (N, H + 1) float64."""
    dev = device()
    means_d = _dev(means, torch.float64, dev)
    acts = _dev(actions, torch.int32, dev)
    rews = _dev(rewards, torch.float64, dev)
    if means_d.dim() != 2 or acts.dim() != 2 or acts.shape != rews.shape or acts.shape[0] != means_d.shape[0]:
        raise ValueError(f"actions {tuple(acts.shape)} / rewards {tuple(rews.shape)} / means {tuple(means_d.shape)} "
                         f"are not (N, H) / (N, H) / (N, A)")
    (N, H), A = (int(x) for x in acts.shape), int(means_d.shape[1])
    out = dict(emp_arm=torch.empty((N, H + 1), dtype=torch.int32, device=dev),
               emp_value=torch.empty((N, H + 1), dtype=torch.float64, device=dev))
    _lib.call("dpt_empirical_recommend", _p(acts) if H else None, _p(rews) if H else None, _p(means_d), N, H, A,
              _p(out["emp_arm"]), _p(out["emp_value"]), _stream())
    out["_keep"] = (acts, rews, means_d)
    return out


# ----------------------------------------------------------------------------- Bayes posterior of the optimal action

def _bandit_type_code(bandit_type):
    code = {"uniform": BANDIT_GAUSSIAN, "gaussian": BANDIT_GAUSSIAN, "bernoulli": BANDIT_BERNOULLI}.get(
        bandit_type, bandit_type)
    if code not in (BANDIT_GAUSSIAN, BANDIT_BERNOULLI):
        raise NotImplementedError(f"bandit type {bandit_type!r}: BANDIT_GAUSSIAN or BANDIT_BERNOULLI")
    return int(code)


def posterior_grid(var, H, bandit_type=BANDIT_GAUSSIAN):
    """The default grid size G of ``bandit_posterior`` for records of H pulls: the smallest power of two
    >= 8 sqrt(H) / var (Gaussian rewards of std ``var``: the posterior of a mean pulled H times has std
    var / sqrt(H), so eight grid points per posterior std) or >= 8 H (Bernoulli: a Beta posterior at an end of
    [0, 1] is as narrow as 1 / H), at least 256.  Above the kernel's 8192 the grid would under-resolve the
    posterior: ValueError (an explicit ``grid=`` of ``bandit_posterior`` overrides this rule).  No device work."""
    H, code = int(H), _bandit_type_code(bandit_type)
    if H < 0:
        raise ValueError(f"posterior_grid: H={H}")
    if code == BANDIT_GAUSSIAN:
        if not float(var) > 0:
            raise ValueError(f"posterior_grid: Gaussian var={var} (the noise std) is not > 0")
        need = 8.0 * float(np.sqrt(H)) / float(var)
    else:
        need = 8.0 * H
    G = 256
    while G < need:
        G *= 2
    if G > _lib.POSTERIOR_MAX_GRID:
        raise ValueError(f"posterior_grid: H={H}" + (f", var={var}" if code == BANDIT_GAUSSIAN else ", Bernoulli") +
                         f" needs a grid of {G} points, above the kernel's {_lib.POSTERIOR_MAX_GRID}: the posterior "
                         f"of a much-pulled arm would be under-resolved (narrower than the grid spacing); pass a "
                         f"shorter record, or an explicit grid= to accept the error")
    return G


def bandit_posterior(actions, rewards, A, var, bandit_type=BANDIT_GAUSSIAN, grid=None, chunk=0):
    """dpt_bandit_posterior: the grid posterior of the optimal arm (prior means ~ U[0,1]^A, reward std
    ``var``) after every prefix of the records actions (N, H) int32 / rewards (N, H) -> post (N, H + 1, A)
    float64 on the device, row t given the first t pulls.  ``grid``: the grid size G (default
    ``posterior_grid(var, H, bandit_type)``); ``chunk``: tasks per launch (0: all at once); a task's rows do
    not depend on it.  No host synchronisation; runs on the current stream."""
    dev = device()
    acts, rews = _dev(actions, torch.int32, dev), _dev(rewards, torch.float64, dev)
    if acts.dim() != 2 or acts.shape != rews.shape or acts.shape[0] < 1:
        raise ValueError(f"actions {tuple(acts.shape)} / rewards {tuple(rews.shape)} are not (N >= 1, H) each")
    if int(chunk) < 0:
        raise ValueError(f"bandit_posterior: chunk={chunk}")
    N, H = (int(x) for x in acts.shape)
    A, code = int(A), _bandit_type_code(bandit_type)
    G = posterior_grid(var, H, code) if grid is None else int(grid)
    step = N if int(chunk) == 0 else min(N, int(chunk))
    need = ctypes.c_int64()
    _lib.call("dpt_bandit_posterior_workspace_numel", step, A, G, ctypes.byref(need))
    ws = torch.empty(need.value, dtype=torch.float64, device=dev)
    post = torch.empty((N, H + 1, A), dtype=torch.float64, device=dev)
    for off in range(0, N, step):
        n = min(step, N - off)
        args = _lib.BanditPosteriorArgs(n, H, A, code, G, 0, float(var), acts[off:].data_ptr() if H else None,
                                        rews[off:].data_ptr() if H else None, ws.data_ptr(), post[off:].data_ptr())
        _lib.call("dpt_bandit_posterior", ctypes.byref(args), _stream())
    for t in (acts, rews, ws):  # the launches are asynchronous: the caching allocator must not hand these
        t.record_stream(torch.cuda.current_stream())  # blocks to another stream before they ran
    return post


def darkroom_posterior(goals, query, next_states, rewards, dim, want_consistent=False):
    """dpt_darkroom_posterior: the posterior of the expert action at ``query`` (N, 2) after every prefix of
    the transitions next_states (N, H, 2) / rewards (N, H), the goal uniform over the rows of ``goals``
    (n_goals, 2) (with multiplicity; identity action permutation) -> post (N, H + 1, 5) float64, and with
    ``want_consistent`` (post, consistent (N, H + 1) int32: how many goals the prefix leaves).  No host
    synchronisation; runs on the current stream."""
    dev = device()
    gl = _dev(goals, torch.int32, dev).reshape(-1, 2)
    q = _dev(query, torch.int32, dev)
    ns, rw = _dev(next_states, torch.int32, dev), _dev(rewards, torch.int32, dev)
    if q.dim() != 2 or q.shape[1] != 2 or q.shape[0] < 1 or rw.dim() != 2 or rw.shape[0] != q.shape[0] or \
            tuple(ns.shape) != tuple(rw.shape) + (2,):
        raise ValueError(f"query {tuple(q.shape)} / next_states {tuple(ns.shape)} / rewards {tuple(rw.shape)} are "
                         f"not (N >= 1, 2) / (N, H, 2) / (N, H)")
    N, H = (int(x) for x in rw.shape)
    post = torch.empty((N, H + 1, 5), dtype=torch.float64, device=dev)
    cons = torch.empty((N, H + 1), dtype=torch.int32, device=dev) if want_consistent else None
    args = _lib.DarkroomPosteriorArgs(N, H, int(dim), int(gl.shape[0]), 0, 0, gl.data_ptr(), q.data_ptr(),
                                      ns.data_ptr() if H else None, rw.data_ptr() if H else None, post.data_ptr(),
                                      None if cons is None else cons.data_ptr())
    _lib.call("dpt_darkroom_posterior", ctypes.byref(args), _stream())
    for t in (gl, q, ns, rw):
        t.record_stream(torch.cuda.current_stream())
    return (post, cons) if want_consistent else post


def posterior_compare(post, logits, targets):
    """dpt_posterior_compare: post (N, T, A) float64 against a model's logits (N, T, A) float32 for the
    optimal actions targets (N) -> dict of (N, T) float64 device tensors nll_model, nll_bayes, kl, entropy
    (all arithmetic in float64).  No host synchronisation; runs on the current stream."""
    dev = device()
    ps, lg = _dev(post, torch.float64, dev), _dev(logits, torch.float32, dev)
    tg = _dev(targets, torch.int64, dev).reshape(-1)
    if ps.dim() != 3 or ps.shape != lg.shape or ps.shape[0] < 1 or tg.numel() != ps.shape[0]:
        raise ValueError(f"post {tuple(ps.shape)} / logits {tuple(lg.shape)} / targets {tg.numel()} are not "
                         f"(N >= 1, T, A) / (N, T, A) / N")
    N, T, A = (int(x) for x in ps.shape)
    out = {k: torch.empty((N, T), dtype=torch.float64, device=dev) for k in ("nll_model", "nll_bayes", "kl", "entropy")}
    args = _lib.PosteriorCompareArgs(N, T, A, 0, ps.data_ptr(), lg.data_ptr(), tg.data_ptr(),
                                     *(out[k].data_ptr() for k in ("nll_model", "nll_bayes", "kl", "entropy")))
    _lib.call("dpt_posterior_compare", ctypes.byref(args), _stream())
    for t in (ps, lg, tg):
        t.record_stream(torch.cuda.current_stream())
    return out


LINEAR_POSTERIOR_GRID = 8192


def linear_posterior_grid():
    """The default number of rays G of ``linear_posterior``: the smallest power of two at which the definition
    (tests/linear_posterior_oracle.py) stays within 1e-6 of its value at G = 65,536 on every row t >= 1 of the
    convergence records of tests/test_linear_posterior_host.py (the reference's 10 arms, six tasks of 20 pulls,
    std 0.3).  Measured worst deviation there: 1.9e-7 at 8,192 (1.9e-6 at 4,096, 1.8e-5 at 2,048: the integrand
    has kinks where the envelope changes arms, so the rule gains about a factor 10 per doubling, not more)."""
    return LINEAR_POSTERIOR_GRID


def linear_posterior(arms, actions, rewards, var, grid=None, chunk=0):
    """dpt_linear_posterior: the posterior of the optimal arm of the linear bandit with ``arms`` (A, 2) in the
    plane (prior theta ~ N(0, I / 2), reward std ``var`` > 0) after every prefix of the records actions (N, H)
    int32 / rewards (N, H) -> post (N, H + 1, A) float64 on the device, row t given the first t pulls; rows
    before the first valid pull are the prior in closed form.  ``grid``: the number of rays G (default
    ``linear_posterior_grid()``); ``chunk``: tasks per launch (0: all at once); a task's rows do not depend on
    it.  Arms of another width: NotImplementedError.  No host synchronisation; runs on the current stream."""
    dev = device()
    x = _dev(arms, torch.float64, dev)
    acts, rews = _dev(actions, torch.int32, dev), _dev(rewards, torch.float64, dev)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"arms {tuple(x.shape)}: expected (A, 2)")
    if acts.dim() != 2 or acts.shape != rews.shape or acts.shape[0] < 1:
        raise ValueError(f"actions {tuple(acts.shape)} / rewards {tuple(rews.shape)} are not (N >= 1, H) each")
    if int(chunk) < 0:
        raise ValueError(f"linear_posterior: chunk={chunk}")
    N, H = (int(v) for v in acts.shape)
    A, lin_d = (int(v) for v in x.shape)
    G = linear_posterior_grid() if grid is None else int(grid)
    step = N if int(chunk) == 0 else min(N, int(chunk))
    need = ctypes.c_int64()
    _lib.call("dpt_linear_posterior_workspace_numel", step, A, lin_d, G, ctypes.byref(need))
    ws = torch.empty(need.value, dtype=torch.float64, device=dev)
    post = torch.empty((N, H + 1, A), dtype=torch.float64, device=dev)
    for off in range(0, N, step):
        n = min(step, N - off)
        args = _lib.LinearPosteriorArgs(n, H, A, lin_d, G, 0, float(var), x.data_ptr(),
                                        acts[off:].data_ptr() if H else None, rews[off:].data_ptr() if H else None,
                                        ws.data_ptr(), post[off:].data_ptr())
        _lib.call("dpt_linear_posterior", ctypes.byref(args), _stream())
    for t in (x, acts, rews, ws):
        t.record_stream(torch.cuda.current_stream())
    return post


def linear_posterior_supported(lin_d, var):
    """None where ``linear_posterior`` covers a linear bandit of width ``lin_d`` and reward std ``var``, else
    the reason, a sentence for a NotImplementedError.  No device work."""
    if int(lin_d) == 2 and float(var) > 0:
        return None
    return ("the linear bandit's posterior over theta is Gaussian, but the probability that an arm is optimal "
            "under it is a lin_d-dimensional integral with no cheap form; supported: lin_d = 2 (a 1-D angular "
            f"quadrature, dpt_hip.linear_posterior) with a noise std var > 0, not lin_d = {lin_d}, var = {var}")


def fresh_posterior(env, batch, grid=None, chunk=0):
    """The Bayes posterior of the optimal action on every prefix of the fresh-task generator's samples
    ``batch`` (``fresh_batch(env, ...)`` with its outputs): (post (n, 1 + H, A) float64, targets (n) int64).
    The records are read back from the tokens, so the posterior is given exactly the context the model is
    given (the rewards as the float32 the tokens hold).  The prior is ``env``'s own: U[0,1]^A means with
    reward std ``env.var`` for a bandit, ``env.goals`` for DarkRoom, theta ~ N(0, I / 2) with ``env.arms`` and
    ``env.var`` for the linear bandit at lin_d = 2 (either rollin: the Thompson rollin depends on theta only
    through the history, so the likelihood of theta is the same).  The linear bandit at another width or at
    var = 0 (no cheap P(arm optimal)) and DarkRoom with a permutation list (the permutation is latent too)
    are not covered."""
    if env.kind == FreshEnv.LINEAR:
        why = linear_posterior_supported(env.lin_d, env.var)
        if why is not None:
            raise NotImplementedError(why)
        A = env.action_dim
        tok = batch["tokens"]
        acts = tok[:, 1:, 1:1 + A].argmax(dim=-1).to(torch.int32)
        return (linear_posterior(env.arms, acts, tok[:, 1:, 2 + A].to(torch.float64), env.var, grid, chunk),
                batch["opt_action"].to(torch.int64))
    tok, tg = batch["tokens"], batch["opt_action"].to(torch.int64)
    if env.kind == _lib.FRESH_BANDIT:
        A = env.action_dim
        acts = tok[:, 1:, 1:1 + A].argmax(dim=-1).to(torch.int32)
        return bandit_posterior(acts, tok[:, 1:, 2 + A].to(torch.float64), A, env.var, env.type, grid, chunk), tg
    if env.perms is not None:
        raise NotImplementedError("DarkRoom with an action-permutation list: the permutation is latent too")
    return darkroom_posterior(env.goals, tok[:, 0, :2].to(torch.int32), tok[:, 1:, 7:9].to(torch.int32),
                              tok[:, 1:, 9].to(torch.int32), env.dim), tg


def set_decode_tile(tile):
    """Tasks per workgroup of the decode kernels (8: two workgroups per CU; 16: one)."""
    _lib.call("dpt_tuning_set", _lib.TUNE_DECODE_TILE, int(tile))


def set_cache_budget(nbytes):
    """Bytes of the Infinity Cache the bandit rollout may fill with its earliest positions' cached
    rows (default policy, resident across steps); 0 streams every row non-temporally.  Cache
    policy only: results are bit-identical for any value."""
    _lib.call("dpt_tuning_set", _lib.TUNE_CACHE_BUDGET, int(nbytes))


def set_ycache_bits(bits):
    """Bandit rollout: storage of the cached ln_1 rows of blocks >= 1, 24 (default: 24-bit fixed
    point, 96 B per position) or 32 (fp32, 128 B: the comparison path)."""
    _lib.call("dpt_tuning_set", _lib.TUNE_YCACHE_BITS, int(bits))


def set_block0_mfma(on):
    """Retired with the matrix-core form of the bandit rollout's block 0: False (one wave per task on
    the vector ALUs, the only form) is accepted, True raises NotImplementedError (DPT_TUNE_BLOCK0_MFMA
    accepts only 0).  Kept so that callers written for the knob get the library's error."""
    _lib.call("dpt_tuning_set", _lib.TUNE_BLOCK0_MFMA, int(bool(on)))


def set_select_fast(on):
    """select_action for 5 and 20 arms: the fp32 cdf with the exact fp64 cdf within 2^-15 of an edge
    (default), or the fp64 cdf for every sample.  Bit-identical either way."""
    _lib.call("dpt_tuning_set", _lib.TUNE_SELECT_FAST, int(bool(on)))


_darkroom_memo = True
_darkroom_ws = True


def darkroom_max_window():
    """Largest window (1 + R*horizon tokens) of the fused DarkRoom rollout: 512 with the per-task
    workspace (16 waves per task above 256 tokens), 256 without it."""
    return 512 if _darkroom_ws else 256


def set_darkroom_workspace(on):
    """DarkRoom rollout: keep the context tokens' layer-0 inputs and queries in a per-task device
    workspace for the episode (default) or recompute them every step (the workspace-free path)."""
    global _darkroom_ws
    _darkroom_ws = bool(on)


def set_darkroom_memo(on):
    """DarkRoom rollout: one window forward per distinct query state per episode (default) or per step.
    Applies to the fused kernel and to the per-step device loop (evals/eval_darkroom.py)."""
    global _darkroom_memo
    _lib.call("dpt_tuning_set", _lib.TUNE_DARKROOM_MEMO, int(bool(on)))
    _darkroom_memo = bool(on)


def darkroom_memo():
    return _darkroom_memo


def set_prefill(on):
    """Windows up to DeviceModel.prefill_max_window() as one MFMA prefill (default) or position by position."""
    _lib.call("dpt_tuning_set", _lib.TUNE_PREFILL, int(bool(on)))


# ----------------------------------------------------------------------------- image act step
from .act import ImageActSession, obs_preprocess, obs_tables  # noqa: E402,F401
