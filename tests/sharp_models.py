"""One family of models whose attention is peaked, as a trained DPT's is (test helper, not a conftest).

Every other model of the suite is GPT-2 initialisation plus a small perturbation: its attention
scores span 0.2-0.4 and its softmax is a plain mean (largest probability 1 / T), so the running-max
rescale of the online softmax, its combination across waves, laps and tiles, the -inf start and a
peaked P in dS = P (dP - sum P dP) all sit on values near 1.  ``transform`` moves a reference
``state_dict`` of any width E off that point, deterministically (np.random.RandomState(seed), drawn
in the mapping's own key order):

* attn.c_attn.weight[:, :2E] (the q and k columns)  x qk
* attn.c_attn.bias                                  + 0.3 N(0, 1)
* ln_1.weight, ln_2.weight                          x U(0.5, gain)
* ln_1.bias, ln_2.bias                              + 0.2 N(0, 1)
* mlp.c_fc.weight, mlp.c_proj.weight                x 3
* pred_actions.weight                               x head (the peaked-head variant: 4)

and rounds every value to fp32.  Levels: ``medium`` qk = 4, gain = 2; ``sharp`` qk = 8, gain = 3.

``attention_stats`` measures, on the float64 oracle's arithmetic, the score span and the top
probability of the last query per block (means over the batch); ``assert_sharp`` holds them to the
level's thresholds, and every test calls it first so that a case cannot fall back to uniform
attention: medium span >= 4 in every block; sharp span >= 30 and top probability >= 0.5.  Where a
width or shape misses a threshold the case raises ``qk`` (never lowers the threshold).

Bars (``bar``): medium and the peaked head keep the project's bars; at sharp the fp32 oracle is itself
close to them, so a case's bar is max(project bar, 2 x the fp32 oracle's error on the same inputs),
the rule of test_prefill_fp16_split_scales_follow_the_weights (2: another summation order, not
another algorithm).

The case builders below borrow the model builders of test_gpu_train_grads, test_gpu_interactive,
test_gpu_image_act and test_gpu_ycache_packed inside functions, and test_gpu_train_grads imports this
module inside _token_level: neither imports the other at module level, which must stay so."""
import functools

import numpy as np

LEVELS = {"medium": dict(qk=4.0, gain=2.0), "sharp": dict(qk=8.0, gain=3.0)}
THRESHOLDS = {"medium": dict(span=4.0, top=0.0), "sharp": dict(span=30.0, top=0.5)}
HEAD_PEAKED = 4.0
LN_EPS = 1e-5


def _np(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


def transform(sd, E, level, qk=None, seed=5, head=1.0):
    """{key: fp32 numpy array} of the mapping ``sd`` (tensors or arrays) moved to ``level``; ``qk``
    overrides the level's factor for a case that needs more."""
    qk = LEVELS[level]["qk"] if qk is None else float(qk)
    gain = LEVELS[level]["gain"]
    rs = np.random.RandomState(seed)
    out = {}
    for k, v in sd.items():
        t = _np(v).astype(np.float64).copy()
        if k.endswith("attn.c_attn.weight"):
            assert t.shape == (E, 3 * E), (k, t.shape)
            t[:, :2 * E] *= qk
        elif k.endswith("attn.c_attn.bias"):
            t += 0.3 * rs.standard_normal(t.shape)
        elif k.endswith("ln_1.weight") or k.endswith("ln_2.weight"):
            t *= rs.uniform(0.5, gain, t.shape)
        elif k.endswith("ln_1.bias") or k.endswith("ln_2.bias"):
            t += 0.2 * rs.standard_normal(t.shape)
        elif k.endswith("mlp.c_fc.weight") or k.endswith("mlp.c_proj.weight"):
            t *= 3.0
        elif k == "pred_actions.weight":
            t *= head
        out[k] = t.astype(np.float32)
    return out


def as_torch(w):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()}


def as_f64(w):
    return {k: np.asarray(v, np.float64) for k, v in w.items()}


def load_into(module, w):
    """the transformed values into a torch module in place (keys the mapping lacks stay)"""
    import torch
    with torch.no_grad():
        own = module.state_dict()
        for k, v in w.items():
            own[k].copy_(torch.from_numpy(np.ascontiguousarray(v)))
    return module


def _ln(x, g, b):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + LN_EPS) * g + b


def _gelu(x):
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def attention_stats(w, n_layer, x):
    """[(mean score span, mean top probability) of the last query, per block] of the GPT-2 stack of
    ``w`` (reference names) on the float64 block input ``x`` (N, T, E): embeddings plus positions."""
    w = as_f64(w)
    x = np.asarray(x, np.float64)
    T, E = x.shape[1:]
    mask = np.triu(np.ones((T, T), bool), 1)
    stats = []
    for i in range(n_layer):
        p = f"transformer.h.{i}."
        h = _ln(x, w[p + "ln_1.weight"], w[p + "ln_1.bias"])
        qkv = h @ w[p + "attn.c_attn.weight"] + w[p + "attn.c_attn.bias"]
        q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
        s = np.where(mask, -np.inf, (q @ np.swapaxes(k, 1, 2)) * E ** -0.5)
        pr = np.exp(s - s.max(-1, keepdims=True))
        pr /= pr.sum(-1, keepdims=True)
        stats.append((float(np.ptp(s[:, -1], axis=-1).mean()), float(pr[:, -1].max(-1).mean())))
        x = x + (pr @ v) @ w[p + "attn.c_proj.weight"] + w[p + "attn.c_proj.bias"]
        h = _ln(x, w[p + "ln_2.weight"], w[p + "ln_2.bias"])
        x = x + _gelu(h @ w[p + "mlp.c_fc.weight"] + w[p + "mlp.c_fc.bias"]) @ w[p + "mlp.c_proj.weight"] \
            + w[p + "mlp.c_proj.bias"]
    return stats


def token_stats(w, n_layer, seq):
    """attention_stats of a token-level model on packed tokens ``seq`` (N, T, F)"""
    seq = np.asarray(seq, np.float64)
    x = seq @ np.asarray(w["embed_transition.weight"], np.float64).T + np.asarray(w["embed_transition.bias"], np.float64)
    return attention_stats(w, n_layer, x + np.asarray(w["transformer.wpe.weight"], np.float64)[:seq.shape[1]])


def assert_sharp(level, stats, label=""):
    """every block over the level's thresholds; prints the figures (``label`` names the case and its level)"""
    th = THRESHOLDS[level]
    print(f"sharp-stats {label}: span " + " ".join(f"{s:.1f}" for s, _ in stats) + "; top probability "
          + " ".join(f"{t:.2f}" for _, t in stats))
    for i, (span, top) in enumerate(stats):
        assert span >= th["span"], (label, level, i, span)
        assert top >= th["top"], (label, level, i, top)


def bar(level, project_bar, fp32_err):
    """the bar of one case: the project's, or at sharp twice the fp32 oracle's own error if larger"""
    return max(project_bar, 2.0 * fp32_err) if level == "sharp" else project_bar


def bandit_tokens(N, C, A, seed):
    """a bandit window (state_dim 1: states 1, as the rollout packs them) -> q, cs, ca, cn, cr (fp32)"""
    rs = np.random.RandomState(seed)
    q = np.ones((N, 1), np.float32)
    cs = np.ones((N, C, 1), np.float32)
    ca = np.eye(A, dtype=np.float32)[rs.randint(0, A, (N, C))]
    cr = rs.randn(N, C).astype(np.float32)
    return q, cs, ca, cs.copy(), cr


def darkroom_tokens(N, C, seed, dim=10):
    """a DarkRoom window: grid states, one-hot actions, 0/1 rewards -> q, cs, ca, cn, cr (fp32)"""
    rs = np.random.RandomState(seed)
    q = rs.randint(0, dim, (N, 2)).astype(np.float32)
    cs = rs.randint(0, dim, (N, C, 2)).astype(np.float32)
    cn = np.clip(cs + rs.randint(-1, 2, (N, C, 2)), 0, dim - 1).astype(np.float32)
    ca = np.eye(5, dtype=np.float32)[rs.randint(0, 5, (N, C))]
    cr = (rs.uniform(size=(N, C)) < 0.2).astype(np.float32)
    return q, cs, ca, cn, cr


# ----------------------------------------------------------------------------- the cases, shared by
# tests/test_sharp_models_host.py (thresholds, fp32-oracle bars, compared fractions, scale derivation)
# and tests/test_gpu_sharp_attention.py (the kernels).  QK: the cases whose default factor misses a
# threshold at their shape (measured on the float64 oracle; spans grow with qk^2), raised, never the
# threshold lowered.

LEVEL_NAMES = ("medium", "sharp")
QK = {
    # the windows, held at every T of (17, 65, 70, 101): at the defaults the 17-token bandit window
    # spans 3.8 in block 1 at medium, and at sharp the bandit's 70-token window 29.7 and the DarkRoom's
    # 17-token window 28.0 in block 3
    ("window", "bandit", "medium"): 4.5, ("window", "bandit", "sharp"): 9.0, ("window", "darkroom", "sharp"): 9.0,
    # the fused rollouts' own trajectories repeat few arms: block 1 spans 3.3-3.9 at qk = 4; the greedy
    # ones are flatter still at sharp (L = 2: span 29.2, top probability 0.44; 20 arms: span 26.7)
    ("rollout", 2, 5, "medium"): 5.0, ("rollout", 4, 5, "medium"): 5.0, ("rollout", 4, 20, "medium"): 5.0,
    ("rollout", 2, 5, "sharp"): 10.0, ("rollout", 4, 20, "sharp"): 9.0,
    ("generic", 16, "medium"): 5.0, ("generic", 18, "medium"): 6.0, ("generic", 18, "sharp"): 10.0,
    # width 16 (scores are sums of 16 products) at the 17- and 129-token windows, width 18 at 65
    ("train", "mfma", 16, 17, "medium"): 6.0, ("train", "mfma", 16, 17, "sharp"): 12.0,
    ("train", "mfma", 16, 129, "medium"): 5.0, ("train", "mfma", 16, 129, "sharp"): 10.0,
    ("train", "last", 18, 65, "medium"): 5.0,
    # the DarkRoom rollout's own windows (block 1 spans 3.3 and 25 at the defaults)
    ("darkroom", "medium"): 5.0, ("darkroom", "sharp"): 10.0,
    # the fused steps' 6-token windows: at qk = 4 their spans are 1.2-3.5; 6 suffices for four of the
    # six and 8 for all, which leaves a margin for records that differ from the oracle's replay
    ("fused", "interactive", 32, "medium"): 8.0, ("fused", "interactive", 18, "medium"): 8.0,
    ("fused", "explorer", 32, "medium"): 8.0, ("fused", "explorer", 18, "medium"): 8.0,
    ("fused", "exploiter", 32, "medium"): 8.0, ("fused", "exploiter", 18, "medium"): 8.0,
}


def qk_of(level, *key):
    return QK.get(key + (level,), LEVELS[level]["qk"])


def _bench_weights(L, sd, A, H, level, qk, head=1.0):
    import bench
    base, _ = bench.synthetic_state_dict(L, sd, A, H)
    return transform(base, 32, level, qk=qk, head=head)


# item 1: the width-32 window forward, bandit (state_dim 1) and DarkRoom (state_dim 2), 4 layers, 5 arms
WINDOW_TS = (1, 17, 65, 101)
CHAIN_T = 70  # the decode-step chain's window
WINDOW_N = 6


@functools.lru_cache(maxsize=None)
def window_weights(env, level):
    return _bench_weights(4, 1 if env == "bandit" else 2, 5, 100, level, qk_of(level, "window", env))


def window_inputs(env, T):
    return bandit_tokens(WINDOW_N, T - 1, 5, 100 + T) if env == "bandit" else darkroom_tokens(WINDOW_N, T - 1, 200 + T)


def window_seq(env, T):
    from oracle import dpt_oracle as O
    return O.pack_tokens(*window_inputs(env, T), 5, 1 if env == "bandit" else 2)


@functools.lru_cache(maxsize=None)
def window_refs(env, level, T):
    """(float64, fp32) oracle preds at every position (N, T, A): rows 1.. are out_mode 1, row -1 out_mode 0"""
    from oracle import dpt_oracle as O
    W = O.split_weights(as_f64(window_weights(env, level)), 4)
    seq = window_seq(env, T)
    out = []
    for dt in (np.float64, np.float32):
        c = lambda a: np.asarray(a, dt)  # noqa: E731
        out.append((O.gpt2_hidden(W, seq, dt) @ c(W["head_w"]).T + c(W["head_b"])).astype(np.float64))
    return tuple(out)


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


# items 2 and 4: bandit rollouts
ROLLOUT_HS = (9, 70, 130)
ROLLOUT_MODELS = ((2, 5), (4, 5), (4, 20))
ROLLOUT_TILES = ((8, 11), (16, 19))
VAR = 0.3


def bandit_means(N, A):
    if A == 5:
        return np.random.RandomState(1).uniform(0, 1, (N, A))
    arms = np.random.RandomState(1234).normal(size=(A, 2)) / np.sqrt(2)
    return np.random.RandomState(2).normal(0, 1, (N, 2)) / np.sqrt(2) @ arms.T


@functools.lru_cache(maxsize=None)
def _bandit_draws_full(N):
    H = max(ROLLOUT_HS)
    rs = np.random.RandomState(1000 * N + H)
    return rs.uniform(size=(H, N)), rs.standard_normal((H, N))


def bandit_draws(N, H):
    """selection uniforms and reward normals (H, N): the first H steps of one 130-step set per N, so
    a rollout over H = 9 or 70 steps is the prefix of the 130-step rollout of the same model, task for
    task (every window it runs is a window of that rollout, whose longest one the thresholds are
    asserted on)"""
    u, g = _bandit_draws_full(N)
    return u[:H], g[:H]


@functools.lru_cache(maxsize=None)
def rollout_weights(L, A, level, head=1.0):
    return _bench_weights(L, 1, A, max(ROLLOUT_HS), level, qk_of(level, "rollout", L, A), head)


@functools.lru_cache(maxsize=None)
def rollout_refs(L, A, level, head, N, H, sample):
    """(float64, fp32) C-oracle rollouts of the width-32 model on the injected draws"""
    import dpt_hip
    from oracle import c_oracle
    blob = dpt_hip.pack_weights(as_torch(rollout_weights(L, A, level, head)), L).numpy()
    u, g = bandit_draws(N, H)
    args = (blob, L, A, 4 * (1 + max(ROLLOUT_HS)), bandit_means(N, A), H, VAR, u, g, sample)
    return (c_oracle.bandit_rollout_f64(*args, False, 1, want_logits=True),
            c_oracle.bandit_rollout(*args, False, 1, want_logits=True))


def bandit_window(actions, rewards, A):
    """the packed window (N, 1 + C, A + 3) of a bandit rollout's records (states 1)"""
    N, C = actions.shape
    tok = np.zeros((N, C + 1, A + 3))
    tok[:, :, 0] = 1.0
    tok[:, 1:, 1:A + 1] = np.eye(A)[actions]
    tok[:, 1:, A + 1] = 1.0
    tok[:, 1:, A + 2] = np.asarray(rewards, np.float64).astype(np.float32)
    return tok


def rollout_compare(out, ref, margin, bar_=1e-5):
    """tests/test_gpu_ycache_packed._check with the case's bar: returns (largest relative logit error
    on the compared steps, compared steps per task, compared fraction)"""
    from test_gpu_ycache_packed import _check
    err, n_cmp = _check(out, ref, margin, bar=bar_)
    H = out["actions"].shape[1]
    return err, n_cmp, float((np.arange(H)[:, None] < n_cmp[None, :]).mean())


GENERIC_ES = (16, 18, 64)
GENERIC = dict(L=2, N=9, H=130, A=5)


def generic_module(E, level):
    """(module on the host in eval mode, fp32 weights) of the generic-width rollout's case"""
    from test_gpu_train_grads import _model
    m, w64 = _model(E, GENERIC["L"], 1, GENERIC["H"], E + GENERIC["L"], test=True)
    w = transform(w64, E, level, qk=qk_of(level, "generic", E))
    return load_into(m, w).eval(), w


@functools.lru_cache(maxsize=None)
def generic_refs(E, level):
    """(float64, fp32) oracle rollouts (the whole window re-forwarded every step) + the float64 margins"""
    from oracle import dpt_oracle as O
    _, w = generic_module(E, level)
    W = O.split_weights(as_f64(w), GENERIC["L"])
    N, H, A = GENERIC["N"], GENERIC["H"], GENERIC["A"]
    u, g = bandit_draws(N, H)
    means = bandit_means(N, A)
    refs = []
    for dt in (np.float64, np.float32):
        r = O.bandit_online_rollout(W, means, H, VAR, u, g, True, dtype=dt)
        r["arm_value"] = r["cum_means"].T
        refs.append(r)
    refs[0]["margin"] = O.boundary_margin(O.softmax_f32(refs[0]["logits"]), u)
    return tuple(refs)


# item 3: the fused DarkRoom rollout; one workgroup per task, so the partial tile is the window's last
# 16-token block (windows 61 and 128) and N = 5 is simply odd
DARKROOM_CASES = ((3, 30, 2), (2, 127, 1))
DARKROOM_N = 5


@functools.lru_cache(maxsize=None)
def darkroom_weights(level):
    return _bench_weights(4, 2, 5, 127, level, qk_of(level, "darkroom"))


def darkroom_setup(Heps, horizon, permuted):
    rs = np.random.RandomState(10 * Heps + horizon + permuted)
    goals = rs.randint(0, 10, (DARKROOM_N, 2))
    perms = None
    if permuted:
        from oracle import dpt_oracle as O
        perms = O.perm_table()[rs.randint(0, 120, DARKROOM_N)].astype(np.int32)
    return goals, perms, rs.uniform(size=(Heps * horizon, DARKROOM_N))


@functools.lru_cache(maxsize=None)
def darkroom_refs(level, Heps, horizon, R, permuted):
    """(float64 C oracle with margins, fp32 numpy oracle) of one DarkRoom case"""
    import dpt_hip
    from oracle import c_oracle
    from oracle import dpt_oracle as O
    w = darkroom_weights(level)
    goals, perms, u = darkroom_setup(Heps, horizon, permuted)
    blob = dpt_hip.pack_weights(as_torch(w), 4).numpy()
    r64 = c_oracle.darkroom_rollout(blob, 4, 512, goals, Heps, horizon, R, u, True, perms=perms, threads=4,
                                    want_logits=True)
    r32 = O.darkroom_online_rollout(O.split_weights(w, 4), goals, Heps, R * horizon, horizon,
                                    u.reshape(Heps, horizon, DARKROOM_N), True, perm=perms, dtype=np.float32)
    return r64, r32


def darkroom_last_window(goals, perms, actions, horizon, R):
    """the packed window (N, 1 + R horizon, 10) the last episode's first step sees: the R episodes
    before it, replayed from the recorded actions"""
    from oracle import dpt_oracle as O
    N, steps = actions.shape
    Heps = steps // horizon
    rows = []
    for ep in range(Heps - 1 - R, Heps - 1):
        s = np.zeros((N, 2), np.int64)
        for t in range(horizon):
            a = actions[:, ep * horizon + t]
            ns, r = O.darkroom_transit(s, a, goals, 10, perms)
            rows.append(np.concatenate([s, np.eye(5)[a], ns, r[:, None]], 1))
            s = ns
    q = np.zeros((N, 1, 10))
    return np.concatenate([q, np.stack(rows, 1)], 1)


def darkroom_compare(out, ref, horizon, bar_=1e-5, label=""):
    """test_gpu_kernels.check_darkroom_tasks with the case's bar on numpy rows (tasks, steps):
    returns (largest relative logit error on the compared steps, compared fraction)"""
    from test_gpu_kernels import compared_steps
    steps = ref["actions"].shape[1]
    n = compared_steps(out["actions"], ref["actions"], ref["margin"])
    sel = np.arange(steps)[:, None] <= np.minimum(n, steps - 1)[None, :]
    err = rel_err(out["logits"][sel], ref["logits"][sel])
    for j in range(len(n)):
        assert np.array_equal(out["returns"][j, :n[j] // horizon], ref["returns"][j, :n[j] // horizon]), j
    frac = float(n.sum()) / n.size / steps
    print(f"  {label}: max rel logit err {err:.3e} (bar {bar_:.1e}), compared {frac:.4f}")
    assert err <= bar_, (label, err, bar_)
    assert frac >= 0.9, (label, frac)
    return err, frac


# item 5: training forward / backward through test_gpu_train_grads._token_level
TRAIN_MFMA = tuple((E, T) for E in (16, 32, 64) for T in (17, 65, 129))
TRAIN_ROWS = ((18, 65), (48, 65))
TRAIN_LAST = tuple((E, T) for E in (32, 18) for T in (65, 130))


def train_shape(kind, E, T):
    """(E, L, sd, B, T, last) as the existing cases of test_gpu_train_grads choose them"""
    if kind == "mfma":
        return E, 2, 2 if E == 32 else 1, 3, T, False
    if kind == "rows":
        return E, 2, 2 if E == 48 else 1, 3, T, False
    return E, 2, 1, 5, T, True


def train_transform(kind, E, T, level):
    return functools.partial(transform, E=E, level=level, qk=qk_of(level, "train", kind, E, T))


# item 6: the fused interactive / explorer-exploiter steps (medium only)
FUSED = dict(K=6, L=2, N=8, A=5)


def fused_transform(E, which):
    return functools.partial(transform, E=E, level="medium", qk=qk_of("medium", "fused", which, E))


# item 7: the image act step, trunk transformed, front end as it is
IMAGE = dict(B=5, C=7)


def image_transform(E, level):
    return functools.partial(transform, E=E, level=level, qk=qk_of(level, "image", E))


def image_stats(w, n_layer, obs, angle, ctx, A):
    """attention_stats of an ImageTransformer's trunk on the float64 front end's embeddings"""
    import torch
    import image_oracle as IO
    P = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in w.items()}
    images, feats = IO.pack(dict(ctx, query_images=obs, query_states=angle), A)
    B, T = images.shape[:2]
    with torch.no_grad():
        emb, _ = IO.front(P, images.reshape(B * T, *images.shape[2:]), feats.reshape(B * T, -1))
    x = emb.reshape(B, T, -1).numpy() + np.asarray(w["transformer.wpe.weight"], np.float64)[:T]
    return attention_stats(w, n_layer, x)


def fused_case(E, which, chunk):
    """means, selection uniforms, reward normals and (explorer / exploiter step) env actions of one
    fused-step case, as tests/test_gpu_train_grads.py and tests/test_gpu_explore.py draw them"""
    K, N, A = FUSED["K"], FUSED["N"], FUSED["A"]
    rs = np.random.RandomState(1000 * K + 10 * E + chunk + (0 if which == "interactive" else 1))
    means = rs.uniform(0, 1, (N, A))
    u, g = rs.uniform(size=(K - 1, N)), rs.normal(size=(K - 1, N))
    ea = rs.randint(0, A, (K - 1, N)).astype(np.int32) if which != "interactive" else None
    return means, u, g, ea


def fused_module(E, which, seed_offset=0):
    """(module on the host, float64 weights) of a fused-step case at medium"""
    from test_gpu_interactive import _model
    m, w64 = _model(E, FUSED["L"], FUSED["K"], 100 * FUSED["K"] + E + seed_offset)
    w = fused_transform(E, which)(w64)
    return load_into(m, w), as_f64(w)


def fused_records(w64, means, u, g, env_actions=None):
    """The float64 oracle's replay of a fused step's K - 1 rollout steps: the selection rule of the
    project on the last-position logits, GPUBanditEnv's fp32 reward arithmetic on the selected arm
    (or on the injected env action) -> (context actions (N, K-1), rewards (N, K-1))."""
    import torch
    from oracle import dpt_oracle as O
    from oracle import dpt_oracle_torch as OT
    N, A = means.shape
    steps = u.shape[0]
    P = OT.state_dict_params(w64, FUSED["L"])
    acts, rews = np.zeros((N, steps), np.int64), np.zeros((N, steps))
    with torch.no_grad():
        for t in range(steps):
            tok = torch.from_numpy(bandit_window(acts[:, :t], rews[:, :t], A))
            lg = OT.forward(P, tok, FUSED["L"])[:, -1].numpy().astype(np.float32)
            acts[:, t] = O.select_actions(lg, u[t])
            arm = acts[:, t] if env_actions is None else env_actions[t]
            rews[:, t] = (means[np.arange(N), arm].astype(np.float32)
                          + g[t].astype(np.float32) * np.float32(VAR)).astype(np.float64)
    return acts, rews


def image_case(E, level):
    """the ImageTransformer (host, eval) with its trunk transformed, its float64 weights, and the
    context / frames of tests/test_gpu_image_act.py at B = 5, C = 7"""
    import test_gpu_image_act as IA
    m = IA.make_model(E, seed=2)
    w = image_transform(E, level)(IA.weights64(m))
    load_into(m, w)
    ctx = IA.make_context(IMAGE["B"], IMAGE["C"], 40 + IMAGE["C"])
    frames, angle = IA.make_frames(IMAGE["B"], (60, 80), 50 + IMAGE["B"])
    return m, as_f64(w), ctx, frames, angle


def fused_losses(which, P, acts, rews, target, P_exploiter=None, beta=0.5):
    """The fused steps' losses on the window built from the records, in the dtype of the leaf
    tensors ``P`` (float64: the reference; float32: the fp32 oracle the kernels are printed next to).
    ``interactive``: the mean last-position cross-entropy (train_interactive.py).  ``explore``:
    (explorer loss, exploiter loss) of tests/test_gpu_explore._reference -- the advantages from K
    prefix-window forwards of ``P_exploiter`` without a graph, the exploiter's mean cross-entropy over
    all N K positions, the explorer's mean of exp(adv / beta) CE(logits_j, context action j)."""
    import torch
    from oracle import dpt_oracle_torch as OT
    L, A = FUSED["L"], FUSED["A"]
    dtype = next(iter(P.values())).dtype
    tok = torch.from_numpy(bandit_window(acts, rews, A)).to(dtype)
    tg = torch.from_numpy(np.asarray(target, np.int64))
    ce = torch.nn.functional.cross_entropy
    if which == "interactive":
        return ce(OT.forward(P, tok, L)[:, -1], tg)
    N, K = tok.shape[:2]
    adv = torch.zeros((N, K - 1), dtype=dtype)
    with torch.no_grad():
        previous = None
        for t in range(K):
            current = ce(OT.forward(P_exploiter, tok[:, :t + 1], L)[:, -1], tg, reduction="none")
            if t > 0:
                adv[:, t - 1] = current - previous
            previous = current
    exploiter_loss = ce(OT.forward(P_exploiter, tok, L).reshape(-1, A), tg[:, None].expand(N, K).reshape(-1))
    logits = OT.forward(P, tok, L)[:, :-1]
    explorer_loss = (ce(logits.reshape(-1, A), torch.from_numpy(np.asarray(acts, np.int64)).reshape(-1),
                        reduction="none").reshape(N, K - 1) * torch.exp(adv * (1 / beta))).mean()
    return explorer_loss, exploiter_loss


def fused_grads(which, w64, acts, rews, target, dtype, w64_exploiter=None, beta=0.5):
    """{name: gradient} of fused_losses at the weights ``w64`` in torch ``dtype``: one mapping for
    ``interactive``, (explorer's, exploiter's) for ``explore``"""
    from oracle import dpt_oracle_torch as OT
    grads = lambda P: {k: v.grad.numpy().astype(np.float64) for k, v in P.items()}  # noqa: E731
    P = OT.state_dict_params(w64, FUSED["L"], dtype=dtype)
    if which == "interactive":
        fused_losses(which, P, acts, rews, target).backward()
        return grads(P)
    Px = OT.state_dict_params(w64_exploiter, FUSED["L"], dtype=dtype)
    le, lx = fused_losses(which, P, acts, rews, target, Px, beta)
    le.backward()
    lx.backward()
    return grads(P), grads(Px)
