"""Float64 restatement of the interactive DarkRoom episode (include/dpt_hip.h, "interactive DarkRoom
(MDP) training step"), a test helper: oracle/dpt_oracle_torch.forward on each window W_t, the selection
rule on those logits, numpy transit and opt_action, and the two losses with autograd's gradient."""
import numpy as np
import torch

from oracle import dpt_oracle_torch as OT

A, F = 5, 10


def model(E, L, H, seed, sharp=None):
    """a perturbed DarkRoom Transformer (state_dim 2, action_dim 5, test mode) on the host and its float64
    weights; ``sharp``: moved to that sharp_models level (sharp attention, larger gains)"""
    from models.net import Transformer
    torch.manual_seed(seed)
    m = Transformer(dict(horizon=H, state_dim=2, action_dim=A, n_layer=L, n_embd=E, n_head=1, dropout=0.0,
                         test=True))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    if sharp is not None:
        import sharp_models
        m.load_state_dict(sharp_models.as_torch(sharp_models.transform(m.state_dict(), E, level=sharp)))
    w64 = {k: v.detach().numpy().astype(np.float64) for k, v in m.state_dict().items()}
    return m, w64


# the records case of the issue: dim 3, 7 envs, 6 steps, goals including (0, 0), (0, 1) and (2, 2), injected
# uniforms whose seed keeps every oracle draw's cdf margin above 1e-5 (asserted on the CPU)
REC_DIM, REC_N, REC_K, REC_L = 3, 7, 6, 2
REC_GOALS = np.array([[0, 0], [0, 1], [2, 2], [1, 2], [2, 0], [1, 1], [0, 2]], np.int32)
REC_UNIFORM_SEED = 11


def records_case(E, permuted=False):
    """(model, w64, uniforms (K - 1, N), perm (N, 5) or None, the oracle's episode) of the records case"""
    m, w64 = model(E, REC_L, REC_K, 1000 + E)
    rs = np.random.RandomState(REC_UNIFORM_SEED)
    u = rs.uniform(size=(REC_K - 1, REC_N))
    perm = np.stack([rs.permutation(5) for _ in range(REC_N)]).astype(np.int32) if permuted else None
    return m, w64, u, perm, episode(w64, REC_L, REC_GOALS, REC_K, REC_DIM, True, u, perm)


def transit(state, action, goal, dim, perm=None):
    """envs/darkroom_env.py:37-55 (+ :100-103 permuted) for N envs: (next state (N, 2), reward (N))."""
    state, action, goal = np.asarray(state, np.int64), np.asarray(action, np.int64), np.asarray(goal, np.int64)
    a = action if perm is None else np.asarray(perm, np.int64)[np.arange(len(action)), action]
    ns = state.copy()
    ns[:, 0] += (a == 0).astype(np.int64) - (a == 1)
    ns[:, 1] += (a == 2).astype(np.int64) - (a == 3)
    ns = np.clip(ns, 0, dim - 1)
    return ns, (ns == goal).all(1).astype(np.int64)


def opt_action(state, goal, perm=None):
    """envs/darkroom_env.py:69-82 (+ :105-111: the index of the expert action inside perm) for N envs."""
    state, goal = np.asarray(state, np.int64), np.asarray(goal, np.int64)
    x, y, gx, gy = state[:, 0], state[:, 1], goal[:, 0], goal[:, 1]
    a = np.where(x < gx, 0, np.where(x > gx, 1, np.where(y < gy, 2, np.where(y > gy, 3, 4))))
    if perm is not None:
        a = (np.asarray(perm, np.int64) == a[:, None]).argmax(1)
    return a


def window(states, actions, rewards, t):
    """W_t (N, t + 1, 10) float64 from the records states (N, K, 2), actions / rewards (N, K - 1)."""
    N = states.shape[0]
    w = np.zeros((N, t + 1, F))
    w[:, 0, :2] = states[:, t]
    for j in range(t):
        w[:, 1 + j, :2] = states[:, j]
        a = actions[:, j]
        ok = (a >= 0) & (a < A)
        w[np.arange(N)[ok], 1 + j, 2 + a[ok]] = 1.0
        w[:, 1 + j, 2 + A:4 + A] = states[:, j + 1]
        w[:, 1 + j, 4 + A] = rewards[:, j]
    return torch.from_numpy(w)


def select(logits, sample, u):
    """The selection rule on float64 logits (N, 5): (actions, margins).  Sampled (temp 1): the count of
    cdf entries <= u, cdf = cumsum(softmax) / its last entry; margin = min_k |cdf_k - u| over the first
    four entries (the last is 1 > u).  Greedy: the first argmax; margin = the gap to the runner-up."""
    x = np.asarray(logits, np.float64)
    if not sample:
        srt = np.sort(x, 1)
        return x.argmax(1), srt[:, -1] - srt[:, -2]
    p = np.exp(x - x.max(1, keepdims=True))
    cdf = np.cumsum(p / p.sum(1, keepdims=True), 1)
    cdf /= cdf[:, -1:]
    u = np.asarray(u, np.float64)[:, None]
    return np.minimum((cdf <= u).sum(1), A - 1), np.abs(cdf[:, :-1] - u).min(1)


def episode(w64, L, goal, K, dim, sample=True, uniforms=None, perm=None):
    """The contract's episode with float64 forwards: a dict of states (N, K, 2), actions (N, K - 1), rewards
    (N, K - 1), targets (N, K) int64, logits (K, N, 5) float64 and margins (K - 1, N)."""
    goal = np.asarray(goal, np.int64)
    N = goal.shape[0]
    P = {k: v.detach() for k, v in OT.state_dict_params(w64, L).items()}
    states, targets = np.zeros((N, K, 2), np.int64), np.zeros((N, K), np.int64)
    actions, rewards = np.zeros((N, K - 1), np.int64), np.zeros((N, K - 1), np.int64)
    logits, margins = np.zeros((K, N, A)), np.zeros((K - 1, N))
    for t in range(K):
        targets[:, t] = opt_action(states[:, t], goal, perm)
        with torch.no_grad():
            logits[t] = OT.forward(P, window(states, actions, rewards, t), L)[:, -1].numpy()
        if t < K - 1:
            actions[:, t], margins[t] = select(logits[t], sample, None if uniforms is None else uniforms[t])
            states[:, t + 1], rewards[:, t] = transit(states[:, t], actions[:, t], goal, dim, perm)
    return dict(states=states, actions=actions, rewards=rewards, targets=targets, logits=logits, margins=margins)


def loss(P, L, rec, mode, targets=None, scale=None):
    """The contract's loss (a float64 torch scalar on the leaf parameters ``P``) conditioned on the records
    ``rec``.  mode 'last': (1 / N) sum_i CE(logits_{K-1,i}, target_{K-1,i}); 'every': (1 / (N K)) sum_t sum_i
    CE(logits_{t,i}, target_{t,i}).  ``targets`` (N, K) / ``scale`` override the records' targets / the
    mode's scale (the control cases)."""
    states, actions, rewards = (np.asarray(rec[k], np.int64) for k in ("states", "actions", "rewards"))
    tg = torch.from_numpy(np.asarray(rec["targets"] if targets is None else targets, np.int64))
    N, K = tg.shape
    steps = range(K) if mode == "every" else [K - 1]
    scale = (1.0 / (N * K) if mode == "every" else 1.0 / N) if scale is None else scale
    total = 0.0
    for t in steps:
        lg = OT.forward(P, window(states, actions, rewards, t), L)[:, -1]
        total = total + scale * torch.nn.functional.cross_entropy(lg, tg[:, t], reduction="sum")
    return total


def loss_and_grads(w64, L, rec, mode, targets=None, scale=None):
    """(loss, {reference parameter name: float64 gradient}) of ``loss`` at the weights ``w64``."""
    P = OT.state_dict_params(w64, L)
    value = loss(P, L, rec, mode, targets, scale)
    value.backward()
    return value.item(), {k: v.grad.numpy() for k, v in P.items()}
