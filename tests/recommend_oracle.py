"""numpy restatements of the explore-then-exploit evaluation's definitions (include/dpt_hip.h,
dpt_recommend_curve / dpt_empirical_recommend): the contract the device kernels are held to."""
import numpy as np


def recommend_curve(logits, means, targets=None):
    """logits (N, T, A) fp32, means (N, A) fp64, targets (N) int64 (default: the first maximum of means) ->
    greedy_arm (N, T) int32, greedy_value / expected_value / p_opt (N, T) fp64, all in fp64 from the fp32
    logits: the first index of the maximum logit, its mean, sum_a softmax(logits)_a means_a with the
    maximum subtracted, and the softmax probability of the target (0 for a target outside [0, A))."""
    logits = np.asarray(logits, np.float32)
    means = np.asarray(means, np.float64)
    N, T, A = logits.shape
    targets = means.argmax(1) if targets is None else np.asarray(targets, np.int64)
    x = logits.astype(np.float64)
    arm = x.argmax(-1)
    rows = np.arange(N)[:, None]
    e = np.exp(x - x.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    inside = (targets >= 0) & (targets < A)
    p_opt = np.where(inside[:, None], p[rows, np.arange(T)[None, :], np.clip(targets, 0, A - 1)[:, None]], 0.0)
    return dict(greedy_arm=arm.astype(np.int32), greedy_value=means[rows, arm],
                expected_value=(p * means[:, None, :]).sum(-1), p_opt=p_opt)


def empirical_recommend(actions, rewards, means):
    """EmpMeanPolicy(online=False) on every prefix, sequentially: sum / cnt accumulate over the pulls
    j < t in pull order in fp64, an action outside [0, A) adds to no arm -> emp_arm (N, H + 1) int32 (the
    first maximum of sum / max(1, cnt)), emp_value (N, H + 1) = means[i, emp_arm]."""
    actions = np.asarray(actions)
    rewards = np.asarray(rewards, np.float64)
    means = np.asarray(means, np.float64)
    N, A = means.shape
    H = actions.shape[1] if actions.ndim == 2 else 0
    arm = np.zeros((N, H + 1), np.int32)
    for i in range(N):
        s, c = np.zeros(A), np.zeros(A)
        for t in range(H + 1):
            arm[i, t] = np.argmax(s / np.maximum(1.0, c))
            if t < H and 0 <= actions[i, t] < A:
                s[actions[i, t]] += rewards[i, t]
                c[actions[i, t]] += 1.0
    return dict(emp_arm=arm, emp_value=means[np.arange(N)[:, None], arm])


def commit_regret(actions, means, greedy_value):
    """cumulative regret of 'explore for t pulls, then play the greedy recommendation for the remaining
    H - t': sum_{j<t} (mu* - mu[a_j]) + (H - t) (mu* - greedy_value[t]), (N, H + 1)"""
    actions = np.asarray(actions)
    means = np.asarray(means, np.float64)
    N, H = actions.shape
    opt = means.max(1)
    gaps = opt[:, None] - means[np.arange(N)[:, None], actions]
    spent = np.concatenate([np.zeros((N, 1)), np.cumsum(gaps, axis=1)], axis=1)
    return spent + (H - np.arange(H + 1))[None, :] * (opt[:, None] - np.asarray(greedy_value))
