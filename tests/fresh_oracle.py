"""numpy restatement of the fresh-task generator (csrc/dpt_fresh.hip, include/dpt_hip.h "fresh-task training
step") on tests/philox_np.py: a test helper.  Every quantity of sample ``first_task + b`` from (seed, its
global index) alone, vectorised over the samples and the steps."""
import numpy as np

import philox_np as P

STREAM_REWARD, STREAM_ROLLIN, STREAM_TASK = 1, 2, 5
COV_GRID = np.array([0.0, .1, .2, .3, .4, .5, .6, .7, .8, .9, 1.0])  # collect_data.py's cov choices
GAUSSIAN, BERNOULLI = 0, 1


BIG = 2 ** 33 + 5  # a first_task whose high word reaches the Philox counter
# The generator cases of tests/test_gpu_fresh.py: (seed, A, H, batch, first_task, type, var).  Every value
# of every axis of the issue (A 2 / 5 / 32, H 1 / 7 / 300, batch 1 / 3 / 64, first_task 0 / 2^33 + 5, both
# types, var 0 / 0.3) occurs, the large ones together; tests/test_fresh_host.py holds each seed to zero
# rollin draws within 1e-12 of a cdf step (the seeds were chosen so).
BANDIT_CASES = [
    (101, 2, 1, 1, 0, GAUSSIAN, 0.0),
    (102, 5, 7, 3, BIG, GAUSSIAN, 0.3),
    (103, 32, 300, 64, 0, GAUSSIAN, 0.3),
    (104, 5, 300, 3, BIG, BERNOULLI, 0.3),
    (105, 32, 7, 64, BIG, BERNOULLI, 0.0),
    (106, 2, 300, 64, BIG, GAUSSIAN, 0.3),
    (107, 5, 1, 64, 0, BERNOULLI, 0.3),
    (108, 32, 1, 3, 0, GAUSSIAN, 0.0),
    (109, 2, 7, 1, BIG, BERNOULLI, 0.3),
    (110, 5, 300, 64, 0, GAUSSIAN, 0.0),
]
# (seed, dim, H, batch, first_task, G, with a 120-row permutation list)
DARKROOM_CASES = [
    (201, 2, 1, 1, 0, 1, False),
    (202, 10, 7, 3, BIG, 80, True),
    (203, 10, 300, 64, 0, 80, False),
    (204, 2, 300, 64, BIG, 1, True),
    (205, 10, 7, 64, 0, 1, True),
    (206, 2, 7, 3, BIG, 80, False),
]
# the batch-independence cases: tasks [0, 64)
SPLIT_BANDIT = (111, 5, 7, GAUSSIAN, 0.3)  # seed, A, H, type, var
SPLIT_DARKROOM = (207, 10, 7, 80, True)    # seed, dim, H, G, perms


def goal_list(dim, G):
    """G goals of a dim x dim room (repeats when G exceeds the grid), (G, 2) int32"""
    g = np.array([[(j, i) for i in range(dim)] for j in range(dim)]).reshape(-1, 2)
    np.random.RandomState(G).shuffle(g)
    return g[np.arange(G) % len(g)].astype(np.int32)


def perm_list():
    """the 120 permutations of the five actions, (120, 5) int32"""
    import itertools
    return np.array(list(itertools.permutations(range(5))), np.int32)


def tasks_of(first_task, n):
    return np.int64(first_task) + np.arange(n, dtype=np.int64)


def bandit_task(seed, first_task, n, A):
    """means (n, A), the Dirichlet part p (n, A), cov index (n), rand index (n), probs (n, A)"""
    t = tasks_of(first_task, n)[:, None]
    k = np.arange(A)[None, :]
    means = P.uniform(seed, k, t, STREAM_TASK)
    e = -np.log(1.0 - P.uniform(seed, A + k, t, STREAM_TASK))
    total = np.zeros(n)
    for j in range(A):  # the device sums in index order
        total = total + e[:, j]
    p = e / total[:, None]
    ci = P.randint(seed, 2 * A, t[:, 0], STREAM_TASK, 0, 11)
    ri = P.randint(seed, 2 * A, t[:, 0], STREAM_TASK, 1, A)
    cov = COV_GRID[ci][:, None]
    onehot = (k == ri[:, None]).astype(np.float64)
    probs = (1 - cov) * p + cov * onehot
    return dict(means=means, p=p, cov_index=ci, rand_index=ri, probs=probs)


def cdf_of(probs):
    """c_k / total of rollin_bandit_arm: the values the uniform is compared with, (n, A)"""
    n, A = probs.shape
    total = np.zeros(n)
    for j in range(A):
        total = total + probs[:, j]
    c, out = np.zeros(n), np.empty_like(probs)
    for j in range(A):
        c = c + probs[:, j]
        out[:, j] = c / total
    return out


def bandit_rollin(seed, first_task, means, probs, H):
    """arms (n, H) int and the rollin uniforms (n, H) of the given tasks"""
    n, A = means.shape
    t = tasks_of(first_task, n)[:, None]
    h = np.arange(H)[None, :]
    u = P.uniform(seed, h, t, STREAM_ROLLIN)
    cdf = cdf_of(probs)
    arms = np.minimum((cdf[:, None, :] <= u[:, :, None]).sum(-1), A - 1)
    return arms, u


def bandit_rewards(seed, first_task, means, arms, bandit_type, var, normals=None):
    """the reward of every step given its arm (n, H); ``normals`` (n, H): the standard normals as the
    library reports them (dpt_hip.draw: the kernels' own log / cospi, within 1e-12 of philox_np.normal),
    which make the Gaussian reward bit-exact"""
    n, H = arms.shape
    t = tasks_of(first_task, n)[:, None]
    h = np.arange(H)[None, :]
    mean = np.take_along_axis(means, arms, 1)
    if bandit_type == BERNOULLI:
        return (P.uniform(seed, h, t, STREAM_REWARD) < mean).astype(np.float64)
    g = P.normal(seed, h, t, STREAM_REWARD) if normals is None else normals
    return mean + (0.0 + var * g)


def first_argmax(means):
    """the label: the first index of the row maximum (a later equal mean does not replace it)"""
    best = np.zeros(len(means), np.int64)
    for k in range(1, means.shape[1]):
        best = np.where(means[:, k] > means[np.arange(len(means)), best], k, best)
    return best


def count_near(u, cdf, eps=1e-12):
    """how many of the uniforms u (n, H) lie within eps of a cdf step (n, A) of their task"""
    return int((np.abs(u[:, :, None] - cdf[:, None, :]) < eps).sum())


def near_ties(seed, first_task, n, A, H, eps=1e-12):
    """how many rollin draws lie within eps of a cdf step of their task (the arm comparison is strict
    only where there are none: the device's probs may differ from numpy's in the last bits)"""
    tk = bandit_task(seed, first_task, n, A)
    t = tasks_of(first_task, n)[:, None]
    u = P.uniform(seed, np.arange(H)[None, :], t, STREAM_ROLLIN)
    return count_near(u, cdf_of(tk["probs"]), eps)


def bandit_tokens(arms, rewards, A):
    """(n, 1 + H, A + 3) float32: row 0 = [1 | 0 ...], row 1 + h = [1 | onehot(arm) | 1 | float32(r)]"""
    n, H = arms.shape
    tok = np.zeros((n, 1 + H, A + 3), np.float32)
    tok[:, :, 0] = 1
    tok[:, 1:, 1:1 + A] = np.eye(A, dtype=np.float32)[arms]
    tok[:, 1:, 1 + A] = 1
    tok[:, 1:, 2 + A] = rewards.astype(np.float32)
    return tok


def darkroom_opt(x, y, gx, gy, perm):
    """the expert action at (x, y) (envs/darkroom_env.py:69-82), as its index inside each row of perm"""
    a = np.where(x < gx, 0, np.where(x > gx, 1, np.where(y < gy, 2, np.where(y > gy, 3, 4))))
    if perm is None:
        return a
    return (perm == a[:, None]).argmax(1)


def darkroom(seed, first_task, n, H, dim, goals, perms=None):
    """goal index, goal, perm index, perm, query, label and the tokens (n, 1 + H, 10) float32"""
    goals = np.asarray(goals).reshape(-1, 2)
    t = tasks_of(first_task, n)
    gi = P.randint(seed, 0, t, STREAM_TASK, 0, len(goals))
    goal = goals[gi]
    pi = perm = None
    if perms is not None:
        perms = np.asarray(perms).reshape(-1, 5)
        pi = P.randint(seed, 0, t, STREAM_TASK, 1, len(perms))
        perm = perms[pi]
    q = np.stack([P.randint(seed, H, t, STREAM_ROLLIN, w, dim) for w in (0, 1)], 1)
    opt = darkroom_opt(q[:, 0], q[:, 1], goal[:, 0], goal[:, 1], perm)
    h = np.arange(H)[None, :]
    x, y = (P.randint(seed, h, t[:, None], STREAM_ROLLIN, w, dim) for w in (0, 1))
    a = P.randint(seed, h, t[:, None], STREAM_ROLLIN, 2, 5)
    ea = a if perm is None else np.take_along_axis(perm, a, 1)
    nx = np.clip(x + (ea == 0) - (ea == 1), 0, dim - 1)
    ny = np.clip(y + (ea == 2) - (ea == 3), 0, dim - 1)
    r = (nx == goal[:, :1]) & (ny == goal[:, 1:])
    tok = np.zeros((n, 1 + H, 10), np.float32)
    tok[:, 0, :2] = q
    tok[:, 1:, 0], tok[:, 1:, 1] = x, y
    tok[:, 1:, 2:7] = np.eye(5, dtype=np.float32)[a]
    tok[:, 1:, 7], tok[:, 1:, 8], tok[:, 1:, 9] = nx, ny, r
    return dict(goal_index=gi, goal=goal, perm_index=pi, perm=perm, query=q, opt_action=opt, tokens=tok,
                targets=np.eye(5, dtype=np.float32)[opt])
