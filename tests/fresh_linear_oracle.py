"""numpy float64 restatement of the linear bandit's fresh-task generator (csrc/dpt_fresh_linear.hip,
include/dpt_hip.h "fresh-task training step: the linear bandit") on tests/philox_np.py: a test helper.

The standard normals come from ``philox_np.normal`` or, with ``draw`` given (``dpt_hip.draw``), from the
library itself: the kernels' own log / cospi lie within 1e-12 of numpy's, and fed the library's normals every
other operation here (+, *, /, sqrt in fp64, in the kernel's order) is bit-exact.  The Thompson chain loops
over the steps and is vectorised over the tasks."""
import numpy as np

import fresh_oracle as FO
import philox_np as P

STREAM_REWARD, STREAM_ROLLIN, STREAM_TASK, STREAM_POLICY = 1, 2, 5, 16
THOMPSON, UNIFORM = 0, 1
CHUNK = 32     # kLinChunk: steps per chunk of the kernel's Thompson rollin
TABLE = 1024   # kLinTable: counts above it take the posterior from arithmetic, not from the LDS table
BIG = 2 ** 33 + 5  # a first_task whose high word reaches the Philox counter

# (seed, first_task, n, A, d, H, var): the issue's three cases ...
CASES = [
    (301, 0, 8, 20, 2, 40, 0.3),
    (302, BIG, 5, 5, 3, 300, 0.3),
    (303, 7, 6, 32, 8, 17, 0.1),
]
# ... and the further horizons: none, one step, around one chunk and past two; and one arm pulled more often
# than the table is long (A = 1: every step pulls it)
H_CASES = [(310 + i, 3, 3, 7, 3, H, 0.3) for i, H in enumerate((0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1))]
H_CASES.append((320, 1, 2, 1, 1, TABLE + 6, 0.3))
SPLIT = (330, 9, 2, 70, 0.3)  # batch independence over tasks [0, 64): seed, A, d, H, var


def case_id(c):
    return "seed%d-ft%d-n%d-A%d-d%d-H%d-var%g" % c


def arms_of(A, d):
    """the arm features of collect_data.py's generate_linear_bandit_histories"""
    return np.random.RandomState(seed=1234).normal(size=(A, d)) / np.sqrt(d)


def normals(seed, counters, first_task, n, stream, draw=None):
    """standard normals (n, len(counters)) of tasks first_task .. first_task + n - 1 at the given counters"""
    counters = np.asarray(counters, np.int64)
    if draw is None:
        return P.normal(seed, counters[None, :], FO.tasks_of(first_task, n)[:, None], stream).reshape(n, len(counters))
    if len(counters) == 0:
        return np.zeros((n, 0))
    return np.stack([draw(1, seed, int(c), first_task, n, stream).cpu().numpy() for c in counters], 1)


def task(seed, first_task, n, arms, draw=None):
    """theta (n, d) = normal / sqrt(d), means (n, A) = arms @ theta as multiply-then-add in index order, and
    the label: the first argmax of means"""
    arms = np.asarray(arms, np.float64)
    A, d = arms.shape
    theta = normals(seed, np.arange(d), first_task, n, STREAM_TASK, draw) / np.sqrt(float(d))
    means = arms[None, :, 0] * theta[:, None, 0]
    for p in range(1, d):
        means = means + arms[None, :, p] * theta[:, None, p]
    return dict(theta=theta, means=means, opt_action=FO.first_argmax(means))


def chain_normals(seed, first_task, n, A, H, draw=None):
    """the Thompson rollin's draws: the posterior normals g (n, H, A) and the reward normals (n, H)"""
    g = np.stack([normals(seed, np.arange(H), first_task, n, STREAM_POLICY + k, draw) for k in range(A)], 2)
    return g.reshape(n, H, A), normals(seed, np.arange(H), first_task, n, STREAM_REWARD, draw)


def posterior_std(count, var):
    """s as a function of the count alone (1 before any pull)"""
    variance = var * var
    return np.where(count > 0, np.sqrt(1.0 / (1.0 + count / variance)), 1.0)


def gaps(v):
    """largest minus second-largest entry of every row of v (..., A); inf where A == 1"""
    if v.shape[-1] < 2:
        return np.full(v.shape[:-1], np.inf)
    top = np.sort(v, -1)
    return top[..., -1] - top[..., -2]


def thompson(means, var, g, g_reward):
    """The adaptive rollin of every task: actions (n, H), rewards (n, H) fp64, the counts before each step
    and after the last (n, H + 1, A), the posterior stds used at each step (n, H, A) and the minimum over all
    tasks and steps of the gap between the two largest v."""
    n, A = means.shape
    H = g.shape[1]
    variance = var * var
    cnt, S = np.zeros((n, A)), np.zeros((n, A))
    m, s = np.zeros((n, A)), np.ones((n, A))
    rows = np.arange(n)
    actions, rewards = np.zeros((n, H), np.int64), np.zeros((n, H))
    counts, stds = np.zeros((n, H + 1, A), np.int64), np.zeros((n, H, A))
    gap = np.inf
    for h in range(H):
        counts[:, h], stds[:, h] = cnt, s
        v = m + s * g[:, h]
        gap = min(gap, float(gaps(v).min()))
        a = v.argmax(1)  # the first index of the maximum
        r = means[rows, a] + (0.0 + var * g_reward[:, h])
        na = cnt[rows, a] + 1
        Sa = S[rows, a] + r
        w = variance / (variance + na * 1.0)
        cnt[rows, a], S[rows, a] = na, Sa
        m[rows, a] = (1.0 - w) * (Sa / na)
        s[rows, a] = np.sqrt(1.0 / (1.0 + na / variance))
        actions[:, h], rewards[:, h] = a, r
    counts[:, H] = cnt
    return dict(actions=actions, rewards=rewards, counts=counts, stds=stds, gap=gap)


def min_gap(case):
    """the case's minimum gap between the largest and second-largest v_k, on philox_np's normals"""
    seed, ft, n, A, d, H, var = case
    t = task(seed, ft, n, arms_of(A, d))
    return thompson(t["means"], var, *chain_normals(seed, ft, n, A, H))["gap"]


def uniform_policy(seed, first_task, n, A, d):
    """the bandit's behaviour policy (fresh_oracle.bandit_task) on the task counters behind theta: d + k -> e_k,
    d + A -> word 0 the cov-grid index, word 1 the point-mass arm"""
    t = FO.tasks_of(first_task, n)[:, None]
    k = np.arange(A)[None, :]
    e = -np.log(1.0 - P.uniform(seed, d + k, t, STREAM_TASK))
    total = np.zeros(n)
    for j in range(A):
        total = total + e[:, j]
    p = e / total[:, None]
    ci = P.randint(seed, d + A, t[:, 0], STREAM_TASK, 0, 11)
    ri = P.randint(seed, d + A, t[:, 0], STREAM_TASK, 1, A)
    cov = FO.COV_GRID[ci][:, None]
    probs = (1 - cov) * p + cov * (k == ri[:, None]).astype(np.float64)
    return dict(p=p, cov_index=ci, rand_index=ri, probs=probs)


def uniform_near_ties(case, eps=1e-12):
    """rollin uniforms within eps of a cdf step of their task's behaviour policy"""
    seed, ft, n, A, d, H, _ = case
    u = P.uniform(seed, np.arange(H)[None, :], FO.tasks_of(ft, n)[:, None], STREAM_ROLLIN).reshape(n, H)
    return FO.count_near(u, FO.cdf_of(uniform_policy(seed, ft, n, A, d)["probs"]), eps)
