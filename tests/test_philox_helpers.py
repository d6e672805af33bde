"""The replay helpers of tests/test_gpu_philox_paths.py, held on the CPU: philox_np.randint against
Python integers, and the oracle's Thompson vote (policy_action sample=False) against a direct
np.bincount computation."""
import numpy as np

from oracle import dpt_oracle as O
import philox_np


def test_randint_is_the_multiply_shift_of_one_word():
    """philox_np.randint == (word_w * n) >> 32 in Python integers (csrc/dpt_env.hip philox_randint),
    for every word, n in {1, 5, 7, 10}, tasks on both sides of 2^32; results lie in [0, n), and a
    word of 2^32 - 1 gives n - 1 (the product never reaches n * 2^32)."""
    seed, step, stream = 0x2545F4914F6CDD1D, 41, 2
    tasks = np.concatenate([np.arange(300), 2 ** 32 - 3 + np.arange(6)])
    words = philox_np.philox(seed, step, tasks, stream)
    for n in (1, 5, 7, 10):
        for w in range(4):
            got = philox_np.randint(seed, step, tasks, stream, w, n)
            assert got.dtype == np.int64 and got.shape == tasks.shape
            assert got.tolist() == [(int(x) * n) >> 32 for x in words[w]]
            assert got.min() >= 0 and got.max() < n
        assert ((2 ** 32 - 1) * n) >> 32 == n - 1
    # the words differ (a replay on the wrong word is a different replay), and n = 10 reaches both ends
    x, y = (philox_np.randint(seed, step, tasks, stream, w, 10) for w in (0, 1))
    assert not np.array_equal(x, y)
    assert x.min() == 0 and x.max() == 9


def test_philox_broadcasts_over_step_task_and_stream():
    """philox_np.philox on arrays of steps, tasks and streams == one scalar-key call per entry (the
    replay tables of the vote are built in one call); the vote's counters (c0 + h) * 128 + s and
    steps past 2^32, whose high word enters the counter with the task's."""
    seed = 0x2545F4914F6CDD1D
    steps = np.array([0, 37 * 128 + 99, 2 ** 32 + 5, 2 ** 40 + 1])
    tasks = np.array([0, 7, 2 ** 32 - 1, 2 ** 32, 2 ** 33 + 3])
    streams = np.array([1, 2, 16, 47])
    got = philox_np.philox(seed, steps[:, None, None], tasks[None, :, None], streams[None, None, :])
    assert all(w.shape == (4, 5, 4) and w.dtype == np.uint64 and w.max() < 2 ** 32 for w in got)
    for a, st in enumerate(steps):
        for c, sm in enumerate(streams):
            one = philox_np.philox(seed, int(st), tasks, int(sm))
            assert all(np.array_equal(got[w][a, :, c], one[w]) and one[w].shape == tasks.shape for w in range(4))
    u = philox_np.uniform(seed, steps[:, None], tasks[None], 2)
    assert np.array_equal(u[2], philox_np.uniform(seed, int(steps[2]), tasks, 2)) and 0 <= u.min() and u.max() < 1


def _vote_ctx(rs, N, A, h):
    acts = rs.randint(0, A, (N, h))
    rews = rs.normal(0.5, 0.5, (N, h))
    return acts, rews


def _posterior(acts, rews, A, ts):
    """Thompson's posterior mean / std per (task, arm), one arm at a time (update_posterior,
    ctrls/ctrl_bandit.py:184-194); held to the oracle's sampled path by the caller."""
    N = len(acts)
    var, pm, pv = ts["std"] ** 2, ts["prior_mean"], ts["prior_var"]
    m, s = np.full((N, A), pm), np.full((N, A), np.sqrt(pv))
    for i in range(N):
        for k in range(A):
            r = rews[i][acts[i] == k]
            if len(r):
                w = var / (var + len(r) * pv)
                m[i, k] = w * pm + (1 - w) * np.mean(r)
                s[i, k] = np.sqrt(1 / (1 / pv + len(r) / var))
    return m, s


def test_thompson_vote_equals_bincount():
    """policy_action('thompson', sample=False): 100 posterior draws (100, N, A), the first most
    frequent argmax -- against np.bincount per task on random draws, and on a constructed tie."""
    rs = np.random.RandomState(5)
    ts = dict(std=0.3, prior_mean=0.5, prior_var=1 / 12.0)
    for N, A, h in ((7, 5, 12), (4, 20, 0), (3, 32, 50), (5, 1, 3)):
        acts, rews = _vote_ctx(rs, N, A, h)
        g = rs.normal(size=(100, N, A))
        got = O.policy_action("thompson", acts, rews, A, ts=ts, ts_g=g, sample=False)
        m, s = _posterior(acts, rews, A, ts)
        want = [int(np.argmax(np.bincount(np.argmax(m[i] + s[i] * g[:, i], axis=-1), minlength=A)))
                for i in range(N)]
        assert got.tolist() == want
        # the sampled path is untouched by the flag's default
        assert np.array_equal(O.policy_action("thompson", acts, rews, A, ts=ts, ts_g=g[0]),
                              np.argmax(m + s * g[0], axis=-1))
    # a frequency tie: with an empty context every arm has the prior, so the draw's own argmax wins;
    # arms 3 and 1 get 40 votes each and arm 4 twenty: the first most frequent arm is 1, and the
    # order of the draws does not matter
    A = 5
    winners = np.array([3] * 40 + [1] * 40 + [4] * 20)
    for order in (np.arange(100), np.arange(100)[::-1], rs.permutation(100)):
        g = np.zeros((100, 2, A))
        g[np.arange(100), 0, winners[order]] = 1.0
        g[np.arange(100), 1, (winners[order] + 1) % A] = 1.0  # task 1: arms 4, 2 and 0 -> arm 2
        got = O.policy_action("thompson", np.zeros((2, 0), np.int64), np.zeros((2, 0)), A, ts=ts, ts_g=g,
                              sample=False)
        assert got.tolist() == [1, 2]


def test_policy_rollout_passes_vote_draws_through():
    """bandit_policy_rollout hands ts_g[h] (100, N, A) to policy_action unchanged: the rollout equals
    the per-step calls chained by hand."""
    rs = np.random.RandomState(6)
    N, A, H = 4, 5, 6
    ts = dict(std=0.3, prior_mean=0.5, prior_var=1 / 12.0)
    means, g, tg = rs.uniform(0, 1, (N, A)), rs.normal(size=(H, N)), rs.normal(size=(H, 100, N, A))
    ref = O.bandit_policy_rollout("thompson", means, H, 0.3, g, ts=ts, ts_g=tg, sample=False)
    acts, rews = np.zeros((N, H), np.int64), np.zeros((N, H))
    for h in range(H):
        acts[:, h] = O.policy_action("thompson", acts[:, :h], rews[:, :h], A, ts=ts, ts_g=tg[h], sample=False)
        rews[:, h] = O.bandit_reward(means, acts[:, h], g[h], 0.3)
    assert np.array_equal(ref["actions"], acts) and np.array_equal(ref["rewards"], rews)
    assert len(np.unique(acts)) > 1
