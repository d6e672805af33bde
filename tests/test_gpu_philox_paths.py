"""The kernels' own Philox draws, held to a numpy Philox replay.

dpt_rollout_policy, dpt_rollin_bandit and dpt_rollin_darkroom each have two paths: injected draws
(pinned to the reference's fixtures and the float64 oracle elsewhere) and
Philox(seed, (counter, first_task + i, stream)) computed in the kernel, the only path production
runs take (collect_data, evals/eval_bandit).  Here every Philox run is replayed: the same draws are
rebuilt outside the kernel from the keys that include/dpt_hip.h and the wrapper docstrings give,
injected, and the outputs must be bit-identical -- to the injected run, to the oracle on those
draws, across task shards, and across a split of the steps.  Uniforms and integers come from
tests/philox_np.py (bit-exact); normals are taken as the library reports them (dpt_draw: the
kernels' own log / cospi) and held to philox_np.normal at 1e-12, the module's only tolerance.
Replays built on a wrong counter, stream, task or word must differ.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import dpt_oracle as O
import philox_np

pytestmark = pytest.mark.gpu

SEED = 0x2545F4914F6CDD1D  # 62 bits: both key words in use
C0 = 37  # Philox counter of step 0
N, H, H1 = 11, 40, 13  # tasks, steps, steps of the first call of the continuation split
H_VOTE = 40  # steps of the 100-draw vote (its injected array is H_VOTE x 100 x N x A doubles)
ARMS = (5, 20, 32)  # 20: three passes of the 8-arms-at-a-time loop; 32 = kMaxA, stream id 47
KMAX = 32
FIRST_TASKS = (0, 2 ** 32 - 3)  # the second puts tasks on both sides of 2^32: the high task word
VAR = 0.3
TS = dict(ts_std=0.3, ts_prior_mean=0.5, ts_prior_var=1 / 12.0)
OTS = dict(std=0.3, prior_mean=0.5, prior_var=1 / 12.0)
STREAM_REWARD, STREAM_ROLLIN, STREAM_POLICY = 1, 2, 16  # include/dpt_hip.h DPT_STREAM_*
OUT = ("actions", "rewards", "arm_value")

# name: (kernel policy, kernel arguments, oracle policy, oracle arguments, Bernoulli rewards)
POLICIES = {
    "emp-online": ("POLICY_EMP", dict(online=True), "emp", dict(online=True), False),
    "emp-offline": ("POLICY_EMP", dict(online=False), "emp", dict(online=False), False),
    "ucb": ("POLICY_UCB", dict(c=1.0), "ucb", dict(c=1.0), False),
    "ucb-bernoulli": ("POLICY_UCB", dict(c=1.0), "ucb", dict(c=1.0), True),
    "lcb": ("POLICY_LCB", dict(c=0.8), "lcb", dict(c=0.8), False),
    "thompson": ("POLICY_THOMPSON", dict(sample=True, **TS), "thompson", dict(ts=OTS), False),
    "vote": ("POLICY_THOMPSON", dict(sample=False, **TS), "thompson", dict(ts=OTS, sample=False), False),
    "linucb-d2": ("POLICY_LINUCB", dict(c=1.0), None, None, False),
    "linucb-d8": ("POLICY_LINUCB", dict(c=1.0), None, None, False),
    "opt": ("POLICY_OPT", {}, "opt", {}, False),
}
ft_id = lambda ft: "task0" if ft == 0 else "task2p32"  # noqa: E731


def dh():
    import dpt_hip
    dpt_hip.device()
    return dpt_hip


def test_stream_ids_are_the_headers():
    from dpt_hip import _lib
    assert (_lib.STREAM_REWARD, _lib.STREAM_ROLLIN, _lib.STREAM_POLICY) == (STREAM_REWARD, STREAM_ROLLIN,
                                                                             STREAM_POLICY)


# ----------------------------------------------------------------------------- draws
def device_draws(kind, seed, counters, first_task, n, streams):
    """(len(counters), len(streams), n) float64: one dpt_draw (the entry dpt_hip.draw wraps) per
    (counter, stream), tasks first_task .. first_task + n, written into one device tensor and copied
    back once."""
    d = dh()
    from dpt_hip import _lib
    out = torch.empty((len(counters), len(streams), n), dtype=torch.float64, device=d.device())
    base, st = out.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    row = 0
    for c in counters:
        for s in streams:
            _lib.call("dpt_draw", int(kind), int(seed), int(c), int(first_task), int(n), int(s),
                      ctypes.c_void_p(base + 8 * n * row), st)
            row += 1
    return out.cpu().numpy()


def hold(g, ref):
    """device normals against philox_np.normal at the project's bar (tests/test_gpu_kernels.py)"""
    assert g.shape == ref.shape
    np.testing.assert_allclose(g, ref, rtol=1e-12, atol=1e-12)


# every table carries one counter / stream / task more than the runs read, so that a replay on a
# wrong key is a shifted slice of the same table
@functools.lru_cache(maxsize=None)
def reward_draws(ft):
    """normals and uniforms (H + 1, N + 1) at (C0 + h, ft + i, STREAM_REWARD)"""
    cs, tasks = C0 + np.arange(H + 1), ft + np.arange(N + 1)
    g = device_draws(1, SEED, cs, ft, N + 1, [STREAM_REWARD])[:, 0]
    hold(g, philox_np.normal(SEED, cs[:, None], tasks[None], STREAM_REWARD))
    return g, philox_np.uniform(SEED, cs[:, None], tasks[None], STREAM_REWARD)


@functools.lru_cache(maxsize=None)
def thompson_draws(ft):
    """posterior normals (H, N + 1, KMAX + 1) at (C0 + h, ft + i, STREAM_POLICY + k)"""
    cs, tasks, streams = C0 + np.arange(H), ft + np.arange(N + 1), STREAM_POLICY + np.arange(KMAX + 1)
    g = device_draws(1, SEED, cs, ft, N + 1, streams)
    hold(g, philox_np.normal(SEED, cs[:, None, None], tasks[None, None], streams[None, :, None]))
    return np.ascontiguousarray(g.transpose(0, 2, 1))


@functools.lru_cache(maxsize=None)
def vote_draws(ft):
    """the vote's normals (H_VOTE, 100, N + 1, KMAX + 1) at ((C0 + h) * 128 + s, ft + i, STREAM_POLICY + k)"""
    cs = ((C0 + np.arange(H_VOTE))[:, None] * 128 + np.arange(100)[None]).reshape(-1)
    tasks, streams = ft + np.arange(N + 1), STREAM_POLICY + np.arange(KMAX + 1)
    g = device_draws(1, SEED, cs, ft, N + 1, streams)
    hold(g, philox_np.normal(SEED, cs[:, None, None], tasks[None, None], streams[None, :, None]))
    return np.ascontiguousarray(g.reshape(H_VOTE, 100, KMAX + 1, N + 1).transpose(0, 1, 3, 2))


def linucb_uniforms(ft):
    """LinUCB's first-arm uniforms (N + 1,) at (C0, ft + i, STREAM_POLICY)"""
    return philox_np.uniform(SEED, C0, ft + np.arange(N + 1), STREAM_POLICY)


def test_device_normals_equal_numpy_philox():
    """dpt_hip.draw(1, ...) against philox_np.normal (1e-12) at the keys only this module uses:
    stream STREAM_POLICY + k, the vote's counter (C0 + h) * 128 + s, tasks on both sides of 2^32;
    the uniforms there bit for bit."""
    d = dh()
    ft = FIRST_TASKS[1]
    tasks = ft + np.arange(N)
    assert tasks[0] < 2 ** 32 <= tasks[-1]
    for k in (0, 19, 31):
        for c in (C0, C0 + H - 1) + tuple((C0 + h) * 128 + s for h in (0, 39) for s in (0, 63, 99)):
            g = d.draw(1, SEED, c, ft, N, STREAM_POLICY + k).cpu().numpy()
            hold(g, philox_np.normal(SEED, c, tasks, STREAM_POLICY + k))
            u = d.draw(0, SEED, c, ft, N, STREAM_POLICY + k).cpu().numpy()
            assert np.array_equal(u, philox_np.uniform(SEED, c, tasks, STREAM_POLICY + k))
    # the high task word is in the key: tasks 2^32 further on share the low word and draw something else
    lo = d.draw(1, SEED, C0, ft, N, STREAM_POLICY).cpu().numpy()
    hi = d.draw(1, SEED, C0, ft + 2 ** 32, N, STREAM_POLICY).cpu().numpy()
    assert not np.array_equal(lo, hi)
    hold(hi, philox_np.normal(SEED, C0, tasks + 2 ** 32, STREAM_POLICY))


# ----------------------------------------------------------------------------- A. dpt_rollout_policy
@functools.lru_cache(maxsize=None)
def bandit_tasks(name, A):
    """(means (N, A), arms (A, d) or None)"""
    if name.startswith("linucb"):
        d_ = int(name[-1])
        rs = np.random.RandomState(1000 * d_ + A)
        arms = rs.normal(size=(A, d_)) / np.sqrt(d_)
        return O.linear_means(arms, rs.normal(size=(N, d_)) / np.sqrt(d_)), arms
    return np.random.RandomState(100 + A).uniform(0, 1, (N, A)), None


def steps_of(name):
    return H_VOTE if name == "vote" else H


def replay_draws(name, A, ft, lo=0, n=N, h0=0, steps=None, dc=0, ds=0, dt_reward=0, dt_policy=0):
    """The draws of tasks lo .. lo + n, steps h0 .. h0 + steps in the layouts dpt_hip.rollout_policy
    documents: noise (steps, n); policy_noise (steps, n, A) for Thompson, (steps, 100, n, A) for the
    vote, (n,) for LinUCB.  dc / ds / dt_*: the same with the reward counter, the policy stream or
    the task off by that much (the wrong keys of test_replay_can_fail)."""
    steps = steps_of(name) - h0 if steps is None else steps
    g, u = reward_draws(ft)
    noise = (u if POLICIES[name][4] else g)[h0 + dc:h0 + dc + steps, lo + dt_reward:lo + dt_reward + n]
    ts = slice(lo + dt_policy, lo + dt_policy + n)
    if name == "thompson":
        pn = thompson_draws(ft)[h0:h0 + steps, ts, ds:ds + A]
    elif name == "vote":
        pn = vote_draws(ft)[h0:h0 + steps, :, ts, ds:ds + A]
    elif name.startswith("linucb"):
        pn = linucb_uniforms(ft)[ts]
    else:
        pn = None
    assert noise.shape == (steps, n)
    return dict(noise=noise, policy_noise=pn)


def run(name, A, ft, lo=0, n=N, h0=0, steps=None, inject=None, ctx=None):
    """One dpt_hip.rollout_policy call for tasks lo .. lo + n, steps h0 .. h0 + steps (ctx: the
    (actions, rewards) of steps 0 .. h0).  inject None: the kernel's own Philox draws (seed, counter
    C0 + h0, first_task ft + lo); else the injected arrays and no key at all."""
    d = dh()
    code, kw, _, _, bern = POLICIES[name]
    means, arms = bandit_tasks(name, A)
    steps = steps_of(name) - h0 if steps is None else steps
    key = dict(seed=SEED, counter=C0 + h0, first_task=ft + lo) if inject is None else inject
    if ctx is not None:
        key = dict(key, ctx_actions=ctx[0], ctx_rewards=ctx[1])
    if arms is not None:
        key = dict(key, arms=arms)
    o = d.rollout_policy(getattr(d, code), means[lo:lo + n], steps, VAR,
                         d.BANDIT_BERNOULLI if bern else d.BANDIT_GAUSSIAN, **kw, **key)
    return {k: o[k].cpu().numpy() for k in OUT}


@functools.lru_cache(maxsize=None)
def philox_run(name, A, ft):
    return run(name, A, ft)


def assert_same(got, ref, what):
    for k in OUT:
        assert got[k].shape == ref[k].shape, (what, k)
        assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:4].tolist())


def cat(a, b, axis):
    return {k: np.concatenate([a[k], b[k]], axis) for k in OUT}


CASES = [pytest.param(name, A, ft, id=f"{name}-A{A}-{ft_id(ft)}")
         for name in POLICIES for A in ARMS for ft in FIRST_TASKS]


@pytest.mark.parametrize("name,A,ft", CASES)
def test_policy_philox_equals_injected_replay(name, A, ft):
    """Nothing injected (seed, counter, first_task) == noise and policy_noise injected, rebuilt from
    the documented keys: reward draws at (C0 + h, ft + i, STREAM_REWARD), Thompson's at stream
    STREAM_POLICY + k, the vote's at counter (C0 + h) * 128 + s, LinUCB's first arm at
    (C0, ft + i, STREAM_POLICY).  Bit for bit in actions, rewards and arm values."""
    phil = philox_run(name, A, ft)
    assert_same(run(name, A, ft, inject=replay_draws(name, A, ft)), phil, name)
    assert phil["actions"].min() >= 0 and phil["actions"].max() < A
    if name in ("emp-online", "ucb", "ucb-bernoulli"):  # unseen arms first, and H >= A: every arm is played
        assert len(np.unique(phil["actions"])) == A
    elif name in ("thompson", "vote") or name.startswith("linucb"):  # the policy's draws choose among arms
        assert len(np.unique(phil["actions"])) > 1


@pytest.mark.parametrize("name,A,ft", [c for c in CASES if not c.values[0].startswith("linucb")])
def test_policy_philox_equals_oracle(name, A, ft):
    """The Philox run == the float64 numpy oracle (oracle/dpt_oracle.py bandit_policy_rollout) on
    the rebuilt draws; the vote through policy_action's sample=False.  LinUCB is left out: numpy's
    BLAS rounds it host-dependently (test_gpu_dropin.py test_policy_wave_kernel_vs_oracle)."""
    _, _, oname, okw, bern = POLICIES[name]
    means, _ = bandit_tasks(name, A)
    dr = replay_draws(name, A, ft)
    Hn = steps_of(name)
    if name == "opt":  # OptPolicy: the optimal arm every step (ctrls/ctrl_bandit.py:22-38)
        acts = np.repeat(means.argmax(1)[:, None], Hn, 1)
        rews = np.stack([O.bandit_reward(means, acts[:, h], dr["noise"][h], VAR) for h in range(Hn)], 1)
        vals = np.stack([O.arm_value(means, acts[:, h]) for h in range(Hn)], 1)
    else:
        ref = O.bandit_policy_rollout(oname, means, Hn, VAR, dr["noise"], bernoulli=bern, ts_g=dr["policy_noise"],
                                      **okw)
        acts, rews, vals = ref["actions"], ref["rewards"], ref["cum_means"].T
    assert_same(philox_run(name, A, ft), dict(actions=acts, rewards=rews, arm_value=vals), name)


@pytest.mark.parametrize("name,A,ft", CASES)
def test_policy_philox_is_shard_invariant(name, A, ft):
    """The 11-task run == a 4-task run at first_task and a 7-task run at first_task + 4."""
    assert_same(cat(run(name, A, ft, lo=0, n=4), run(name, A, ft, lo=4, n=7), 0), philox_run(name, A, ft), name)


@pytest.mark.parametrize("name,A,ft", [c for c in CASES if c.values[0] in ("ucb", "thompson", "vote", "linucb-d2",
                                                                          "linucb-d8")])
def test_policy_philox_continues_from_a_prefix_context(name, A, ft):
    """The per-step loop's contract at var = 0.3: H steps == H1 = 13 steps, then the rest in a call
    that gets the first call's actions and rewards as prefix context and counter = C0 + 13."""
    first = run(name, A, ft, steps=H1)
    rest = run(name, A, ft, h0=H1, ctx=(first["actions"], first["rewards"]))
    assert rest["actions"].shape == (N, steps_of(name) - H1)
    assert_same(cat(first, rest, 1), philox_run(name, A, ft), name)


@pytest.mark.parametrize("ft", FIRST_TASKS, ids=ft_id)
@pytest.mark.parametrize("name", ["thompson", "vote", "ucb", "linucb-d2"])
def test_replay_can_fail(name, ft):
    """One thing wrong in the replay and it no longer equals the Philox run: the reward draws at
    counter C0 + 1 + h; Thompson's and the vote's at stream STREAM_POLICY + k + 1; the task
    first_task + i + 1 (Thompson's and the vote's posterior draws, UCB's reward draws, LinUCB's
    first arm)."""
    A = 20
    phil = philox_run(name, A, ft)
    wrong = lambda **kw: run(name, A, ft, inject=replay_draws(name, A, ft, **kw))  # noqa: E731
    assert_same(wrong(), phil, name)  # the right keys do
    assert not np.array_equal(wrong(dc=1)["rewards"], phil["rewards"])
    if name in ("thompson", "vote"):
        assert not np.array_equal(wrong(ds=1)["actions"], phil["actions"])
        assert not np.array_equal(wrong(dt_policy=1)["actions"], phil["actions"])
    elif name == "ucb":
        assert not np.array_equal(wrong(dt_reward=1)["rewards"], phil["rewards"])
    else:
        assert not np.array_equal(wrong(dt_policy=1)["actions"][:, 0], phil["actions"][:, 0])


def test_null_workspace_is_accepted():
    """include/dpt_hip.h: dpt_policy_rollout_args.workspace is unused and may be NULL (ABI 7).  One
    dpt_rollout_policy call through the binding with the field NULL == dpt_hip.rollout_policy,
    which always hands a buffer over."""
    d = dh()
    from dpt_hip import _lib
    A, ft = 5, FIRST_TASKS[1]
    dev = d.device()
    means = torch.as_tensor(bandit_tasks("ucb", A)[0], dtype=torch.float64, device=dev).contiguous()
    acts = torch.full((N, H), -1, dtype=torch.int32, device=dev)
    rews = torch.full((N, H), float("nan"), dtype=torch.float64, device=dev)
    vals = torch.full((N, H), float("nan"), dtype=torch.float64, device=dev)
    args = _lib.PolicyRolloutArgs(N, H, A, d.POLICY_UCB, 1, d.BANDIT_GAUSSIAN, 1, 0, ft, VAR, 1.0, TS["ts_std"],
                                  TS["ts_prior_mean"], TS["ts_prior_var"], SEED, means.data_ptr(), None, None, None,
                                  None, acts.data_ptr(), rews.data_ptr(), vals.data_ptr(), 0, C0, None, None)
    assert args.workspace is None
    _lib.call("dpt_rollout_policy", ctypes.byref(args), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    got = dict(actions=acts.cpu().numpy(), rewards=rews.cpu().numpy(), arm_value=vals.cpu().numpy())
    assert_same(got, philox_run("ucb", A, ft), "null workspace")


# ----------------------------------------------------------------------------- B. dpt_rollin_bandit
ROLLIN_SEED = 0x3C6EF372FE94F82B  # 62 bits
ROLLIN_SHAPES = [(7, 37, 5), (3, 300, 20), (5, 9, 1)]  # N * H no multiple of the 256-thread block


@functools.lru_cache(maxsize=None)
def rollin_tasks(n, A):
    """(means, behaviour policies): collect_data.behaviour_policies' rows, and by hand a pure point
    mass (row 0), a row scaled by 3 (row 1: the kernel divides by the running total, as numpy's
    legacy choice does) and a row with a leading zero (row 2, where there is a second arm)."""
    import collect_data
    np.random.seed(4242 + A)
    p = collect_data.behaviour_policies(n, A)
    p[0] = 0.0
    p[0, A // 2] = 1.0
    p[1] *= 3.0
    if A > 1:
        p[2, 0] = 0.0
    return np.random.RandomState(7 + A).uniform(0, 1, (n, A)), p


@functools.lru_cache(maxsize=None)
def rollin_draws(n, Hn, ft):
    """selection uniforms at (h, ft + i, STREAM_ROLLIN); reward uniforms and normals at STREAM_REWARD;
    each (Hn, n)"""
    hs, tasks = np.arange(Hn), ft + np.arange(n)
    g = device_draws(1, ROLLIN_SEED, hs, ft, n, [STREAM_REWARD])[:, 0]
    hold(g, philox_np.normal(ROLLIN_SEED, hs[:, None], tasks[None], STREAM_REWARD))
    return (philox_np.uniform(ROLLIN_SEED, hs[:, None], tasks[None], STREAM_ROLLIN),
            philox_np.uniform(ROLLIN_SEED, hs[:, None], tasks[None], STREAM_REWARD), g)


def rollin_bandit(n, Hn, A, bern, rows=slice(None), **kw):
    d = dh()
    means, p = rollin_tasks(n, A)
    a, r = d.rollin_bandit(means[rows], p[rows], Hn, VAR, d.BANDIT_BERNOULLI if bern else d.BANDIT_GAUSSIAN, **kw)
    return a.cpu().numpy(), r.cpu().numpy()


@pytest.mark.parametrize("ft", FIRST_TASKS, ids=ft_id)
@pytest.mark.parametrize("bern", [False, True], ids=["gaussian", "bernoulli"])
@pytest.mark.parametrize("n,Hn,A", ROLLIN_SHAPES)
def test_rollin_bandit_philox_equals_replay_and_oracle(n, Hn, A, bern, ft):
    """dpt_rollin_bandit on its own draws == the run with uniforms (h, ft + i, STREAM_ROLLIN) and
    noise (STREAM_REWARD) injected == O.choice_from_uniform + O.bandit_reward / O.bernoulli_reward
    on those draws; a replay that selects on the reward stream's uniforms differs."""
    means, p = rollin_tasks(n, A)
    u_sel, u_rew, g = rollin_draws(n, Hn, ft)
    noise = u_rew if bern else g
    acts, rews = rollin_bandit(n, Hn, A, bern, seed=ROLLIN_SEED, first_task=ft)
    ia, ir = rollin_bandit(n, Hn, A, bern, uniforms=u_sel, noise=noise)
    assert np.array_equal(acts, ia) and np.array_equal(rews, ir)
    oa = O.choice_from_uniform(p[None], u_sel)  # (Hn, n)
    orw = np.stack([O.bernoulli_reward(means, oa[h], noise[h]) if bern else O.bandit_reward(means, oa[h], noise[h], VAR)
                    for h in range(Hn)])
    assert np.array_equal(acts, oa.T) and np.array_equal(rews, orw.T)
    # the hand-made rows do what they are there for (asserted on the replay)
    assert (oa[:, 0] == A // 2).all() and (A == 1 or (oa[:, 2] != 0).all())
    if A > 1:
        wa, _ = rollin_bandit(n, Hn, A, bern, uniforms=u_rew, noise=noise)
        assert not np.array_equal(wa, acts)


@pytest.mark.parametrize("ft", FIRST_TASKS, ids=ft_id)
@pytest.mark.parametrize("bern", [False, True], ids=["gaussian", "bernoulli"])
def test_rollin_bandit_philox_is_shard_invariant(bern, ft):
    """7 tasks == 3 tasks at first_task and 4 at first_task + 3."""
    n, Hn, A = ROLLIN_SHAPES[0]
    full = rollin_bandit(n, Hn, A, bern, seed=ROLLIN_SEED, first_task=ft)
    lo = rollin_bandit(n, Hn, A, bern, slice(0, 3), seed=ROLLIN_SEED, first_task=ft)
    hi = rollin_bandit(n, Hn, A, bern, slice(3, 7), seed=ROLLIN_SEED, first_task=ft + 3)
    for k in range(2):
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), full[k])


# ----------------------------------------------------------------------------- C. dpt_rollin_darkroom
DARK_SEED = 0x1F83D9ABFB41BD6B  # 62 bits; its (6, 50, 10) replay covers every action and both walls
DARK_SHAPES = [(6, 50, 10), (4, 300, 7), (3, 5, 1)]
DARK_OUT = ("states", "actions", "next_states", "rewards", "query", "opt_action")
MIXED_PERMS = (0, 57, 0, 119, 23, 7)  # identity and non-identity rows of O.perm_table()
EXPERT_PERMS = (0, 1, 7, 23, 57, 64, 100, 119)


def dark_tasks(n, dim, permuted):
    goals = np.random.RandomState(31 * n + dim).randint(0, dim, (n, 2))
    return goals, O.perm_table()[list(MIXED_PERMS[:n])] if permuted else None


def query_replay(seed, goals, Hn, dim, perm, ft):
    """query state: words 0 and 1 at step Hn; its expert label"""
    tasks = ft + np.arange(len(goals))
    q = np.stack([philox_np.randint(seed, Hn, tasks, STREAM_ROLLIN, w, dim) for w in (0, 1)], -1)
    return dict(query=q, opt_action=O.darkroom_opt_action(q, goals, perm))


def uniform_replay(seed, goals, Hn, dim, perm, ft, xword=0):
    """Uniform mode outside the kernel: x, y, a = multiply-shift of words 0, 1, 2 at
    (seed, h, ft + i, STREAM_ROLLIN), transitions and labels by the oracle."""
    n = len(goals)
    tasks, hs = (ft + np.arange(n))[:, None], np.arange(Hn)[None]
    x, y = (philox_np.randint(seed, hs, tasks, STREAM_ROLLIN, w, dim) for w in (xword, 1))
    a = philox_np.randint(seed, hs, tasks, STREAM_ROLLIN, 2, 5)
    s = np.stack([x, y], -1)
    ns, r = O.darkroom_transit(s.reshape(-1, 2), a.reshape(-1), np.repeat(goals, Hn, 0), dim,
                               None if perm is None else np.repeat(perm, Hn, 0))
    return dict(states=s, actions=a, next_states=ns.reshape(n, Hn, 2), rewards=r.reshape(n, Hn),
                **query_replay(seed, goals, Hn, dim, perm, ft))


def expert_replay(seed, goals, Hn, dim, perm, ft):
    """Expert mode outside the kernel: the walk from (0, 0), each step the expert's action
    (collect_data.py:83-111 with rollin_type 'expert')."""
    s = np.zeros((len(goals), 2), np.int64)
    out = {k: [] for k in DARK_OUT[:4]}
    for _ in range(Hn):
        a = O.darkroom_opt_action(s, goals, perm)
        ns, r = O.darkroom_transit(s, a, goals, dim, perm)
        for k, v in zip(DARK_OUT[:4], (s, a, ns, r)):
            out[k].append(v)
        s = ns
    return dict({k: np.stack(v, 1) for k, v in out.items()}, **query_replay(seed, goals, Hn, dim, perm, ft))


def rollin_darkroom(goals, Hn, dim, perm, mode, **kw):
    o = dh().rollin_darkroom(goals, Hn, dim, perm, mode, **kw)
    return {k: o[k].cpu().numpy() for k in DARK_OUT}


def assert_dark(got, ref, what):
    for k in DARK_OUT:
        assert got[k].shape == ref[k].shape, (what, k)
        assert np.array_equal(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:4].tolist())


@pytest.mark.parametrize("ft", FIRST_TASKS, ids=ft_id)
@pytest.mark.parametrize("permuted", [False, True], ids=["plain", "permuted"])
@pytest.mark.parametrize("n,Hn,dim", DARK_SHAPES)
def test_rollin_darkroom_uniform_equals_replay(n, Hn, dim, permuted, ft):
    """Uniform mode on its own draws == philox_np.randint of words 0 / 1 / 2 with the oracle's
    transitions, the query at step H and its expert label == the run with those states and actions
    injected == two shards; a replay with word 1 for x differs."""
    goals, perm = dark_tasks(n, dim, permuted)
    ref = uniform_replay(DARK_SEED, goals, Hn, dim, perm, ft)
    if (n, Hn, dim) == DARK_SHAPES[0]:  # the replay alone is no narrow sample
        assert set(ref["actions"].ravel()) == set(range(5))
        assert all({0, dim - 1} <= set(ref["states"][..., c].ravel()) for c in (0, 1))
    phil = rollin_darkroom(goals, Hn, dim, perm, 0, seed=DARK_SEED, first_task=ft)
    assert_dark(phil, ref, "replay")
    inj = rollin_darkroom(goals, Hn, dim, perm, 0, states=ref["states"], actions=ref["actions"], seed=DARK_SEED,
                          first_task=ft)
    assert_dark(inj, phil, "injected")
    k = n // 2
    lo = rollin_darkroom(goals[:k], Hn, dim, None if perm is None else perm[:k], 0, seed=DARK_SEED, first_task=ft)
    hi = rollin_darkroom(goals[k:], Hn, dim, None if perm is None else perm[k:], 0, seed=DARK_SEED,
                         first_task=ft + k)
    assert_dark({key: np.concatenate([lo[key], hi[key]]) for key in DARK_OUT}, phil, "shards")
    if dim > 1:
        wrong = uniform_replay(DARK_SEED, goals, Hn, dim, perm, ft, xword=1)
        assert not np.array_equal(wrong["states"], phil["states"])


@pytest.mark.parametrize("dim,Hn,ft", [(10, 25, FIRST_TASKS[1]), (7, 15, 0)], ids=["dim10", "dim7"])
@pytest.mark.parametrize("permuted", [False, True], ids=["plain", "permuted"])
def test_rollin_darkroom_expert_equals_walk(dim, Hn, ft, permuted):
    """Expert mode, every goal of the room, H past the longest walk (2 (dim - 1) steps), plain and
    under eight permutations: states, actions, next states and rewards == the walk from (0, 0) by
    O.darkroom_opt_action and O.darkroom_transit; query and label as in uniform mode."""
    goals = np.array([(x, y) for x in range(dim) for y in range(dim)])
    assert Hn > 2 * (dim - 1)
    perm = O.perm_table()[[EXPERT_PERMS[i % 8] for i in range(len(goals))]] if permuted else None
    ref = expert_replay(DARK_SEED, goals, Hn, dim, perm, ft)
    assert (ref["rewards"][:, -1] == 1).all() and ref["rewards"][-1].sum() == Hn - 2 * (dim - 1) + 1
    assert_dark(rollin_darkroom(goals, Hn, dim, perm, 1, seed=DARK_SEED, first_task=ft), ref, "expert")


# ----------------------------------------------------------------------------- D. through the host code
def test_rollout_policy_fused_is_shard_invariant_and_replayable():
    """evals/eval_bandit.rollout_policy_fused with a ThompsonSamplingPolicy whose stream is set to
    (SEED, C0): 11 tasks == shards at first_task 0 and 4 == the direct kernel call on the replayed
    draws; the stream advances by the horizon."""
    from ctrls.ctrl_bandit import ThompsonSamplingPolicy
    from envs.bandit_env import BanditEnv, BanditEnvVec
    from evals import eval_bandit
    A = 5
    means, _ = bandit_tasks("thompson", A)
    envs = [BanditEnv(mu, H, var=VAR) for mu in means]

    def fused(lo, hi, **kw):
        c = ThompsonSamplingPolicy(envs[0], std=TS["ts_std"], sample=True, prior_mean=TS["ts_prior_mean"],
                                   prior_var=TS["ts_prior_var"], batch_size=hi - lo)
        c._stream.seed, c._stream.counter = SEED, C0
        o = eval_bandit.rollout_policy_fused(BanditEnvVec(envs[lo:hi]), c, H, **kw)
        assert c._stream.counter == C0 + H
        return {k: o[k].cpu().numpy() for k in OUT}

    full = fused(0, N)
    assert_same(cat(fused(0, 4, first_task=0), fused(4, N, first_task=4), 0), full, "shards")
    assert_same(run("thompson", A, 0, inject=replay_draws("thompson", A, 0)), full, "replay")


def test_collect_data_bandit_histories_are_the_replay():
    """collect_data.generate_bandit_histories_from_envs under np.random.seed: the trajectories'
    contexts == the replay from the seed dpt_hip.next_seed() yields under the same numpy state
    (after the behaviour policies' draws); the n_hists repetitions of a task are separate global
    task ids, so they get distinct draws."""
    import collect_data
    from envs.bandit_env import BanditEnv
    d = dh()
    E, n_hists, n_samples, Hn, A = 3, 2, 2, 9, 5
    means = np.random.RandomState(3).uniform(0, 1, (E, A))
    for kind, bern in (("uniform", False), ("bernoulli", True)):
        envs = [BanditEnv(mu, Hn, var=VAR, type=kind) for mu in means]
        np.random.seed(77)
        trajs = collect_data.generate_bandit_histories_from_envs(envs, n_hists, n_samples, cov=0.0, type=kind)
        np.random.seed(77)
        M = E * n_hists
        p = collect_data.behaviour_policies(M, A)
        seed = d.next_seed()
        hs, tasks = np.arange(Hn), np.arange(M)
        u = philox_np.uniform(seed, hs[:, None], tasks[None], STREAM_ROLLIN)
        g = device_draws(1, seed, hs, 0, M, [STREAM_REWARD])[:, 0]
        hold(g, philox_np.normal(seed, hs[:, None], tasks[None], STREAM_REWARD))
        noise = philox_np.uniform(seed, hs[:, None], tasks[None], STREAM_REWARD) if bern else g
        rep = np.repeat(means, n_hists, 0)
        acts = O.choice_from_uniform(p[None], u)
        rews = np.stack([O.bernoulli_reward(rep, acts[h], noise[h]) if bern else O.bandit_reward(rep, acts[h], noise[h],
                                                                                                  VAR)
                         for h in range(Hn)])
        assert len(trajs) == M * n_samples
        for m in range(M):
            for k in range(n_samples):
                t = trajs[m * n_samples + k]
                assert np.array_equal(t["context_actions"], np.eye(A)[acts[:, m]]), (kind, m)
                assert np.array_equal(t["context_rewards"], rews[:, m]), (kind, m)
                assert np.array_equal(t["means"], means[m // n_hists])
        for e in range(E):  # the two repetitions of env e: other uniforms, other noise
            m0, m1 = e * n_hists, e * n_hists + 1
            assert not np.array_equal(u[:, m0], u[:, m1]) and not np.array_equal(noise[:, m0], noise[:, m1])
            assert not np.array_equal(trajs[m0 * n_samples]["context_rewards"],
                                      trajs[m1 * n_samples]["context_rewards"])


@pytest.mark.parametrize("rollin_type", ["uniform", "expert"])
def test_collect_data_mdp_histories_are_the_replay(rollin_type):
    """collect_data.generate_mdp_histories_from_envs under np.random.seed (plain and permuted envs):
    the contexts == the replay from dpt_hip.next_seed() under the same numpy state; in uniform mode
    the n_hists repetitions of an env draw distinct states."""
    import collect_data
    from envs.darkroom_env import DarkroomEnv, DarkroomEnvPermuted
    d = dh()
    dim, Hn, n_hists, n_samples = 10, 12, 2, 2
    envs = [DarkroomEnv(dim, (3, 7), Hn), DarkroomEnvPermuted(dim, 57, Hn), DarkroomEnv(dim, (0, 9), Hn)]
    np.random.seed(78)
    trajs = collect_data.generate_mdp_histories_from_envs(envs, n_hists, n_samples, rollin_type)
    np.random.seed(78)
    seed = d.next_seed()
    rep = [e for e in envs for _ in range(n_hists)]
    goals = np.stack([e.goal for e in rep])
    perm = np.stack([np.asarray(e.perm if e.perm is not None else range(5)) for e in rep])
    ref = (uniform_replay if rollin_type == "uniform" else expert_replay)(seed, goals, Hn, dim, perm, 0)
    assert len(trajs) == len(rep) * n_samples
    for m in range(len(rep)):
        for k in range(n_samples):
            t = trajs[m * n_samples + k]
            assert np.array_equal(t["context_states"], ref["states"][m]), m
            assert np.array_equal(t["context_actions"], np.eye(5)[ref["actions"][m]]), m
            assert np.array_equal(t["context_next_states"], ref["next_states"][m]), m
            assert np.array_equal(t["context_rewards"], ref["rewards"][m]), m
            assert np.array_equal(t["goal"], goals[m])
    if rollin_type == "uniform":
        for e in range(len(envs)):
            a, b = trajs[e * n_hists * n_samples], trajs[(e * n_hists + 1) * n_samples]
            assert not np.array_equal(a["context_states"], b["context_states"])
