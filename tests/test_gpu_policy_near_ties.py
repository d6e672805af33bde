"""dpt_rollout_policy on inputs whose arm index hangs on the last bit of a statistic
(tests/policy_near_ties.py): twin arms and the mirror arm against the float64 numpy oracle
(oracle.dpt_oracle.bandit_policy_rollout, np.sum over every arm's rewards), LinUCB near ties against the
header's own recorded decisions (tests/golden/policy_near_ties.npz).  Actions, rewards and arm values
of every task, exactly.  test_policy_near_ties_host.py shows that five wrong summation orders each fail
these cases."""
import numpy as np
import pytest

import policy_near_ties as T
from oracle import dpt_oracle as O

pytestmark = pytest.mark.gpu

POLICY_IDS = dict(emp="POLICY_EMP", ucb="POLICY_UCB", lcb="POLICY_LCB", thompson="POLICY_THOMPSON")


def run_case(pol, case):
    import dpt_hip
    bt = T.build(case, pol)
    c = T.policy_constant(pol, case)
    out = dpt_hip.rollout_policy(getattr(dpt_hip, POLICY_IDS[pol.oracle]), bt.means, case.H, T.VAR, noise=bt.noise,
                                 policy_noise=bt.policy_noise, ctx_actions=bt.ctx_actions,
                                 ctx_rewards=bt.ctx_rewards, **T.device_kwargs(pol, c))
    ref = O.bandit_policy_rollout(pol.oracle, bt.means, case.H, T.VAR, bt.noise, ts_g=bt.policy_noise,
                                  ctx_actions=bt.ctx_actions.astype(np.int64), ctx_rewards=bt.ctx_rewards,
                                  **T.oracle_kwargs(pol, c))
    acts = out["actions"].cpu().numpy()
    bad = np.argwhere(acts != ref["actions"])
    assert bad.size == 0, (pol.key, case, f"{len(bad)} (task, step) differ, first {bad[:4].tolist()}")
    assert np.array_equal(out["rewards"].cpu().numpy(), ref["rewards"]), (pol.key, case)
    assert np.array_equal(out["arm_value"].cpu().numpy().T, ref["cum_means"]), (pol.key, case)
    return acts.shape[0]


@pytest.mark.parametrize("cls", T.CLASSES)  # twins of 1020 reach a fourth halving (1020 -> 516 -> 260 -> 132)
@pytest.mark.parametrize("key", list(T.POLICIES))
def test_twin_arms(key, cls):
    """two arms hold the same rewards in different orders, in different 8-arm passes and chunk layouts;
    the last bits of their pairwise sums pick the arm (the H = 9 cases go on appending behind the prefix)"""
    pol = T.POLICIES[key]
    cases = [c for c in T.twin_cases(pol) if T.count_class(c.n) == cls]
    assert cases
    tasks = sum(run_case(pol, c) for c in cases)
    print(f"twin arms {key} {cls}: {len(cases)} launches, {tasks} tasks")


@pytest.mark.parametrize("key", [k for k, p in T.POLICIES.items() if p.mirror])
def test_mirror_arm(key):
    """one arm of n <= 2046 rewards against an arm whose single reward is np.sum(x) / n: an exact tie
    under numpy's order down to the fifth halving, the lower index plays (UCB / LCB at c = 0.0)"""
    pol = T.POLICIES[key]
    cases = T.mirror_cases(pol)
    tasks = sum(run_case(pol, c) for c in cases)
    print(f"mirror arm {key}: {len(cases)} launches, {tasks} tasks")


def linucb_launch(case, c_bits, H=1):
    import dpt_hip
    seed, d, A, n, _ = (int(x) for x in case)
    c = float(np.uint64(c_bits).view(np.float64))
    arms, acts, rews, means, g, u = T.linucb_context(seed, d, A, n)
    ctx = dict(ctx_actions=acts, ctx_rewards=rews) if n else {}
    out = dpt_hip.rollout_policy(dpt_hip.POLICY_LINUCB, means, H, T.VAR, c=c, arms=arms, noise=g[:H],
                                 policy_noise=u, **ctx)
    return out, means, g


@pytest.mark.parametrize("d", T.LIN_D)
def test_linucb_near_ties(d):
    """the lane code of the LinUCB branch (X^T X entries, linucb_m on d A lanes in passes of 64, theta on d
    lanes) at a constant c* where the best two arms are within an ulp: the arm of all four tasks as the
    header's linucb_choose recorded it, up to 32 arms and 2047 rows"""
    fx = dict(np.load(T.GOLDEN))
    rows = [j for j in range(len(fx["cases"])) if fx["cases"][j, 1] == d]
    assert len(rows) >= 2
    for j in rows:
        out, means, g = linucb_launch(fx["cases"][j], fx["c_bits"][j])
        acts = out["actions"].cpu().numpy()[:, 0]
        assert np.array_equal(acts, fx["expected"][j]), (fx["cases"][j].tolist(), acts, fx["expected"][j])
        assert np.array_equal(out["arm_value"].cpu().numpy()[:, 0], means[np.arange(T.LIN_TASKS), acts])
        assert np.array_equal(out["rewards"].cpu().numpy()[:, 0], O.bandit_reward(means, acts, g[0], T.VAR))
    print(f"linucb near ties d={d}: {len(rows)} launches, {len(rows) * T.LIN_TASKS} tasks")


def test_linucb_empty_context_and_steps_behind_a_long_prefix():
    """n = 0 plays min(int(u A), A - 1) of the injected uniform; H = 5 behind C = 2040 starts at a near
    tie and runs on to 2044 rows"""
    fx = dict(np.load(T.GOLDEN))
    out, means, _ = linucb_launch(fx["first_case"], np.float64(1.0).view(np.uint64))
    acts = out["actions"].cpu().numpy()[:, 0]
    assert np.array_equal(acts, fx["first_expected"])
    assert np.array_equal(out["arm_value"].cpu().numpy()[:, 0], means[np.arange(T.LIN_TASKS), acts])
    H = T.LIN_STEPS[1]
    out, means, g = linucb_launch(fx["steps_case"], fx["steps_c_bits"][0], H=H)
    acts = out["actions"].cpu().numpy()
    assert np.array_equal(acts, fx["steps_expected"]), (acts, fx["steps_expected"])
    for h in range(H):
        assert np.array_equal(out["rewards"].cpu().numpy()[:, h], O.bandit_reward(means, acts[:, h], g[h], T.VAR))
