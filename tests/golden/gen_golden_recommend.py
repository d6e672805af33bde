"""Generate tests/golden/recommend_emp.npz by running the REFERENCE's EmpMeanPolicy.

Test infrastructure only (as gen_golden.py, whose stubs and reference location it uses): the reference
checkout is imported at generation time and data is recorded, never code.  For each case, random
bandits and random recorded pulls are drawn, and ``EmpMeanPolicy(online=False).act_numpy_vec``
(ctrls/ctrl_bandit.py:91-117) is run on EVERY prefix t = 0 .. H of the pulls: the arm it names is what
dpt_empirical_recommend must return for budget t.

numpy sums each arm's rewards pairwise, the kernel in pull order, so the two can differ in the last
bits.  The fixture is therefore only written from a seed at which, at every recorded prefix, every
``b_mean`` entry is either bit-equal to the maximum or at least 1e-9 below it: no summation order can
then change the first index of the maximum.  (Exact ties are expected: unpulled arms are exactly 0, and
Bernoulli sums are exact integers.  They resolve to the first index on both sides.)

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_recommend.py [reference checkout]
"""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True  # never leave __pycache__ in the reference tree

OUT = os.path.dirname(os.path.abspath(__file__))
VAR, GAP = 0.3, 1e-9
# name, N, H, A, reward kind
CASES = (("gauss5", 7, 40, 5, "gauss"), ("gauss17", 3, 70, 17, "gauss"), ("bern3", 7, 40, 3, "bern"))


def draw_case(seed, N, H, A, kind):
    rs = np.random.RandomState(seed)
    means = rs.uniform(0, 1, (N, A))
    actions = rs.randint(0, A, (N, H)).astype(np.int32)
    mu = means[np.arange(N)[:, None], actions]
    if kind == "gauss":
        rewards = mu + VAR * rs.standard_normal((N, H))
    else:
        rewards = (rs.uniform(size=(N, H)) < mu).astype(np.float64)
    return means, actions, rewards


def clear_of_near_ties(actions, rewards, A):
    """at every prefix, every b_mean (numpy's own sums, as the reference takes them) is the maximum
    itself or at least GAP below it"""
    N, H = actions.shape
    for t in range(H + 1):
        for i in range(N):
            b = np.array([np.sum(rewards[i, :t][actions[i, :t] == c]) for c in range(A)])
            n = np.array([(actions[i, :t] == c).sum() for c in range(A)])
            bm = b / np.maximum(1, n)
            if ((bm != bm.max()) & (bm > bm.max() - GAP)).any():
                return False
    return True


def reference_arms(EmpMeanPolicy, actions, rewards, A):
    N, H = actions.shape
    env = types.SimpleNamespace(dim=A)
    arms = np.zeros((N, H + 1), np.int32)
    for t in range(H + 1):
        ctrl = EmpMeanPolicy(env, online=False, batch_size=N)
        ctrl.set_batch_numpy_vec({"context_actions": np.eye(A)[actions[:, :t]],
                                  "context_rewards": rewards[:, :t, None]})
        a = ctrl.act_numpy_vec(None)
        assert a.shape == (N, A) and (a.sum(1) == 1).all()
        arms[:, t] = a.argmax(1)
    return arms


def main():
    sys.path.insert(0, OUT)
    import gen_golden
    ref = sys.argv[1] if len(sys.argv) > 1 else gen_golden.REF
    if not os.path.isfile(os.path.join(ref, "ctrls", "ctrl_bandit.py")):
        raise SystemExit("reference checkout not present; the fixture is committed")
    gen_golden._install_stubs()
    sys.path[:0] = [ref]
    from ctrls.ctrl_bandit import EmpMeanPolicy
    out = {}
    for name, N, H, A, kind in CASES:
        seed = 0
        while True:
            means, actions, rewards = draw_case(seed, N, H, A, kind)
            if clear_of_near_ties(actions, rewards, A):
                break
            seed += 1
        arms = reference_arms(EmpMeanPolicy, actions, rewards, A)
        assert (arms[:, 0] == 0).all()
        out.update({f"{name}/means": means, f"{name}/actions": actions, f"{name}/rewards": rewards,
                    f"{name}/emp_arm": arms, f"{name}/seed": np.int64(seed)})
        print(f"{name}: N={N} H={H} A={A} seed {seed}")
    np.savez_compressed(os.path.join(OUT, "recommend_emp.npz"), **out)


if __name__ == "__main__":
    main()
