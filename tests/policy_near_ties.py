"""Inputs on which the classical-policy kernel's arm index hangs on the last bit of a statistic
(dpt_rollout_policy, csrc/dpt_policies.hip), and the host arithmetic that says so.

Random tasks separate their best two arms by ~1e-2, so a device sum taken in another order than
numpy's moves a mean by an ulp and picks the same arm.  Two constructions make the order decide:

* twin arms: arms a and b received the same n Gaussian rewards in different orders (b's list is a
  permutation of a's).  Under numpy's pairwise order the two sums differ in their last bits in a good
  share of the tasks, and those bits pick the winner.  Every other arm has one pull of -50, which keeps
  the play-an-unseen-arm rule and every bonus out of the way.  Thompson's twins share one injected
  posterior normal per step (per vote draw).
* mirror arm: arm a holds n rewards x, arm b the single reward np.sum(x) / n.  The two means tie exactly
  under numpy's order, argmax takes the lower index; b sits below a in the even tasks (a device sum that
  is too high shows) and above it in the odd ones (too low).  One arm can hold all of C + H <= 2048, so
  this reaches the fourth and fifth halving of the recursion.

The counts follow from pairwise_sum's recursion (leaves <= 128, halving at multiples of 8), they are
not sampled.  ``pairwise`` restates that recursion on the rows of a (tasks, n) array -- elementwise adds
round as scalar ones do -- and WRONG_ORDERS are five near misses of it a kernel could plausibly
implement; ``chosen`` evaluates the two candidate arms under any of them
(tests/test_policy_near_ties_host.py: numpy's order reproduces the oracle, every wrong one flips arms).

LinUCB (dpt_linucb.h orders on the lanes of a wave): ``linucb_fixture`` searches seeded contexts for an
arm pair (a, b) and the constant c* at which their values cross, so that at c = c* the two are 0-1 ulp
apart, and records the header's own decision (linucb_choose, compiled by g++: the harness of
tests/test_linucb_orders.py).  ``python tests/policy_near_ties.py`` rewrites the fixture
tests/golden/policy_near_ties.npz.
"""
import os
from collections import namedtuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_near_ties.npz")

N_TASKS = 48
CAP = 2048  # dpt_rollout_policy: C + H <= 2048
VAR = 0.3  # the env's reward variance (H > 1 cases)
TS = dict(std=0.3, prior_mean=0.5, prior_var=1 / 12.0)
OTHER_REWARD = -50.0

# ----------------------------------------------------------------------------- summation orders


def _leaf(X, combine="np"):
    """numpy pairwise_sum's unrolled leaf on every row of X (tasks, m): m < 8 left to right from 0;
    else eight chains r[c] += x[8t + c], combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the tail"""
    m = X.shape[1]
    if m < 8:
        res = np.zeros(X.shape[0])
        for i in range(m):
            res = res + X[:, i]
        return res
    r = X[:, 0:8].copy()
    full = m - m % 8
    for i in range(8, full, 8):
        r = r + X[:, i:i + 8]
    if combine == "np":
        res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    else:  # a xor 4 / 2 / 1 butterfly
        res = ((r[:, 0] + r[:, 4]) + (r[:, 2] + r[:, 6])) + ((r[:, 1] + r[:, 5]) + (r[:, 3] + r[:, 7]))
    for i in range(full, m):
        res = res + X[:, i]
    return res


def _pairwise(X, leaf=128, round8=True, combine="np", depth=None):
    n = X.shape[1]
    if n <= leaf or depth == 0:
        return _leaf(X, combine)
    h = n // 2
    if round8:
        h -= h % 8
    d = None if depth is None else depth - 1
    return _pairwise(X[:, :h], leaf, round8, combine, d) + _pairwise(X[:, h:], leaf, round8, combine, d)


def pairwise(X):
    """np.sum of every row of X in numpy's own order (loops_utils.h.src pairwise_sum)"""
    return _pairwise(np.asarray(X, np.float64))


def np_sum(X):
    """np.sum row by row, on a contiguous 1-D array each as the oracle's rews[acts == k] is"""
    return np.array([np.sum(np.ascontiguousarray(x)) for x in np.asarray(X, np.float64)])


def _left_to_right(X):
    X = np.asarray(X, np.float64)
    res = np.zeros(X.shape[0])
    for i in range(X.shape[1]):
        res = res + X[:, i]
    return res


WRONG_ORDERS = {
    "left_to_right": _left_to_right,
    "no_multiple_of_8": lambda X: _pairwise(np.asarray(X, np.float64), round8=False),
    "leaf_64": lambda X: _pairwise(np.asarray(X, np.float64), leaf=64),
    "butterfly_r0_r4": lambda X: _pairwise(np.asarray(X, np.float64), combine="xor4"),
    "two_halvings": lambda X: _pairwise(np.asarray(X, np.float64), depth=2),
}


def halvings(n):
    """depth of pairwise_sum's recursion over n elements"""
    if n <= 128:
        return 0
    h = n // 2
    h -= h % 8
    return 1 + max(halvings(h), halvings(n - h))


CLASSES = ("leaf", "one", "two", "three", "four_five")


def count_class(n):
    return CLASSES[min(halvings(n), 4)]


# ----------------------------------------------------------------------------- the policies

Policy = namedtuple("Policy", "key oracle online c sample mirror")
POLICIES = {p.key: p for p in (
    Policy("emp_online", "emp", True, None, True, True),
    Policy("emp_offline", "emp", False, None, True, True),
    Policy("ucb", "ucb", True, 1.0, True, True),
    Policy("lcb", "lcb", True, 0.8, True, True),
    Policy("ts_sample", "thompson", True, None, True, False),
    Policy("ts_vote", "thompson", True, None, False, False),
)}


def oracle_kwargs(pol, c=None):
    """keyword arguments of oracle.dpt_oracle.policy_action / bandit_policy_rollout"""
    if pol.oracle == "emp":
        return dict(online=pol.online)
    if pol.oracle in ("ucb", "lcb"):
        return dict(c=pol.c if c is None else c)
    return dict(ts=TS, sample=pol.sample)


def device_kwargs(pol, c=None):
    """keyword arguments of dpt_hip.rollout_policy (the policy constant apart)"""
    if pol.oracle == "emp":
        return dict(online=pol.online)
    if pol.oracle in ("ucb", "lcb"):
        return dict(c=pol.c if c is None else c)
    return dict(ts_std=TS["std"], ts_prior_mean=TS["prior_mean"], ts_prior_var=TS["prior_var"], sample=pol.sample)


# ----------------------------------------------------------------------------- cases

# (A, a, b): the twins in different 8-arm passes of the kernel's per-arm loop and in both index orders,
# at every arm count next to a pass boundary
LAYOUTS = ((2, 0, 1), (2, 1, 0), (8, 7, 0), (8, 2, 5), (9, 8, 0), (9, 3, 8), (16, 7, 8), (16, 15, 0),
           (17, 16, 1), (17, 0, 16), (24, 23, 8), (24, 9, 16), (25, 24, 0), (25, 7, 24), (32, 3, 31),
           (32, 31, 3), (32, 8, 9), (32, 0, 24))
ARRIVALS = ("blocks", "alternating", "shuffled")
TWIN_COUNTS = (1, 7, 8, 9, 15, 16, 17, 120, 127, 128,  # leaf edges
               129, 130, 135, 136, 137, 255, 256, 257,  # first split
               263, 264, 300, 511, 512, 513, 519,  # second split
               1000, 1016, 1020)  # third split (1020: a fourth, 132 > 128), the most two arms can hold
TWIN_STEPS_COUNTS = (7, 8, 9, 136)  # H = 9 behind the prefix: appends into a partly filled chunk and a new one
MIRROR_COUNTS = (1023, 1024, 1025, 1031, 1500, 2039, 2040, 2046)

Case = namedtuple("Case", "kind n A a b arrival H seed")
# a, b: the two candidate arms (mirror cases swap them in the odd tasks: see positions())


def _layout(n_ctx, H, j):
    ok = [L for L in LAYOUTS if n_ctx + L[0] - 2 + H <= CAP]
    return ok[j % len(ok)]


def twin_cases(pol):
    """the twin-arm cases of one policy: every count at every arrival order, the layouts in rotation
    (shifted per policy), and the H = 9 cases"""
    shift = 5 * list(POLICIES).index(pol.key)
    out = []
    for ci, n in enumerate(TWIN_COUNTS):
        for ai, arrival in enumerate(ARRIVALS):
            j = ci * len(ARRIVALS) + ai
            A, a, b = _layout(2 * n, 1, j + shift)
            out.append(Case("twin", n, A, a, b, arrival, 1, 7000 + j))
    for ci, n in enumerate(TWIN_STEPS_COUNTS):
        j = 3 * ci + shift
        A, a, b = _layout(2 * n, 9, j + 1)
        out.append(Case("twin", n, A, a, b, ARRIVALS[ci % 3], 9, 7500 + ci))
    return out


def mirror_cases(pol):
    if not pol.mirror:
        return []
    shift = 5 * list(POLICIES).index(pol.key)
    out = []
    for ci, n in enumerate(MIRROR_COUNTS):
        A, a, b = (2, 1, 0) if n == 2046 else _layout(n + 1, 1, 2 * ci + shift)
        out.append(Case("mirror", n, A, a, b, ARRIVALS[ci % 3], 1, 8000 + ci))
    return out


def all_cases(pol):
    return twin_cases(pol) + mirror_cases(pol)


def positions(case):
    """(N_TASKS,) index of arm a and of arm b per task"""
    a = np.full(N_TASKS, case.a)
    b = np.full(N_TASKS, case.b)
    if case.kind == "mirror":  # b below a in the even tasks, above it in the odd ones
        lo, hi = min(case.a, case.b), max(case.a, case.b)
        odd = np.arange(N_TASKS) % 2 == 1
        a, b = np.where(odd, lo, hi), np.where(odd, hi, lo)
    return a, b


Built = namedtuple("Built", "case xa xb pos_a pos_b ctx_actions ctx_rewards means noise policy_noise")


def build(case, pol):
    """The launch of one case: xa, xb (N_TASKS, n_a) / (N_TASKS, n_b) the candidates' reward lists in
    arrival order, the prefix context (N_TASKS, C), the env means, the reward normals (H, N_TASKS) and the
    policy's injected normals (Thompson: (H, N, A) sampled, (H, 100, N, A) for the vote; else None)."""
    rs = np.random.RandomState(case.seed)
    N, n, A, H = N_TASKS, case.n, case.A, case.H
    xa = rs.normal(0.5, 0.3, (N, n))
    if case.kind == "twin":
        xb = np.stack([x[rs.permutation(n)] for x in xa])
    else:
        xb = (np_sum(xa) / n)[:, None]
    pos_a, pos_b = positions(case)
    nb = xb.shape[1]
    C = n + nb + A - 2
    acts = np.zeros((N, C), np.int32)
    rews = np.zeros((N, C))
    for i in range(N):
        others = [k for k in range(A) if k not in (pos_a[i], pos_b[i])]
        if case.arrival == "blocks":  # the other arms, all of a, all of b
            lab = others + [pos_a[i]] * n + [pos_b[i]] * nb
        elif case.arrival == "alternating":  # a b a b ..., the longer list's rest, the other arms
            m = min(n, nb)
            lab = [v for _ in range(m) for v in (pos_a[i], pos_b[i])] + [pos_a[i]] * (n - m) + [pos_b[i]] * (nb - m)
            lab = lab + others
        else:
            lab = list(rs.permutation(others + [pos_a[i]] * n + [pos_b[i]] * nb))
        lab = np.asarray(lab, np.int32)
        acts[i] = lab
        rews[i] = OTHER_REWARD
        rews[i][lab == pos_a[i]] = xa[i]
        rews[i][lab == pos_b[i]] = xb[i]
    means = np.full((N, A), OTHER_REWARD)
    means[np.arange(N), pos_a] = 0.45
    means[np.arange(N), pos_b] = 0.55
    noise = rs.normal(size=(H, N))
    pn = None
    if pol.oracle == "thompson":
        shape = (H, N, A) if pol.sample else (H, 100, N, A)
        pn = rs.normal(size=shape)
        twin = 0.05 * rs.normal(size=shape[:-1])  # small: the sum m + s g stays in m's binade
        ia, ib = np.broadcast_to(pos_a, shape[:-1])[..., None], np.broadcast_to(pos_b, shape[:-1])[..., None]
        np.put_along_axis(pn, ia, twin[..., None], -1)
        np.put_along_axis(pn, ib, twin[..., None], -1)
    return Built(case, xa, xb, pos_a, pos_b, acts, rews, means, noise, pn)


def _value(pol, s, n, c, g):
    """a candidate arm's value from the sum s of its n rewards, as the oracle's policy_action rounds it
    (g: the arm's injected normal (N,), or (100, N) for the vote)"""
    n = float(n)
    if pol.oracle == "thompson":
        var, pm, pv = TS["std"] ** 2, TS["prior_mean"], TS["prior_var"]
        w = var / (var + n * pv)
        mean = w * pm + (1 - w) * (s / n)
        return mean + np.sqrt(1 / (1 / pv + n / var)) * g
    v = s / max(1.0, n)
    if pol.oracle in ("ucb", "lcb"):
        bon = c / max(1.0, np.sqrt(n))
        v = v + bon if pol.oracle == "ucb" else v - bon
    return v


def policy_constant(pol, case):
    """UCB / LCB run the mirror cases with c = 0.0: the bonus is +0.0 and the bonus code still runs"""
    if pol.c is None:
        return None
    return 0.0 if case.kind == "mirror" else pol.c


def candidate_values(bt, pol, sumfn):
    """(va, vb): the two candidates' values at step 0 under the summation ``sumfn``"""
    c = policy_constant(pol, bt.case)
    ga = gb = None
    if bt.policy_noise is not None:
        pn = bt.policy_noise[0]
        ga = np.take_along_axis(pn, np.broadcast_to(bt.pos_a, pn.shape[:-1])[..., None], -1)[..., 0]
        gb = np.take_along_axis(pn, np.broadcast_to(bt.pos_b, pn.shape[:-1])[..., None], -1)[..., 0]
    va = _value(pol, sumfn(bt.xa), bt.xa.shape[1], c, ga)
    vb = _value(pol, sumfn(bt.xb), bt.xb.shape[1], c, gb)
    return va, vb


def chosen(bt, pol, sumfn):
    """(N_TASKS,) the arm step 0 plays if only the two candidates matter (third_best_gap shows they do):
    the first maximum, or for the vote the first arm with the most of the 100 draws' maxima"""
    va, vb = candidate_values(bt, pol, sumfn)
    lo_is_a = bt.pos_a < bt.pos_b
    lo, hi = np.where(lo_is_a, bt.pos_a, bt.pos_b), np.where(lo_is_a, bt.pos_b, bt.pos_a)
    vlo, vhi = np.where(lo_is_a, va, vb), np.where(lo_is_a, vb, va)
    if va.ndim == 2:  # the vote
        votes_hi = (vhi > vlo).sum(0)
        return np.where(votes_hi > va.shape[0] - votes_hi, hi, lo)
    return np.where(vhi > vlo, hi, lo)


def third_best_gap(bt, pol):
    """the least margin, over tasks (and vote draws), of the lower candidate above every other arm"""
    va, vb = candidate_values(bt, pol, np_sum)
    if bt.case.A == 2:
        return np.inf
    c = policy_constant(pol, bt.case)
    g = None
    if bt.policy_noise is not None:
        pn = bt.policy_noise[0].copy()
        np.put_along_axis(pn, np.broadcast_to(bt.pos_a, pn.shape[:-1])[..., None], -np.inf, -1)
        np.put_along_axis(pn, np.broadcast_to(bt.pos_b, pn.shape[:-1])[..., None], -np.inf, -1)
        g = pn.max(-1)  # the other arms share count and sum: the largest normal is the best of them
    other = _value(pol, np.full(N_TASKS, OTHER_REWARD), 1, c, g)
    return float((np.minimum(va, vb) - other).min())


# ----------------------------------------------------------------------------- LinUCB

LIN_D = (2, 3, 4, 5, 6, 7, 8)
LIN_A = (2, 12, 32)
LIN_N = (5, 383, 384, 385, 767, 768, 769, 1151, 1152, 1153, 1535, 2040, 2047)
LIN_CASES = 120
LIN_TASKS = 4
LIN_STEPS = (2040, 5)  # the H = 5 case: C, H


def linucb_context(seed, d, A, n):
    """arms (A, d) at envs/bandit_env.py sample_linear's scale, the four tasks' contexts acts / rews
    (4, n), their env means (4, A), reward normals g (8, 4) and first-arm uniforms u (4,), all from one
    frozen RandomState stream"""
    rs = np.random.RandomState(seed)
    arms = rs.normal(0, 1, (A, d)) / np.sqrt(d)
    acts = rs.randint(0, A, (LIN_TASKS, n)).astype(np.int32)
    rews = rs.normal(0, 1, (LIN_TASKS, n))
    theta = rs.normal(0, 1, (LIN_TASKS, d)) / np.sqrt(d)
    means = np.stack([np.array([float(np.sum(arm * t)) for arm in arms]) for t in theta])
    return arms, acts, rews, means, rs.normal(size=(8, LIN_TASKS)), rs.uniform(size=LIN_TASKS)


def _crossing(run, lib, arms, act, rew):
    """(c*, a, b) at which arms a and b cross as the top two with the third >= 1e-6 below, or None.
    t and cov_inv come from the header (c = 0 leaves value = theta . arm); q in plain elementwise
    arithmetic, so the search does not depend on the host's BLAS."""
    A, d = arms.shape
    _, ci, t = run(lib, arms, act, rew, 0.0)
    qq = np.zeros(A)
    for p in range(d):
        for j in range(d):
            qq = qq + arms[:, p] * ci[p, j] * arms[:, j]
    q = np.sqrt(qq)
    for a in range(A):
        for b in range(A):
            if a == b or q[b] == q[a]:
                continue
            c = (t[a] - t[b]) / (q[b] - q[a])
            if not 0.05 < c < 20:
                continue
            v = t + c * q
            top = np.argsort(-v, kind="stable")[:3]
            if set(top[:2]) != {a, b}:
                continue
            # q above is not the header's q to the last bit and q_b - q_a cancels: Newton steps on the
            # header's own values v_a(c) - v_b(c), whose slope is q_a - q_b, until they are within an ulp
            for _ in range(4):
                v = run(lib, arms, act, rew, float(c))[2]
                if abs(v[a] - v[b]) <= np.spacing(max(abs(v[a]), abs(v[b]))):
                    break
                c = c - (v[a] - v[b]) / (q[a] - q[b])
            else:
                continue
            if not 0.05 < c < 20:
                continue
            if A > 2 and np.delete(v, [a, b]).max() > min(v[a], v[b]) - 1e-6:
                continue
            return float(c), a, b
    return None


def linucb_steps(run, lib, arms, acts, rews, means, g, c, H):
    """H decisions of every task by the header's linucb_choose, the env step as the oracle's
    bandit_reward: (4, H) arms"""
    from oracle import dpt_oracle as O
    acts, rews = [list(a) for a in acts], [list(r) for r in rews]
    out = np.zeros((LIN_TASKS, H), np.int64)
    for h in range(H):
        a = np.array([run(lib, arms, np.asarray(acts[i], np.int32), np.asarray(rews[i]), c)[0]
                      for i in range(LIN_TASKS)])
        r = O.bandit_reward(means, a, g[h], VAR)
        for i in range(LIN_TASKS):
            acts[i].append(int(a[i]))
            rews[i].append(float(r[i]))
        out[:, h] = a
    return out


def _search(run, lib, j, d, A, n, H=1):
    ti = j % LIN_TASKS
    for attempt in range(400):
        seed = 1000 * j + attempt
        arms, acts, rews, means, g, _ = linucb_context(seed, d, A, n)
        hit = _crossing(run, lib, arms, acts[ti], rews[ti])
        if hit is None:
            continue
        c = hit[0]
        return seed, c, ti, linucb_steps(run, lib, arms, acts, rews, means, g, c, H)
    raise RuntimeError(f"no crossing pair for case {j} (d={d}, A={A}, n={n})")


def linucb_fixture(run, lib):
    """The fixture's arrays.  cases (LIN_CASES, 5) int64: seed, d, A, n, the near-tie task's index; c_bits
    (LIN_CASES,) uint64 the constant's bits; expected (LIN_CASES, 4) the header's arm per task.  steps_*:
    the same for the one H = 5 case behind C = 2040 (expected (4, 5)).  first_*: the empty context, whose
    arm is min(int(u A), A - 1) of the injected uniform."""
    cases, bits, expected = [], [], []
    for j in range(LIN_CASES):
        d, A, n = LIN_D[j % len(LIN_D)], LIN_A[j % len(LIN_A)], LIN_N[j % len(LIN_N)]
        seed, c, ti, arm = _search(run, lib, j, d, A, n)
        cases.append((seed, d, A, n, ti))
        bits.append(np.float64(c).view(np.uint64))
        expected.append(arm[:, 0])
    C, H = LIN_STEPS
    seed, c, ti, arm = _search(run, lib, LIN_CASES, 8, 32, C, H)
    first = (1000 * (LIN_CASES + 1), 8, 32, 0, 0)
    u = linucb_context(*first[:4])[5]
    return dict(cases=np.array(cases, np.int64), c_bits=np.array(bits, np.uint64),
                expected=np.array(expected, np.int64),
                steps_case=np.array((seed, 8, 32, C, ti), np.int64),
                steps_c_bits=np.array([np.float64(c).view(np.uint64)], np.uint64), steps_expected=arm,
                first_case=np.array(first, np.int64),
                first_expected=np.minimum((u * 32).astype(np.int64), 31))


def load_harness():
    """the g++ harness of tests/test_linucb_orders.py outside a pytest run: (run, lib)"""
    import tempfile
    from pathlib import Path

    import test_linucb_orders as T
    fn = T.harness
    fn = fn._get_wrapped_function() if hasattr(fn, "_get_wrapped_function") else getattr(fn, "__wrapped__", fn)

    class Factory:
        def mktemp(self, name):
            return Path(tempfile.mkdtemp(prefix=name))

    return T.run, fn(Factory())


if __name__ == "__main__":
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.dirname(os.path.abspath(__file__))]
    fx = linucb_fixture(*load_harness())
    np.savez(GOLDEN, **fx)
    print(f"{GOLDEN}: {len(fx['cases'])} cases, {os.path.getsize(GOLDEN)} bytes")
