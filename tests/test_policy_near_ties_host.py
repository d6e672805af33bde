"""The near-tie cases of tests/policy_near_ties.py on the host: that they are what they claim (numpy's
order restated, the oracle reproduced from the two candidate arms alone), that they can fail (five
wrong summation orders each change arms), the LinUCB fixture regenerated, and dpt_hip.rollout_policy's
refusal of arm indices outside [0, A).  The device runs the same cases in test_gpu_policy_near_ties.py."""
import numpy as np
import pytest

import policy_near_ties as T
from oracle import dpt_oracle as O
from test_linucb_orders import harness, run  # noqa: F401  (the g++ harness of dpt_linucb.h, reused)

MIN_FLIPS = 3  # a cap, not a measurement: every wrong order must change at least this many arms


@pytest.fixture(scope="module")
def built():
    return {key: [T.build(case, pol) for case in T.all_cases(pol)] for key, pol in T.POLICIES.items()}


def test_case_table():
    """the counts sit where the recursion changes depth, every class and layout is met, and every launch
    fits the entry point's C + H <= 2048 (the mirror at 2046 exactly)"""
    assert [T.halvings(n) for n in (128, 129, 256, 257, 263, 512, 519, 1024, 1031, 2040, 2039, 2047)] == \
        [0, 1, 1, 2, 2, 2, 3, 3, 4, 4, 5, 5]
    for pol in T.POLICIES.values():
        cases = T.all_cases(pol)
        assert {c.n for c in cases if c.kind == "twin"} == set(T.TWIN_COUNTS)
        assert {(c.n, c.arrival) for c in cases if c.kind == "twin" and c.H == 1} == \
            {(n, a) for n in T.TWIN_COUNTS for a in T.ARRIVALS}
        assert {c.n for c in cases if c.H == 9} == set(T.TWIN_STEPS_COUNTS)
        assert {c.A for c in cases} == {2, 8, 9, 16, 17, 24, 25, 32}
        assert {(c.A, c.a, c.b) for c in cases} >= set(T.LAYOUTS)
        for c in cases:
            C = (2 * c.n if c.kind == "twin" else c.n + 1) + c.A - 2
            assert C + c.H <= T.CAP, c
        if pol.mirror:
            assert {c.n for c in cases if c.kind == "mirror"} == set(T.MIRROR_COUNTS)
            assert any(c.n + 1 + c.A - 2 + c.H == T.CAP for c in cases if c.kind == "mirror")
            assert {T.count_class(c.n) for c in cases} == set(T.CLASSES)


def test_pairwise_restatement_is_numpy(built):
    """the Python restatement of pairwise_sum equals np.sum on every case vector, bit for bit"""
    for bts in built.values():
        for bt in bts:
            for X in (bt.xa, bt.xb):
                assert np.array_equal(T.pairwise(X), T.np_sum(X)), bt.case


@pytest.mark.parametrize("key", list(T.POLICIES))
def test_two_candidates_reproduce_the_oracle(built, key):
    """np.sum over the two candidates' lists gives the oracle's step-0 arm in every task, and the best of
    the other arms is at least 1.0 below both"""
    pol = T.POLICIES[key]
    for bt in built[key]:
        kw = T.oracle_kwargs(pol, T.policy_constant(pol, bt.case))
        ts_g = None if bt.policy_noise is None else bt.policy_noise[0]
        ref = O.policy_action(pol.oracle, bt.ctx_actions.astype(np.int64), bt.ctx_rewards, bt.case.A, ts_g=ts_g, **kw)
        assert np.array_equal(T.chosen(bt, pol, T.np_sum), ref), bt.case
        assert T.third_best_gap(bt, pol) >= 1.0, bt.case
        if bt.case.kind == "mirror":  # the means tie exactly: the lower index plays
            va, vb = T.candidate_values(bt, pol, T.np_sum)
            assert np.array_equal(va, vb) and np.array_equal(ref, np.minimum(bt.pos_a, bt.pos_b)), bt.case


def test_wrong_orders_change_arms(built, capsys):
    """Each wrong summation order changes the played arm in at least MIN_FLIPS tasks of the case set, and
    left to right in at least MIN_FLIPS tasks of every (policy, count class) cell.  Prints the table."""
    cells = {}  # (order, policy, class) -> [flips, tasks]
    differs = {name: set() for name in T.WRONG_ORDERS}
    for key, pol in T.POLICIES.items():
        for bt in built[key]:
            right = T.chosen(bt, pol, T.pairwise)
            for name, fn in T.WRONG_ORDERS.items():
                cell = cells.setdefault((name, key, T.count_class(bt.case.n)), [0, 0])
                cell[0] += int((T.chosen(bt, pol, fn) != right).sum())
                cell[1] += T.N_TASKS
                if not (np.array_equal(fn(bt.xa), T.pairwise(bt.xa)) and np.array_equal(fn(bt.xb), T.pairwise(bt.xb))):
                    differs[name].add(bt.case.n)
    with capsys.disabled():
        print("\nflipped arms / tasks per wrong order, policy and count class")
        print(f"{'order':18s}{'policy':13s}" + "".join(f"{c:>12s}" for c in T.CLASSES))
        for name in T.WRONG_ORDERS:
            for key in T.POLICIES:
                row = [cells.get((name, key, c)) for c in T.CLASSES]
                print(f"{name:18s}{key:13s}" + "".join(f"{'-' if r is None else f'{r[0]}/{r[1]}':>12s}" for r in row))
    for name in T.WRONG_ORDERS:
        total = sum(v[0] for k, v in cells.items() if k[0] == name)
        assert total >= MIN_FLIPS, (name, total)
    for (name, key, cls), (flips, _) in cells.items():
        if name == "left_to_right":
            assert flips >= MIN_FLIPS, (key, cls, flips)
    # the two orders that differ from numpy's only at some counts meet such counts
    assert {130, 300, 1000, 1020, 2040} <= differs["no_multiple_of_8"]
    assert {1000, 1020, 2040} <= differs["two_halvings"]


def test_linucb_fixture_regenerates(harness):  # noqa: F811
    """the recorded LinUCB near ties are what the header's linucb_choose gives here, cover every lin_d,
    arm count and context length at least twice, and sit at a crossing (0.05 < c* < 20)"""
    fx = dict(np.load(T.GOLDEN))
    new = T.linucb_fixture(run, harness)
    assert sorted(fx) == sorted(new)
    for k in new:
        assert fx[k].dtype == new[k].dtype and np.array_equal(fx[k], new[k]), k
    cases = fx["cases"]
    assert len(cases) == T.LIN_CASES
    for col, vals in ((1, T.LIN_D), (2, T.LIN_A), (3, T.LIN_N)):
        for v in vals:
            assert (cases[:, col] == v).sum() >= 2, (col, v)
    assert set(cases[:, 4]) == set(range(T.LIN_TASKS))
    c = fx["c_bits"].view(np.float64)
    assert ((c > 0.05) & (c < 20)).all()


def test_linucb_fixture_is_numpys(harness):  # noqa: F811
    """numpy's own expressions (the oracle's policy_action) play the recorded arms -- on a host whose BLAS
    rounds as the recording host's does (the proviso of test_linucb_orders.py) -- and at c* the top two
    values are within an ulp of each other"""
    fx = dict(np.load(T.GOLDEN))
    for (seed, d, A, n, ti), bits, exp in zip(fx["cases"], fx["c_bits"], fx["expected"]):
        c = float(np.uint64(bits).view(np.float64))
        arms, acts, rews = T.linucb_context(seed, d, A, n)[:3]
        got = O.policy_action("linucb", acts.astype(np.int64), rews, A, c=c, arms=arms)
        assert np.array_equal(got, exp), (seed, d, A, n)
        v = np.sort(run(harness, arms, acts[ti], rews[ti], c)[2])
        assert v[-1] - v[-2] <= np.spacing(max(abs(v[-1]), abs(v[-2]))), (seed, d, A, n, v[-1] - v[-2])
        assert len(v) == 2 or v[-2] - v[-3] >= 1e-6, (seed, d, A, n)


def test_rollout_policy_refuses_arms_out_of_range():
    """ctx_actions outside [0, A) would index the kernel's LDS tables out of range (include/dpt_hip.h);
    a host array is checked before anything reaches the device"""
    import dpt_hip
    means = np.zeros((2, 5))
    rew = np.zeros((2, 3))
    for bad in (5, -1, 255):
        acts = np.array([[0, 1, 2], [3, bad, 4]], np.int32)
        with pytest.raises(ValueError, match="ctx_actions"):
            dpt_hip.rollout_policy(dpt_hip.POLICY_EMP, means, 1, 0.3, ctx_actions=acts, ctx_rewards=rew)
