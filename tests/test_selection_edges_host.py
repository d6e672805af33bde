"""tests/selection_edges.py on the oracles' own rollouts (oracle/dpt_oracle.py, float64 forwards, fp32
logits), without a GPU: the construction the GPU file runs on the fused rollouts reaches its conditions on
the reference alone.  At the DarkRoom (3, 30, 2) shape (the golden model, 5 tasks, temperatures 1, 0.5
and 2) and the bandit L = 2, H = 70, A = 5 shape, and on the `medium` models of tests/sharp_models.py: at
least 0.9 of the task-steps are placed at every delta, at least 0.9 of the placed draws with delta <=
2.9e-5 lie within 2^-15 of an edge, both sides of an edge occur, the oracle's trajectory is unchanged under
the steady deltas (here under the razor ones too: the cdf the draws are placed on is the oracle's own),
and the control (every placed draw moved 2 delta across its edge) changes the action at every placed
step.  The oracle never decides the other side than its own cdf, so the razor rounds (re-placing the draws
after a task's first departure) are run on a toy rollout whose edges sit 5e-9 off numpy's."""
import numpy as np
import pytest

import selection_edges as SE
from conftest import golden
from oracle import dpt_oracle as O

N = 5


def _darkroom(W, goals, Heps, horizon, R, temp, perm=None):
    def rollout(u):
        r = O.darkroom_online_rollout(W, goals, Heps, R * horizon, horizon, u.reshape(Heps, horizon, -1), True,
                                      perm=perm, temp=temp)
        return dict(logits=r["logits"], actions=r["actions"].T)
    return rollout


def _bandit(W, means, H, g):
    def rollout(u):
        r = O.bandit_online_rollout(W, means, H, 0.3, u, g)
        return dict(logits=r["logits"], actions=r["actions"].T)
    return rollout


def _razor_unchanged(lines):
    """on the oracle the razor deltas keep the trajectory too (same cdf, bit for bit)"""
    runs = [ln for ln in lines if " delta=" in ln]
    assert len(runs) == len(SE.STEADY + SE.RAZOR) and all(ln.endswith("same_as_run1=1") for ln in runs), lines


@pytest.mark.parametrize("temp", [1.0, 0.5, 2.0])
def test_darkroom_oracle_reaches_the_conditions(temp):
    g = golden("forward_darkroom.npz")
    W = O.split_weights({k[2:]: v for k, v in g.items() if k.startswith("w/")}, 4)
    rs = np.random.RandomState(41)
    goals = rs.randint(0, 10, (N, 2))
    u0 = rs.uniform(size=(90, N))
    rollout = _darkroom(W, goals, 3, 30, 2, temp)
    _razor_unchanged(SE.run_case(f"oracle darkroom (3, 30, 2) temp {temp}", rollout, SE.oracle_select, u0, temp=temp,
                                 seed=3))


def test_bandit_oracle_reaches_the_conditions():
    import bench
    L, A, H = 2, 5, 70
    sd, _ = bench.synthetic_state_dict(L, 1, A, H)
    W = O.split_weights({k: v.numpy() for k, v in sd.items()}, L)
    rs = np.random.RandomState(42)
    means = rs.uniform(0, 1, (N, A))
    u0, gn = rs.uniform(size=(H, N)), rs.standard_normal((H, N))
    rollout = _bandit(W, means, H, gn)
    _razor_unchanged(SE.run_case("oracle bandit L 2 H 70 A 5", rollout, SE.oracle_select, u0, seed=4))


def test_medium_models_reach_the_placed_share():
    """the `medium` models of tests/sharp_models.py (peaked attention, larger gains: some arms are narrow):
    the DarkRoom (3, 30, 2) case and the bandit L = 2, A = 5 case at H = 70 keep the 0.9 placed share"""
    import sharp_models as SM
    goals, perms, u0 = SM.darkroom_setup(3, 30, True)
    W = O.split_weights(SM.as_f64(SM.darkroom_weights("medium")), 4)
    SE.run_case("oracle darkroom medium (3, 30, 2)", _darkroom(W, goals, 3, 30, 2, 1.0, perms), SE.oracle_select, u0,
                seed=5)
    Nb, H = 5, 70
    W = O.split_weights(SM.as_f64(SM.rollout_weights(2, 5, "medium")), 2)
    u0, gn = SM.bandit_draws(Nb, H)
    SE.run_case("oracle bandit medium L 2 H 70 A 5", _bandit(W, SM.bandit_means(Nb, 5), H, gn), SE.oracle_select, u0,
                seed=6)


def test_control_and_placement_on_known_logits():
    """the helper itself on a hand-made row: cdf edges 0.1, 0.3, 0.6, 0.8; arm 2 chosen at u0 = 0.5"""
    p = np.array([0.1, 0.2, 0.3, 0.2, 0.2])
    lg = np.log(p).astype(np.float32)[None, None]
    c = SE.cdf(lg, 1.0)[0, 0]
    a = np.array([[2]])
    u0 = np.array([[0.5]])
    for seed in range(4):
        pl = SE.place(lg, a, u0, 1.0, 1e-5, seed)
        assert pl.placed.all()
        want = c[2] - 1e-5 if pl.upper[0, 0] else c[1] + 1e-5
        assert pl.u[0, 0] == want and SE.oracle_select(lg, pl.u, True, 1.0)[0, 0] == 2
        moved = SE.oracle_select(lg, SE.control(pl, 1e-5), True, 1.0)[0, 0]
        assert moved == (3 if pl.upper[0, 0] else 1)
        assert SE.in_band(lg, pl.u, 1.0).all()
    # the outer arms take their interior edge; an interval no wider than 4 delta keeps u0
    assert SE.place(lg, np.array([[0]]), u0, 1.0, 1e-5, 0).upper.all()
    assert not SE.place(lg, np.array([[4]]), u0, 1.0, 1e-5, 0).upper.any()
    pl = SE.place(lg, a, u0, 1.0, 0.08, 0)
    assert not pl.placed.any() and pl.u[0, 0] == 0.5
    assert not SE.in_band(lg, np.array([[0.45]]), 1.0).any()


def _toy(steps, N, shift):
    """a rollout whose logits depend on its own past actions and whose cdf edges sit ``shift`` (signed per
    row) off numpy's, with the selection that is its definition: what the razor rounds meet on the device"""
    def edges(logits):
        sign = np.where(logits[..., 0] > 0, 1.0, -1.0)[..., None]
        return SE.cdf(logits, 1.0) + shift * sign

    def select(logits, u, sample, temp):
        return np.minimum((edges(logits) <= np.asarray(u)[..., None]).sum(-1), 4)

    def rollout(u):
        logits, acts = np.zeros((steps, N, 5), np.float32), np.zeros((steps, N), np.int64)
        h = np.arange(N, dtype=np.int64) + 1
        for t in range(steps):
            for j in range(N):
                logits[t, j] = np.random.RandomState(int(h[j] % (2 ** 31))).randn(5)
            acts[t] = select(logits[t], u[t], True, 1.0)
            h = h * 6364136223846793005 % (2 ** 61 - 1) + acts[t] + 7 * t
        return dict(logits=logits, actions=acts)
    return rollout, select


@pytest.mark.parametrize("steps", [8, 40])
def test_razor_rounds_on_a_rollout_that_decides_the_other_side(steps):
    """edges 5e-9 off numpy's: the steady runs and 1e-8, 1e-7 repeat run 1; at 1e-9 about half the re-placed
    steps fall the other way, each round moves every task's first departure on, and a rollout of no more
    steps than the round limit (16 here) ends with no departure and the in-band share of the issue (asserted inside)"""
    N = 6
    rollout, select = _toy(steps, N, 5e-9)
    u0 = np.random.RandomState(steps).uniform(size=(steps, N))
    lines = SE.run_case(f"toy {steps} steps", rollout, select, u0, seed=9, rounds=16)
    razor = {ln.split("delta=")[1].split()[0]: ln for ln in lines if " runs=" in ln}
    assert " runs=1 " in razor["1e-08"] and " runs=1 " in razor["1e-07"]
    assert " runs=1 " not in razor["1e-09"] and razor["1e-09"].endswith("same_as_run1=0")
    assert ("departs_nowhere=1" in razor["1e-09"]) == (steps <= 16)
    assert lines[-1].endswith(">= 1e-09, < 1e-06")
