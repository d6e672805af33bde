"""The fresh-task generator on the device (csrc/dpt_fresh.hip, dpt_hip.fresh_batch) at the cases of
tests/fresh_oracle.py:

1. against the numpy restatement: means, the cov and rand indices (recovered from probs_out), goals,
   permutations, queries, labels and every DarkRoom token bit-equal; probs_out within 4 ulp (the device's log
   against numpy's); the arm of every row equal (strict: tests/test_fresh_host.py holds the seeds to zero
   rollin draws within 1e-12 of a cdf step); the rewards bit-equal given the arm (Gaussian noise as the
   library reports its normals, the convention of tests/test_gpu_philox_paths.py);
2. composition: tokens and targets bit-identical to dpt_train_pack_batch over what dpt_rollin_bandit /
   dpt_rollin_darkroom give for the generator's own task outputs;
3. batch independence: tasks [0, 64) at once, as 1 + 3 + 60, and as two rank-style halves.
"""
import ctypes

import numpy as np
import pytest
import torch

import fresh_oracle as FO

pytestmark = pytest.mark.gpu


def bits(x):
    """a float array's bytes as integers (NaN-proof equality, -0.0 != 0.0)"""
    x = np.ascontiguousarray(x)
    return x.view({4: np.int32, 8: np.int64}[x.dtype.itemsize])


def host(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def bandit_env(A, H, btype, var):
    import dpt_hip
    return dpt_hip.FreshEnv.bandit(A, H, var, btype)


def darkroom_env(dim, H, G, with_perms):
    import dpt_hip
    return dpt_hip.FreshEnv.darkroom(dim, H, FO.goal_list(dim, G), FO.perm_list() if with_perms else None)


def pack(data, sd, A, H):
    """dpt_train_pack_batch over a dataset dict (identity index order) -> tokens, targets"""
    from dpt_hip import _lib, _p, _stream
    from dpt_hip import train as tr
    dd = tr.DeviceData(data)
    n = dd.n
    d = tr.desc(1, 32, sd, A, 1 + H, n, 1 + H)
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    tokens = torch.empty((n, 1 + H, 2 * sd + A + 1), dtype=torch.float32, device="cuda")
    targets = torch.empty((n, A), dtype=torch.float32, device="cuda")
    _lib.call("dpt_train_pack_batch", ctypes.byref(d), ctypes.byref(dd.struct), _p(idx), None, n, _p(tokens),
              _p(targets), _stream())
    return tokens.cpu().numpy(), targets.cpu().numpy()


def recover_policy_indices(probs, p):
    """the (cov index, rand index) pairs whose mixture of the Dirichlet part p reproduces probs, per task:
    boolean (n, 11, A).  p is the oracle's (within a few ulp of the device's), so a candidate matches
    within 16 ulp; grid points are 0.1 apart, far outside that."""
    A = p.shape[1]
    cov = FO.COV_GRID[None, :, None, None]
    cand = (1 - cov) * p[:, None, None, :] + cov * np.eye(A)[None, None, :, :]
    return (np.abs(cand - probs[:, None, None, :]) <= 16 * np.spacing(np.maximum(cand, 1e-300))).all(-1)


@pytest.mark.parametrize("case", FO.BANDIT_CASES, ids=lambda c: "seed%d-A%d-H%d-n%d-ft%d-type%d-var%g" % c)
def test_bandit_samples_match_the_oracle_and_the_rollin_kernel(case):
    import dpt_hip
    seed, A, H, n, ft, btype, var = case
    o = host(dpt_hip.fresh_batch(bandit_env(A, H, btype, var), seed, ft, n))
    t = FO.bandit_task(seed, ft, n, A)
    # 1. the task
    assert np.array_equal(bits(o["means"]), bits(t["means"]))
    err = np.abs(o["probs"] - t["probs"]) / np.spacing(np.maximum(t["probs"], 1e-300))
    print(f"probs: max {err.max():.2f} ulp from the oracle")
    assert err.max() <= 4
    match = recover_policy_indices(o["probs"], t["p"])
    for i in range(n):
        ci, ri = int(t["cov_index"][i]), int(t["rand_index"][i])
        assert set(np.nonzero(match[i].any(1))[0]) == {ci}, (i, ci)
        if ci > 0:  # at cov 0 the point mass has no weight: every arm reproduces probs
            assert set(np.nonzero(match[i, ci])[0]) == {ri}, (i, ri)
    best = FO.first_argmax(t["means"])
    assert np.array_equal(o["opt_action"], best)
    assert np.array_equal(bits(o["targets"]), bits(np.eye(A, dtype=np.float32)[best]))
    # the rows: one-hot arms equal to the oracle's, the rewards bit-equal given the arm
    tok = o["tokens"]
    assert tok.shape == (n, 1 + H, A + 3)
    onehot = tok[:, 1:, 1:1 + A]
    assert ((onehot == 0) | (onehot == 1)).all() and (onehot.sum(-1) == 1).all()
    arms = onehot.argmax(-1)
    want_arms, _ = FO.bandit_rollin(seed, ft, t["means"], t["probs"], H)
    assert np.array_equal(arms, want_arms)
    normals = None
    if btype == FO.GAUSSIAN and var != 0:
        normals = np.stack([dpt_hip.draw(1, seed, h, ft, n, dpt_hip.STREAM_REWARD).cpu().numpy() for h in range(H)], 1)
    rewards = FO.bandit_rewards(seed, ft, o["means"], arms, btype, var, normals)
    assert np.array_equal(bits(tok), bits(FO.bandit_tokens(arms, rewards, A)))
    # 2. composition: the rollin kernel on the generator's own task, then the pack
    acts, rews = dpt_hip.rollin_bandit(o["means"], o["probs"], H, var, btype, seed=seed, first_task=ft)
    ones = torch.ones((n, H, 1), dtype=torch.float32, device="cuda")
    data = {"query_states": ones[:, 0], "context_states": ones, "context_next_states": ones,
            "context_actions": torch.eye(A, dtype=torch.float32, device="cuda")[acts.long()],
            "context_rewards": rews.to(torch.float32),
            "optimal_actions": torch.eye(A, dtype=torch.float32)[torch.from_numpy(o["means"].argmax(1))].cuda()}
    ptok, ptgt = pack(data, 1, A, H)
    assert np.array_equal(bits(tok), bits(ptok)) and np.array_equal(bits(o["targets"]), bits(ptgt))


@pytest.mark.parametrize("case", FO.DARKROOM_CASES, ids=lambda c: "seed%d-dim%d-H%d-n%d-ft%d-G%d-perm%d" % c)
def test_darkroom_samples_match_the_oracle_and_the_rollin_kernel(case):
    import dpt_hip
    seed, dim, H, n, ft, G, with_perms = case
    env = darkroom_env(dim, H, G, with_perms)
    o = host(dpt_hip.fresh_batch(env, seed, ft, n))
    r = FO.darkroom(seed, ft, n, H, dim, FO.goal_list(dim, G), FO.perm_list() if with_perms else None)
    # 1. everything bit-equal
    assert np.array_equal(o["goal"], r["goal"]) and np.array_equal(o["query"], r["query"])
    assert np.array_equal(o["perm"], r["perm"] if with_perms else np.tile(np.arange(5), (n, 1)))
    assert np.array_equal(o["opt_action"], r["opt_action"])
    assert np.array_equal(bits(o["tokens"]), bits(r["tokens"]))
    assert np.array_equal(bits(o["targets"]), bits(r["targets"]))
    if H >= 300 and dim > 2:  # the rollin really moves and sometimes stands on the goal
        assert 0 < o["tokens"][:, 1:, 9].mean() < 0.5
    # 2. composition: the rollin kernel on the generator's own goals and permutations, then the pack
    k = dpt_hip.rollin_darkroom(o["goal"], H, dim, o["perm"] if with_perms else None, seed=seed, first_task=ft)
    assert np.array_equal(k["query"].cpu().numpy(), o["query"])
    assert np.array_equal(k["opt_action"].cpu().numpy(), o["opt_action"])
    f = torch.float32
    data = {"query_states": k["query"].to(f), "context_states": k["states"].to(f),
            "context_next_states": k["next_states"].to(f), "context_rewards": k["rewards"].to(f),
            "context_actions": torch.eye(5, dtype=f, device="cuda")[k["actions"].long()],
            "optimal_actions": torch.eye(5, dtype=f, device="cuda")[k["opt_action"].long()]}
    ptok, ptgt = pack(data, 2, 5, H)
    assert np.array_equal(bits(o["tokens"]), bits(ptok)) and np.array_equal(bits(o["targets"]), bits(ptgt))


def _joined(env, seed, cuts):
    import dpt_hip
    parts = [host(dpt_hip.fresh_batch(env, seed, lo, hi - lo)) for lo, hi in zip(cuts[:-1], cuts[1:])]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


@pytest.mark.parametrize("kind", ["bandit", "darkroom"])
def test_a_sample_does_not_depend_on_how_the_run_is_cut(kind):
    """tasks [0, 64) at once == 1 + 3 + 60 == the rank-style blocks [0, 32) + [32, 64), byte for byte"""
    if kind == "bandit":
        seed, A, H, btype, var = FO.SPLIT_BANDIT
        env = bandit_env(A, H, btype, var)
    else:
        seed, dim, H, G, with_perms = FO.SPLIT_DARKROOM
        env = darkroom_env(dim, H, G, with_perms)
    whole = _joined(env, seed, [0, 64])
    for cuts in ([0, 1, 4, 64], [0, 32, 64]):
        got = _joined(env, seed, cuts)
        assert set(got) == set(whole)
        for k in whole:
            assert np.array_equal(whole[k].view(np.uint8), got[k].view(np.uint8)), (cuts, k)
    # and the samples differ from each other and from another key's
    assert len({whole["tokens"][i].tobytes() for i in range(64)}) == 64
    assert not np.array_equal(_joined(env, seed + 1, [0, 64])["tokens"], whole["tokens"])
