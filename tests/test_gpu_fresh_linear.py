"""The linear bandit's fresh-task generator on the device (csrc/dpt_fresh_linear.hip, dpt_hip.fresh_batch on
``FreshEnv.linear_bandit``) at the cases of tests/fresh_linear_oracle.py:

1. against the numpy restatement fed the library's own normals (``dpt_hip.draw``): theta, means, the label,
   the action of every row and every token bit-equal -- tests/test_fresh_linear_host.py holds every case's
   arg-max gap above 1e-9, so the comparison is strict; under the uniform rollin probs within 4 ulp and the
   arms strict (no cdf near-tie at 1e-12), as tests/test_gpu_fresh.py;
2. composition: tokens and targets bit-identical to dpt_train_pack_batch over what dpt_rollout_policy
   (Thompson, sample, ts_std = var, prior 0 / 1) gives on the generator's own means -- and two controls the
   comparison rejects: the policy's default prior, and ts_std 0.1 at var 0.3; the uniform rollin the same over
   dpt_rollin_bandit on means_out / probs_out;
3. batch independence: tasks [0, 64) at once, as 1 + 3 + 60, and as two halves by first_task;
4. repeatability, and dirty buffers / a non-default stream behind a delay: the same bytes.
"""
import functools

import numpy as np
import pytest
import torch

import entry_point_cases as EC
import fresh_linear_oracle as LO
import fresh_oracle as FO
from test_gpu_dirty_buffers import run_case
from test_gpu_fresh import bits, host, pack
from test_gpu_side_stream import on_side_stream, reference

pytestmark = pytest.mark.gpu

ALL_CASES = LO.CASES + LO.H_CASES


def env_of(A, d, H, var, rollin):
    import dpt_hip
    return dpt_hip.FreshEnv.linear_bandit(LO.arms_of(A, d), H, var, rollin)


def check_task(o, seed, ft, n, A, d):
    """theta, means, label and target against the oracle on the library's normals: bit-equal"""
    import dpt_hip
    t = LO.task(seed, ft, n, LO.arms_of(A, d), draw=dpt_hip.draw)
    assert np.array_equal(bits(o["theta"]), bits(t["theta"]))
    assert np.array_equal(bits(o["means"]), bits(t["means"]))
    assert np.array_equal(o["opt_action"], t["opt_action"])
    assert np.array_equal(bits(o["targets"]), bits(np.eye(A, dtype=np.float32)[t["opt_action"]]))
    # numpy's own normals give the same task to 1e-12
    assert np.abs(LO.task(seed, ft, n, LO.arms_of(A, d))["means"] - o["means"]).max() < 1e-12
    return t


def arms_of_tokens(tok, A):
    onehot = tok[:, 1:, 1:1 + A]
    assert ((onehot == 0) | (onehot == 1)).all() and (onehot.sum(-1) == 1).all()
    return onehot.argmax(-1)


def packed(acts, rews, means, A, H):
    """dpt_train_pack_batch over a bandit dataset of these actions and rewards"""
    n = acts.shape[0]
    ones = torch.ones((n, H, 1), dtype=torch.float32, device="cuda")
    data = {"query_states": torch.ones((n, 1), dtype=torch.float32, device="cuda"), "context_states": ones,
            "context_next_states": ones,
            "context_actions": torch.eye(A, dtype=torch.float32, device="cuda")[acts.long()].reshape(n, H, A),
            "context_rewards": rews.to(torch.float32).reshape(n, H),
            "optimal_actions": torch.eye(A, dtype=torch.float32)[torch.from_numpy(means.argmax(1))].cuda()}
    return pack(data, 1, A, H)


@pytest.mark.parametrize("case", ALL_CASES, ids=LO.case_id)
def test_thompson_samples_match_the_oracle_and_the_policy_kernel(case):
    import dpt_hip
    seed, ft, n, A, d, H, var = case
    o = host(dpt_hip.fresh_batch(env_of(A, d, H, var, "thompson"), seed, ft, n))
    assert "probs" not in o
    # 1. the task and the chain
    t = check_task(o, seed, ft, n, A, d)
    tok = o["tokens"]
    assert tok.shape == (n, 1 + H, A + 3)
    r = LO.thompson(t["means"], var, *LO.chain_normals(seed, ft, n, A, H, draw=dpt_hip.draw))
    print(f"minimum gap on the library's normals: {r['gap']:.3g}")
    assert r["gap"] > 1e-9
    assert np.array_equal(arms_of_tokens(tok, A), r["actions"])
    assert np.array_equal(bits(tok), bits(FO.bandit_tokens(r["actions"], r["rewards"], A)))
    if H == 0:
        return
    # 2. composition: the policy kernel on the generator's own means, then the pack
    roll = functools.partial(dpt_hip.rollout_policy, dpt_hip.POLICY_THOMPSON, o["means"], H, var, sample=True,
                             seed=seed, first_task=ft)
    k = roll(ts_std=var, ts_prior_mean=0.0, ts_prior_var=1.0)
    ptok, ptgt = packed(k["actions"], k["rewards"], o["means"], A, H)
    assert np.array_equal(bits(tok), bits(ptok)) and np.array_equal(bits(o["targets"]), bits(ptgt))
    if case in LO.CASES and var == 0.3:  # the controls: another prior, another policy std
        for other in (dict(ts_std=var), dict(ts_std=0.1, ts_prior_mean=0.0, ts_prior_var=1.0)):
            c = roll(**other)
            ctok, _ = packed(c["actions"], c["rewards"], o["means"], A, H)
            assert not np.array_equal(bits(tok), bits(ctok)), other


@pytest.mark.parametrize("case", LO.CASES + LO.H_CASES[:2] + LO.H_CASES[-1:], ids=LO.case_id)
def test_uniform_samples_match_the_oracle_and_the_rollin_kernel(case):
    import dpt_hip
    seed, ft, n, A, d, H, var = case
    o = host(dpt_hip.fresh_batch(env_of(A, d, H, var, "uniform"), seed, ft, n))
    t = check_task(o, seed, ft, n, A, d)
    u = LO.uniform_policy(seed, ft, n, A, d)
    err = np.abs(o["probs"] - u["probs"]) / np.spacing(np.maximum(u["probs"], 1e-300))
    print(f"probs: max {err.max():.2f} ulp from the oracle")
    assert err.max() <= 4
    tok = o["tokens"]
    arms = arms_of_tokens(tok, A)
    want_arms, _ = FO.bandit_rollin(seed, ft, t["means"], u["probs"], H)
    assert np.array_equal(arms, want_arms)
    normals = LO.normals(seed, np.arange(H), ft, n, LO.STREAM_REWARD, draw=dpt_hip.draw)
    rewards = FO.bandit_rewards(seed, ft, o["means"], arms, FO.GAUSSIAN, var, normals)
    assert np.array_equal(bits(tok), bits(FO.bandit_tokens(arms, rewards, A)))
    if H == 0:
        return
    acts, rews = dpt_hip.rollin_bandit(o["means"], o["probs"], H, var, FO.GAUSSIAN, seed=seed, first_task=ft)
    ptok, ptgt = packed(acts, rews, o["means"], A, H)
    assert np.array_equal(bits(tok), bits(ptok)) and np.array_equal(bits(o["targets"]), bits(ptgt))
    # the two rollins share the task and differ in the rows
    th = host(dpt_hip.fresh_batch(env_of(A, d, H, var, "thompson"), seed, ft, n))
    assert np.array_equal(bits(th["means"]), bits(o["means"])) and np.array_equal(th["targets"], o["targets"])
    if H >= 17 and A > 1:
        assert not np.array_equal(th["tokens"], tok)


def _joined(env, seed, cuts):
    import dpt_hip
    parts = [host(dpt_hip.fresh_batch(env, seed, lo, hi - lo)) for lo, hi in zip(cuts[:-1], cuts[1:])]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


@pytest.mark.parametrize("rollin", ["thompson", "uniform"])
def test_a_sample_does_not_depend_on_how_the_run_is_cut(rollin):
    """tasks [0, 64) at once == 1 + 3 + 60 == the halves [0, 32) + [32, 64), byte for byte; and twice the same"""
    seed, A, d, H, var = LO.SPLIT
    env = env_of(A, d, H, var, rollin)
    whole = _joined(env, seed, [0, 64])
    for cuts in ([0, 64], [0, 1, 4, 64], [0, 32, 64]):
        got = _joined(env, seed, cuts)
        assert set(got) == set(whole)
        for k in whole:
            assert np.array_equal(whole[k].view(np.uint8), got[k].view(np.uint8)), (cuts, k)
    assert len({whole["tokens"][i].tobytes() for i in range(64)}) == 64
    assert not np.array_equal(_joined(env, seed + 1, [0, 64])["tokens"], whole["tokens"])


# ----------------------------------------------------------------------------- dirty buffers, side streams
A_ISO, D_ISO = 9, 3


def arm_inputs(seed):
    return dict(arms=EC.f64(EC.rs_of(seed, 43).normal(size=(A_ISO, D_ISO)) / np.sqrt(D_ISO)))


def batch_call(rollin, H, obj, inp, dirty):
    import dpt_hip
    env = dpt_hip.FreshEnv.linear_bandit(inp["arms"], H, 0.3, rollin)
    assert env.arms.data_ptr() == inp["arms"].data_ptr()
    return dpt_hip.fresh_batch(env, 35, 2 ** 33 + 5, 5)


def trainer_case(rollin):
    from dpt_hip import train as tr
    Hm = 12
    model = functools.partial(EC.transformer, 32, 2, Hm, 1, A_ISO, 140)

    def inputs(seed):
        return dict(blob=EC.blob_of(model(), seed), **arm_inputs(seed))

    def prepare(inp):
        import dpt_hip
        t = tr.FreshTrainer(model(), dpt_hip.FreshEnv.linear_bandit(inp["arms"], Hm, 0.3, rollin), lr=1e-3, seed=36,
                            first_task=7)
        t.state.blob = inp["blob"]
        return t

    def call(t, inp, dirty):
        t.step(8)
        dirty(t._ws)
        t.step(5)
        dirty(t._ws)
        t.eval_loss(100, 11, seed=37, batch=8)
        return dict(blob=t.blob, m=t.m, v=t.v, loss=t.loss)
    return EC.Case(f"fresh_trainer-linear-{rollin}", inputs, call, prepare)


# H 150: five chunks of the Thompson chain, the last one partial; H 300: the uniform lanes take a second chunk of steps
ISO_CASES = [EC.Case("fresh_batch-linear-thompson", arm_inputs, functools.partial(batch_call, "thompson", 150)),
             EC.Case("fresh_batch-linear-uniform", arm_inputs, functools.partial(batch_call, "uniform", 300)),
             trainer_case("thompson"), trainer_case("uniform")]


@pytest.mark.parametrize("case", ISO_CASES, ids=[c.name for c in ISO_CASES])
def test_results_do_not_depend_on_what_the_buffers_held(case):
    clean, log = run_case(case, 0x00)
    again, _ = run_case(case, 0x00)
    assert not EC.same_bytes(clean, again), f"not reproducible on clean buffers: {EC.same_bytes(clean, again)}"
    assert len(log) >= 1, "nothing allocated through torch.empty: the poison reached no buffer"
    for pattern in (0xFF, 0x7F):
        got, _ = run_case(case, pattern)
        diff = EC.same_bytes(clean, got)
        assert not diff, f"pattern {pattern:#04x}: {diff} differ from the run on zeroed buffers"


@pytest.mark.parametrize("case", ISO_CASES, ids=[c.name for c in ISO_CASES])
def test_side_stream_behind_a_delay(case):
    ref, run_ms = reference(case)
    got, busy = on_side_stream(case, run_ms)
    assert busy, (f"the stream was idle when the binding returned (run time {run_ms:.2f} ms): the call blocked "
                  f"the host, or the delay was too short to prove anything")
    diff = EC.same_bytes(ref, got)
    assert not diff, f"{diff} differ from the default-stream reference: a launch, memset or copy off the given stream"
