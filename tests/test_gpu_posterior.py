"""The Bayes posterior of the optimal action on the device (csrc/dpt_posterior.hip; include/dpt_hip.h, "Bayes
posterior of the optimal action") against its numpy restatement tests/posterior_oracle.py, which
tests/test_posterior_host.py holds to Monte Carlo and to the generator.

- dpt_bandit_posterior: N = 3 tasks at every A in {1, 2, 5, 32} x G in {64, 192, 1024, 8192} x H in {0, 1, 7,
  65} for Gaussian rewards of std 0.3 and 0.05 and for Bernoulli rewards (every A meets G = 8192: A = 1 keeps
  its weights in LDS there, the others take the workspace path).  The tasks hold a 1e-3 near-tie with two
  out-of-range actions, all pulls on one arm (Bernoulli: all rewards 1), and means at both ends of [0, 1]
  (Bernoulli: all rewards 0).  Bar: relative 1e-9 on every entry >= 1e-100, absolute 1e-100 below.  The
  log-likelihoods are bit-equal by construction (same operation order, no fused multiply-add); exp / log
  differ by a few ulp on arguments of magnitude <= 1e5, i.e. 1e5 * 2^-53 absolute; sums of <= 8192
  non-negative terms differ by <= G * 2^-53: together about 1e-12, so the bar leaves three orders of margin.
- Row 0 is 1 / A to 1e-12, repeated calls are bit-identical, and a task's rows are the same bits alone, among
  70 tasks and under chunk=2.
- dpt_darkroom_posterior: bit-equal to the oracle (``consistent`` included) on dpt_rollin_darkroom's records
  and on a hand-made contradictory record.
- dpt_posterior_compare: rtol 1e-12 against numpy, with a zero posterior entry and an infinite nll_bayes.
- End to end on the device generator: calibration of the kernel's posterior, train_fresh.py --bayes_floor
  against the oracle's floor, evals/eval_posterior.py on random models of width 32 and 16.
- Every new entry point under dirty buffers and on a side stream behind a delay, byte for byte."""
import functools
import importlib
import json
import os

import numpy as np
import pytest
import torch

import buffer_poison as BP  # noqa: F401  (the helpers below use it through the two modules)
import entry_point_cases as EC
import fresh_oracle as FO
import posterior_oracle as PO

pytestmark = pytest.mark.gpu

H_MAX, HS = 65, (0, 1, 7, 65)
KINDS = {"gauss0.3": (PO.GAUSSIAN, 0.3), "gauss0.05": (PO.GAUSSIAN, 0.05), "bernoulli": (PO.BERNOULLI, 0.3)}


@functools.lru_cache(maxsize=None)
def records(kind, A):
    """actions (3, 65) int32 / rewards (3, 65) of the three tasks of the module docstring"""
    bandit_type, var = KINDS[kind]
    rs = np.random.RandomState(100 * A + len(kind))
    H = H_MAX
    means = rs.uniform(0, 1, (3, A))
    means[0, 0], means[0, 1 % A] = 0.5, 0.501  # (A = 1: the one arm)
    means[2] = np.where(np.arange(A) % 2 == 0, 0.001, 0.999)
    acts = rs.randint(0, A, (3, H)).astype(np.int32)
    acts[1] = A - 1
    mu = np.take_along_axis(means, acts, 1)
    if bandit_type == PO.BERNOULLI:
        rews = (rs.uniform(size=mu.shape) < mu).astype(np.float64)
        rews[1], rews[2] = 1.0, 0.0
    else:
        rews = mu + var * rs.normal(size=mu.shape)
    acts[0, 0], acts[0, 5] = A, -1  # out of range: the first one is inside every H >= 1
    return acts, rews


@functools.lru_cache(maxsize=None)
def oracle(kind, A, G):
    bandit_type, var = KINDS[kind]
    acts, rews = records(kind, A)
    return PO.bandit_posterior(acts, rews, A, var, bandit_type, G)


def assert_close(got, ref, what):
    big = np.abs(ref) >= 1e-100
    err = np.abs(got - ref)
    rel = (err[big] / np.abs(ref[big])).max() if big.any() else 0.0
    small = err[~big].max() if (~big).any() else 0.0
    print(f"{what}: max relative error {rel:.3e} on {big.sum()} entries >= 1e-100, max absolute {small:.3e} below")
    assert np.isfinite(got).all() and rel <= 1e-9 and small <= 1e-100, what


@pytest.mark.parametrize("G", [64, 192, 1024, 8192])
@pytest.mark.parametrize("A", [1, 2, 5, 32])
@pytest.mark.parametrize("kind", list(KINDS))
def test_bandit_posterior_against_the_oracle(kind, A, G):
    import dpt_hip
    bandit_type, var = KINDS[kind]
    acts, rews = records(kind, A)
    ref = oracle(kind, A, G)
    for H in HS:
        got = dpt_hip.bandit_posterior(acts[:, :H], rews[:, :H], A, var, bandit_type, grid=G)
        assert got.shape == (3, H + 1, A) and got.dtype == torch.float64
        got = got.cpu().numpy()
        assert_close(got, ref[:, :H + 1], f"{kind} A={A} G={G} H={H}")
        assert np.abs(got[:, 0] - 1 / A).max() <= 1e-12
        assert np.abs(got.sum(-1) - 1).max() <= 1e-12
        if H >= 1:
            assert np.array_equal(got[0, 1], got[0, 0])  # the out-of-range first action leaves the row unchanged
        if A == 1:
            assert np.array_equal(got, np.ones_like(got))


@pytest.mark.parametrize("A,G", [(5, 1024), (2, 8192)], ids=["lds", "workspace"])
@pytest.mark.parametrize("kind", ["gauss0.3", "bernoulli"])
def test_bandit_posterior_is_reproducible_and_independent_of_the_batch(kind, A, G):
    import dpt_hip
    bandit_type, var = KINDS[kind]
    acts, rews = records(kind, A)
    H = 7
    acts, rews = acts[:, :H], rews[:, :H]
    one = dpt_hip.bandit_posterior(acts, rews, A, var, bandit_type, grid=G)
    again = dpt_hip.bandit_posterior(acts, rews, A, var, bandit_type, grid=G)
    assert torch.equal(one.view(torch.int64), again.view(torch.int64))
    # the same three tasks at rows 11, 40 and 69 of 70
    rs = np.random.RandomState(9)
    big_a = rs.randint(0, A, (70, H)).astype(np.int32)
    big_r = rs.uniform(0, 1, (70, H)).round() if bandit_type else rs.normal(0.5, 0.3, (70, H))
    at = [11, 40, 69]
    big_a[at], big_r[at] = acts, rews
    many = dpt_hip.bandit_posterior(big_a, big_r, A, var, bandit_type, grid=G)
    assert torch.equal(many[at].view(torch.int64), one.view(torch.int64))
    for chunk in (2, 33):
        split = dpt_hip.bandit_posterior(big_a, big_r, A, var, bandit_type, grid=G, chunk=chunk)
        assert torch.equal(split.view(torch.int64), many.view(torch.int64))
    default = dpt_hip.bandit_posterior(acts, rews, A, var, bandit_type)  # G = posterior_grid(var, 7, type) = 256
    assert_close(default.cpu().numpy(), PO.bandit_posterior(acts, rews, A, var, bandit_type, 256), "default grid")


# ----------------------------------------------------------------------------- DarkRoom
def goal_lists(dim):
    rs = np.random.RandomState(dim)
    cells = np.array([(x, y) for x in range(dim) for y in range(dim)], np.int32)
    seven = cells[rs.permutation(len(cells))[:7]]
    return {"one": cells[4:5], "seven": seven, "repeats": np.concatenate([seven[:4], seven[:2], seven[:1], cells[:70]])}


@pytest.mark.parametrize("H", [0, 1, 33])
@pytest.mark.parametrize("which", ["one", "seven", "repeats"])
@pytest.mark.parametrize("dim", [3, 10])
def test_darkroom_posterior_is_the_count(dim, which, H):
    import dpt_hip
    goals = goal_lists(dim)[which]
    rs = np.random.RandomState(7 * dim + H)
    N = 9
    true_goal = goals[rs.randint(0, len(goals), N)]
    if H == 0:  # no record: the prior's counts at a query of the test's own
        query, ns, rw = rs.randint(0, dim, (N, 2)).astype(np.int32), np.zeros((N, 0, 2), np.int32), np.zeros((N, 0), np.int32)
    else:
        rec = dpt_hip.rollin_darkroom(true_goal, H, dim=dim, seed=21 + H, first_task=3)
        query, ns, rw = (rec[k].cpu().numpy().copy() for k in ("query", "next_states", "rewards"))
    if H >= 1:  # sample 0 contradicts itself: a reward at a goal cell, then (H = 33) the same cell without one
        ns[0, 0], rw[0, 0] = goals[0], 1
        if H > 1:
            ns[0, 1], rw[0, 1] = goals[0], 0
    post, cons = dpt_hip.darkroom_posterior(goals, query, ns, rw, dim, want_consistent=True)
    ref_post, ref_cons = PO.darkroom_posterior(goals, query, ns, rw)
    assert post.shape == (N, H + 1, 5) and cons.shape == (N, H + 1) and cons.dtype == torch.int32
    assert np.array_equal(cons.cpu().numpy(), ref_cons)
    assert np.array_equal(post.cpu().numpy().view(np.int64), ref_post.view(np.int64))
    alone = dpt_hip.darkroom_posterior(goals, query, ns, rw, dim)
    assert torch.equal(alone.view(torch.int64), post.view(torch.int64))
    if H > 1:
        assert ref_cons[0, 2] == 0 and not post[0, 2:].any()
    # the true goal stays consistent with the generator's own records, and the label keeps posterior mass
    if H >= 1:
        opt = rec["opt_action"].cpu().numpy()
        assert (ref_cons[1:] >= 1).all() and (ref_post[np.arange(1, N), -1, opt[1:]] > 0).all()


# ----------------------------------------------------------------------------- compare
@pytest.mark.parametrize("A", [1, 5, 32])
@pytest.mark.parametrize("T", [1, 66])
def test_posterior_compare_against_numpy(T, A):
    import dpt_hip
    rs = np.random.RandomState(10 * T + A)
    N = 70
    # (numpy's one-element Dirichlet is x * (1 / x), not always 1.0: one action has posterior exactly 1)
    post = rs.dirichlet(np.ones(A), (N, T)) if A > 1 else np.ones((N, T, 1))
    logits = (3 * rs.normal(size=(N, T, A))).astype(np.float32)
    targets = rs.randint(0, A, N)
    if A > 1:
        post[3, 0, targets[3]] = 0.0  # a zero entry at the target: nll_bayes = +inf, kl and entropy skip it
        post[3, 0] /= post[3, 0].sum()
        post[5, T - 1, (targets[5] + 1) % A] = 0.0  # a zero entry elsewhere
        post[5, T - 1] /= post[5, T - 1].sum()
    got = dpt_hip.posterior_compare(post, logits, targets)
    ref = PO.compare(post, logits, targets)
    for k in ("nll_model", "nll_bayes", "kl", "entropy"):
        g = got[k].cpu().numpy()
        assert g.shape == (N, T)
        np.testing.assert_allclose(g, ref[k], rtol=1e-12, atol=0, err_msg=k)
    if A > 1:
        assert np.isposinf(got["nll_bayes"][3, 0].item()) and np.isfinite(got["kl"].cpu().numpy()).all()
    else:
        assert not got["kl"].any() and not got["entropy"].any() and not got["nll_bayes"].any()


# ----------------------------------------------------------------------------- end to end on the device generator
@pytest.mark.parametrize("bandit_type", ["uniform", "bernoulli"])
def test_calibration_of_the_kernel_on_the_device_generator(bandit_type):
    """4,096 fresh samples, H = 40, 5 arms, std 0.3, the default grid: E[nll] = E[entropy] within |z| <= 4.5"""
    import dpt_hip
    env = dpt_hip.FreshEnv.bandit(5, 40, 0.3, bandit_type)
    batch = dpt_hip.fresh_batch(env, 20240611, 0, 4096)
    post, targets = dpt_hip.fresh_posterior(env, batch)
    c = dpt_hip.posterior_compare(post, torch.zeros(post.shape, dtype=torch.float32, device=post.device), targets)
    d = (c["nll_bayes"] - c["entropy"])[:, 1:].mean(1).cpu().numpy()
    z = d.mean() / (d.std(ddof=1) / np.sqrt(len(d)))
    print(f"{bandit_type}: z {z:.3f}, nll {c['nll_bayes'][:, 1:].mean().item():.5f}, "
          f"entropy {c['entropy'][:, 1:].mean().item():.5f}")
    assert np.isfinite(d).all() and abs(z) <= 4.5


@pytest.mark.parametrize("env", ["bandit", "bandit_thompson", "darkroom", "darkroom_heldout"])
def test_train_fresh_bayes_floor_is_the_oracles(env, tmp_path, monkeypatch):
    import dpt_hip
    train_fresh = importlib.import_module("train_fresh")
    monkeypatch.chdir(tmp_path)
    H, dim = 12, 5
    flags = ["--env", env, "--envs", "320", "--H", str(H), "--dim", str(dim), "--num_epochs", "1", "--layer", "2",
             "--var", "0.3"]
    train_fresh.main(flags + ["--bayes_floor"])
    logs = [f for f in os.listdir(tmp_path / "figs" / "loss") if f.endswith("_logs.txt")]
    assert len(logs) == 1
    log = open(tmp_path / "figs" / "loss" / logs[0]).read()
    lines = [x for x in log.splitlines() if x.startswith("\tBayes floor (test): ")]
    assert len(lines) == 1 and log.index("\tBayes floor (test): ") < log.index("Epoch: 1")
    floor = float(lines[0].split(": ")[1])
    # the oracle on the same 64 test samples (320 - int(0.8 * 320)), read from the generator's tokens
    key = train_fresh.generator_key(0, "test")
    if env.startswith("darkroom"):
        fenv = dpt_hip.FreshEnv.darkroom(dim, H, train_fresh.darkroom_goals(env, dim)[1])
    else:
        fenv = dpt_hip.FreshEnv.bandit(dim, H, 0.3, "uniform" if env == "bandit" else "bernoulli")
    batch = dpt_hip.fresh_batch(fenv, key, 0, 64)
    tok, tg = batch["tokens"].cpu().numpy(), batch["opt_action"].cpu().numpy()
    if env.startswith("darkroom"):
        ref = PO.darkroom_posterior(fenv.goals.cpu().numpy(), tok[:, 0, :2].astype(np.int32),
                                    tok[:, 1:, 7:9].astype(np.int32), tok[:, 1:, 9].astype(np.int32))[0]
    else:
        ref = PO.bandit_posterior(tok[:, 1:, 1:1 + dim].argmax(-1).astype(np.int32), tok[:, 1:, 2 + dim].astype(np.float64),
                                  dim, 0.3, fenv.type, dpt_hip.posterior_grid(0.3, H, fenv.type))
    want = PO.bayes_floor(ref, tg)
    print(f"{env}: floor {floor!r}, oracle {want!r}")
    assert np.isfinite(want) and want > 0 and abs(floor - want) <= 1e-9
    # without the flag the log is the same but for that line (and the times)
    monkeypatch.chdir(tmp_path / "figs")  # a fresh run directory
    train_fresh.main(flags)
    log2 = open(tmp_path / "figs" / "figs" / "loss" / logs[0]).read()
    strip = lambda s: [x for x in s.splitlines() if " time: " not in x]  # noqa: E731
    assert "Bayes floor" not in log2 and strip(log2) == [x for x in strip(log) if not x.startswith("\tBayes floor")]


@pytest.mark.parametrize("embd,env,context", [(32, "bandit", "fresh"), (16, "bandit", "online"),
                                              (32, "bandit_thompson", "online"), (16, "darkroom", "fresh"),
                                              (32, "darkroom_heldout", "fresh")])
def test_eval_posterior_runs(embd, env, context, tmp_path, monkeypatch):
    from models.net import Transformer
    ev = importlib.import_module("evals.eval_posterior")
    monkeypatch.chdir(tmp_path)
    H, dim = 10, 5
    dark = env.startswith("darkroom")
    torch.manual_seed(embd)
    model = Transformer(dict(horizon=H, state_dim=2 if dark else 1, action_dim=5 if dark else dim, n_layer=2,
                             n_embd=embd, n_head=1, dropout=0, test=True))
    torch.save(model.state_dict(), tmp_path / "model.pt")
    ev.main(["--env", env, "--context", context, "--n_eval", "8", "--H", str(H), "--dim", str(dim), "--embd", str(embd),
             "--layer", "2", "--var", "0.3", "--model_path", str(tmp_path / "model.pt"), "--chunk", "3"])
    out = tmp_path / "figs" / "eval_posterior"
    assert (out / "posterior_gap.png").stat().st_size > 0
    res = json.load(open(out / "posterior_gap.json"))
    for k in ev.KEYS:
        assert len(res[k]["mean"]) == H + 1 and len(res[k]["sem"]) == H + 1
    kl = np.array(res["kl"]["mean"])
    assert np.isfinite(kl).all() and (kl >= -1e-12).all()
    assert np.isfinite(res["nll_model"]["mean"]).all() and np.isfinite(res["entropy"]["mean"]).all()
    if not dark:  # before any pull the posterior is the prior: every arm 1 / A
        assert abs(res["p_opt_bayes"]["mean"][0] - 1 / dim) <= 1e-12 and res["p_opt_bayes"]["sem"][0] <= 1e-12


# ----------------------------------------------------------------------------- dirty buffers and a side stream
def _cases():
    import dpt_hip
    cases = []

    def bandit(name, N, H, A, G, bandit_type, chunk):
        def inputs(seed):
            rs = EC.rs_of(seed, 40)
            r = rs.randint(0, 2, (N, H)) if bandit_type else rs.normal(0.5, 0.4, (N, H))
            return dict(actions=EC.i32(rs.randint(0, A, (N, H))), rewards=EC.f64(r))

        def call(obj, inp, dirty):
            return dict(post=dpt_hip.bandit_posterior(inp["actions"], inp["rewards"], A, 0.3, bandit_type, grid=G,
                                                      chunk=chunk))
        cases.append(EC.Case(name, inputs, call))
    bandit("bandit_posterior-lds-gaussian", 5, 9, 5, 256, PO.GAUSSIAN, 0)
    bandit("bandit_posterior-lds-bernoulli-chunk2", 5, 9, 5, 1024, PO.BERNOULLI, 2)
    bandit("bandit_posterior-workspace-gaussian", 3, 5, 2, 8192, PO.GAUSSIAN, 0)
    bandit("bandit_posterior-workspace-bernoulli-chunk2", 3, 5, 3, 8192, PO.BERNOULLI, 2)

    def dr_inputs(seed):
        rs = EC.rs_of(seed, 41)
        return dict(goals=EC.i32(rs.randint(0, 4, (80, 2))), query=EC.i32(rs.randint(0, 4, (6, 2))),
                    next_states=EC.i32(rs.randint(0, 4, (6, 11, 2))), rewards=EC.i32(rs.randint(0, 2, (6, 11)) * (rs.uniform(size=(6, 11)) < 0.2)))

    def dr_call(obj, inp, dirty):
        post, cons = dpt_hip.darkroom_posterior(inp["goals"], inp["query"], inp["next_states"], inp["rewards"], 4,
                                                want_consistent=True)
        return dict(post=post, consistent=cons)
    cases.append(EC.Case("darkroom_posterior", dr_inputs, dr_call))

    def pc_inputs(seed):
        rs = EC.rs_of(seed, 42)
        return dict(post=EC.f64(rs.dirichlet(np.ones(5), (67, 7))), logits=EC.f32(rs.normal(size=(67, 7, 5))),
                    targets=EC.i64(rs.randint(0, 5, 67)))

    def pc_call(obj, inp, dirty):
        return dpt_hip.posterior_compare(inp["post"], inp["logits"], inp["targets"])
    cases.append(EC.Case("posterior_compare", pc_inputs, pc_call))
    return cases


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_results_do_not_depend_on_what_the_buffers_held(case):
    from test_gpu_dirty_buffers import run_case
    clean, log = run_case(case, 0x00)
    again, _ = run_case(case, 0x00)
    assert not EC.same_bytes(clean, again)
    assert len(log) >= 1, "nothing allocated through torch.empty: the poison reached no buffer"
    for pattern in (0xFF, 0x7F):
        got, _ = run_case(case, pattern)
        diff = EC.same_bytes(clean, got)
        assert not diff, f"pattern {pattern:#04x}: {diff} differ from the run on zeroed buffers"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_side_stream_behind_a_delay(case):
    from test_gpu_side_stream import on_side_stream, reference
    ref, run_ms = reference(case)
    got, busy = on_side_stream(case, run_ms)
    assert busy, f"the stream was idle when the binding returned (run time {run_ms:.2f} ms)"
    diff = EC.same_bytes(ref, got)
    assert not diff, f"{diff} differ from the default-stream reference: a launch off the given stream"
