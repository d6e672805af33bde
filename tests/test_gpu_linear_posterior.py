"""The linear bandit's Bayes posterior of the optimal arm at lin_d = 2 on the device
(csrc/dpt_posterior_linear.hip; include/dpt_hip.h, "Linear bandit, lin_d = 2") against its numpy restatement
tests/linear_posterior_oracle.py, which tests/test_linear_posterior_host.py holds to Monte Carlo.

- dpt_linear_posterior: N = 7 tasks at every A in {2, 5, 20, 32} x G in {64, 256} x H in {0, 1, 37}, at reward
  std 0.3 and 0.05.  The tasks (linear_posterior_oracle.gpu_records) hold the actions -1 and A, a leading run of
  four invalid actions (rows 1 .. 4 still the prior), rewards all 0 (the mean at the apex), every pull on one
  arm (at std 0.05 a concentrated, ill-conditioned precision) and uniform and Thompson-like runs; the arms
  (gpu_arms) hold two identical arms, three collinear arms on an edge of the hull, an arm at the origin and an
  arm strictly inside the hull.
  Bar: relative 1e-7 on every entry >= 1e-100, absolute 1e-100 below, all finite, rows summing to 1 within 1e-12.
  The relative bar is 100 eps0 rounded up to a power of ten, where eps0 = 2.3e-10 is the float64 definition's
  own rounding floor against long double on these very inputs (test_linear_posterior_host.py measures and
  bounds it; worst at A = 32, std 0.05, G = 256); the factor 100 covers the device's exp, sin and cos differing
  from numpy's by a few ulp and the reordered sums (measured worst on the device: 1.3e-11).  The copy, the
  middle collinear arm and the interior arm are exactly 0.
- Rows before the first valid pull equal the oracle's closed-form prior to 1e-12.
- Repeated calls are bit-identical, and a task's rows are the same bits alone, among 7 and under chunk=3.
- Dirty buffers and a side stream behind a delay, byte for byte.
- End to end on the device generator: calibration under both rollins, train_fresh.py --bayes_floor against the
  oracle's floor, evals/eval_posterior.py --env linear_bandit in both contexts."""
import functools
import importlib
import json
import os

import numpy as np
import pytest
import torch

import buffer_poison as BP  # noqa: F401  (the helpers below use it through the two modules)
import entry_point_cases as EC
import linear_posterior_oracle as LO
import posterior_oracle as PO

pytestmark = pytest.mark.gpu

HS = (0, 1, LO.GPU_H)
REL_BAR = 1e-7


@functools.lru_cache(maxsize=None)
def oracle(A, var, G):
    acts, rews = LO.gpu_records(A, var)
    return LO.linear_posterior(LO.gpu_arms(A), acts, rews, var, G)


def assert_close(got, ref, what):
    big = np.abs(ref) >= 1e-100
    err = np.abs(got - ref)
    rel = (err[big] / np.abs(ref[big])).max() if big.any() else 0.0
    small = err[~big].max() if (~big).any() else 0.0
    print(f"{what}: max relative error {rel:.3e} on {big.sum()} entries >= 1e-100, max absolute {small:.3e} below")
    assert np.isfinite(got).all() and rel <= REL_BAR and small <= 1e-100, what


@pytest.mark.parametrize("G", LO.GPU_GS)
@pytest.mark.parametrize("var", LO.GPU_VARS)
@pytest.mark.parametrize("A", LO.GPU_AS)
def test_linear_posterior_against_the_oracle(A, var, G):
    import dpt_hip
    arms = LO.gpu_arms(A)
    acts, rews = LO.gpu_records(A, var)
    ref = oracle(A, var, G)
    prior = LO.prior(arms)
    for H in HS:
        got = dpt_hip.linear_posterior(arms, acts[:, :H], rews[:, :H], var, grid=G)
        assert got.shape == (LO.GPU_N, H + 1, A) and got.dtype == torch.float64
        got = got.cpu().numpy()
        assert_close(got, ref[:, :H + 1], f"A={A} var={var} G={G} H={H}")
        assert np.abs(got.sum(-1) - 1).max() <= 1e-12
        assert np.abs(got[:, 0] - prior).max() <= 1e-12  # row 0, and below the rows behind invalid actions
        if H >= 1:
            assert np.array_equal(got[0, 1], got[0, 0])  # the out-of-range first action leaves the row unchanged
        if H >= 5:
            assert np.abs(got[1, :5] - prior).max() <= 1e-12 and np.array_equal(got[0, 6], got[0, 5])
        if A == 5:
            assert not got[:, :, 2].any()  # the copy of arm 0
        if A >= 20:
            assert not got[:, :, [3, 5, 8]].any()  # the copy, the arm inside an edge, the arm inside the hull


@pytest.mark.parametrize("A,G", [(5, 256), (20, 64)])
def test_linear_posterior_is_reproducible_and_independent_of_the_batch(A, G):
    import dpt_hip
    arms, var = LO.gpu_arms(A), 0.3
    acts, rews = LO.gpu_records(A, var)
    many = dpt_hip.linear_posterior(arms, acts, rews, var, grid=G)
    again = dpt_hip.linear_posterior(arms, acts, rews, var, grid=G)
    assert torch.equal(many.view(torch.int64), again.view(torch.int64))
    for n in (0, 3, 6):
        alone = dpt_hip.linear_posterior(arms, acts[n:n + 1], rews[n:n + 1], var, grid=G)
        assert torch.equal(alone.view(torch.int64), many[n:n + 1].view(torch.int64)), n
    split = dpt_hip.linear_posterior(arms, acts, rews, var, grid=G, chunk=3)
    assert torch.equal(split.view(torch.int64), many.view(torch.int64))
    default = dpt_hip.linear_posterior(arms, acts[:2, :5], rews[:2, :5], var)  # G = linear_posterior_grid()
    assert_close(default.cpu().numpy(), LO.linear_posterior(arms, acts[:2, :5], rews[:2, :5], var,
                                                            dpt_hip.linear_posterior_grid()), "default grid")


# ----------------------------------------------------------------------------- end to end on the device generator
@pytest.mark.parametrize("rollin", ["thompson", "uniform"])
def test_calibration_of_the_kernel_on_the_device_generator(rollin):
    """512 fresh samples, the reference's 10 arms, H = 50, std 0.3, the default grid: E[nll] = E[entropy] within
    |z| <= 4.5 (tests/test_gpu_posterior.py's threshold).  Independent of the quadrature rule; a wrong prior
    precision or noise scale shows here."""
    import dpt_hip
    env = dpt_hip.FreshEnv.linear_bandit(LO.reference_arms(10), 50, 0.3, rollin)
    batch = dpt_hip.fresh_batch(env, 20240611, 0, 512)
    post, targets = dpt_hip.fresh_posterior(env, batch)
    z, nll, ent = PO.calibration_z(post.cpu().numpy(), targets.cpu().numpy())
    print(f"{rollin}: z {z:.3f}, nll {nll:.5f}, entropy {ent:.5f}")
    assert np.isfinite(z) and abs(z) <= 4.5


@pytest.mark.parametrize("data_type", ["thompson", "uniform"])
def test_train_fresh_bayes_floor_is_the_oracles(data_type, tmp_path, monkeypatch):
    import dpt_hip
    train_fresh = importlib.import_module("train_fresh")
    monkeypatch.chdir(tmp_path)
    H, dim = 12, 5
    train_fresh.main(["--env", "linear_bandit", "--data_type", data_type, "--lin_d", "2", "--var", "0.3", "--envs", "320",
                      "--H", str(H), "--dim", str(dim), "--num_epochs", "1", "--layer", "2", "--bayes_floor"])
    logs = [f for f in os.listdir(tmp_path / "figs" / "loss") if f.endswith("_logs.txt")]
    assert len(logs) == 1
    log = open(tmp_path / "figs" / "loss" / logs[0]).read()
    lines = [x for x in log.splitlines() if x.startswith("\tBayes floor (test): ")]
    assert len(lines) == 1 and log.index("\tBayes floor (test): ") < log.index("Epoch: 1")
    floor = float(lines[0].split(": ")[1])
    # the oracle on the same 64 test samples (320 - int(0.8 * 320)), read from the generator's tokens
    arms = LO.reference_arms(dim)
    fenv = dpt_hip.FreshEnv.linear_bandit(arms, H, 0.3, data_type)
    batch = dpt_hip.fresh_batch(fenv, train_fresh.generator_key(0, "test"), 0, 64)
    tok, tg = batch["tokens"].cpu().numpy(), batch["opt_action"].cpu().numpy()
    ref = LO.linear_posterior(arms, tok[:, 1:, 1:1 + dim].argmax(-1).astype(np.int32), tok[:, 1:, 2 + dim].astype(np.float64),
                              0.3, dpt_hip.linear_posterior_grid())
    want = PO.bayes_floor(ref, tg)
    print(f"{data_type}: floor {floor!r}, oracle {want!r}")
    assert np.isfinite(want) and want > 0 and abs(floor - want) <= 1e-9


@pytest.mark.parametrize("embd,context,data_type", [(32, "fresh", "thompson"), (16, "fresh", "uniform"),
                                                    (32, "online", "thompson")])
def test_eval_posterior_runs(embd, context, data_type, tmp_path, monkeypatch):
    from models.net import Transformer
    ev = importlib.import_module("evals.eval_posterior")
    monkeypatch.chdir(tmp_path)
    H, dim = 10, 5
    torch.manual_seed(embd)
    model = Transformer(dict(horizon=H, state_dim=1, action_dim=dim, n_layer=2, n_embd=embd, n_head=1, dropout=0,
                             test=True))
    torch.save(model.state_dict(), tmp_path / "model.pt")
    ev.main(["--env", "linear_bandit", "--context", context, "--data_type", data_type, "--lin_d", "2", "--n_eval", "8",
             "--H", str(H), "--dim", str(dim), "--embd", str(embd), "--layer", "2", "--var", "0.3", "--model_path",
             str(tmp_path / "model.pt"), "--chunk", "3"])
    out = tmp_path / "figs" / "eval_posterior"
    assert (out / "posterior_gap.png").stat().st_size > 0
    res = json.load(open(out / "posterior_gap.json"))
    for k in ev.KEYS:
        assert len(res[k]["mean"]) == H + 1 and len(res[k]["sem"]) == H + 1
    kl = np.array(res["kl"]["mean"])
    assert np.isfinite(kl).all() and (kl >= -1e-12).all()
    assert np.isfinite(res["nll_model"]["mean"]).all() and np.isfinite(res["entropy"]["mean"]).all()
    # before any pull the posterior is the prior: every task's optimal arm has its closed-form share
    per_task = ev.run(model.to(ev.dpt_hip.device()).eval(), "linear_bandit", context, 8, dim, H, 0.3, "uniform", 0,
                      chunk=3, lin_d=2, data_type=data_type)
    prior = LO.prior(LO.reference_arms(dim))
    row0 = per_task["p_opt_bayes"][:, 0]
    assert (np.abs(row0[:, None] - prior[prior > 0][None]).min(1) <= 1e-12).all(), (row0, prior)
    assert (per_task["kl"] >= -1e-12).all()
    lo, hi = prior[prior > 0].min(), prior.max()
    assert lo - 1e-12 <= res["p_opt_bayes"]["mean"][0] <= hi + 1e-12


# ----------------------------------------------------------------------------- dirty buffers and a side stream
def _cases():
    import dpt_hip
    cases = []

    def linear(name, N, H, A, G, chunk):
        arms = LO.gpu_arms(A)

        def inputs(seed):
            rs = EC.rs_of(seed, 43)
            return dict(arms=EC.f64(arms), actions=EC.i32(rs.randint(-1, A + 1, (N, H))),
                        rewards=EC.f64(rs.normal(0.2, 0.5, (N, H))))

        def call(obj, inp, dirty):
            return dict(post=dpt_hip.linear_posterior(inp["arms"], inp["actions"], inp["rewards"], 0.3, grid=G,
                                                      chunk=chunk))
        cases.append(EC.Case(name, inputs, call))
    linear("linear_posterior-5arms", 5, 9, 5, 256, 0)
    linear("linear_posterior-20arms-chunk2", 5, 9, 20, 64, 2)
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
