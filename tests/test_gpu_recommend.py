"""The explore-then-exploit evaluation on the device (csrc/dpt_recommend.hip, dpt_hip.recommend_curve /
empirical_recommend, dpt_hip.train.exploit_curve, ExploreExploitTrainer.exploit_curve,
evals/eval_explore_exploit.py).

dpt_recommend_curve against the numpy restatement (tests/recommend_oracle.py): arms and their values
exactly, the softmax quantities within 1e-12 absolute for means in [0, 1] (32 terms of a few ulps each,
two orders of margin).  dpt_empirical_recommend against the reference's EmpMeanPolicy on every prefix
(tests/golden/recommend_emp.npz) and against the sequential restatement, exactly.  dpt_exploit_eval's
logits bit-equal to the forward-only training forward on the packed tokens and within the project's
1e-5 max(1, |x|) of the float64 oracle, its four outputs bit-equal to dpt_recommend_curve on those
logits -- the kernel's correctness apart from the model's numerics, so no near-tie allowance is needed.
Row t of the curve against a test-mode model call on the first t transitions; the command-line tool end
to end."""
import ctypes
import os

import numpy as np
import pytest
import torch

import recommend_oracle as RO
from conftest import golden
from test_gpu_interactive import _model, _tokens64

pytestmark = pytest.mark.gpu

VALUE_TOL = 1e-12  # expected_value / p_opt, absolute
LOGIT_TOL = 1e-5   # the project's forward bar, relative to max(1, |x|)
KEYS = ("greedy_arm", "greedy_value", "expected_value", "p_opt")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _np(out, keys=KEYS):
    return {k: out[k].cpu().numpy() for k in keys}


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


# ----------------------------------------------------------------------------- dpt_recommend_curve
def _logit_sets(rs, N, T, A):
    ties = rs.randint(0, 3, (N, T, A)).astype(np.float32)  # small integers: exact ties at the maximum
    return {"random": (3.0 * rs.standard_normal((N, T, A))).astype(np.float32),
            "scaled": rs.uniform(-1e4, 1e4, (N, T, A)).astype(np.float32),
            "ties": ties}


def _check_curve(got, ref, what):
    assert got["greedy_arm"].dtype == np.int32
    assert np.array_equal(got["greedy_arm"], ref["greedy_arm"]), what
    assert np.array_equal(got["greedy_value"], ref["greedy_value"]), what
    for k in ("expected_value", "p_opt"):
        err = np.abs(got[k] - ref[k]).max()
        print(f"{what} {k}: max abs err {err:.3e}")
        assert err <= VALUE_TOL, (what, k, err)


@pytest.mark.parametrize("A", [1, 2, 5, 17, 32])
@pytest.mark.parametrize("N", [1, 7, 67])
def test_recommend_curve_equals_the_restatement(N, A):
    """random logits, logits of +-1e4 (the max subtraction), exact ties at the maximum (first index) and
    targets outside [0, A) (p_opt 0), at T = 1, 2, 66 (more than one wave of rows) and 131"""
    import dpt_hip
    for T in (1, 2, 66, 131):
        rs = np.random.RandomState(1000 * N + 10 * T + A)
        means = rs.uniform(0, 1, (N, A))
        sets = _logit_sets(rs, N, T, A)
        if A > 1 and N * T >= 66:
            top = sets["ties"].max(-1, keepdims=True)
            assert ((sets["ties"] == top).sum(-1) > 1).any()
        for name, lg in sets.items():
            got = _np(dpt_hip.recommend_curve(lg, means))
            ref = RO.recommend_curve(lg, means)
            _check_curve(got, ref, f"N={N} T={T} A={A} {name}")
            assert got["greedy_arm"].min() >= 0 and got["greedy_arm"].max() < A
            assert got["expected_value"].min() >= -VALUE_TOL and got["expected_value"].max() <= 1 + VALUE_TOL
        outside = np.array([-1, A, 2 ** 40, -2 ** 40, 0])[np.arange(N) % 5]
        got = _np(dpt_hip.recommend_curve(sets["random"], means, targets=outside))
        ref = RO.recommend_curve(sets["random"], means, targets=outside)
        _check_curve(got, ref, f"N={N} T={T} A={A} targets outside")
        assert (got["p_opt"][outside != 0] == 0).all() and (got["p_opt"][outside == 0] > 0).all()


def test_recommend_curve_arm_is_in_range_whatever_the_logits_hold():
    """infinities and NaNs: the arm is np.argmax's (the first NaN when there is one), always in [0, A)"""
    import dpt_hip
    N, T, A = 3, 5, 5
    rs = np.random.RandomState(3)
    lg = rs.standard_normal((N, T, A)).astype(np.float32)
    lg[0, 0] = -np.inf
    lg[0, 1, 2] = np.inf
    lg[0, 2, 3] = np.nan
    lg[0, 3, [1, 4]] = np.nan
    lg[1, 0, 0] = np.nan
    lg[1, 1] = np.nan
    lg[1, 2, [2, 4]] = np.inf
    means = rs.uniform(0, 1, (N, A))
    got = _np(dpt_hip.recommend_curve(lg, means))
    assert np.array_equal(got["greedy_arm"], lg.argmax(-1))
    assert got["greedy_arm"].min() >= 0 and got["greedy_arm"].max() < A
    assert np.array_equal(got["greedy_value"], means[np.arange(N)[:, None], lg.argmax(-1)])
    clean = np.isfinite(lg).all(-1)
    ref = RO.recommend_curve(np.where(np.isfinite(lg), lg, 0), means)
    assert np.abs(got["expected_value"] - ref["expected_value"])[clean].max() <= VALUE_TOL


def test_recommend_curve_null_outputs_and_repeats():
    """any output may be NULL (targets too when p_opt is); what is written does not depend on what is
    left out; repeated calls are bit-identical"""
    import dpt_hip
    from dpt_hip import _lib
    N, T, A = 7, 66, 5
    rs = np.random.RandomState(5)
    lg = torch.from_numpy((3.0 * rs.standard_normal((N, T, A))).astype(np.float32)).cuda()
    means = torch.from_numpy(rs.uniform(0, 1, (N, A))).cuda()
    full = _np(dpt_hip.recommend_curve(lg, means))
    again = _np(dpt_hip.recommend_curve(lg, means))
    for k in KEYS:
        assert np.array_equal(full[k], again[k]), k
    tg = means.argmax(1)
    for keep in KEYS:
        bufs = {k: torch.full((N, T), -7, dtype=torch.int32 if k == "greedy_arm" else torch.float64, device="cuda")
                for k in KEYS}
        ptr = {k: _p(bufs[k]) if k == keep else None for k in KEYS}
        _lib.call("dpt_recommend_curve", _p(lg), _p(means), _p(tg) if keep == "p_opt" else None, N, T, A,
                  ptr["greedy_arm"], ptr["greedy_value"], ptr["expected_value"], ptr["p_opt"], _stream())
        torch.cuda.synchronize()
        for k in KEYS:
            assert np.array_equal(bufs[k].cpu().numpy(), full[k]) if k == keep else (bufs[k] == -7).all(), (keep, k)
    _lib.call("dpt_recommend_curve", _p(lg), _p(means), None, N, T, A, None, None, None, None, _stream())
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- dpt_empirical_recommend
@pytest.mark.parametrize("name", ["gauss5", "gauss17", "bern3"])
def test_empirical_recommend_equals_the_reference(name):
    """EmpMeanPolicy(online=False).act_numpy_vec on every prefix, recorded from the reference: exactly
    (the fixture's seeds keep every prefix clear of near-ties; exact ties go to the first index)"""
    import dpt_hip
    g = golden("recommend_emp.npz")
    means, acts, rews, arms = (g[f"{name}/{k}"] for k in ("means", "actions", "rewards", "emp_arm"))
    out = _np(dpt_hip.empirical_recommend(acts, rews, means), ("emp_arm", "emp_value"))
    assert out["emp_arm"].dtype == np.int32 and np.array_equal(out["emp_arm"], arms)
    assert np.array_equal(out["emp_value"], means[np.arange(len(means))[:, None], arms])
    assert (out["emp_arm"][:, 0] == 0).all()


def test_empirical_recommend_equals_the_sequential_restatement():
    """(N, H, A) = (67, 131, 32): three 64-pull chunks, every lane of the arm half holds an arm; a second
    record with out-of-range actions, which add to no arm; bit-identical repeats"""
    import dpt_hip
    N, H, A = 67, 131, 32
    rs = np.random.RandomState(11)
    means = rs.uniform(0, 1, (N, A))
    acts = rs.randint(0, A, (N, H)).astype(np.int32)
    rews = means[np.arange(N)[:, None], acts] + 0.3 * rs.standard_normal((N, H))
    for a in (acts, np.where(rs.uniform(size=(N, H)) < 0.2, rs.choice([-1, A, 40, 64, -2 ** 31, 2 ** 31 - 1], (N, H)),
                             acts).astype(np.int32)):
        ref = RO.empirical_recommend(a, rews, means)
        out = _np(dpt_hip.empirical_recommend(a, rews, means), ("emp_arm", "emp_value"))
        assert np.array_equal(out["emp_arm"], ref["emp_arm"])
        assert np.array_equal(out["emp_value"], ref["emp_value"])
        again = _np(dpt_hip.empirical_recommend(a, rews, means), ("emp_arm", "emp_value"))
        assert np.array_equal(out["emp_arm"], again["emp_arm"]) and np.array_equal(out["emp_value"], again["emp_value"])
    assert not np.array_equal(ref["emp_arm"], RO.empirical_recommend(acts, rews, means)["emp_arm"])


@pytest.mark.parametrize("A", [1, 5])
def test_empirical_recommend_without_pulls(A):
    """H = 0: the empty record names arm 0"""
    import dpt_hip
    means = np.random.RandomState(A).uniform(0, 1, (3, A))
    out = dpt_hip.empirical_recommend(np.zeros((3, 0), np.int32), np.zeros((3, 0)), means)
    assert out["emp_arm"].shape == (3, 1) and (out["emp_arm"] == 0).all()
    assert np.array_equal(out["emp_value"].cpu().numpy(), means[:, :1])


# ----------------------------------------------------------------------------- dpt_exploit_eval
N_EVAL, A_EVAL, L_EVAL, H_MODEL = 5, 5, 2, 70


def _records(rs, N, H, A):
    means = rs.uniform(0, 1, (N, A))
    acts = rs.randint(0, A, (N, H)).astype(np.int32)
    rews = means[np.arange(N)[:, None], acts] + 0.3 * rs.standard_normal((N, H))
    return means, acts, rews


def _packed_forward(m, acts, rews, A):
    """dpt_hip.train.forward (forward-only, every position) on dpt_interactive_pack's tokens"""
    from dpt_hip import _lib
    from dpt_hip import train as tr
    N, H = acts.shape
    a_d, r_d = torch.from_numpy(acts).cuda(), torch.from_numpy(rews).cuda()
    tokens = torch.empty((N, H + 1, A + 3), device="cuda")
    _lib.call("dpt_interactive_pack", _p(a_d) if H else None, _p(r_d) if H else None, N, H, A, _p(tokens), _stream())
    d = tr.desc(m.n_layer, m.n_embd, 1, A, m.n_positions, N, H + 1, flags=tr.FORWARD_ONLY)
    preds, _ = tr.forward(d, tr.pack_params(tr.param_list(m)), tokens)
    return preds


@pytest.mark.parametrize("chunk", [0, 3])
@pytest.mark.parametrize("H", [0, 1, 6, 70])
@pytest.mark.parametrize("E", [32, 18])
def test_exploit_curve_is_one_forward_and_one_reduction(E, H, chunk):
    """5 tasks, 5 arms, 2 layers; width 32 on the matrix-core kernels and 18 on the row kernels; all tasks
    at once and chunks of 3 and 2.  The logits equal the forward-only training forward on the packed
    tokens bit for bit and meet the 1e-5 bar against the float64 oracle on the same tokens; the four
    outputs equal dpt_recommend_curve on those logits bit for bit; chunked equals unchunked bit for bit."""
    import dpt_hip
    from dpt_hip import train as tr
    from oracle import dpt_oracle_torch as OT
    N, A, L = N_EVAL, A_EVAL, L_EVAL
    m, w64 = _model(E, L, H_MODEL, 7 * E + H)
    m = m.cuda()
    means, acts, rews = _records(np.random.RandomState(100 * H + E), N, H, A)
    out = tr.exploit_curve(m, acts, rews, means, chunk=chunk, want_logits=True)
    assert out["logits"].shape == (N, H + 1, A) and out["logits"].dtype == torch.float32
    assert all(out[k].shape == (N, H + 1) for k in KEYS)
    assert torch.equal(out["logits"], _packed_forward(m, acts, rews, A))
    with torch.no_grad():
        ref = OT.forward(OT.state_dict_params(w64, L), _tokens64(acts, rews, A), L).numpy()
    err = _rel(out["logits"].cpu().numpy(), ref)
    print(f"E={E} H={H} chunk={chunk}: logits vs float64 oracle {err:.3e}")
    assert err <= LOGIT_TOL, err
    direct = dpt_hip.recommend_curve(out["logits"], means)
    for k in KEYS:
        assert torch.equal(out[k], direct[k]), k
    assert tr.exploit_curve(m, acts, rews, means, chunk=chunk)["logits"] is None
    if chunk:
        whole = tr.exploit_curve(m, acts, rews, means, chunk=0, want_logits=True)
        for k in KEYS + ("logits",):
            assert torch.equal(out[k], whole[k]), k
    # targets given explicitly: only p_opt depends on them
    tg = (means.argmax(1) + 1) % A
    other = tr.exploit_curve(m, acts, rews, means, targets=tg, chunk=chunk)
    assert torch.equal(other["greedy_arm"], out["greedy_arm"]) and torch.equal(other["expected_value"],
                                                                               out["expected_value"])
    assert torch.equal(other["p_opt"], dpt_hip.recommend_curve(out["logits"], means, targets=tg)["p_opt"])


def test_logit_bar_tells_a_perturbed_model():
    """The bar can fail: the curve's logits against the oracle run on weights whose last
    mlp.c_proj.weight is scaled by 1 + 1e-3 violate it (while they meet it on the true weights)."""
    from dpt_hip import train as tr
    from oracle import dpt_oracle_torch as OT
    N, A, L, E, H = N_EVAL, A_EVAL, L_EVAL, 32, 70
    m, w64 = _model(E, L, H_MODEL, 7 * E + H)
    means, acts, rews = _records(np.random.RandomState(100 * H + E), N, H, A)
    got = tr.exploit_curve(m.cuda(), acts, rews, means, want_logits=True)["logits"].cpu().numpy()
    k = f"transformer.h.{L - 1}.mlp.c_proj.weight"
    with torch.no_grad():
        ref = OT.forward(OT.state_dict_params(w64, L), _tokens64(acts, rews, A), L).numpy()
        ref2 = OT.forward(OT.state_dict_params(dict(w64, **{k: w64[k] * (1.0 + 1e-3)}), L),
                          _tokens64(acts, rews, A), L).numpy()
    assert _rel(got, ref) <= LOGIT_TOL
    assert _rel(got, ref2) > LOGIT_TOL, _rel(got, ref2)


@pytest.mark.parametrize("E", [32, 18])
def test_row_t_is_the_model_after_t_transitions(E):
    """At H = 6 the curve's row t equals the last-position logits of a test-mode model(batch) on the first
    t transitions, for every t, within the 1e-5 bar: the one-forward argument, checked."""
    from dpt_hip import train as tr
    N, A, H = N_EVAL, A_EVAL, 6
    m, _ = _model(E, L_EVAL, H, 31 + E)
    m = m.cuda().eval()
    assert m.test
    means, acts, rews = _records(np.random.RandomState(E), N, H, A)
    curve = tr.exploit_curve(m, acts, rews, means, want_logits=True)["logits"].cpu().numpy()
    onehot = torch.nn.functional.one_hot(torch.from_numpy(acts).long(), A).float().cuda()
    r32 = torch.from_numpy(rews).float().cuda()[..., None]
    for t in range(H + 1):
        batch = {"query_states": torch.ones((N, 1), device="cuda"),
                 "context_states": torch.ones((N, t, 1), device="cuda"), "context_actions": onehot[:, :t],
                 "context_next_states": torch.ones((N, t, 1), device="cuda"), "context_rewards": r32[:, :t]}
        with torch.no_grad():
            last = m(batch).cpu().numpy()
        assert last.shape == (N, A)
        err = _rel(curve[:, t], last)
        print(f"E={E} t={t}: row t vs model(prefix) {err:.3e}")
        assert err <= LOGIT_TOL, (t, err)


@pytest.mark.parametrize("E", [32, 18])
def test_trainer_wrapper_reads_the_master_blob(E):
    """ExploreExploitTrainer.exploit_curve after a step, with no sync: equal, bit for bit, to the function
    on the synced module -- and different from the curve of the weights before the step"""
    from dpt_hip import train as tr
    N, A, H = N_EVAL, A_EVAL, 6
    explorer, _ = _model(E, L_EVAL, H, 1 + E)
    exploiter, _ = _model(E, L_EVAL, H, 2 + E)
    explorer, exploiter = explorer.cuda(), exploiter.cuda()
    rs = np.random.RandomState(E)
    means, acts, rews = _records(rs, N, H, A)
    before = tr.exploit_curve(exploiter, acts, rews, means, want_logits=True)
    trainer = tr.ExploreExploitTrainer(explorer, exploiter, lr=1e-2, chunk=3)
    trainer.step(rs.uniform(0, 1, (8, A)), H + 1, 0.3, "uniform", 1.0, seed=5)
    got = trainer.exploit_curve(acts, rews, means, want_logits=True)
    assert not torch.equal(got["logits"], before["logits"])
    stale = tr.exploit_curve(exploiter, acts, rews, means, want_logits=True)  # the module is not synced yet
    assert torch.equal(stale["logits"], before["logits"])
    trainer.sync_to_models()
    ref = tr.exploit_curve(exploiter, acts, rews, means, chunk=3, want_logits=True)
    for k in KEYS + ("logits",):
        assert torch.equal(got[k], ref[k]), k


def test_refusals_from_python():
    import dpt_hip
    from dpt_hip import train as tr
    from models.net import Transformer
    cfg = dict(horizon=4, state_dim=1, action_dim=5, n_layer=1, n_embd=16, n_head=1, dropout=0.0, test=True)
    means, acts, rews = _records(np.random.RandomState(0), 3, 4, 5)
    m = Transformer(cfg).cuda()
    with pytest.raises(ValueError, match="state_dim"):
        tr.exploit_curve(Transformer(dict(cfg, state_dim=2)).cuda(), acts, rews, means)
    md = Transformer(dict(cfg, dropout=0.1)).cuda()
    md.train()
    with pytest.raises(ValueError, match="dropout"):
        tr.exploit_curve(md, acts, rews, means)
    md.eval()
    assert tr.exploit_curve(md, acts, rews, means)["greedy_arm"].shape == (3, 5)  # eval mode: no dropout in play
    with pytest.raises(ValueError, match="n_positions"):
        tr.exploit_curve(m, np.zeros((3, 20), np.int32), np.zeros((3, 20)), means)
    with pytest.raises(ValueError, match="action_dim"):
        tr.exploit_curve(m, acts, rews, means[:, :4])
    with pytest.raises(ValueError, match="actions"):
        tr.exploit_curve(m, acts[:2], rews, means)
    with pytest.raises(ValueError, match="targets"):
        tr.exploit_curve(m, acts, rews, means, targets=[0, 1])
    with pytest.raises(ValueError, match="chunk"):
        tr.exploit_curve(m, acts, rews, means, chunk=-1)
    wide = dict(cfg, action_dim=33)
    with pytest.raises(NotImplementedError, match="action_dim"):
        tr.exploit_curve(Transformer(wide).cuda(), np.zeros((3, 4), np.int32), rews, np.zeros((3, 33)))
    with pytest.raises(NotImplementedError, match="action_dim"):
        dpt_hip.recommend_curve(np.zeros((2, 3, 33), np.float32), np.zeros((2, 33)))
    with pytest.raises(NotImplementedError, match="action_dim"):
        dpt_hip.empirical_recommend(np.zeros((2, 3), np.int32), np.zeros((2, 3)), np.zeros((2, 33)))
    with pytest.raises(ValueError, match="logits"):
        dpt_hip.recommend_curve(np.zeros((2, 3, 5), np.float32), np.zeros((3, 5)))
    with pytest.raises(ValueError, match="targets"):
        dpt_hip.recommend_curve(np.zeros((2, 3, 5), np.float32), np.zeros((2, 5)), targets=[0])
    with pytest.raises(ValueError, match="actions"):
        dpt_hip.empirical_recommend(np.zeros((2, 3), np.int32), np.zeros((2, 4)), np.zeros((2, 5)))


# ----------------------------------------------------------------------------- command line
def test_cli_eval_explore_exploit(tmp_path, monkeypatch):
    """evals/eval_explore_exploit.py on two tiny checkpoints: the twelve result keys, curves over the
    budgets 0 .. H, every collector's emp row starting from arm 0, the plot file; --random_env (and
    another width, chunked) runs too."""
    import importlib

    import matplotlib
    matplotlib.use("Agg")
    ev = importlib.import_module("evals.eval_explore_exploit")
    monkeypatch.chdir(tmp_path)
    n_eval, H, A = 8, 6, 5
    base = ["--n_eval", str(n_eval), "--H", str(H), "--dim", str(A), "--layer", "2"]
    keys = {f"{c}/{r}" for c in ("Explorer", "Uniform", "UCB1.0", "Thomp") for r in ("exploiter", "exploiter_soft",
                                                                                    "emp")}
    assert len(keys) == 12

    def check(results, seed):
        for part in ("simple_regret_means", "simple_regret_sems", "commit_regret_means"):
            assert set(results[part]) == keys, part
            for k, v in results[part].items():
                assert v.shape == (H + 1,) and np.isfinite(v).all(), (part, k)
        assert set(results["p_opt_means"]) == {k for k in keys if k.endswith("/exploiter")}
        for v in results["p_opt_means"].values():
            assert v.shape == (H + 1,) and (v > 0).all() and (v < 1).all()
        # the bandits the script drew (generate_eval_trajs under its seed): budget 0 of every emp row is arm 0
        np.random.seed(seed)
        means = np.stack([t["means"] for t in ev.generate_eval_trajs(n_eval, A, "uniform")])
        arm0 = (means.max(1) - means[:, 0]).mean()
        for c in ("Explorer", "Uniform", "UCB1.0", "Thomp"):
            assert abs(results["simple_regret_means"][f"{c}/emp"][0] - arm0) <= 1e-12, c
            assert (results["simple_regret_means"][f"{c}/emp"] >= 0).all()
            # nothing is spent before the first pull: committing at budget 0 costs H times the simple regret
            for r in ("exploiter", "exploiter_soft", "emp"):
                k = f"{c}/{r}"
                assert abs(results["commit_regret_means"][k][0] - H * results["simple_regret_means"][k][0]) <= 1e-9
        # the exploiter at budget 0 has seen no pulls: its row does not depend on the collector
        for r in ("exploiter", "exploiter_soft"):
            assert abs(results["simple_regret_means"][f"Explorer/{r}"][0]
                       - results["simple_regret_means"][f"Thomp/{r}"][0]) <= 1e-12

    for E, extra in ((32, []), (16, ["--embd", "16", "--random_env", "--chunk", "3", "--seed", "4"])):
        paths = []
        for role, seed in (("explorer", 1), ("exploiter", 2)):
            m, _ = _model(E, 2, H, seed + E, A=A)
            paths.append(f"{role}_{E}.pt")
            torch.save(m.state_dict(), paths[-1])
        results = ev.main(base + extra + ["--explorer_path", paths[0], "--exploiter_path", paths[1]])
        check(results, 4 if extra else 0)
        assert os.path.getsize("figs/eval_explore_exploit/simple_regret.png") > 0
        os.remove("figs/eval_explore_exploit/simple_regret.png")
