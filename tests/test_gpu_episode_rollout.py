"""The in-episode DarkRoom rollout in one launch (csrc/dpt_prefill.hip rollout_darkroom_episode_kernel,
dpt_rollout_darkroom_episode, dpt_hip.rollout_darkroom_episode) and the evaluation built on it
(evals/eval_interactive_darkroom.py).

Every device comparison runs against the float64 restatement tests/interactive_mdp_oracle.py on the cases
of tests/episode_rollout_cases.py, whose oracle margins tests/test_episode_rollout_host.py asserts without a
GPU: the records equal the oracle's exactly and every step's logits lie within 1e-5 max(1, |x|) of the
oracle's (the project's reference logit bar).  Then: the same logits from the existing width-32 window
forward on windows rebuilt from the kernel's own records; the records of the chain of
dpt_interactive_mdp_grad; the Philox path against the numpy replay and under chunking; repeatability; a model
with peaked attention; two controls the comparison must reject; the shapes the kernel refuses; and the tool."""
import os

import numpy as np
import pytest
import torch

import episode_rollout_cases as EC
import interactive_mdp_oracle as MO
import philox_np

pytestmark = pytest.mark.gpu

REC_KEYS = ("states", "actions", "rewards", "targets")


def _run(m, goals, K, dim, **kw):
    import dpt_hip
    out = dpt_hip.rollout_darkroom_episode(m.cuda().eval(), goals, K, dim, **kw)
    torch.cuda.synchronize()
    return out


def _np(rec):
    return {k: v.cpu().numpy() for k, v in rec.items()}


def _logit_err(lg, ref):
    """max over steps, envs and actions of |device - oracle| / max(1, |oracle|); device (N, K, 5), oracle
    (K, N, 5)"""
    ref = np.transpose(ref, (1, 0, 2))
    return float((np.abs(lg.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


def _same_records(rec, ep):
    return all(np.array_equal(rec[k], ep[k]) for k in REC_KEYS)


def _check(m, goals, u, sample, dim, ep, perm=None):
    K = ep["targets"].shape[1]
    rec, ret, lg = _run(m, goals, K, dim, sample=sample, perm=perm, uniforms=u if sample and K > 1 else None,
                        seed=1, logits=True)
    rec, lg = _np(rec), lg.cpu().numpy()
    assert lg.shape == (len(goals), K, 5) and ret.dtype == torch.int64
    err = _logit_err(lg, ep["logits"])
    print(f"K={K} N={len(goals)} logit error {err:.3e} min margin "
          f"{ep['margins'].min() if ep['margins'].size else float('nan'):.3e}")
    for k in REC_KEYS:
        assert rec[k].dtype == np.int32 and np.array_equal(rec[k], ep[k]), k
    assert np.array_equal(ret.cpu().numpy(), ep["rewards"].sum(1))
    assert err <= 1e-5, err
    return rec, lg


@pytest.mark.parametrize("name", list(EC.TABLE))
def test_records_and_logits_follow_the_float64_oracle(name):
    """K = 1 and 2 (no and one transition); T = 16 -> 17 (a second block; waves with 0, 1 and 2 blocks);
    32 -> 33; 128 -> 129 (the 8-wave geometry); 256 -> 257 (16 waves); sampled and greedy"""
    m, goals, u, sample, dim, _, ep = EC.table_case(name)
    assert not ep["margins"].size or ep["margins"].min() > EC.MARGIN
    _check(m, goals, u, sample, dim, ep)


@pytest.mark.parametrize("permuted", [False, True])
def test_records_case_follows_the_oracle_and_the_chain(permuted):
    """the records case of the interactive training step (dim 3, 7 envs, 6 steps, 2 layers; plain and with
    action permutations): the oracle's records and logits, and the records of rollout_darkroom_interactive"""
    from dpt_hip.train import rollout_darkroom_interactive
    m, goals, u, sample, dim, _, ep, perm = EC.records_case(permuted)
    rec, _ = _check(m, goals, u, sample, dim, ep, perm)
    assert (rec["rewards"] == 1).any()
    chain, chain_ret = rollout_darkroom_interactive(m.cuda().eval(), goals, MO.REC_K, dim, sample=True, perm=perm,
                                                    uniforms=u)
    chain = _np(chain)
    for k in REC_KEYS:
        assert np.array_equal(chain[k], rec[k]), k
    assert np.array_equal(chain_ret.cpu().numpy(), rec["rewards"].sum(1))


def test_logits_equal_the_window_forward_on_the_kernels_own_records():
    """K = 33: every step's window rebuilt from the kernel's records and run through dpt_forward_window
    (out_mode 0, the prefill) gives the kernel's logits within the reference bar; whether they are bit-identical
    is printed (DESIGN.md records it), not required"""
    m, goals, u, sample, dim, _, ep = EC.table_case("K33")
    K = 33
    rec, _, lg = _run(m, goals, K, dim, sample=sample, uniforms=u, logits=True)
    st = rec["states"].float()
    onehot = torch.nn.functional.one_hot(rec["actions"].long(), num_classes=5).float()
    rw = rec["rewards"].float()
    dm = m.device_model()
    worst, same = 0.0, True
    for t in range(K):
        ref = dm.forward_window(st[:, t], st[:, :t], onehot[:, :t], st[:, 1:t + 1], rw[:, :t]) if t else \
            dm.forward_window(st[:, 0])
        got = lg[:, t]
        same = same and torch.equal(got, ref)
        worst = max(worst, float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max()))
    print(f"episode kernel vs dpt_forward_window over {K} windows: worst relative difference {worst:.3e}, "
          f"bit-identical: {same}")
    assert worst <= 1e-5, worst


def test_philox_path_and_chunking():
    """uniforms=None: the records equal a run on the numpy replay of Philox(seed, counter + t, first_task + i,
    select stream); envs [0:3] and [3:5] as two calls with first_task 5 and 8 equal the single call"""
    m, goals, _, _, dim, _, _ = EC.table_case("K17")
    K, N, seed, first = 17, len(goals), 0x5EED1234ABCD, 5
    rec, ret, lg = _run(m, goals, K, dim, sample=True, seed=seed, first_task=first, logits=True)
    u = np.stack([philox_np.uniform(seed, t, first + np.arange(N), 0) for t in range(K - 1)])
    rec_u, ret_u, lg_u = _run(m, goals, K, dim, sample=True, uniforms=u, logits=True)
    for k in REC_KEYS:
        assert torch.equal(rec[k], rec_u[k]), k
    assert torch.equal(ret, ret_u) and torch.equal(lg, lg_u)
    assert len(np.unique(rec["actions"].cpu().numpy())) > 1
    parts = [_run(m, goals[a:b], K, dim, sample=True, seed=seed, first_task=first + a, logits=True)
             for a, b in ((0, 3), (3, 5))]
    for k in REC_KEYS:
        assert torch.equal(torch.cat([p[0][k] for p in parts]), rec[k]), k
    assert torch.equal(torch.cat([p[1] for p in parts]), ret)
    assert torch.equal(torch.cat([p[2] for p in parts]), lg)


def test_two_calls_are_bit_identical():
    m, goals, u, sample, dim, _, _ = EC.table_case("K33")
    a, b = (_run(m, goals, 33, dim, sample=True, uniforms=u, logits=True) for _ in range(2))
    for k in REC_KEYS:
        assert torch.equal(a[0][k], b[0][k]), k
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_sharp_attention_model_follows_the_oracle():
    import sharp_models
    m, w64, goals, u, sample, dim, L, ep = EC.sharp_case()
    assert ep["margins"].min() > EC.MARGIN
    tok = MO.window(ep["states"], ep["actions"], ep["rewards"], 16).numpy()
    sharp_models.assert_sharp(EC.SHARP_LEVEL, sharp_models.token_stats(w64, L, tok), "episode rollout")
    _check(m, goals, u, sample, dim, ep)


def test_the_comparison_rejects_a_dropped_permutation_and_shifted_targets():
    """controls: the permuted device records differ from an oracle episode run without the permutation, and
    from the oracle's targets shifted by one step"""
    m, goals, u, sample, dim, _, ep, perm = EC.records_case(True)
    rec, _ = _run(m, goals, MO.REC_K, dim, sample=True, perm=perm, uniforms=u)
    rec = _np(rec)
    assert _same_records(rec, ep)
    assert not _same_records(rec, EC.unpermuted_control())
    shifted = dict(ep, targets=np.roll(ep["targets"], 1, axis=1))
    assert not _same_records(rec, shifted)


def test_unsupported_shapes_raise_and_the_tool_falls_back(capsys):
    import dpt_hip
    from dpt_hip.train import rollout_darkroom_interactive
    from evals.eval_interactive_darkroom import MODEL, run_online_eval
    goals = MO.REC_GOALS
    m18, _ = MO.model(18, 2, MO.REC_K, 7)
    m18 = m18.cuda().eval()
    with pytest.raises(NotImplementedError):
        dpt_hip.rollout_darkroom_episode(m18, goals, MO.REC_K, MO.REC_DIM)
    big, _ = MO.model(32, 1, 600, 3)
    big = big.cuda().eval()
    window = big.device_model().prefill_max_window()
    assert 0 < window < 600
    with pytest.raises(NotImplementedError):
        dpt_hip.rollout_darkroom_episode(big, goals, window + 1, MO.REC_DIM)
    with pytest.raises(ValueError):
        dpt_hip.rollout_darkroom_episode(big, goals, 0, MO.REC_DIM)
    with pytest.raises(ValueError):
        dpt_hip.rollout_darkroom_episode(big, goals, 4, 256)
    res = run_online_eval(m18, goals, MO.REC_K, MO.REC_DIM, sample=False)
    assert "rollout_darkroom_interactive" in capsys.readouterr().out
    rec, ret = rollout_darkroom_interactive(m18, goals, MO.REC_K, MO.REC_DIM, sample=False)
    r = rec["rewards"].cpu().numpy().astype(np.float64)
    assert np.array_equal(res[MODEL]["reward_mean"], r.mean(0))
    assert res[MODEL]["final_return"] == float(ret.cpu().numpy().astype(np.float64).mean())
    assert np.array_equal(res[MODEL]["return_mean"], np.cumsum(r, 1).mean(0))


@pytest.mark.parametrize("with_baseline", [False, True])
def test_cli_eval_interactive_darkroom(with_baseline, tmp_path, monkeypatch):
    """main() on a saved tiny checkpoint (dim 3, K 6, 2 layers, 8 goals), with and without a baseline: the
    plot, the expert's closed-form return, the curves' lengths and the shares' ranges"""
    from evals import eval_interactive_darkroom as tool
    monkeypatch.chdir(tmp_path)
    dim, K, n = 3, 6, 8
    m, _ = MO.model(32, 2, K, 21)
    torch.save(m.state_dict(), tmp_path / "model.pt")
    argv = ["--dim", str(dim), "--H", str(K), "--layer", "2", "--n_eval", str(n), "--model_path",
            str(tmp_path / "model.pt"), "--save", str(tmp_path / "figs"), "--seed", "3"]
    if with_baseline:
        b, _ = MO.model(32, 2, 2 * K, 22)  # a longer horizon, as an offline checkpoint has
        torch.save(b.state_dict(), tmp_path / "base.pt")
        argv += ["--baseline_path", str(tmp_path / "base.pt"), "--sample"]
    res = tool.main(argv)
    assert os.path.getsize(tmp_path / "figs" / "online.png") > 0
    goals = res["goals"]
    assert goals.shape == (n, 2) and res["K"] == K
    closed = np.clip(K - 1 - np.maximum(np.abs(goals).sum(1) - 1, 0), 0, None).sum() / n
    assert res[tool.EXPERT]["final_return"] == pytest.approx(closed, abs=1e-12)
    names = [tool.EXPERT, tool.MODEL, tool.RANDOM] + ([tool.BASELINE] if with_baseline else [])
    assert (tool.BASELINE in res) == with_baseline
    for name in names:
        st = res[name]
        for key in ("reward_mean", "reward_sem", "return_mean", "return_sem"):
            assert st[key].shape == (K - 1,), (name, key)
        assert 0.0 <= st["reached"] <= 1.0 and 0.0 <= st["first_hit"] <= K - 1
        assert st["return_mean"][-1] == pytest.approx(st["final_return"])
    assert 0.0 <= res[tool.MODEL]["agreement"] <= 1.0 and "agreement" not in res[tool.EXPERT]
    assert res[tool.EXPERT]["final_return"] >= res[tool.RANDOM]["final_return"]
