"""The fused interactive bandit training step (csrc/dpt_interactive.hip,
dpt_hip.train.InteractiveTrainer, train_interactive.py, evals/eval_interactive_bandit.py).

The pack kernel against Transformer._tokens bit for bit; the last-position cross-entropy against a
float64 restatement under test_gpu_train_step.test_ce_loss_and_gradient's bars; the fp32 reward
flag of dpt_rollout_bandit_generic against numpy's float32 arithmetic bit for bit; three fused steps
against the float64 oracle conditioned on the step's own records, under the bars of
test_gpu_train_step._fused_steps_vs_oracle; the records against a direct rollout call; the gradient
of the last-position top block (DPT_TRAIN_LAST_LOSS) against the float64 oracle, held to twice the
full backward's error; and the two command-line tools end to end."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_gpu_train import GRAD_TOL

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23


def _lib_call(name, *args):
    from dpt_hip import _lib
    _lib.call(name, *args)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _model(E, L, H, seed, A=5):
    """a perturbed Transformer (state_dim 1, test mode) on the host, and its float64 weights"""
    from models.net import Transformer
    torch.manual_seed(seed)
    m = Transformer(dict(horizon=H, state_dim=1, action_dim=A, n_layer=L, n_embd=E, n_head=1, dropout=0.0,
                         test=True))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    w64 = {k: v.detach().numpy().astype(np.float64) for k, v in m.state_dict().items()}
    return m, w64


# ----------------------------------------------------------------------------- pack
@pytest.mark.parametrize("A", [5, 2])
@pytest.mark.parametrize("Hc", [0, 1, 4])
def test_pack_equals_tokens(Hc, A):
    """dpt_interactive_pack on rollout records == Transformer._tokens (models/net.py:42-54) on the
    batch those records make, bit for bit: rewards with negative values and doubles that fp32 cannot
    represent; Hc = 0 gives the query row alone."""
    from models.net import Transformer
    N = 3
    rs = np.random.RandomState(10 * Hc + A)
    acts = rs.randint(0, A, (N, Hc)).astype(np.int32)
    rew = rs.normal(0, 1, (N, Hc)) + 1e-9 * rs.normal(0, 1, (N, Hc))
    if Hc:
        rew[0, 0] = -0.1  # not an fp32 number
        assert (rew < 0).any() and (rew.astype(np.float32).astype(np.float64) != rew).any()
    a_d, r_d = torch.from_numpy(acts).cuda(), torch.from_numpy(rew).cuda()
    tokens = torch.full((N, Hc + 1, A + 3), float("nan"), device="cuda")
    _lib_call("dpt_interactive_pack", _p(a_d) if Hc else None, _p(r_d) if Hc else None, N, Hc, A, _p(tokens),
              _stream())
    m = Transformer(dict(horizon=4, state_dim=1, action_dim=A, n_layer=1, n_embd=16, n_head=1, dropout=0.0,
                         test=True))
    batch = {"query_states": torch.ones((N, 1)), "context_states": torch.ones((N, Hc, 1)),
             "context_actions": torch.nn.functional.one_hot(torch.from_numpy(acts).long(), A).float(),
             "context_next_states": torch.ones((N, Hc, 1)),
             "context_rewards": torch.from_numpy(rew).float()[..., None]}
    ref = m._tokens(batch)
    assert tokens.shape == ref.shape and torch.equal(tokens, ref)
    assert torch.equal(tokens[:, 0].cpu(), torch.tensor([1.0] + [0.0] * (A + 2)).expand(N, -1))


# ----------------------------------------------------------------------------- cross-entropy
def _ce_last(preds, targets, scale, want_grad=True, acc=None):
    B, T, A = preds.shape
    dp = torch.full_like(preds, float("nan")) if want_grad else None
    partial = torch.empty(B, dtype=torch.float64, device="cuda")
    acc = torch.zeros(1, dtype=torch.float64, device="cuda") if acc is None else acc
    _lib_call("dpt_train_ce_last", _p(preds), _p(targets), B, T, A, ctypes.c_double(scale), _p(dp), _p(partial),
              _p(acc), _stream())
    return acc, dp


@pytest.mark.parametrize("B,T,A", [(3, 1, 5), (4, 9, 20), (2, 5, 1)])
def test_ce_last_loss_and_gradient(B, T, A):
    """dpt_train_ce_last (CrossEntropyLoss() on preds[:, -1] against class indices, scale = 1 / B)
    against a float64 restatement on the same fp32 logits of magnitude up to 30: dpreds within twice
    the error of torch's own fp32 gradient plus 2^-23, the loss within 1e-5 relative, every row but
    the last exactly zero, two calls bit-identical, the loss-only call the same loss, and the
    accumulator accumulates."""
    rs = np.random.RandomState(B * 100 + T * 10 + A)
    x = (rs.uniform(-1, 1, (B, T, A)) * rs.choice([1.0, 5.0, 30.0], (B, T, 1))).astype(np.float32)
    t = rs.randint(0, A, B).astype(np.int64)
    preds, targets = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    scale = 1.0 / B
    x64 = x.astype(np.float64)[:, -1]
    mx = x64.max(-1, keepdims=True)
    lse = mx + np.log(np.exp(x64 - mx).sum(-1, keepdims=True))
    ref_loss = float(scale * (lse[:, 0] - x64[np.arange(B), t]).sum())
    ref_d = np.zeros((B, T, A))
    ref_d[:, -1] = scale * (np.exp(x64 - lse) - np.eye(A)[t])
    pt = preds.clone().requires_grad_(True)
    torch.nn.CrossEntropyLoss()(pt[:, -1], targets).backward()
    torch_err = np.abs(pt.grad.cpu().numpy() - ref_d).max()

    acc, dp = _ce_last(preds, targets, scale)
    acc2, dp2 = _ce_last(preds, targets, scale)
    acc3, _ = _ce_last(preds, targets, scale, want_grad=False)
    loss, got = acc.item(), dp.cpu().numpy()
    err = np.abs(got - ref_d).max()
    print(f"ce_last {B}x{T}x{A}: dpreds err {err:.3e} (torch {torch_err:.3e}), loss {loss!r} ref {ref_loss!r}")
    assert err <= 2 * torch_err + ULP
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss)
    assert not got[:, :-1].any()
    assert torch.equal(acc, acc2) and torch.equal(dp, dp2) and torch.equal(acc, acc3)
    _ce_last(preds, targets, scale, want_grad=False, acc=acc)
    assert acc.item() == 2 * loss


# ----------------------------------------------------------------------------- fp32 rewards
def test_generic_rollout_f32_rewards():
    """DPT_BANDIT_F32 in dpt_rollout_bandit_generic: Gaussian rewards are
    float32(means[a]) + float32(g) * float32(var) bit for bit at the kernel's own actions; without the
    flag the fp64 formula holds (and the two differ on these inputs); Bernoulli rewards do not
    depend on the flag."""
    from dpt_hip import train as tr
    E, L, N, H, var = 16, 2, 37, 6, 0.3
    m, _ = _model(E, L, H, 3)
    m = m.cuda().eval()
    rs = np.random.RandomState(21)
    means = rs.uniform(0, 1, (N, 5))
    u, g = rs.uniform(size=(H, N)), rs.normal(size=(H, N))
    rows = np.arange(N)[:, None]

    def run(kind, f32, noise):
        out = tr.rollout_bandit_generic(m, means, H, var, True, kind, uniforms=u, noise=noise, f32=f32)
        return out["actions"].cpu().numpy(), out["rewards"].cpu().numpy(), out["arm_value"].cpu().numpy()

    a32, r32, v32 = run(0, True, g)
    mean_a = means[rows, a32]
    want32 = (mean_a.astype(np.float32) + g.T.astype(np.float32) * np.float32(var)).astype(np.float64)
    want64 = mean_a + (0.0 + var * g.T)
    assert (want32 != want64).any()
    assert r32.dtype == np.float64 and np.array_equal(r32, want32)
    assert np.array_equal(v32, mean_a)
    a64, r64, _ = run(0, False, g)
    assert np.array_equal(r64, means[rows, a64] + (0.0 + var * g.T))
    assert np.array_equal(a64[:, 0], a32[:, 0])  # step 0 sees no reward yet
    ub = rs.uniform(size=(H, N))
    b0, b1 = run(1, False, ub), run(1, True, ub)
    assert all(np.array_equal(x, y) for x, y in zip(b0, b1))
    assert set(np.unique(b0[1])) <= {0.0, 1.0}


# ----------------------------------------------------------------------------- fused step
def _tokens64(actions, rewards, A):
    """the window of models/net.py:42-54 from records, in float64 (rewards through fp32, as the model sees them)"""
    N, Hc = actions.shape
    tok = np.zeros((N, Hc + 1, A + 3))
    tok[:, :, 0] = 1.0
    tok[:, 1:, 1:A + 1] = np.eye(A)[actions]
    tok[:, 1:, A + 1] = 1.0
    tok[:, 1:, A + 2] = rewards.astype(np.float32).astype(np.float64)
    return torch.from_numpy(tok)


@pytest.mark.parametrize("chunk", [0, 3])
@pytest.mark.parametrize("E", [32, 18])
@pytest.mark.parametrize("K", [1, 2, 6])
def test_interactive_steps_track_the_float64_oracle(K, E, chunk):
    """Three InteractiveTrainer.steps (8 envs, 5 arms, 2 layers; width 32 on the matrix-core kernels
    and 18 on the row kernels; all envs at once and chunks of 3, 3, 2) with injected draws.  After
    each step the float64 oracle forwards the window built from the step's own recorded actions and
    rewards, takes the mean cross-entropy of the last position against argmax(means) and the same
    AdamW step: loss within 1e-5 relative, at least 0.995 of the parameter entries within 1e-5, max
    difference at most 2 lr steps + 1e-5 (test_gpu_train_step._fused_steps_vs_oracle's bars).  The
    comparison is conditioned on the records, so no near-tie action can hide a failure.  Each chunk's
    records equal a direct dpt_rollout_bandit_generic call on the same blob, bit for bit."""
    from dpt_hip import train as tr
    from oracle import dpt_oracle_torch as OT
    N, A, L, lr, steps, var = 8, 5, 2, 1e-3, 3, 0.3
    m, w64 = _model(E, L, 6, 100 * K + E)
    m = m.cuda()
    P = OT.state_dict_params(w64, L)
    names = list(P)
    opt_ref = torch.optim.AdamW([P[k] for k in names], lr=lr, weight_decay=1e-4)
    wte = m.transformer.wte.weight.detach().clone()
    trainer = tr.InteractiveTrainer(m, lr=lr, weight_decay=1e-4, chunk=chunk)
    rs = np.random.RandomState(K * 7 + E + chunk)
    for s in range(steps):
        means = rs.uniform(0, 1, (N, A))
        u, g = rs.uniform(size=(K - 1, N)), rs.normal(size=(K - 1, N))
        blob = trainer.blob.clone()
        actions, rewards = trainer.step(means, K, var, "uniform", uniforms=u, noise=g)
        loss = trainer.read_loss()
        assert actions.shape == (N, K - 1) and actions.dtype == torch.int32
        assert rewards.shape == (N, K - 1) and rewards.dtype == torch.float64
        acts, rews = actions.cpu().numpy(), rewards.cpu().numpy()
        if K > 1:
            for off, n in tr.chunk_plan(N, chunk):
                d = tr.rollout_bandit_generic(m, means[off:off + n], K - 1, var, True, 0, first_task=off,
                                              uniforms=u[:, off:off + n], noise=g[:, off:off + n], f32=True,
                                              blob=blob)
                assert np.array_equal(d["actions"].cpu().numpy(), acts[off:off + n]), (s, off)
                assert np.array_equal(d["rewards"].cpu().numpy(), rews[off:off + n]), (s, off)
        opt_ref.zero_grad()
        preds = OT.forward(P, _tokens64(acts, rews, A), L)[:, -1]
        ref_loss = torch.nn.functional.cross_entropy(preds, torch.from_numpy(means.argmax(1)))
        ref_loss.backward()
        opt_ref.step()
        print(f"K={K} E={E} chunk={chunk} step {s}: loss {loss!r} ref {ref_loss.item()!r}")
        assert abs(loss - ref_loss.item()) <= 1e-5 * abs(ref_loss.item()), (loss, ref_loss.item())
    assert trainer.read_loss() == 0.0 and trainer.steps == steps
    trainer.sync_to_model()
    params = dict(m.named_parameters())
    assert torch.equal(params["transformer.wte.weight"], wte)
    diffs = np.concatenate([np.abs(params[k].detach().cpu().numpy() - P[k].detach().numpy()).ravel()
                            for k in names])
    print(f"K={K} E={E} chunk={chunk}: within 1e-5 {(diffs <= 1e-5).mean():.5f}, max {diffs.max():.3e}")
    assert (diffs <= 1e-5).mean() >= 0.995, (diffs <= 1e-5).mean()
    assert diffs.max() <= 2 * lr * steps + 1e-5


@pytest.mark.parametrize("chunk", [0, 3])
def test_interactive_step_philox_records(chunk):
    """With Philox draws: two steps from the same state and seed give identical records and
    identical blobs; each chunk's records equal a direct rollout call keyed by the same seed and
    the chunk's offset as first_task; another seed gives other records."""
    from dpt_hip import train as tr
    N, K, var = 8, 6, 0.3
    m, _ = _model(32, 2, 6, 5)
    m = m.cuda()
    means = np.random.RandomState(4).uniform(0, 1, (N, 5))
    runs = []
    for seed in (77, 77, 78):
        t = tr.InteractiveTrainer(m, lr=1e-3, chunk=chunk)
        blob = t.blob.clone()
        a, r = t.step(means, K, var, "uniform", seed=seed)
        runs.append((a.cpu().numpy(), r.cpu().numpy(), t.blob.clone(), t.read_loss()))
        assert not torch.equal(t.blob, blob)
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2]) and runs[0][3] == runs[1][3]
    assert not np.array_equal(runs[0][1], runs[2][1])
    for off, n in tr.chunk_plan(N, chunk):
        d = tr.rollout_bandit_generic(m, means[off:off + n], K - 1, var, True, 0, seed=77, first_task=off, f32=True,
                                      blob=blob)
        assert np.array_equal(d["actions"].cpu().numpy(), runs[0][0][off:off + n])
        assert np.array_equal(d["rewards"].cpu().numpy(), runs[0][1][off:off + n])


# ----------------------------------------------------------------------------- last-position top block
@pytest.mark.parametrize("E", [32, 18])
@pytest.mark.parametrize("T", [1, 2, 9])
def test_last_loss_gradient_vs_oracle(T, E):
    """DPT_TRAIN_LAST_LOSS (the last block's c_proj, ln_2, MLP, then ln_f and the head on the B last
    rows; one query row per sequence in the attention backward) against the float64 oracle's gradient
    of sum(preds[:, -1] * dpreds[:, -1]): 5 sequences, windows 1 (the full path), 2 and 9, width 32
    (matrix cores) and 18 (row kernels).  Its max error is within twice the error of the existing
    full backward fed dpreds that are zero except at the last row, plus 2^-23 max|g|, and every
    parameter's gradient is within 5 * GRAD_TOL of its largest float64 entry (test_gpu_train_grads'
    absolute bar, which does not lean on the full backward); the last row of preds is within 1e-5
    of the full forward's."""
    from dpt_hip import train as tr
    from oracle import dpt_oracle_torch as OT
    B, A, L = 5, 5, 2
    m, w64 = _model(E, L, 9, 10 * T + E)
    rs = np.random.RandomState(T * 100 + E)
    acts = rs.randint(0, A, (B, T - 1))
    rews = rs.normal(0.5, 0.5, (B, T - 1))
    tok64 = _tokens64(acts, rews, A)
    dp = np.zeros((B, T, A), dtype=np.float32)
    dp[:, -1] = rs.normal(0, 1, (B, A)).astype(np.float32)
    P = OT.state_dict_params(w64, L)
    (OT.forward(P, tok64, L) * torch.from_numpy(dp).double()).sum().backward()
    name_of = {id(p): k for k, p in m.named_parameters()}
    params = tr.param_list(m)
    g64 = [P[name_of[id(p)]].grad for p in params]
    n = len(g64)
    ends = np.cumsum([g.numel() for g in g64])
    g64 = torch.cat([(g.t() if i in (0, n - 2) else g).reshape(-1) for i, g in enumerate(g64)]).numpy()
    m = m.cuda()
    blob = tr.pack_params(tr.param_list(m))
    tok, dpd = tok64.float().cuda().contiguous(), torch.from_numpy(dp).cuda()
    out = {}
    for name, flags in (("full", 0), ("last", tr.LAST_LOSS)):
        d = tr.desc(L, E, 1, A, m.n_positions, B, T, flags=flags)
        preds, ws = tr.forward(d, blob, tok)
        out[name] = (preds[:, -1].cpu().numpy(), tr.backward(d, blob, tok, ws, dpd).cpu().numpy().astype(np.float64))
    assert np.abs(out["last"][0] - out["full"][0]).max() <= 1e-5
    err_full = np.abs(out["full"][1] - g64).max()
    err_last = np.abs(out["last"][1] - g64).max()
    print(f"last-loss T={T} E={E}: err {err_last:.3e} (full backward {err_full:.3e}), max|g| {np.abs(g64).max():.3e}")
    assert err_last <= 2 * err_full + ULP * np.abs(g64).max()
    for p, lo, hi in zip(params, ends - [g.numel() for g in params], ends):  # the absolute bar, per parameter
        e, scale = np.abs(out["last"][1][lo:hi] - g64[lo:hi]).max(), np.abs(g64[lo:hi]).max()
        assert e <= 5 * GRAD_TOL * scale, (name_of[id(p)], e / scale)
    if T == 1:
        assert np.array_equal(out["last"][1], out["full"][1])


def test_full_width_flag_gives_the_same_step():
    """DPT_INTERACTIVE_FULL_WIDTH (the A/B's other arm) runs the same step with the last block at
    full width: identical records, the loss and the gradient equal up to fp32 summation order."""
    from dpt_hip import train as tr
    N, K = 8, 6
    m, _ = _model(32, 2, 6, 9)
    m = m.cuda()
    means = np.random.RandomState(1).uniform(0, 1, (N, 5))
    res = []
    for full in (False, True):
        t = tr.InteractiveTrainer(m, lr=1e-3, chunk=3, full_width=full)
        a, r = t.step(means, K, 0.3, "uniform", seed=5)
        res.append((a.cpu().numpy(), r.cpu().numpy(), t.read_loss(), t.dblob.cpu().numpy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert abs(res[0][2] - res[1][2]) <= 1e-5 * abs(res[1][2])
    assert np.abs(res[0][3] - res[1][3]).max() <= 1e-5 * np.abs(res[1][3]).max()


def test_interactive_trainer_rejects_what_it_cannot_run():
    from dpt_hip import train as tr
    from models.net import Transformer
    cfg = dict(horizon=4, state_dim=1, action_dim=5, n_layer=1, n_embd=16, n_head=1, dropout=0.0, test=True)
    with pytest.raises(ValueError, match="dropout"):
        tr.InteractiveTrainer(Transformer(dict(cfg, dropout=0.1)).cuda(), lr=1e-3)
    with pytest.raises(ValueError, match="state_dim"):
        tr.InteractiveTrainer(Transformer(dict(cfg, state_dim=2)).cuda(), lr=1e-3)
    t = tr.InteractiveTrainer(Transformer(cfg).cuda(), lr=1e-3)
    with pytest.raises(ValueError, match="n_positions"):
        t.step(np.full((2, 5), 0.5), 21, 0.3, "uniform")
    with pytest.raises(ValueError, match="uniforms"):
        t.step(np.full((2, 5), 0.5), 3, 0.3, "uniform", uniforms=np.zeros((3, 2)))
    assert t.steps == 0 and not t.m.any()


# ----------------------------------------------------------------------------- command line
def test_cli_train_interactive_and_eval(tmp_path, monkeypatch, capsys):
    """train_interactive.py for 2 epochs of 3 episodes in a scratch directory: two finite loss lines,
    a checkpoint that loads strictly into Transformer and differs from the initial weights; the same
    run with --dropout 0.1 takes the plain per-step path and completes; then
    evals/eval_interactive_bandit.py on the first checkpoint writes its plot and returns the five
    result keys."""
    import importlib

    import matplotlib
    matplotlib.use("Agg")
    from models.net import Transformer
    ti = importlib.import_module("train_interactive")
    ev = importlib.import_module("evals.eval_interactive_bandit")
    monkeypatch.chdir(tmp_path)
    base = ["--env", "bandit", "--envs", "16", "--H", "4", "--dim", "5", "--embd", "16", "--layer", "2"]
    run = base + ["--num_epochs", "2", "--episodes_per_epoch", "3"]

    def losses():
        out = capsys.readouterr().out
        assert out.rstrip().endswith("Done.")
        found = re.findall(r"^Epoch (\d)/2 - loss: (\S+) - time: \S+s$", out, flags=re.M)
        assert [int(i) for i, _ in found] == [1, 2], out
        return [float(v) for _, v in found]

    ti.main(run)
    vals = losses()
    assert np.isfinite(vals).all() and min(vals) > 0, vals
    path = "trained_models/interactive_bandit.pt"
    sd = torch.load(path, map_location="cpu", weights_only=True)
    torch.manual_seed(0)
    fresh = Transformer(dict(horizon=4, state_dim=1, action_dim=5, n_layer=2, n_embd=16, n_head=1, dropout=0.0,
                             test=True))
    init = {k: v.clone() for k, v in fresh.state_dict().items()}
    assert set(sd) == set(init)
    fresh.load_state_dict(sd, strict=True)
    assert torch.equal(sd["transformer.wte.weight"], init["transformer.wte.weight"])
    for k in ("embed_transition.weight", "transformer.h.1.attn.c_attn.weight", "pred_actions.bias"):
        assert not torch.equal(sd[k], init[k]), k
    os.rename(path, "fused.pt")

    ti.main(run + ["--dropout", "0.1"])
    vals = losses()
    assert np.isfinite(vals).all() and min(vals) > 0, vals
    assert os.path.exists(path)

    results = ev.main(base + ["--n_eval", "8", "--model_path", "fused.pt", "--save", "figs/out"])
    assert os.path.exists("figs/out/online.png")
    keys = {"opt", "Interactive", "Emp", "UCB1.0", "Thomp"}
    for part in ("means", "sems", "regret_means", "regret_sems", "all_means"):
        assert set(results[part]) == keys, part
    assert all(v.shape == (8, 4) for v in results["all_means"].values())
    assert all(np.isfinite(v).all() for v in results["regret_means"].values())
