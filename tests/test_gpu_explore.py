"""The fused explorer/exploiter bandit training step (csrc/dpt_explore.hip, the separate env action
of rollout_bandit_generic in csrc/dpt_generic.hip, dpt_hip.train.ExploreExploitTrainer,
train_explorer_exploiter.py).

The every-position cross-entropy and the advantage weights against float64 restatements; the rollout
whose env action is not the context action against numpy's fp32 reward arithmetic and the float64
oracle's logits; the step's records against the float64 oracle's selection on every prefix window;
both models' gradients (their dblob before AdamW) against a float64 reference that computes the
advantages the reference's way -- K separate forwards of the growing prefix windows -- so the
one-forward shortcut is itself under test, with a control that the bar can fail; three steps against
the oracle's two AdamW runs; determinism; and the command-line tool on both of its paths.

Shapes: 8 envs, 5 arms, 2 layers, lr 1e-3; widths 32 (matrix-core kernels) and 18 (row kernels);
K in {2, 3, 6}; all envs at once and chunks of 3 (3, 3, 2).  Draws and env actions are injected."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_gpu_interactive import _model, _tokens64
from test_gpu_train import GRAD_TOL
from test_gpu_train_grads import _names, _split64, _worst

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
BAR = 5 * GRAD_TOL
N, A, L, LR, VAR = 8, 5, 2, 1e-3, 0.3


def _lib_call(name, *args):
    from dpt_hip import _lib
    _lib.call(name, *args)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------- every-position cross-entropy
def _ce_rows(preds, tseq, trow, weights, scale, want_grad=True, acc=None):
    B, T, A_ = preds.shape
    dp = torch.full_like(preds, float("nan")) if want_grad else None
    rowloss = torch.full((B, T), float("nan"), dtype=torch.float64, device="cuda")
    acc = torch.zeros(1, dtype=torch.float64, device="cuda") if acc is None else acc
    _lib_call("dpt_train_ce_rows", _p(preds), _p(tseq), _p(trow), _p(weights), B, T, A_, ctypes.c_double(scale),
              _p(rowloss), _p(dp), _p(acc), _stream())
    return acc, rowloss, dp


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("form", ["seq", "row"])
@pytest.mark.parametrize("B,T,A_", [(1, 1, 1), (3, 4, 5), (5, 9, 20), (300, 2, 32)])
def test_ce_rows_loss_and_gradient(B, T, A_, form, weighted):
    """dpt_train_ce_rows against a float64 restatement on the same fp32 logits of magnitude up to 30,
    with per-sequence int64 targets (broadcast over the positions) and per-row int32 targets, without
    weights and with random ones that hold exact zeros: the loss within 1e-12 relative, the unweighted
    row losses within 1e-12 max(1, |lse|) (lse - x[target] cancels, which leaves a few ulps of lse as an
    absolute error), dpreds within twice the error of torch's own fp32 gradient plus 2^-23
    (test_ce_last_loss_and_gradient's bar), rows of weight 0 and rows whose target is outside [0, A)
    exactly zero, two calls bit-identical, the loss-only call the same loss, and the accumulator
    accumulates."""
    rs = np.random.RandomState(B * 100 + T * 10 + A_ + (1000 if form == "row" else 0) + (5000 if weighted else 0))
    x = (rs.uniform(-1, 1, (B, T, A_)) * rs.choice([1.0, 5.0, 30.0], (B, T, 1))).astype(np.float32)
    if form == "seq":
        t = rs.randint(0, A_, B).astype(np.int64)
        if B >= 3:
            t[0], t[B - 1] = A_, -1  # outside [0, A): no loss, no gradient
        t_rows = np.repeat(t[:, None], T, 1)
    else:
        t = rs.randint(0, A_, (B, T)).astype(np.int32)
        if B >= 3:
            t[0, 0], t[B - 1, T - 1] = A_, -1
        t_rows = t.astype(np.int64)
    w = np.ones((B, T))
    if weighted:
        w = rs.uniform(0, 2, (B, T))
        if B * T > 1:
            w[rs.uniform(size=(B, T)) < 0.3] = 0.0
            w[-1, 0] = 0.0
            assert (w == 0).any() and (w != 0).any()
    preds = torch.from_numpy(x).cuda()
    targets = torch.from_numpy(t).cuda()
    w_d = torch.from_numpy(w).cuda() if weighted else None
    scale = 1.0 / (B * T)
    valid = (t_rows >= 0) & (t_rows < A_)
    tc = np.where(valid, t_rows, 0)
    x64 = x.astype(np.float64)
    mx = x64.max(-1, keepdims=True)
    lse = mx + np.log(np.exp(x64 - mx).sum(-1, keepdims=True))
    ref_rows = np.where(valid, lse[..., 0] - np.take_along_axis(x64, tc[..., None], -1)[..., 0], 0.0)
    ref_loss = float(scale * (w * ref_rows).sum())
    ref_d = (scale * w * valid)[..., None] * (np.exp(x64 - lse) - np.eye(A_)[tc])
    pt = preds.clone().requires_grad_(True)
    per_row = torch.nn.functional.cross_entropy(pt.reshape(-1, A_), torch.from_numpy(tc.reshape(-1)).cuda(),
                                                reduction="none")
    (per_row * torch.from_numpy((scale * w * valid).reshape(-1)).float().cuda()).sum().backward()
    torch_err = np.abs(pt.grad.cpu().numpy() - ref_d).max()

    call = (lambda **kw: _ce_rows(preds, targets if form == "seq" else None, targets if form == "row" else None,
                                  w_d, scale, **kw))
    acc, rl, dp = call()
    acc2, rl2, dp2 = call()
    acc3, rl3, _ = call(want_grad=False)
    loss, rows, got = acc.item(), rl.cpu().numpy(), dp.cpu().numpy()
    err = np.abs(got - ref_d).max()
    row_err = np.abs(rows - ref_rows).max()
    print(f"ce_rows {B}x{T}x{A_} {form} weighted={weighted}: dpreds err {err:.3e} (torch {torch_err:.3e}), "
          f"rowloss err {row_err:.3e}, loss {loss!r} ref {ref_loss!r}")
    assert err <= 2 * torch_err + ULP
    assert abs(loss - ref_loss) <= 1e-12 * abs(ref_loss)
    assert (np.abs(rows - ref_rows) <= 1e-12 * np.maximum(1.0, np.abs(lse[..., 0]))).all()
    assert not got[w == 0].any() and not got[~valid].any() and not rows[~valid].any()
    assert np.isfinite(got).all()
    assert torch.equal(acc, acc2) and torch.equal(dp, dp2) and torch.equal(rl, rl2)
    assert torch.equal(acc, acc3) and torch.equal(rl, rl3)
    call(want_grad=False, acc=acc)
    assert acc.item() == 2 * loss


@pytest.mark.parametrize("beta", [1.0, 0.5])
@pytest.mark.parametrize("B,T", [(1, 2), (7, 6)])
def test_explore_weights(B, T, beta):
    """dpt_explore_weights against numpy in float64: w[b][j] = exp((l[b][j+1] - l[b][j]) / beta) for
    j < T - 1 and exactly 0 in the last column.  The difference and the product are the same IEEE
    operations on both sides (the library is built without contraction), so only exp() differs: one
    ulp each for the device's and numpy's, held to 4 ulps of double."""
    rs = np.random.RandomState(10 * B + T)
    rl = rs.uniform(0, 3, (B, T))
    rl_d = torch.from_numpy(rl).cuda()
    w_d = torch.full((B, T), float("nan"), dtype=torch.float64, device="cuda")
    _lib_call("dpt_explore_weights", _p(rl_d), B, T, ctypes.c_double(1.0 / beta), _p(w_d), _stream())
    w = w_d.cpu().numpy()
    ref = np.exp((rl[:, 1:] - rl[:, :-1]) * (1.0 / beta))
    rel = np.abs(w[:, :-1] - ref) / ref
    print(f"explore_weights {B}x{T} beta={beta}: max rel err {rel.max():.3e}")
    assert (rel <= 4 * 2.0 ** -52).all()
    assert (w[:, -1] == 0).all() and not np.signbit(w[:, -1]).any()


# ----------------------------------------------------------------------------- the rollout's separate env action
def _rollout_case():
    E, H = 16, 6
    m, w64 = _model(E, L, H, 3)
    rs = np.random.RandomState(21)
    means = rs.uniform(0, 1, (37, A))
    u, g = rs.uniform(size=(H, 37)), rs.normal(size=(H, 37))
    return m.cuda().eval(), w64, means, u, g, H


def test_rollout_env_option_off_is_bit_identical():
    """dpt_rollout_bandit_generic_env with no env action given steps the env with the selected action:
    every output equals dpt_rollout_bandit_generic's bit for bit (Gaussian fp64 and fp32, Bernoulli),
    and env_actions_out echoes the selected actions."""
    from dpt_hip import train as tr
    m, _, means, u, g, H = _rollout_case()
    for kind, f32 in ((0, False), (0, True), (1, False)):
        a = tr.rollout_bandit_generic(m, means, H, VAR, True, kind, uniforms=u, noise=g, f32=f32, want_logits=True)
        b = tr.rollout_bandit_generic(m, means, H, VAR, True, kind, uniforms=u, noise=g, f32=f32, want_logits=True,
                                      random_env=False)
        for k in ("actions", "rewards", "arm_value", "logits"):
            assert torch.equal(a[k], b[k]), (kind, f32, k)
        assert "env_actions" not in a and torch.equal(b["env_actions"], b["actions"])


def test_rollout_injected_env_action():
    """env_actions injected as arm 0 everywhere while the explorer's context actions vary: every
    Gaussian reward is float32(means[i, 0]) + float32(g) * float32(var) bit for bit (DPT_BANDIT_F32)
    and every Bernoulli reward is (noise < means[i, 0]); arm_value is means[i, 0]; actions_out holds
    the selected actions, env_actions_out echoes the injection (clamped when outside [0, A)); and the
    NEXT TOKEN carries the selected action: the float64 oracle's logits on the window built from the
    selected actions and the recorded rewards match the rollout's at every step within 1e-5, while the
    window built from the env actions does not."""
    from dpt_hip import train as tr
    from oracle import dpt_oracle_torch as OT
    m, w64, means, u, g, H = _rollout_case()
    Nn = means.shape[0]
    zeros = np.zeros((H, Nn), np.int32)
    out = tr.rollout_bandit_generic(m, means, H, VAR, True, 0, uniforms=u, noise=g, f32=True, want_logits=True,
                                    env_actions=zeros)
    acts, rews = out["actions"].cpu().numpy(), out["rewards"].cpu().numpy()
    want = (means[:, :1].astype(np.float32) + g.T.astype(np.float32) * np.float32(VAR)).astype(np.float64)
    assert np.array_equal(rews, want)
    assert np.array_equal(out["arm_value"].cpu().numpy(), np.repeat(means[:, :1], H, 1))
    assert not out["env_actions"].any().item()
    assert len(np.unique(acts)) > 1 and (acts != 0).any()  # the context actions vary
    P = OT.state_dict_params(w64, L)
    with torch.no_grad():
        ref = OT.forward(P, _tokens64(acts[:, :H - 1], rews[:, :H - 1], A), L).numpy()  # (N, H, A): row h = step h
        env_ctx = OT.forward(P, _tokens64(np.zeros_like(acts[:, :H - 1]), rews[:, :H - 1], A), L).numpy()
    lg = out["logits"].cpu().numpy().transpose(1, 0, 2)
    assert (np.abs(lg - ref) <= 1e-5 * np.maximum(1, np.abs(ref))).all(), np.abs(lg - ref).max()
    assert np.abs(lg - env_ctx).max() > 1e-3
    # the same selection as a plain rollout's at step 0 (no reward seen yet)
    plain = tr.rollout_bandit_generic(m, means, H, VAR, True, 0, uniforms=u, noise=g, f32=True)
    assert np.array_equal(plain["actions"].cpu().numpy()[:, 0], acts[:, 0])
    # Bernoulli: dr < mean of arm 0
    ub = np.random.RandomState(5).uniform(size=(H, Nn))
    bern = tr.rollout_bandit_generic(m, means, H, VAR, True, 1, uniforms=u, noise=ub, env_actions=zeros)
    assert np.array_equal(bern["rewards"].cpu().numpy(), (ub.T < means[:, :1]).astype(np.float64))
    # varying injected arms are echoed and pay; values outside [0, A) are clamped (device memory: the host
    # cannot reject them)
    ea = np.random.RandomState(6).randint(0, A, (H, Nn)).astype(np.int32)
    ea[0, 0], ea[1, 1] = -3, A + 2
    out = tr.rollout_bandit_generic(m, means, H, VAR, True, 0, uniforms=u, noise=g, f32=True, env_actions=ea)
    got = out["env_actions"].cpu().numpy()
    assert np.array_equal(got, np.clip(ea, 0, A - 1).T)
    assert np.array_equal(out["arm_value"].cpu().numpy(), means[np.arange(Nn)[:, None], got])


def test_rollout_philox_env_action():
    """The env action drawn from DPT_STREAM_ENVACT: inside [0, A), min(A - 1, floor(u A)) of the
    library's own draw keyed by (seed, counter + h, first_task + i), identical across two calls and
    across chunkings (keyed by the global env index), different for another seed and not the
    selection stream's draw."""
    import dpt_hip
    from dpt_hip import _lib
    from dpt_hip import train as tr
    m, _, means, _, _, H = _rollout_case()
    Nn = means.shape[0]

    def run(seed, off=0, n=Nn):
        out = tr.rollout_bandit_generic(m, means[off:off + n], H, VAR, True, 0, seed=seed, first_task=off, f32=True,
                                        random_env=True)
        return {k: out[k].cpu().numpy() for k in ("actions", "env_actions", "rewards", "arm_value")}

    a, b, c = run(77), run(77), run(78)
    ea = a["env_actions"]
    assert ea.min() >= 0 and ea.max() < A and len(np.unique(ea)) == A
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(ea, c["env_actions"])
    assert np.array_equal(a["arm_value"], means[np.arange(Nn)[:, None], ea])
    for off, n in ((0, 16), (16, 16), (32, 5)):
        part = run(77, off, n)
        assert all(np.array_equal(part[k], a[k][off:off + n]) for k in a), off
    draws = np.stack([dpt_hip.draw(0, 77, h, 0, Nn, _lib.STREAM_ENVACT).cpu().numpy() for h in range(H)])
    assert np.array_equal(ea, np.minimum(A - 1, np.floor(draws * A)).astype(np.int32).T)
    sel = np.stack([dpt_hip.draw(0, 77, h, 0, Nn, _lib.STREAM_SELECT).cpu().numpy() for h in range(H)])
    assert not np.array_equal(draws, sel)


# ----------------------------------------------------------------------------- the fused step
def _case(K, E, chunk, step=0):
    """the injected inputs of one step of the (K, E, chunk) case: means, selection uniforms, reward
    normals and env actions"""
    rs = np.random.RandomState(1000 * K + 10 * E + chunk + 7919 * step)
    means = rs.uniform(0, 1, (N, A))
    u, g = rs.uniform(size=(K - 1, N)), rs.normal(size=(K - 1, N))
    ea = rs.randint(0, A, (K - 1, N)).astype(np.int32)
    return means, u, g, ea


def _models(K, E):
    explorer, w_explorer = _model(E, L, 6, 100 * K + E)
    exploiter, w_exploiter = _model(E, L, 6, 100 * K + E + 1)
    return explorer.cuda(), w_explorer, exploiter.cuda(), w_exploiter


def _check_records(acts, env_acts, rews, means, g, ea):
    """the records' own arithmetic: the env is stepped with the injected arm, in GPUBanditEnv's fp32"""
    assert acts.dtype == np.int32 and env_acts.dtype == np.int32 and rews.dtype == np.float64
    assert np.array_equal(env_acts, ea.T)
    m_a = means[np.arange(N)[:, None], env_acts]
    assert np.array_equal(rews, (m_a.astype(np.float32) + g.T.astype(np.float32) * np.float32(VAR)).astype(np.float64))


def _reference(P_explorer, P_exploiter, P_adv, acts, rews, target, beta):
    """The two losses of train_explorer_exploiter.py:102-192 in float64 on the window built from the
    records.  The advantages are computed the reference's way, from K separate forwards of the growing
    prefix windows through the weights ``P_adv`` (without a graph): l_t = CE(last-position logits,
    target), adv[:, t-1] = l_t - l_{t-1}."""
    from oracle import dpt_oracle_torch as OT
    K = acts.shape[1] + 1
    tok = _tokens64(acts, rews, A)
    tg = torch.from_numpy(target)
    ce = torch.nn.functional.cross_entropy
    adv = torch.zeros((N, K - 1), dtype=torch.float64)
    with torch.no_grad():
        previous = None
        for t in range(K):
            current = ce(OT.forward(P_adv, tok[:, :t + 1], L)[:, -1], tg, reduction="none")
            if t > 0:
                adv[:, t - 1] = current - previous
            previous = current
    logits = OT.forward(P_exploiter, tok, L)
    exploiter_loss = ce(logits.reshape(-1, A), tg[:, None].expand(N, K).reshape(-1))  # mean over N K, position 0 in
    logits = OT.forward(P_explorer, tok, L)[:, :-1]
    weight = torch.exp(adv * (1 / beta))
    explorer_loss = (ce(logits.reshape(-1, A), torch.from_numpy(acts.astype(np.int64)).reshape(-1),
                        reduction="none").reshape(N, K - 1) * weight).mean()
    return explorer_loss, exploiter_loss


@pytest.mark.parametrize("chunk", [0, 3])
@pytest.mark.parametrize("E", [32, 18])
@pytest.mark.parametrize("K", [2, 3, 6])
def test_records_follow_the_oracle_selection(K, E, chunk):
    """After one step, the float64 oracle forwards every prefix window built from the step's own
    records through the explorer's pre-step weights; at every (env, step) the recorded context action
    is the one the project's selection rule (float32 softmax, float64 cdf, the injected uniform) picks
    from the oracle's last-position logits.  The oracle's own cdf margin exceeds 1e-5 at every draw --
    asserted first: the draw seeds of _case are chosen so, and a changed oracle or seed fails loudly
    instead of flaking.  The env actions echo the injection and the rewards are its arms' fp32
    arithmetic, whatever the explorer chose."""
    from dpt_hip import train as tr
    from oracle import dpt_oracle as O
    from oracle import dpt_oracle_torch as OT
    explorer, w_explorer, exploiter, _ = _models(K, E)
    means, u, g, ea = _case(K, E, chunk)
    trainer = tr.ExploreExploitTrainer(explorer, exploiter, lr=LR, chunk=chunk)
    actions, env_acts, rewards = trainer.step(means, K, VAR, "uniform", 1.0, uniforms=u, noise=g, env_actions=ea)
    assert actions.shape == env_acts.shape == rewards.shape == (N, K - 1)
    acts, rews = actions.cpu().numpy(), rewards.cpu().numpy()
    _check_records(acts, env_acts.cpu().numpy(), rews, means, g, ea)
    P = OT.state_dict_params(w_explorer, L)
    tok = _tokens64(acts, rews, A)
    picked, margins = [], []
    with torch.no_grad():
        for t in range(K - 1):
            lg = OT.forward(P, tok[:, :t + 1], L)[:, -1].numpy().astype(np.float32)
            margins.append(O.boundary_margin(O.softmax_f32(lg), u[t]))
            picked.append(O.select_actions(lg, u[t]))
    margin = np.min(margins)
    print(f"explore records K={K} E={E} chunk={chunk}: oracle cdf margin {margin:.3e}")
    assert margin > 1e-5, margin
    assert np.array_equal(acts, np.stack(picked, 1))


def _grads_of(trainer, explorer):
    from dpt_hip import train as tr
    params = tr.param_list(explorer)  # the two models share one shape
    return tuple({k: v.cpu().numpy() for k, v in zip(_names(explorer), tr.unpack_grads(db, params))}
                 for db in (trainer.explorer_dblob, trainer.exploiter_dblob))


def _hold(label, got, P):
    ref = {k: v.grad.numpy() for k, v in P.items()}
    worst, at = _worst(got, ref)
    print(f"explore grads {label}: kernel {worst:.3e} of max|g| ({at})")
    for k, r in ref.items():
        e = np.abs(np.asarray(got[k], np.float64) - r).max()
        assert e <= BAR * np.abs(r).max(), (label, k, e / np.abs(r).max())


@pytest.mark.parametrize("beta", [1.0, 0.5])
@pytest.mark.parametrize("chunk", [0, 3])
@pytest.mark.parametrize("E", [32, 18])
@pytest.mark.parametrize("K", [2, 3, 6])
def test_explore_step_gradients(K, E, chunk, beta):
    """Both models' dblob after one ExploreExploitTrainer.step (before AdamW touches them; all envs at
    once, and unequal chunks of 3, 3, 2 added with DPT_EXPLORE_ACCUMULATE) against the float64
    reference conditioned on the step's own records, at the pre-step weights: the advantages from K
    separate prefix-window forwards of the exploiter (the one-forward shortcut is under test), the
    exploiter's mean cross-entropy over all N K positions, the explorer's mean over N (K - 1) of
    exp(adv / beta) CE(logits_j, context action j).  Both losses within 1e-5 relative, every
    parameter's gradient within 5 GRAD_TOL of its largest float64 entry.  At K = 2 the explorer's only
    weighted row is position 0 (no gradient reaches the context token's features)."""
    from dpt_hip import train as tr
    from oracle import dpt_oracle_torch as OT
    explorer, w_explorer, exploiter, w_exploiter = _models(K, E)
    means, u, g, ea = _case(K, E, chunk)
    trainer = tr.ExploreExploitTrainer(explorer, exploiter, lr=LR, weight_decay=1e-4, chunk=chunk)
    actions, env_acts, rewards = trainer.step(means, K, VAR, "uniform", beta, uniforms=u, noise=g, env_actions=ea)
    loss_explorer, loss_exploiter = trainer.read_losses()
    acts, rews = actions.cpu().numpy(), rewards.cpu().numpy()
    _check_records(acts, env_acts.cpu().numpy(), rews, means, g, ea)
    got_explorer, got_exploiter = _grads_of(trainer, explorer)
    P_explorer, P_exploiter = OT.state_dict_params(w_explorer, L), OT.state_dict_params(w_exploiter, L)
    ref_explorer, ref_exploiter = _reference(P_explorer, P_exploiter, P_exploiter, acts, rews, means.argmax(1), beta)
    ref_explorer.backward()
    ref_exploiter.backward()
    print(f"explore step K={K} E={E} chunk={chunk} beta={beta}: explorer loss {loss_explorer!r} ref "
          f"{ref_explorer.item()!r}, exploiter loss {loss_exploiter!r} ref {ref_exploiter.item()!r}")
    assert abs(loss_explorer - ref_explorer.item()) <= 1e-5 * abs(ref_explorer.item())
    assert abs(loss_exploiter - ref_exploiter.item()) <= 1e-5 * abs(ref_exploiter.item())
    label = f"K={K} E={E} chunk={chunk} beta={beta}"
    _hold(label + " exploiter", got_exploiter, P_exploiter)
    _hold(label + " explorer", got_explorer, P_explorer)
    if K == 2:  # position 0 is the query token [1, 0_A, 0, 0]: only its state feature carries a gradient
        assert not got_explorer["embed_transition.weight"][:, 1:].any()
        assert got_explorer["embed_transition.weight"][:, 0].any()
        assert not got_explorer["transformer.wpe.weight"][1:].any()


@pytest.mark.parametrize("E", [32, 18])
def test_the_gradient_bar_can_fail(E):
    """The control of test_explore_step_gradients: the same comparison with the test's reference
    taking the advantages from the exploiter's POST-update weights (the trainer's own blob after its
    AdamW step), or with beta doubled, violates the explorer's bar -- while the right reference holds
    it on the same records.  (The exploiter's loss reads no advantage and is not part of the control.)"""
    from dpt_hip import train as tr
    from oracle import dpt_oracle_torch as OT
    K, chunk, beta = 6, 3, 0.5
    explorer, w_explorer, exploiter, w_exploiter = _models(K, E)
    means, u, g, ea = _case(K, E, chunk)
    trainer = tr.ExploreExploitTrainer(explorer, exploiter, lr=LR, weight_decay=1e-4, chunk=chunk)
    actions, _, rewards = trainer.step(means, K, VAR, "uniform", beta, uniforms=u, noise=g, env_actions=ea)
    acts, rews = actions.cpu().numpy(), rewards.cpu().numpy()
    got_explorer, _ = _grads_of(trainer, explorer)
    w_post = _split64(trainer.exploiter_blob.cpu().numpy().astype(np.float64), exploiter)
    w_post["transformer.wte.weight"] = w_exploiter["transformer.wte.weight"]
    assert np.abs(w_post["pred_actions.weight"] - w_exploiter["pred_actions.weight"]).max() > 0.1 * LR

    def worst(w_adv, b):
        P_explorer, P_exploiter = OT.state_dict_params(w_explorer, L), OT.state_dict_params(w_exploiter, L)
        loss, _ = _reference(P_explorer, P_exploiter, OT.state_dict_params(w_adv, L), acts, rews, means.argmax(1), b)
        loss.backward()
        return _worst(got_explorer, {k: v.grad.numpy() for k, v in P_explorer.items()})[0]

    right, post, doubled = worst(w_exploiter, beta), worst(w_post, beta), worst(w_exploiter, 2 * beta)
    print(f"explore control E={E}: right {right:.3e}, post-update advantages {post:.3e}, beta doubled {doubled:.3e} "
          f"of max|g| (bar {BAR:.1e})")
    assert right <= BAR
    assert post > BAR and doubled > BAR


@pytest.mark.parametrize("chunk", [0, 3])
@pytest.mark.parametrize("E", [32, 18])
@pytest.mark.parametrize("K", [2, 3, 6])
def test_explore_steps_track_the_float64_oracle(K, E, chunk):
    """Three ExploreExploitTrainer.steps with injected draws.  After each step the float64 reference
    (conditioned on the step's records, advantages from the exploiter's weights of before its update)
    takes both losses and one AdamW step per model: losses within 1e-5 relative; at the end, per model,
    at least 0.995 of the parameter entries within 1e-5, max difference at most 2 lr steps + 1e-5
    (test_interactive_steps_track_the_float64_oracle's bars), wte untouched."""
    from dpt_hip import train as tr
    from oracle import dpt_oracle_torch as OT
    steps = 3
    explorer, w_explorer, exploiter, w_exploiter = _models(K, E)
    P_explorer, P_exploiter = OT.state_dict_params(w_explorer, L), OT.state_dict_params(w_exploiter, L)
    names = list(P_explorer)
    opts = [torch.optim.AdamW([P[k] for k in names], lr=LR, weight_decay=1e-4) for P in (P_explorer, P_exploiter)]
    wte = [m.transformer.wte.weight.detach().clone() for m in (explorer, exploiter)]
    trainer = tr.ExploreExploitTrainer(explorer, exploiter, lr=LR, weight_decay=1e-4, chunk=chunk)
    for s in range(steps):
        means, u, g, ea = _case(K, E, chunk, step=s)
        actions, env_acts, rewards = trainer.step(means, K, VAR, "uniform", 0.5, uniforms=u, noise=g, env_actions=ea)
        got = trainer.read_losses()
        acts, rews = actions.cpu().numpy(), rewards.cpu().numpy()
        _check_records(acts, env_acts.cpu().numpy(), rews, means, g, ea)
        for o in opts:
            o.zero_grad()
        ref = _reference(P_explorer, P_exploiter, P_exploiter, acts, rews, means.argmax(1), 0.5)
        for loss in ref:
            loss.backward()
        for o in opts:  # after both backwards: the advantages used the pre-update exploiter
            o.step()
        print(f"explore track K={K} E={E} chunk={chunk} step {s}: losses {got!r} ref "
              f"{(ref[0].item(), ref[1].item())!r}")
        for x, r in zip(got, ref):
            assert abs(x - r.item()) <= 1e-5 * abs(r.item()), (x, r.item())
    assert trainer.read_losses() == (0.0, 0.0) and trainer.steps == steps
    trainer.sync_to_models()
    for which, m, P, w0 in (("explorer", explorer, P_explorer, wte[0]), ("exploiter", exploiter, P_exploiter, wte[1])):
        params = dict(m.named_parameters())
        assert torch.equal(params["transformer.wte.weight"], w0)
        diffs = np.concatenate([np.abs(params[k].detach().cpu().numpy() - P[k].detach().numpy()).ravel()
                                for k in names])
        print(f"explore track K={K} E={E} chunk={chunk} {which}: within 1e-5 {(diffs <= 1e-5).mean():.5f}, "
              f"max {diffs.max():.3e}")
        assert (diffs <= 1e-5).mean() >= 0.995, (which, (diffs <= 1e-5).mean())
        assert diffs.max() <= 2 * LR * steps + 1e-5


@pytest.mark.parametrize("chunk", [0, 3])
def test_explore_step_is_deterministic(chunk):
    """With Philox draws: two steps from the same state and seed give identical records, losses and
    bit-identical blobs for both models, every blob moves, another seed gives other records, and the
    records equal a direct rollout call keyed by the same seed and the chunk's offset."""
    from dpt_hip import train as tr
    K = 6
    explorer, _, exploiter, _ = _models(K, 32)
    means = np.random.RandomState(4).uniform(0, 1, (N, A))
    runs = []
    for seed in (77, 77, 78):
        t = tr.ExploreExploitTrainer(explorer, exploiter, lr=LR, chunk=chunk)
        before = (t.explorer_blob.clone(), t.exploiter_blob.clone())
        records = t.step(means, K, VAR, "uniform", 1.0, seed=seed)
        runs.append(([r.cpu().numpy() for r in records], t.explorer_blob.clone(), t.exploiter_blob.clone(),
                     t.read_losses()))
        assert not torch.equal(t.explorer_blob, before[0]) and not torch.equal(t.exploiter_blob, before[1])
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][0], runs[1][0]))
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2]) and runs[0][3] == runs[1][3]
    assert np.isfinite(runs[0][3]).all() and min(runs[0][3]) > 0
    assert not np.array_equal(runs[0][0][1], runs[2][0][1]) and not np.array_equal(runs[0][0][2], runs[2][0][2])
    for off, n in tr.chunk_plan(N, chunk):
        d = tr.rollout_bandit_generic(explorer, means[off:off + n], K - 1, VAR, True, 0, seed=77, first_task=off,
                                      f32=True, blob=before[0], random_env=True)
        for k, got in zip(("actions", "env_actions", "rewards"), runs[0][0]):
            assert np.array_equal(d[k].cpu().numpy(), got[off:off + n]), (k, off)


def test_explore_trainer_rejects_what_it_cannot_run():
    from dpt_hip import train as tr
    from models.net import Transformer
    cfg = dict(horizon=4, state_dim=1, action_dim=5, n_layer=1, n_embd=16, n_head=1, dropout=0.0, test=False)
    ok, other = Transformer(cfg).cuda(), Transformer(cfg).cuda()
    with pytest.raises(ValueError, match="dropout"):
        tr.ExploreExploitTrainer(ok, Transformer(dict(cfg, dropout=0.1)).cuda(), lr=LR)
    with pytest.raises(ValueError, match="differ in shape"):
        tr.ExploreExploitTrainer(ok, Transformer(dict(cfg, n_layer=2)).cuda(), lr=LR)
    with pytest.raises(ValueError, match="one module"):
        tr.ExploreExploitTrainer(ok, ok, lr=LR)
    t = tr.ExploreExploitTrainer(ok, other, lr=LR)
    with pytest.raises(ValueError, match="K >= 2"):
        t.step(np.full((2, 5), 0.5), 1, VAR, "uniform", 1.0)
    with pytest.raises(ValueError, match="n_positions"):
        t.step(np.full((2, 5), 0.5), 21, VAR, "uniform", 1.0)
    with pytest.raises(ValueError, match="beta"):
        t.step(np.full((2, 5), 0.5), 3, VAR, "uniform", 0.0)
    with pytest.raises(ValueError, match="env_actions"):
        t.step(np.full((2, 5), 0.5), 3, VAR, "uniform", 1.0, env_actions=np.zeros((3, 2), np.int32))
    assert t.steps == 0 and not t.explorer_state.m.any() and not t.exploiter_state.m.any()


# ----------------------------------------------------------------------------- command line
def test_cli_train_explorer_exploiter(tmp_path, monkeypatch, capsys):
    """train_explorer_exploiter.py with 8 envs, K = 4, 1 epoch of 2 episodes in a scratch directory:
    the reference's epoch line with finite losses, both checkpoints, each loading strictly into
    Transformer and differing from the initial weights; the same run with --dropout 0.1 takes the plain
    path: finite losses, and both models' parameters change."""
    import importlib

    from models.net import Transformer
    te = importlib.import_module("train_explorer_exploiter")
    monkeypatch.chdir(tmp_path)
    run = ["--env", "bandit", "--envs", "8", "--H", "4", "--K", "4", "--dim", "5", "--embd", "16", "--layer", "2",
           "--num_epochs", "1", "--episodes_per_epoch", "2", "--beta", "0.5"]
    paths = ("trained_models/explorer_bandit.pt", "trained_models/exploiter_bandit.pt")

    def check(dropout):
        out = capsys.readouterr().out
        assert out.rstrip().endswith("Done.")
        found = re.findall(r"^Epoch 1/1 - explorer_loss: (\S+) - exploiter_loss: (\S+) - time: \S+s$", out, flags=re.M)
        assert len(found) == 1, out
        vals = [float(v) for v in found[0]]
        assert np.isfinite(vals).all() and min(vals) > 0, vals
        torch.manual_seed(0)
        cfg = dict(horizon=4, state_dim=1, action_dim=5, n_layer=2, n_embd=16, n_head=1, dropout=dropout, test=False)
        inits = [Transformer(cfg), Transformer(cfg)]  # the script's two models, in its order, after set_seeds(0)
        sds = []
        for path, fresh in zip(paths, inits):
            assert os.path.exists(path)
            sd = torch.load(path, map_location="cpu", weights_only=True)
            init = {k: v.clone() for k, v in fresh.state_dict().items()}
            assert set(sd) == set(init)
            fresh.load_state_dict(sd, strict=True)
            assert torch.equal(sd["transformer.wte.weight"], init["transformer.wte.weight"])
            for k in ("embed_transition.weight", "transformer.h.1.attn.c_attn.weight", "pred_actions.bias"):
                assert not torch.equal(sd[k], init[k]), (path, k)
            sds.append(sd)
            os.remove(path)
        assert not torch.equal(sds[0]["pred_actions.weight"], sds[1]["pred_actions.weight"])

    te.main(run)
    check(0.0)
    te.main(run + ["--dropout", "0.1"])
    check(0.1)
