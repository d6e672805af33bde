"""The fused interactive DarkRoom training step (csrc/dpt_interactive_mdp.hip,
dpt_hip.train.InteractiveMDPTrainer / rollout_darkroom_interactive, envs/gpu_darkroom_env.py,
train_interactive_darkroom.py).

The pack kernel against Transformer._tokens bit for bit; the act step against the three-call chain
dpt_select_action -> dpt_darkroom_step -> dpt_darkroom_opt_action bit for bit (and its Philox draws against
dpt_draw and the numpy replay); the device records against the float64 oracle's episode on inputs whose
draws are clear of near-ties; the gradient blob before AdamW against the float64 autograd gradient of the
contract's loss conditioned on the step's own records (loss within 1e-5 relative, every parameter within
5 GRAD_TOL of its largest float64 entry), with two controls that the same bar rejects; the trainer's
plumbing; and the command-line tool on both of its paths."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import interactive_mdp_oracle as MO
import philox_np
from test_gpu_train import GRAD_TOL

pytestmark = pytest.mark.gpu

A = 5


def _lib_call(name, *args):
    from dpt_hip import _lib
    _lib.call(name, *args)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _np(rec):
    return {k: v.cpu().numpy() for k, v in rec.items()}


# ----------------------------------------------------------------------------- pack
@pytest.mark.parametrize("t", [0, 1, 4])
def test_pack_equals_tokens(t):
    """dpt_mdp_pack on records == Transformer._tokens (models/net.py:42-54) on the batch those records make at
    step t, bit for bit; an action outside [0, 5) packs a zero one-hot; N K spans more than one block."""
    from models.net import Transformer
    N, K, dim = 37, 5, 10
    rs = np.random.RandomState(t)
    states = rs.randint(0, dim, (N, K, 2)).astype(np.int32)
    acts = rs.randint(0, A, (N, K - 1)).astype(np.int32)
    acts[1, 0], acts[2, min(t, K - 2)] = 7, -1
    rews = rs.randint(0, 2, (N, K - 1)).astype(np.int32)
    s_d, a_d, r_d = (torch.from_numpy(x).cuda() for x in (states, acts, rews))
    tokens = torch.full((N, t + 1, 10), float("nan"), device="cuda")
    _lib_call("dpt_mdp_pack", _p(s_d), _p(a_d), _p(r_d), N, K, t, _p(tokens), _stream())
    m = Transformer(dict(horizon=K, state_dim=2, action_dim=A, n_layer=1, n_embd=16, n_head=1, dropout=0.0,
                         test=True))
    onehot = (torch.from_numpy(acts).long()[..., None] == torch.arange(A)).float()
    batch = {"query_states": torch.from_numpy(states[:, t]).float(),
             "context_states": torch.from_numpy(states[:, :t]).float(), "context_actions": onehot[:, :t],
             "context_next_states": torch.from_numpy(states[:, 1:t + 1]).float(),
             "context_rewards": torch.from_numpy(rews[:, :t]).float()[..., None]}
    ref = m._tokens(batch)
    assert tokens.shape == ref.shape and torch.equal(tokens, ref)
    assert torch.equal(tokens.cpu().double(), MO.window(states, acts, rews, t))
    if t >= 1:
        assert not tokens[1, 1, 2:7].any()


# ----------------------------------------------------------------------------- act step
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("mode", ["injected", "philox", "greedy"])
def test_act_step_equals_the_three_call_chain(mode, permuted):
    """dpt_darkroom_act_step == dpt_select_action (temp 1) -> dpt_darkroom_step -> dpt_darkroom_opt_action on
    the same last-position logits, bit for bit, for 300 envs (two blocks) at window 3: sampled with injected
    uniforms, sampled with Philox draws (which are dpt_draw's and the numpy replay's) and greedy, with tied
    and near-tied logits; it writes step t's action and reward, step t + 1's state and target, the int64
    copy of that target, and nothing else."""
    import dpt_hip
    N, window, K, t, dim, seed, counter, first = 300, 3, 6, 2, 4, 99, 7, 1000
    rs = np.random.RandomState(5 + permuted)
    logits = rs.normal(0, 2, (N, window, A)).astype(np.float32)
    logits[0, -1] = 1.5  # all tied
    logits[1, -1, 3] = logits[1, -1, 1] = logits[1, -1].max() + 1  # two maxima
    logits[2, -1] = [0.0, np.float32(1e-7), 0.0, 0.0, 0.0]
    sample = 0 if mode == "greedy" else 1
    u = rs.uniform(size=N) if mode == "injected" else None
    goals = rs.randint(0, dim, (N, 2)).astype(np.int32)
    perm = np.stack([rs.permutation(5) for _ in range(N)]).astype(np.int32) if permuted else None
    states = np.full((N, K, 2), -9, np.int32)
    states[:, t] = rs.randint(0, dim, (N, 2))
    states[:40, t] = [[0, 0], [dim - 1, dim - 1], [0, dim - 1], [dim - 1, 0]] * 10  # corners: clipped moves
    lg_d, g_d, s_d = (torch.from_numpy(x).cuda() for x in (logits, goals, states))
    pm_d = None if perm is None else torch.from_numpy(perm).cuda()
    u_d = None if u is None else torch.from_numpy(u).cuda()
    acts = torch.full((N, K - 1), -9, dtype=torch.int32, device="cuda")
    rews, tgts = torch.full_like(acts, -9), torch.full((N, K), -9, dtype=torch.int32, device="cuda")
    nxt = torch.full((N,), -9, dtype=torch.int64, device="cuda")
    _lib_call("dpt_darkroom_act_step", _p(lg_d), N, window, K, t, dim, sample, _p(u_d), seed, counter, first,
              _p(g_d), _p(pm_d), _p(s_d), _p(acts), _p(rews), _p(tgts), _p(nxt), _stream())

    a_ref = dpt_hip.select_action(lg_d[:, -1].contiguous(), sample, 1.0, u_d, seed=seed, counter=counter,
                                  first_task=first)
    ns_ref, r_ref = dpt_hip.darkroom_step(s_d[:, t].contiguous(), a_ref, g_d, pm_d, dim)
    tg_ref = dpt_hip.darkroom_opt_action(ns_ref, g_d, pm_d)
    assert torch.equal(acts[:, t], a_ref) and torch.equal(rews[:, t], r_ref)
    assert torch.equal(s_d[:, t + 1], ns_ref) and torch.equal(tgts[:, t + 1], tg_ref)
    assert torch.equal(nxt, tg_ref.long())
    keep = np.ones(K, bool)
    keep[[t, t + 1]] = False
    assert (s_d.cpu().numpy()[:, keep] == -9).all() and np.array_equal(s_d.cpu().numpy()[:, t], states[:, t])
    assert (np.delete(acts.cpu().numpy(), t, 1) == -9).all() and (np.delete(rews.cpu().numpy(), t, 1) == -9).all()
    assert (np.delete(tgts.cpu().numpy(), t + 1, 1) == -9).all()
    a = a_ref.cpu().numpy()
    if mode == "greedy":
        assert np.array_equal(a, logits[:, -1].argmax(1)) and a[0] == 0 and a[1] == 1 and a[2] == 1
    if mode == "philox":
        draws = dpt_hip.draw(0, seed, counter, first, N, dpt_hip.STREAM_SELECT)
        assert np.array_equal(draws.cpu().numpy(), philox_np.uniform(seed, counter, first + np.arange(N), 0))
        assert torch.equal(dpt_hip.select_action(lg_d[:, -1].contiguous(), 1, 1.0, draws), a_ref)
    # the float64 helper agrees wherever its draw is clear of a near-tie
    if sample:
        uu = u if u is not None else philox_np.uniform(seed, counter, first + np.arange(N), 0)
        a64, margin = MO.select(logits[:, -1], True, uu)
        clear = margin > 1e-5
        assert clear.mean() > 0.99 and np.array_equal(a64[clear], a[clear])
    ns64, r64 = MO.transit(states[:, t], a, goals, dim, perm)
    assert np.array_equal(ns64, ns_ref.cpu().numpy()) and np.array_equal(r64, r_ref.cpu().numpy())
    assert np.array_equal(MO.opt_action(ns64, goals, perm), tg_ref.cpu().numpy())
    moved = a if perm is None else perm[np.arange(N), a]
    assert ((moved != 4) & (ns64 == states[:, t]).all(1)).any() and (r64 == 1).any()


# ----------------------------------------------------------------------------- records
@pytest.mark.parametrize("E,permuted", [(32, False), (18, False), (32, True)])
def test_records_follow_the_float64_oracle(E, permuted):
    """dim 3, 7 envs, 6 steps, goals including (0, 0), (0, 1) and (2, 2), injected uniforms, widths 32 (matrix
    cores) and 18 (row kernels), one case with permuted actions.  Every oracle draw has a cdf margin above
    1e-5 and the oracle's records hold a reward 1 and a clipped move (conditions on the inputs, also checked
    without a GPU in test_interactive_mdp_host.py); then the device's states, actions, rewards and targets
    equal the oracle's exactly."""
    from dpt_hip import train as tr
    m, _, u, perm, ep = MO.records_case(E, permuted)
    assert ep["margins"].min() > 1e-5 and (ep["rewards"] == 1).any()
    moved = ep["actions"] if perm is None else perm[np.arange(MO.REC_N)[:, None], ep["actions"]]
    assert ((moved != 4) & (ep["states"][:, 1:] == ep["states"][:, :-1]).all(-1)).any()
    rec, ret = tr.rollout_darkroom_interactive(m.cuda(), MO.REC_GOALS, MO.REC_K, MO.REC_DIM, True, perm=perm,
                                               uniforms=u)
    got = _np(rec)
    for k in ("states", "actions", "rewards", "targets"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ep[k]), k
    assert np.array_equal(ret.cpu().numpy(), ep["rewards"].sum(1))


# ----------------------------------------------------------------------------- gradient
def _blob_order(m, grads):
    """the float64 gradients {name: array} flattened in blob order, and each parameter's (name, lo, hi)"""
    from dpt_hip import train as tr
    name_of = {id(p): k for k, p in m.named_parameters()}
    params = tr.param_list(m)
    n = len(params)
    flat = [(grads[name_of[id(p)]].T if i in (0, n - 2) else grads[name_of[id(p)]]).reshape(-1)
            for i, p in enumerate(params)]
    ends = np.cumsum([g.size for g in flat])
    return np.concatenate(flat), [(name_of[id(p)], hi - g.size, hi) for p, g, hi in zip(params, flat, ends)]


def _bar_violations(loss, dblob, ref_loss, ref_grads, m):
    """what of the project's bar fails: the loss beyond 1e-5 relative, parameters beyond 5 GRAD_TOL max|ref|"""
    g64, spans = _blob_order(m, ref_grads)
    bad = [] if abs(loss - ref_loss) <= 1e-5 * abs(ref_loss) else [("loss", loss, ref_loss)]
    for name, lo, hi in spans:
        e, scale = np.abs(dblob[lo:hi] - g64[lo:hi]).max(), np.abs(g64[lo:hi]).max()
        if not e <= 5 * GRAD_TOL * scale:
            bad.append((name, e, scale))
    return bad


def _one_step(E, K, N, mode, chunk, seed, sharp=None, dim=3):
    """one InteractiveMDPTrainer.step with injected uniforms on a fresh model: (model, float64 weights, loss,
    the gradient blob before AdamW as float64, the records)"""
    from dpt_hip import train as tr
    m, w64 = MO.model(E, 2, K, seed, sharp)
    m = m.cuda()
    rs = np.random.RandomState(seed)
    goals = rs.randint(0, dim, (N, 2)).astype(np.int32)
    u = rs.uniform(size=(K - 1, N))
    trainer = tr.InteractiveMDPTrainer(m, lr=1e-3, chunk=chunk, loss=mode)
    blob = trainer.blob.clone()
    rec = _np(trainer.step(goals, K, dim, uniforms=u))
    loss, dblob = trainer.read_loss(), trainer.dblob.cpu().numpy().astype(np.float64)
    assert trainer.steps == 1 and not torch.equal(trainer.blob, blob)
    assert rec["states"].shape == (N, K, 2) and rec["targets"].shape == (N, K)
    assert rec["actions"].shape == rec["rewards"].shape == (N, K - 1)
    assert (rec["states"][:, 0] == 0).all()
    assert np.array_equal(rec["targets"], np.stack([MO.opt_action(rec["states"][:, t], goals) for t in range(K)], 1))
    return m, w64, loss, dblob, rec


@pytest.mark.parametrize("chunk", [0, 3])
@pytest.mark.parametrize("E", [32, 18])
@pytest.mark.parametrize("mode", ["every", "last"])
@pytest.mark.parametrize("K", [1, 2, 6])
def test_gradient_vs_float64_oracle(K, mode, E, chunk):
    """dblob before AdamW against the float64 autograd gradient of the contract's loss conditioned on the
    step's own records (7 envs, 2 layers; all envs at once and chunks of 3, 3, 1): the loss within 1e-5
    relative, every parameter within 5 GRAD_TOL of its largest float64 entry."""
    m, w64, loss, dblob, rec = _one_step(E, K, 7, mode, chunk, 100 * K + E + chunk)
    ref_loss, ref_grads = MO.loss_and_grads(w64, 2, rec, mode)
    print(f"K={K} {mode} E={E} chunk={chunk}: loss {loss!r} ref {ref_loss!r}")
    assert _bar_violations(loss, dblob, ref_loss, ref_grads, m) == []


@pytest.mark.parametrize("mode", ["every", "last"])
def test_gradient_vs_float64_oracle_long_window(mode):
    """K = 66, 3 envs, width 32: the windows cross the 64 / 65 edges of the matrix-core kernels and the
    second lap of the last-position attention kernel."""
    m, w64, loss, dblob, rec = _one_step(32, 66, 3, mode, 0, 66, dim=5)
    ref_loss, ref_grads = MO.loss_and_grads(w64, 2, rec, mode)
    print(f"K=66 {mode}: loss {loss!r} ref {ref_loss!r}")
    assert _bar_violations(loss, dblob, ref_loss, ref_grads, m) == []


def test_gradient_vs_float64_oracle_sharp_attention():
    """the same bar on a sharp_models 'medium' model (peaked attention, larger LayerNorm gains)"""
    m, w64, loss, dblob, rec = _one_step(32, 6, 7, "every", 0, 31, sharp="medium")
    ref_loss, ref_grads = MO.loss_and_grads(w64, 2, rec, "every")
    print(f"sharp: loss {loss!r} ref {ref_loss!r}")
    assert _bar_violations(loss, dblob, ref_loss, ref_grads, m) == []


def test_the_bar_rejects_a_shifted_target_and_a_wrong_scale():
    """Controls: the same bar is violated when the oracle scores step t against target_{t+1} in place of
    target_t, and when 'every' is scored with 'last's scale 1 / N."""
    K, N = 6, 7
    m, w64, loss, dblob, rec = _one_step(32, K, N, "every", 0, 17)
    assert _bar_violations(loss, dblob, *MO.loss_and_grads(w64, 2, rec, "every"), m) == []
    shifted = rec["targets"].copy()
    shifted[:, :-1] = rec["targets"][:, 1:]
    assert (shifted != rec["targets"]).any()
    assert _bar_violations(loss, dblob, *MO.loss_and_grads(w64, 2, rec, "every", targets=shifted), m) != []
    assert _bar_violations(loss, dblob, *MO.loss_and_grads(w64, 2, rec, "every", scale=1.0 / N), m) != []
    m, w64, loss, dblob, rec = _one_step(32, K, N, "last", 0, 17)
    assert _bar_violations(loss, dblob, *MO.loss_and_grads(w64, 2, rec, "last"), m) == []
    assert _bar_violations(loss, dblob, *MO.loss_and_grads(w64, 2, rec, "every"), m) != []


# ----------------------------------------------------------------------------- plumbing
@pytest.mark.parametrize("mode,chunk", [("every", 0), ("last", 3)])
def test_trainer_steps_track_float64_adamw(mode, chunk):
    """Three InteractiveMDPTrainer.steps against the same AdamW steps on the float64 oracle's gradients,
    each conditioned on the step's own records, under test_gpu_train_step._fused_steps_vs_oracle's bars:
    the loss within 1e-5 relative, at least 0.995 of the parameter entries within 1e-5, the largest
    difference at most 2 lr steps + 1e-5; wte is untouched."""
    from dpt_hip import train as tr
    from oracle import dpt_oracle_torch as OT
    N, K, dim, L, lr, steps = 8, 5, 3, 2, 1e-3, 3
    m, w64 = MO.model(32, L, K, 7)
    m = m.cuda()
    P = OT.state_dict_params(w64, L)
    names = list(P)
    opt_ref = torch.optim.AdamW([P[k] for k in names], lr=lr, weight_decay=1e-4)
    wte = m.transformer.wte.weight.detach().clone()
    trainer = tr.InteractiveMDPTrainer(m, lr=lr, weight_decay=1e-4, chunk=chunk, loss=mode)
    rs = np.random.RandomState(3)
    for s in range(steps):
        goals = rs.randint(0, dim, (N, 2))
        rec = _np(trainer.step(goals, K, dim, uniforms=rs.uniform(size=(K - 1, N))))
        loss = trainer.read_loss()
        opt_ref.zero_grad()
        ref_loss = MO.loss(P, L, rec, mode)
        ref_loss.backward()
        opt_ref.step()
        assert abs(loss - ref_loss.item()) <= 1e-5 * abs(ref_loss.item()), (s, loss, ref_loss.item())
    assert trainer.read_loss() == 0.0 and trainer.steps == steps
    trainer.sync_to_model()
    params = dict(m.named_parameters())
    assert torch.equal(params["transformer.wte.weight"], wte)
    diffs = np.concatenate([np.abs(params[k].detach().cpu().numpy() - P[k].detach().numpy()).ravel()
                            for k in names])
    assert (diffs <= 1e-5).mean() >= 0.995, (diffs <= 1e-5).mean()
    assert diffs.max() <= 2 * lr * steps + 1e-5


def test_records_do_not_depend_on_the_chunking_and_calls_repeat():
    """Under Philox draws the chunked (3, 3, 2) and the unchunked step write bit-equal records (first_task =
    the chunk's offset), whose first actions are dpt_select_action's on dpt_draw's uniforms; a repeated call
    from the same state is bit-identical in records, gradient blob, loss and updated weights; another seed
    gives other records."""
    from dpt_hip import train as tr
    N, K, dim = 8, 6, 4
    m, _ = MO.model(32, 2, K, 5)
    m = m.cuda()
    goals = np.random.RandomState(4).randint(0, dim, (N, 2))
    runs = []
    for chunk, seed in ((0, 77), (0, 77), (3, 77), (0, 78)):
        t = tr.InteractiveMDPTrainer(m, lr=1e-3, chunk=chunk)
        rec = _np(t.step(goals, K, dim, seed=seed))
        runs.append((rec, t.dblob.clone(), t.read_loss(), t.blob.clone()))
    for k in ("states", "actions", "rewards", "targets"):
        assert np.array_equal(runs[0][0][k], runs[1][0][k]) and np.array_equal(runs[0][0][k], runs[2][0][k]), k
    assert torch.equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2] and torch.equal(runs[0][3], runs[1][3])
    assert abs(runs[0][2] - runs[2][2]) <= 1e-5 * abs(runs[0][2])
    assert not np.array_equal(runs[0][0]["actions"], runs[3][0]["actions"])
    # the Philox records are those of the same step fed the numpy replay of its uniforms
    u = np.stack([philox_np.uniform(77, t, np.arange(N), 0) for t in range(K - 1)])
    t = tr.InteractiveMDPTrainer(m, lr=1e-3, chunk=3)
    rec = _np(t.step(goals, K, dim, uniforms=u))
    for k in ("states", "actions", "rewards", "targets"):
        assert np.array_equal(runs[0][0][k], rec[k]), k


def test_loss_none_writes_the_same_records_and_no_gradient():
    """DPT_MDP_LOSS_NONE (rollout_darkroom_interactive) writes the records of a loss mode's step from the same
    weights and uniforms, in sampled and greedy mode, and touches neither a gradient blob nor a loss
    accumulator handed to it."""
    from dpt_hip import _lib
    from dpt_hip import train as tr
    N, K, dim = 8, 6, 4
    m, _ = MO.model(18, 2, K, 9)
    m = m.cuda()
    rs = np.random.RandomState(2)
    goals, u = rs.randint(0, dim, (N, 2)), rs.uniform(size=(K - 1, N))
    for sample in (True, False):
        t = tr.InteractiveMDPTrainer(m, lr=1e-3, chunk=3, loss="last")
        blob = t.blob.clone()
        rec0, ret = tr.rollout_darkroom_interactive(m, goals, K, dim, sample, uniforms=u, blob=blob)
        rec1, _ = t.rollout(goals, K, dim, sample, uniforms=u)
        rec2 = t.step(goals, K, dim, sample=sample, uniforms=u)
        for k in ("states", "actions", "rewards", "targets"):
            assert torch.equal(rec0[k], rec1[k]) and torch.equal(rec0[k], rec2[k]), (sample, k)
        assert torch.equal(ret, rec2["rewards"].sum(1))
        g, pm, ud, seed = tr._mdp_episode(goals, K, None, u, 0, blob.device)
        dblob = torch.full_like(blob, 7.0)
        acc = torch.full((1,), 3.0, dtype=torch.float64, device=blob.device)
        tr._mdp_run(t._d, blob, lambda n: tr._mdp_workspace(t._d, n, K, _lib.MDP_LOSS_NONE, blob.device, "test", 0), 0,
                    _lib.MDP_LOSS_NONE, g, K, dim, sample, pm, ud, seed, dblob, acc)
        assert (dblob == 7.0).all() and acc.item() == 3.0


def test_trainer_rejects_what_it_cannot_run():
    from dpt_hip import train as tr
    from models.net import Transformer
    cfg = dict(horizon=4, state_dim=2, action_dim=5, n_layer=1, n_embd=16, n_head=1, dropout=0.0, test=True)
    with pytest.raises(ValueError, match="dropout"):
        tr.InteractiveMDPTrainer(Transformer(dict(cfg, dropout=0.1)).cuda(), lr=1e-3)
    with pytest.raises(ValueError, match="state_dim"):
        tr.InteractiveMDPTrainer(Transformer(dict(cfg, state_dim=1)).cuda(), lr=1e-3)
    with pytest.raises(ValueError, match="loss"):
        tr.InteractiveMDPTrainer(Transformer(cfg).cuda(), lr=1e-3, loss="sum")
    t = tr.InteractiveMDPTrainer(Transformer(cfg).cuda(), lr=1e-3)
    goals = np.zeros((2, 2), np.int32)
    with pytest.raises(ValueError, match="n_positions"):
        t.step(goals, 21, 3)
    with pytest.raises(ValueError, match="uniforms"):
        t.step(goals, 3, 3, uniforms=np.zeros((3, 2)))
    with pytest.raises(ValueError, match="goals"):
        t.step(np.zeros((2, 3), np.int32), 3, 3)
    with pytest.raises(ValueError, match="dim"):
        t.step(goals, 3, 0)
    assert t.steps == 0 and not t.m.any()


def test_gpu_darkroom_env_steps_like_the_kernels():
    """GPUDarkroomEnv: goals from the device generator inside the room, reset to (0, 0), step through
    dpt_darkroom_step, opt_action, and the episode's end."""
    from envs.gpu_darkroom_env import GPUDarkroomEnv
    torch.manual_seed(3)
    env = GPUDarkroomEnv(4, 50, 3)
    goals = env.goals.cpu().numpy()
    assert goals.shape == (50, 2) and goals.min() >= 0 and goals.max() < 4 and len(np.unique(goals, axis=0)) > 5
    torch.manual_seed(3)
    assert torch.equal(GPUDarkroomEnv(4, 50, 3).goals, env.goals)
    s = env.reset()
    assert s.shape == (50, 2) and not s.any()
    rs = np.random.RandomState(0)
    state = np.zeros((50, 2), np.int64)
    for step in range(3):
        assert np.array_equal(env.opt_action().cpu().numpy(), MO.opt_action(state, goals))
        a = rs.randint(0, 5, 50)
        ns, r, done, _ = env.step(torch.nn.functional.one_hot(torch.from_numpy(a), 5).float().cuda())
        state, r64 = MO.transit(state, a, goals, 4)
        assert np.array_equal(ns.cpu().numpy(), state) and np.array_equal(r.cpu().numpy(), r64)
        assert bool(done.all()) == (step == 2)
    with pytest.raises(ValueError, match="already ended"):
        env.step(torch.zeros((50, 5)))


# ----------------------------------------------------------------------------- command line
def test_cli_train_interactive_darkroom(tmp_path, monkeypatch, capsys):
    """train_interactive_darkroom.py for 2 epochs of 3 episodes in a scratch directory on the fused path: two
    finite loss / return lines, the evaluation line with the expert's return, a checkpoint that loads
    strictly into Transformer and differs from the initial weights; the same run with --loss last; and with
    --dropout 0.1, the plain per-step path."""
    import importlib

    from models.net import Transformer
    ti = importlib.import_module("train_interactive_darkroom")
    monkeypatch.chdir(tmp_path)
    run = ["--env", "darkroom", "--envs", "16", "--H", "5", "--dim", "3", "--embd", "16", "--layer", "2",
           "--num_epochs", "2", "--episodes_per_epoch", "3", "--n_eval", "8"]

    def lines():
        out = capsys.readouterr().out
        assert out.rstrip().endswith("Done.")
        found = re.findall(r"^Epoch (\d)/2 - loss: (\S+) - return: (\S+) - time: \S+s$", out, flags=re.M)
        assert [int(i) for i, _, _ in found] == [1, 2], out
        ev = re.findall(r"^Eval \(8 goals, greedy, K=5\) - return: (\S+) - expert: (\S+)$", out, flags=re.M)
        assert len(ev) == 1, out
        value, expert = float(ev[0][0]), float(ev[0][1])
        assert 0 <= value <= expert <= 4
        return [float(v) for _, v, _ in found], [float(v) for _, _, v in found]

    path = "trained_models/interactive_darkroom.pt"
    for extra in ([], ["--loss", "last", "--chunk", "5"], ["--dropout", "0.1"]):
        ti.main(run + extra)
        losses, returns = lines()
        assert np.isfinite(losses).all() and min(losses) > 0, losses
        assert np.isfinite(returns).all() and min(returns) >= 0 and max(returns) <= 4, returns
        sd = torch.load(path, map_location="cpu", weights_only=True)
        torch.manual_seed(0)
        fresh = Transformer(dict(horizon=5, state_dim=2, action_dim=5, n_layer=2, n_embd=16, n_head=1, dropout=0.0,
                                 test=True))
        init = {k: v.clone() for k, v in fresh.state_dict().items()}
        assert set(sd) == set(init)
        fresh.load_state_dict(sd, strict=True)
        for k in ("embed_transition.weight", "transformer.h.1.attn.c_attn.weight", "pred_actions.bias"):
            assert not torch.equal(sd[k], init[k]), (extra, k)
        os.remove(path)


@pytest.mark.parametrize("mode", ["every", "last"])
def test_plain_step_agrees_with_the_fused_step(mode):
    """interactive_mdp_step_plain (the per-step loop on the module with torch.optim.AdamW) and the fused step
    fed the same goals and the same Philox seed: the same first-episode loss to 1e-5 relative and the same
    mean return."""
    import importlib

    from dpt_hip import train as tr
    from envs.gpu_darkroom_env import GPUDarkroomEnv
    ti = importlib.import_module("train_interactive_darkroom")
    N, K, dim, seed = 8, 5, 3, 123
    m, _ = MO.model(16, 2, K, 21)
    m = m.cuda()
    env = GPUDarkroomEnv(dim, N, K)
    trainer = tr.InteractiveMDPTrainer(m, lr=1e-3, weight_decay=1e-4, loss=mode)
    rec = trainer.step(env.goals, K, dim, seed=seed)
    fused = trainer.read_loss()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
    loss, ret = ti.interactive_mdp_step_plain(m, opt, env, K, mode, seed=seed)
    print(f"{mode}: fused {fused!r} plain {loss.item()!r}")
    assert abs(loss.item() - fused) <= 1e-5 * abs(fused)
    assert ret.item() == rec["rewards"].sum().item() / N
