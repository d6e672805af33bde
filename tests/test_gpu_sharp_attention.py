"""Every forward and gradient path on models with sharp attention (tests/sharp_models.py), held to
the float64 oracle.

The other parity tests run models whose attention is near-uniform (score spans 0.2-0.4, largest
probability 1 / T): the running-max rescale of the online softmax, its combination across waves, laps
and 16-key tiles, the -inf start, a peaked P in dS = P (dP - sum P dP), the fp16 split products' scales,
the queries on the folded attention weights, gelu beyond |h| = 2 and the 24-bit y cache under a large
G all sit on easy values there.  Here the same paths run at two levels, ``medium`` (spans 4-15) and
``sharp`` (spans 30-250, top probability 0.5-1.0), asserted first on the float64 oracle in every test.

Bars: medium and the peaked head keep the project's (logits 1e-5 max(1, |x|); every gradient within
5 GRAD_TOL of the largest entry of its float64 gradient; actions, rewards, arm values and returns exact
up to a task's first differing action, which must sit on a near-tie draw; >= 0.9 of the task-steps
compared).  At sharp a case's bar is max(project bar, 2 x the fp32 oracle's error on the same inputs);
the fp32 reference is always an oracle, never a kernel.  Each case prints the kernel's worst error next
to the fp32 oracle's (lines starting SHARP-ERR; profiles/sharp_attention/errors.txt is one run's record).
tests/test_sharp_models_host.py checks the family itself without a GPU."""
import re

import numpy as np
import pytest
import torch

import sharp_models as SM
from test_gpu_kernels import compared_steps

pytestmark = pytest.mark.gpu

LOGIT_BAR = 1e-5
LEVELS = SM.LEVEL_NAMES


def dh():
    import dpt_hip
    dpt_hip.device()
    return dpt_hip


@pytest.fixture(autouse=True)
def _defaults():
    yield
    import dpt_hip
    dpt_hip.set_decode_tile(8)
    dpt_hip.set_ycache_bits(24)
    dpt_hip.set_prefill(True)
    dpt_hip.set_darkroom_workspace(True)
    dpt_hip.set_darkroom_memo(True)


def _scaled_c_attn(w, block, rel=1e-3):
    """the bar-can-fail control: one block's c_attn.weight off by a relative ``rel``"""
    w = dict(w)
    k = f"transformer.h.{block}.attn.c_attn.weight"
    w[k] = (w[k].astype(np.float64) * (1 + rel)).astype(np.float32)
    return w


# ----------------------------------------------------------------------------- 1. window forward
def _window_errors(m, env, level, T, prefill, out_mode):
    """(kernel error, fp32 oracle error) of one dpt_forward_window call against the float64 oracle"""
    d = dh()
    r64, r32 = SM.window_refs(env, level, T)
    rows = slice(-1, None) if out_mode == 0 else slice(1, None)
    q, cs, ca, cn, cr = SM.window_inputs(env, T)
    d.set_prefill(prefill)
    args = (q,) if T == 1 else (q, cs, ca, cn, cr)
    got = m.forward_window(*args, out_mode=out_mode).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    if out_mode == 0:
        got = got[:, None]
    return SM.rel_err(got, r64[:, rows]), SM.rel_err(r32[:, rows], r64[:, rows])


def _assert_window_sharp(env, level, T):
    SM.assert_sharp(level, SM.token_stats(SM.window_weights(env, level), 4, SM.window_seq(env, T)),
                    f"window {env} T={T} {level}")


def _window_model(env, level, w=None):
    d = dh()
    w = SM.window_weights(env, level) if w is None else w
    return d.DeviceModel(SM.as_torch(w), 4, 1 if env == "bandit" else 2, 5, 404)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("env", ["bandit", "darkroom"])
def test_window_forward(env, level):
    """dpt_forward_window at T = 1, 17, 65, 101, MFMA prefill and position by position, last-position
    logits and every context row"""
    for T in SM.WINDOW_TS[1:]:  # T = 1 has one score and no span
        _assert_window_sharp(env, level, T)
    m = _window_model(env, level)
    worst = (0.0, 0.0)
    for T in SM.WINDOW_TS:
        for prefill in (True, False):
            for out_mode in ((0,) if T == 1 else (0, 1)):
                err, err32 = _window_errors(m, env, level, T, prefill, out_mode)
                bar = SM.bar(level, LOGIT_BAR, err32)
                print(f"  window {env} {level} T={T} prefill={int(prefill)} out_mode={out_mode}: kernel {err:.3e}, "
                      f"fp32 oracle {err32:.3e}, bar {bar:.1e}")
                assert err <= bar, (T, prefill, out_mode, err, bar)
                worst = max(worst, (err, err32))
    print(f"SHARP-ERR item=1 window {env} {level}: kernel {worst[0]:.3e}, fp32 oracle {worst[1]:.3e}")


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("env", ["bandit", "darkroom"])
def test_decode_chain_equals_positionwise_window(env, level):
    """70 dpt_decode_step calls leave the logits of the position-by-position window, bit for bit, and
    both sit within the bar of the oracle"""
    from oracle import dpt_oracle as O
    d = dh()
    T, sd = SM.CHAIN_T, 1 if env == "bandit" else 2
    _assert_window_sharp(env, level, T)
    m = _window_model(env, level)
    q, cs, ca, cn, cr = SM.window_inputs(env, T)
    seq = O.pack_tokens(q, cs, ca, cn, cr, 5, sd).astype(np.float32)
    kv = torch.empty(m.kv_numel(SM.WINDOW_N, T), dtype=torch.float32, device=d.device())
    for p in range(T):
        lg = m.decode_step(kv, T, p, seq[:, p]).cpu().numpy()
    d.set_prefill(False)
    win = m.forward_window(q, cs, ca, cn, cr).cpu().numpy()
    assert np.array_equal(lg, win)
    r64, r32 = SM.window_refs(env, level, T)
    err, err32 = SM.rel_err(lg, r64[:, -1]), SM.rel_err(r32[:, -1], r64[:, -1])
    print(f"SHARP-ERR item=1 decode chain {env} {level} T={T}: kernel {err:.3e}, fp32 oracle {err32:.3e}")
    assert err <= SM.bar(level, LOGIT_BAR, err32), err


# ----------------------------------------------------------------------------- 2. fused bandit rollout
def _run_bandit(m, L, A, N, H, sample):
    u, g = SM.bandit_draws(N, H)
    o = m.rollout_bandit(SM.bandit_means(N, A), H, SM.VAR, sample, uniforms=u, noise=g, want_logits=True)
    return {k: o[k].cpu().numpy() for k in ("actions", "rewards", "arm_value", "logits")}


def _fp32_rollout_error(r32, r64):
    """the fp32 oracle's largest relative logit error on the steps it follows the float64 oracle"""
    H = r64["actions"].shape[1]
    n = compared_steps(np.asarray(r32["actions"]), np.asarray(r64["actions"]), r64["margin"])
    sel = np.arange(H)[:, None] <= np.minimum(n, H - 1)[None, :]
    return SM.rel_err(r32["logits"][sel], r64["logits"][sel])


@pytest.mark.parametrize("L,A,level,head", [(L, A, level, 1.0) for L, A in SM.ROLLOUT_MODELS for level in LEVELS]
                         + [(4, 5, "medium", SM.HEAD_PEAKED)])
@pytest.mark.parametrize("tile,N", SM.ROLLOUT_TILES)
def test_bandit_rollout(tile, N, L, A, level, head):
    """dpt_rollout_bandit against c_oracle.bandit_rollout_f64 on injected draws: H = 9, 70, 130,
    sampled and greedy, the 24-bit and the fp32 y cache; the two cache forms within the bar of each other
    on the steps both followed the oracle.  ``head`` 4: the peaked-head variant, on the project's bar."""
    from test_gpu_ycache_packed import _logit_diff
    d = dh()
    w = SM.rollout_weights(L, A, level, head)
    for sample in (True, False):  # the rollouts over 9 and 70 steps are prefixes of these (SM.bandit_draws)
        r64, _ = SM.rollout_refs(L, A, level, head, N, max(SM.ROLLOUT_HS), sample)
        SM.assert_sharp(level, SM.token_stats(w, L, SM.bandit_window(r64["actions"][:, :-1], r64["rewards"][:, :-1], A)),
                        f"rollout L={L} A={A} N={N} sample={int(sample)} {level} head x{head:g}")
    m = d.DeviceModel(SM.as_torch(w), L, 1, A, 4 * (1 + max(SM.ROLLOUT_HS)))
    d.set_decode_tile(tile)
    worst = {24: 0.0, 32: 0.0, "24v32": 0.0, "fp32": 0.0, "frac": 1.0}
    for H in SM.ROLLOUT_HS:
        for sample in (True, False):
            r64, r32 = SM.rollout_refs(L, A, level, head, N, H, sample)
            err32 = _fp32_rollout_error(r32, r64)
            bar = SM.bar(level, LOGIT_BAR, err32)
            worst["fp32"] = max(worst["fp32"], err32)
            outs, n_cmp = {}, {}
            for bits in (24, 32):
                d.set_ycache_bits(bits)
                print(f"tile {tile} N {N} L {L} A {A} {level} head x{head:g} H {H} sample {int(sample)} "
                      f"bits {bits} (fp32 oracle {err32:.3e}, bar {bar:.1e}):")
                outs[bits] = _run_bandit(m, L, A, N, H, sample)
                err, n_cmp[bits], frac = SM.rollout_compare(outs[bits], r64, r64["margin"], bar)
                worst[bits] = max(worst[bits], err)
                worst["frac"] = min(worst["frac"], frac)
            diff = _logit_diff(outs[24], outs[32], np.minimum(n_cmp[24], n_cmp[32]))
            print(f"  24 vs 32: max rel logit diff {diff:.3e}")
            assert diff <= bar, (diff, bar)
            worst["24v32"] = max(worst["24v32"], diff)
    print(f"SHARP-ERR item=2 rollout tile={tile} N={N} L={L} A={A} {level} head x{head:g}: kernel 24-bit "
          f"{worst[24]:.3e}, 32-bit {worst[32]:.3e}, 24 vs 32 {worst['24v32']:.3e}, fp32 oracle {worst['fp32']:.3e}, "
          f"compared >= {worst['frac']:.4f}")


# ----------------------------------------------------------------------------- 3. fused DarkRoom rollout
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("Heps,horizon,R", SM.DARKROOM_CASES)
def test_darkroom_rollout(Heps, horizon, R, permuted, level):
    """dpt_rollout_darkroom against c_oracle.darkroom_rollout on injected uniforms: windows 61 (a
    partial last 16-token block) and 128 (the 4-wave kernel's largest), with the per-episode workspace
    and without, the logits memo on and off, plain and permuted actions"""
    d = dh()
    r64, r32 = SM.darkroom_refs(level, Heps, horizon, R, permuted)
    goals, perms, u = SM.darkroom_setup(Heps, horizon, permuted)
    w = SM.darkroom_weights(level)
    label = f"darkroom {Heps}x{horizon} R={R} permuted={int(permuted)} {level}"
    SM.assert_sharp(level, SM.token_stats(w, 4, SM.darkroom_last_window(goals, perms, r64["actions"], horizon, R)), label)
    steps = Heps * horizon
    n32 = compared_steps(r32["actions"], r64["actions"], r64["margin"])
    sel = np.arange(steps)[:, None] <= np.minimum(n32, steps - 1)[None, :]
    err32 = SM.rel_err(r32["logits"][sel], r64["logits"][sel])
    bar = SM.bar(level, LOGIT_BAR, err32)
    m = d.DeviceModel(SM.as_torch(w), 4, 2, 5, 512)
    worst, fracs = 0.0, []
    for ws in (True, False):
        for memo in (True, False):
            d.set_darkroom_workspace(ws)
            d.set_darkroom_memo(memo)
            o = m.rollout_darkroom(goals, Heps, horizon, R, perms=perms, uniforms=u, want_actions=True,
                                   want_logits=True)
            out = {k: o[k].cpu().numpy() for k in ("actions", "logits", "returns")}
            err, frac = SM.darkroom_compare(out, r64, horizon, bar, f"{label} workspace={int(ws)} memo={int(memo)}")
            worst = max(worst, err)
            fracs.append(frac)
    print(f"SHARP-ERR item=3 {label}: kernel {worst:.3e}, fp32 oracle {err32:.3e}, compared >= {min(fracs):.4f}")


# ----------------------------------------------------------------------------- 4. generic-width rollout
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("E", SM.GENERIC_ES)
def test_generic_rollout(E, level):
    """dpt_rollout_bandit_generic at widths 16, 18 and 64 over 130 steps (the decode attention past
    one 64-key lap, with a running maximum that moves) against the oracle's re-forward-every-step rollout"""
    from dpt_hip import train as tr
    dh()
    r64, r32 = SM.generic_refs(E, level)
    m, w = SM.generic_module(E, level)
    N, H, A, L = (SM.GENERIC[k] for k in ("N", "H", "A", "L"))
    SM.assert_sharp(level, SM.token_stats(w, L, SM.bandit_window(r64["actions"][:, :-1], r64["rewards"][:, :-1], A)),
                    f"generic E={E} {level}")
    err32 = _fp32_rollout_error(r32, r64)
    bar = SM.bar(level, LOGIT_BAR, err32)
    u, g = SM.bandit_draws(N, H)
    o = tr.rollout_bandit_generic(m.cuda().eval(), SM.bandit_means(N, A), H, SM.VAR, True, 0, uniforms=u, noise=g,
                                  want_logits=True)
    out = {k: o[k].cpu().numpy() for k in ("actions", "rewards", "arm_value", "logits")}
    print(f"generic E={E} {level} (fp32 oracle {err32:.3e}, bar {bar:.1e}):")
    err, _, frac = SM.rollout_compare(out, r64, r64["margin"], bar)
    print(f"SHARP-ERR item=4 generic E={E} {level}: kernel {err:.3e}, fp32 oracle {err32:.3e}, compared {frac:.4f}")


# ----------------------------------------------------------------------------- 5. training forward / backward
def _train_case(kind, E, T, level, perturb=None):
    from test_gpu_train_grads import _token_level
    E, L, sd, B, T, last = SM.train_shape(kind, E, T)
    label = f"{kind} E={E} T={T} {level}"
    return label, _token_level(label, E, L, sd, B, T, last, transform=SM.train_transform(kind, E, T, level),
                               level=level, perturb=perturb)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("E,T", SM.TRAIN_MFMA)
def test_training_matrix_core_widths(E, T, level):
    """tr_attn_fwd_mfma / tr_attn_bwd_dq_mfma / tr_attn_bwd_dkv_mfma at one tile and one past it, one
    workgroup and one past it, and 129; every parameter held separately, a second run bit-identical"""
    label, f = _train_case("mfma", E, T, level)
    print(f"SHARP-ERR item=5 train {label}: grads kernel {f['grad']:.3e}, fp32 oracle {f['grad32']:.3e} of max|g|; "
          f"preds kernel {f['preds']:.3e}")


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("E,T", SM.TRAIN_ROWS)
def test_training_row_kernels(E, T, level):
    """tr_attn_fwd / tr_attn_bwd_ds,dq,dkv at widths mm_fast does not take, past one lap over the keys"""
    label, f = _train_case("rows", E, T, level)
    print(f"SHARP-ERR item=5 train {label}: grads kernel {f['grad']:.3e}, fp32 oracle {f['grad32']:.3e} of max|g|; "
          f"preds kernel {f['preds']:.3e}")


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("E,T", SM.TRAIN_LAST)
def test_training_last_position_path(E, T, level):
    """DPT_TRAIN_LAST_LOSS (tr_attn_last / tr_attn_last_bwd) into its second and third lap"""
    label, f = _train_case("last", E, T, level)
    print(f"SHARP-ERR item=5 train {label}: grads kernel {f['grad']:.3e}, fp32 oracle {f['grad32']:.3e} of max|g|; "
          f"preds kernel {f['preds']:.3e}")


# ----------------------------------------------------------------------------- 6. fused steps (medium)
@pytest.mark.parametrize("chunk", [0, 3])
@pytest.mark.parametrize("E", [32, 18])
def test_interactive_step_gradient(E, chunk):
    """the gradient inside dpt_interactive_grad (InteractiveTrainer.dblob after one step, K = 6) by the
    rule of test_gpu_train_grads.test_interactive_step_gradient, on a medium model"""
    from dpt_hip import train as tr
    from oracle import dpt_oracle_torch as OT
    from test_gpu_interactive import _tokens64
    from test_gpu_train_grads import _assert_grads, _names, _worst
    K, L, A = SM.FUSED["K"], SM.FUSED["L"], SM.FUSED["A"]
    m, w64 = SM.fused_module(E, "interactive")
    means, u, gn, _ = SM.fused_case(E, "interactive", chunk)
    m = m.cuda()
    trainer = tr.InteractiveTrainer(m, lr=1e-3, weight_decay=1e-4, chunk=chunk)
    actions, rewards = trainer.step(means, K, SM.VAR, "uniform", uniforms=u, noise=gn)
    loss = trainer.read_loss()
    acts, rews = actions.cpu().numpy(), rewards.cpu().numpy()
    label = f"interactive K={K} E={E} chunk={chunk} medium"
    SM.assert_sharp("medium", SM.token_stats(w64, L, SM.bandit_window(acts, rews, A)), label)
    got = {k: v.cpu().numpy() for k, v in zip(_names(m), tr.unpack_grads(trainer.dblob, tr.param_list(m)))}
    P = OT.state_dict_params(w64, L)
    preds = OT.forward(P, _tokens64(acts, rews, A), L)[:, -1]
    ref_loss = torch.nn.functional.cross_entropy(preds, torch.from_numpy(means.argmax(1)))
    ref_loss.backward()
    ref = {k: v.grad.numpy() for k, v in P.items()}
    g32 = SM.fused_grads("interactive", w64, acts, rews, means.argmax(1), torch.float32)
    print(f"SHARP-ERR item=6 {label}: grads kernel {_worst(got, ref)[0]:.3e}, fp32 oracle {_worst(g32, ref)[0]:.3e} "
          f"of max|g|; loss {loss!r} ref {ref_loss.item()!r}")
    assert abs(loss - ref_loss.item()) <= 1e-5 * abs(ref_loss.item()), (loss, ref_loss.item())
    _assert_grads(label, got, ref)


@pytest.mark.parametrize("chunk", [0, 3])
@pytest.mark.parametrize("E", [32, 18])
def test_explore_step_gradients(E, chunk):
    """the gradients inside dpt_explore_grad (both models' dblob after one ExploreExploitTrainer.step,
    K = 6, beta 0.5) by the rule of test_gpu_explore.test_explore_step_gradients, on medium models"""
    import test_gpu_explore as X
    from dpt_hip import train as tr
    from oracle import dpt_oracle_torch as OT
    K, L, A, beta = SM.FUSED["K"], SM.FUSED["L"], SM.FUSED["A"], 0.5
    assert (X.N, X.A, X.L, X.VAR) == (SM.FUSED["N"], A, L, SM.VAR)
    explorer, w_explorer = SM.fused_module(E, "explorer")
    exploiter, w_exploiter = SM.fused_module(E, "exploiter", 1)
    explorer, exploiter = explorer.cuda(), exploiter.cuda()
    means, u, g, ea = SM.fused_case(E, "explorer", chunk)
    trainer = tr.ExploreExploitTrainer(explorer, exploiter, lr=X.LR, weight_decay=1e-4, chunk=chunk)
    actions, env_acts, rewards = trainer.step(means, K, SM.VAR, "uniform", beta, uniforms=u, noise=g, env_actions=ea)
    loss_explorer, loss_exploiter = trainer.read_losses()
    acts, rews = actions.cpu().numpy(), rewards.cpu().numpy()
    X._check_records(acts, env_acts.cpu().numpy(), rews, means, g, ea)
    label = f"explore K={K} E={E} chunk={chunk} medium"
    for name, w in (("explorer", w_explorer), ("exploiter", w_exploiter)):
        SM.assert_sharp("medium", SM.token_stats(w, L, SM.bandit_window(acts, rews, A)), f"{name} of {label}")
    got_explorer, got_exploiter = X._grads_of(trainer, explorer)
    P_explorer, P_exploiter = OT.state_dict_params(w_explorer, L), OT.state_dict_params(w_exploiter, L)
    ref_explorer, ref_exploiter = X._reference(P_explorer, P_exploiter, P_exploiter, acts, rews, means.argmax(1), beta)
    ref_explorer.backward()
    ref_exploiter.backward()
    refs = [{k: v.grad.numpy() for k, v in P.items()} for P in (P_explorer, P_exploiter)]
    g32 = SM.fused_grads("explore", w_explorer, acts, rews, means.argmax(1), torch.float32, w_exploiter, beta)
    worst = [X._worst(got, ref)[0] for got, ref in zip((got_explorer, got_exploiter), refs)]
    worst32 = [X._worst(g, ref)[0] for g, ref in zip(g32, refs)]
    print(f"SHARP-ERR item=6 {label}: grads kernel explorer {worst[0]:.3e}, exploiter {worst[1]:.3e}; fp32 oracle "
          f"explorer {worst32[0]:.3e}, exploiter {worst32[1]:.3e} of max|g|")
    assert abs(loss_explorer - ref_explorer.item()) <= 1e-5 * abs(ref_explorer.item())
    assert abs(loss_exploiter - ref_exploiter.item()) <= 1e-5 * abs(ref_exploiter.item())
    X._hold(label + " exploiter", got_exploiter, P_exploiter)
    X._hold(label + " explorer", got_explorer, P_explorer)


# ----------------------------------------------------------------------------- 7. image act step
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("E", [32, 18])
def test_image_act_step(E, level):
    """logits of dpt_image_act_step with a transformed trunk (the front end keeps its weights) against
    image_oracle in float64 and against the plain module forward, B = 5, C = 7"""
    import dpt_hip
    import image_oracle as IO
    import test_gpu_image_act as IA
    dh()
    m, w64, ctx, frames, angle = SM.image_case(E, level)
    obs = IA.oracle_obs(frames)
    SM.assert_sharp(level, SM.image_stats(w64, IA.LAYERS, obs, angle, ctx, IA.A), f"image E={E} {level}")
    ref = IA.oracle_logits(w64, obs, angle, ctx)
    images, feats = IO.pack(dict(ctx, query_images=obs, query_states=angle), IA.A, torch.float32)
    with torch.no_grad():
        p32, _ = IO.forward({k: torch.tensor(v, dtype=torch.float32) for k, v in w64.items()}, images, feats, IA.LAYERS)
    err32 = SM.rel_err(p32[:, -1].numpy(), ref)
    bar = SM.bar(level, LOGIT_BAR, err32)
    m = m.cuda()
    s = dpt_hip.ImageActSession(m, SM.IMAGE["B"], (60, 80))
    s.set_context(IA.gpu(ctx))
    s.act(frames, angle, sample=False)
    got = s.logits.cpu().numpy()
    with torch.no_grad():
        plain = m(dict(IA.gpu(ctx), query_images=s.obs, query_states=torch.as_tensor(angle, device="cuda"))).cpu().numpy()
    err, err_plain = IA.fwd_violation(got, ref), IA.fwd_violation(got, plain)
    print(f"SHARP-ERR item=7 image act E={E} {level}: kernel {err:.3e}, fp32 oracle {err32:.3e}; vs model(batch) "
          f"{err_plain:.3e}, model(batch) vs oracle {IA.fwd_violation(plain, ref):.3e}")
    assert err <= bar, (err, bar)
    assert err_plain <= bar, (err_plain, bar)


# ----------------------------------------------------------------------------- 8. the bars can fail
@pytest.mark.parametrize("env", ["bandit", "darkroom"])
def test_the_window_bar_can_fail(env):
    """block 2's c_attn.weight off by a relative 1e-3 on the device: the comparison of
    test_window_forward reports a violation at sharp, both window paths"""
    _assert_window_sharp(env, "sharp", 101)
    m = _window_model(env, "sharp", _scaled_c_attn(SM.window_weights(env, "sharp"), 2))
    for prefill in (True, False):
        err, err32 = _window_errors(m, env, "sharp", 101, prefill, 0)
        print(f"window control {env} prefill={int(prefill)}: {err:.3e} against a bar of "
              f"{SM.bar('sharp', LOGIT_BAR, err32):.1e}")
        assert err > SM.bar("sharp", LOGIT_BAR, err32)


@pytest.mark.parametrize("kind,E,T", [("mfma", 32, 65), ("rows", 18, 65), ("last", 32, 130)])
def test_the_gradient_bar_can_fail(kind, E, T):
    """block 1's c_attn.weight off by a relative 1e-3 in the module the kernels run: the comparison
    of _token_level reports a violation of a gradient's bar at sharp"""
    def perturb(m):
        with torch.no_grad():
            m.transformer.h[1].attn.c_attn.weight.mul_(1 + 1e-3)

    # _assert_grads' message is (label, parameter name, error / max|g|); assert_sharp's carries the label
    # too, but a level and a block number after it, which this pattern does not match
    with pytest.raises(AssertionError, match=re.escape(f"'{kind} E={E} T={T} sharp', '") + r"[a-z_]+\.[a-z0-9_.]+', "):
        _train_case(kind, E, T, "sharp", perturb)
