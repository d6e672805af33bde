"""The sharp-attention model family (tests/sharp_models.py) on the host: what the GPU file
tests/test_gpu_sharp_attention.py relies on, checked with the oracles alone.

* every (shape, level) that file runs meets the level's sharpness thresholds on the float64 oracle:
  the windows at every T > 1 (one token has no span); a rollout on the last window of its 130-step
  trajectory, sampled and greedy (the 9- and 70-step rollouts are prefixes of it, asserted here);
* at ``medium`` and with the peaked head the fp32 oracle alone meets the project's bars (the head at
  half the bar or less), so those bars leave room for another summation order; the fused steps too;
* the fp32 oracle's rollouts follow the float64 oracle's on >= 0.9 of the task-steps, so the GPU
  file's compared fraction is reachable;
* the scale derivation of dpt_model_create (csrc/dpt_abi.hip fwd_scales, restated here from the
  weights in numpy) refuses neither level and brings no exponent to its lower clamp.

The fp32 oracle's errors are printed (pytest -s) next to each assertion."""
import numpy as np
import pytest
import torch

import sharp_models as SM
from test_gpu_train import GRAD_TOL

LOGIT_BAR = 1e-5
GRAD_BAR = 5 * GRAD_TOL
HEADS = (("medium", 1.0), ("sharp", 1.0), ("medium", SM.HEAD_PEAKED))


# ----------------------------------------------------------------------------- the transform itself
def test_transform_is_deterministic_and_touches_what_it_names():
    import bench
    base, _ = bench.synthetic_state_dict(2, 1, 5, 10)
    a, b = SM.transform(base, 32, "sharp"), SM.transform(base, 32, "sharp")
    assert list(a) == list(base) and all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 for k in a)
    p = "transformer.h.1."
    w0 = base[p + "attn.c_attn.weight"].numpy()
    assert np.array_equal(a[p + "attn.c_attn.weight"][:, :64], (w0[:, :64].astype(np.float64) * 8).astype(np.float32))
    assert np.array_equal(a[p + "attn.c_attn.weight"][:, 64:], w0[:, 64:])
    assert np.array_equal(a[p + "mlp.c_fc.weight"], base[p + "mlp.c_fc.weight"].numpy() * np.float32(3))
    ratio = a[p + "ln_2.weight"] / base[p + "ln_2.weight"].numpy()
    assert 0.5 <= ratio.min() and ratio.max() <= 3.0 and np.ptp(ratio) > 1.0
    for k in ("embed_transition.weight", "transformer.wpe.weight", "transformer.ln_f.weight", "pred_actions.weight",
              p + "attn.c_proj.weight", p + "mlp.c_fc.bias"):
        assert np.array_equal(a[k], base[k].numpy()), k
    h = SM.transform(base, 32, "medium", head=SM.HEAD_PEAKED)
    assert np.array_equal(h["pred_actions.weight"], base["pred_actions.weight"].numpy() * np.float32(4))
    # today's models, for the record: the softmax is a plain mean
    stats = SM.token_stats({k: v.numpy() for k, v in base.items()}, 2, SM.bandit_window(
        np.random.RandomState(0).randint(0, 5, (4, 9)), np.random.RandomState(1).randn(4, 9), 5))
    assert all(span < 1.0 and top < 0.2 for span, top in stats), stats


# ----------------------------------------------------------------------------- item 1: windows
@pytest.mark.parametrize("level", SM.LEVEL_NAMES)
@pytest.mark.parametrize("env", ["bandit", "darkroom"])
def test_window_models(env, level):
    w = SM.window_weights(env, level)
    for T in SM.WINDOW_TS + (SM.CHAIN_T,):
        if T > 1:  # a one-token window has one score: no span to hold
            SM.assert_sharp(level, SM.token_stats(w, 4, SM.window_seq(env, T)), f"window {env} T={T} {level}")
        r64, r32 = SM.window_refs(env, level, T)
        err = SM.rel_err(r32, r64)
        print(f"sharp-host window {env} {level} T={T}: fp32 oracle {err:.3e}")
        if level == "medium":
            assert err <= LOGIT_BAR, err


# ----------------------------------------------------------------------------- items 2-4: rollouts
def _bandit_fp32_vs_f64(r64, r32, level, head, label):
    from test_gpu_kernels import compared_steps
    H = r64["actions"].shape[1]
    n_cmp = compared_steps(r32["actions"], r64["actions"], r64["margin"])
    step = np.arange(H)[:, None]
    sel = step <= np.minimum(n_cmp, H - 1)[None, :]
    err = SM.rel_err(r32["logits"][sel], r64["logits"][sel])
    frac = float((step < n_cmp[None, :]).mean())
    print(f"sharp-host {label} {level} head x{head:g}: fp32 oracle {err:.3e}, compared {frac:.4f}")
    assert frac >= 0.9, frac
    if head != 1.0:
        assert err <= 0.5 * LOGIT_BAR, err  # the issue's condition for keeping the project's bar at the head
    elif level == "medium":
        assert err <= LOGIT_BAR, err
    return err


@pytest.mark.parametrize("L,A,level,head", [(L, A, level, 1.0) for L, A in SM.ROLLOUT_MODELS for level in SM.LEVEL_NAMES]
                         + [(4, 5, "medium", SM.HEAD_PEAKED)])
def test_bandit_rollout_models(L, A, level, head):
    w = SM.rollout_weights(L, A, level, head)
    for tile, N in SM.ROLLOUT_TILES:
        for H in SM.ROLLOUT_HS:
            for sample in (True, False):
                r64, r32 = SM.rollout_refs(L, A, level, head, N, H, sample)
                if H == max(SM.ROLLOUT_HS):
                    SM.assert_sharp(level, SM.token_stats(w, L, SM.bandit_window(
                        r64["actions"][:, :-1], r64["rewards"][:, :-1], A)),
                        f"rollout L={L} A={A} N={N} sample={int(sample)} {level} head x{head:g}")
                else:  # the shorter rollouts are prefixes of that one (SM.bandit_draws): no window of their own
                    full = SM.rollout_refs(L, A, level, head, N, max(SM.ROLLOUT_HS), sample)[0]
                    assert np.array_equal(r64["actions"], full["actions"][:, :H])
                    assert np.array_equal(r64["logits"], full["logits"][:H])
                _bandit_fp32_vs_f64(r64, r32, level, head, f"rollout L={L} A={A} N={N} H={H} sample={int(sample)}")


@pytest.mark.parametrize("level", SM.LEVEL_NAMES)
@pytest.mark.parametrize("E", SM.GENERIC_ES)
def test_generic_rollout_models(E, level):
    r64, r32 = SM.generic_refs(E, level)
    _, w = SM.generic_module(E, level)
    SM.assert_sharp(level, SM.token_stats(w, SM.GENERIC["L"], SM.bandit_window(
        r64["actions"][:, :-1], r64["rewards"][:, :-1], 5)), f"generic E={E} {level}")
    _bandit_fp32_vs_f64(r64, r32, level, 1.0, f"generic E={E}")


@pytest.mark.parametrize("level", SM.LEVEL_NAMES)
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("Heps,horizon,R", SM.DARKROOM_CASES)
def test_darkroom_rollout_models(Heps, horizon, R, permuted, level):
    from test_gpu_kernels import compared_steps
    r64, r32 = SM.darkroom_refs(level, Heps, horizon, R, permuted)
    goals, perms, _ = SM.darkroom_setup(Heps, horizon, permuted)
    SM.assert_sharp(level, SM.token_stats(SM.darkroom_weights(level), 4, SM.darkroom_last_window(
        goals, perms, r64["actions"], horizon, R)), f"darkroom {Heps}x{horizon} R={R} permuted={int(permuted)} {level}")
    steps = Heps * horizon
    n = compared_steps(r32["actions"], r64["actions"], r64["margin"])
    sel = np.arange(steps)[:, None] <= np.minimum(n, steps - 1)[None, :]
    err = SM.rel_err(r32["logits"][sel], r64["logits"][sel])
    frac = float(n.sum()) / n.size / steps
    print(f"sharp-host darkroom {Heps}x{horizon} R={R} permuted={int(permuted)} {level}: fp32 oracle {err:.3e}, "
          f"compared {frac:.4f}")
    assert frac >= 0.9, frac
    if level == "medium":
        assert err <= LOGIT_BAR, err


# ----------------------------------------------------------------------------- item 5: training
TRAIN = ([("mfma", E, T) for E, T in SM.TRAIN_MFMA] + [("rows", E, T) for E, T in SM.TRAIN_ROWS]
         + [("last", E, T) for E, T in SM.TRAIN_LAST])


@pytest.mark.parametrize("level", SM.LEVEL_NAMES)
@pytest.mark.parametrize("kind,E,T", TRAIN)
def test_training_models(kind, E, T, level):
    from test_gpu_train_grads import _oracle, _token_inputs, _worst
    E, L, sd, B, T, last = SM.train_shape(kind, E, T)
    _, w64, tok, dp = _token_inputs(E, L, sd, B, T, last, SM.train_transform(kind, E, T, level))
    SM.assert_sharp(level, SM.token_stats(w64, L, tok.numpy()), f"train {kind} E={E} T={T} {level}")
    p64, g64 = _oracle(w64, L, tok, dp, torch.float64)
    p32, g32 = _oracle(w64, L, tok, dp, torch.float32)
    rows = slice(T - 1, T) if last else slice(None)
    worst, at = _worst(g32, g64)
    perr = SM.rel_err(p32[:, rows], p64[:, rows])
    print(f"sharp-host train {kind} E={E} T={T} {level}: fp32 oracle grads {worst:.3e} of max|g| ({at}), preds {perr:.3e}")
    if level == "medium":
        assert worst <= GRAD_BAR and perr <= LOGIT_BAR, (worst, perr)


# ----------------------------------------------------------------------------- item 6: fused steps
@pytest.mark.parametrize("chunk", [0, 3])
@pytest.mark.parametrize("E", [32, 18])
@pytest.mark.parametrize("which", ["interactive", "explorer", "exploiter"])
def test_fused_step_models(which, E, chunk):
    """the fused steps' models on the oracle's own replay of the step's records (the GPU file asserts
    the same on the device's records), and the fp32 oracle's gradient on them inside the project's bar"""
    from test_gpu_train_grads import _worst
    means, u, g, ea = SM.fused_case(E, which, chunk)
    _, w64 = SM.fused_module(E, which, 1 if which == "exploiter" else 0)
    w_explorer = SM.fused_module(E, "explorer")[1]
    acts, rews = SM.fused_records(w_explorer if which == "exploiter" else w64, means, u, g, ea)
    SM.assert_sharp("medium", SM.token_stats(w64, SM.FUSED["L"], SM.bandit_window(acts, rews, SM.FUSED["A"])),
                    f"fused {which} E={E} chunk={chunk} medium")
    target = means.argmax(1)
    if which == "interactive":
        g64, g32 = (SM.fused_grads(which, w64, acts, rews, target, dt) for dt in (torch.float64, torch.float32))
    else:
        w_exploiter = SM.fused_module(E, "exploiter", 1)[1]
        pick = 0 if which == "explorer" else 1
        g64, g32 = (SM.fused_grads("explore", w_explorer, acts, rews, target, dt, w_exploiter)[pick]
                    for dt in (torch.float64, torch.float32))
    worst, at = _worst(g32, g64)
    print(f"sharp-host fused {which} E={E} chunk={chunk} medium: fp32 oracle grads {worst:.3e} of max|g| ({at})")
    assert worst <= GRAD_BAR, (worst, at)


def test_fused_losses_restate_the_explore_reference():
    """SM.fused_losses in float64 is tests/test_gpu_explore._reference (which the GPU test holds the
    kernels to), so its float32 run is the fp32 oracle of the same loss"""
    import test_gpu_explore as X
    from oracle import dpt_oracle_torch as OT
    E = 18
    means, u, g, ea = SM.fused_case(E, "explorer", 0)
    w_explorer, w_exploiter = SM.fused_module(E, "explorer")[1], SM.fused_module(E, "exploiter", 1)[1]
    acts, rews = SM.fused_records(w_explorer, means, u, g, ea)
    P, Px = OT.state_dict_params(w_explorer, 2), OT.state_dict_params(w_exploiter, 2)
    mine = SM.fused_losses("explore", P, acts, rews, means.argmax(1), Px, 0.5)
    theirs = X._reference(P, Px, Px, acts, rews, means.argmax(1), 0.5)
    assert mine[0].item() == theirs[0].item() and mine[1].item() == theirs[1].item()


# ----------------------------------------------------------------------------- item 7: image act step
@pytest.mark.parametrize("level", SM.LEVEL_NAMES)
@pytest.mark.parametrize("E", [32, 18])
def test_image_models(E, level):
    import image_oracle as IO
    import test_gpu_image_act as IA
    m, w64, ctx, frames, angle = SM.image_case(E, level)
    obs = IA.oracle_obs(frames)
    SM.assert_sharp(level, SM.image_stats(w64, IA.LAYERS, obs, angle, ctx, IA.A), f"image E={E} {level}")
    ref = IA.oracle_logits(w64, obs, angle, ctx)
    images, feats = IO.pack(dict(ctx, query_images=obs, query_states=angle), IA.A, torch.float32)
    with torch.no_grad():
        p32, _ = IO.forward({k: torch.tensor(v, dtype=torch.float32) for k, v in w64.items()}, images, feats, IA.LAYERS)
    err = SM.rel_err(p32[:, -1].numpy(), ref)
    print(f"sharp-host image E={E} {level}: fp32 oracle {err:.3e}")
    if level == "medium":
        assert err <= LOGIT_BAR, err
    # the front end keeps its weights: the transform touched the trunk only
    for k, v in IA.weights64(IA.make_model(E, seed=2)).items():
        if not k.startswith("transformer.h."):
            assert np.array_equal(w64[k], v), k


# ----------------------------------------------------------------------------- the scale derivation
def fwd_scales_host(w, n_layer, E=32):
    """csrc/dpt_abi.hip fwd_scales from a state_dict: the five power-of-two exponents of the fp16
    two-part products, before clamping, and whether dpt_model_create refuses the model.  A restatement
    by hand (with derive_l0_kernel's folding of G, g0 and Wvp): the library does not report its
    exponents, so nothing ties the two together, and a change of the bounds in the C++ has to be
    made here too.  The GPU file creates every one of these models through dpt_model_create, which is
    where a refusal by the real derivation would show."""
    w = SM.as_f64(w)
    wmax, amax, gw, ymax, qmax = 0.0, 1.0, 0.0, 1.0, 1.0
    for i in range(n_layer):
        p = f"transformer.h.{i}."
        aw, ab = w[p + "attn.c_attn.weight"], w[p + "attn.c_attn.bias"]
        wq, wk, wv = aw[:, :E], aw[:, E:2 * E], aw[:, 2 * E:]
        G = (wq @ wk.T).astype(np.float32).astype(np.float64)  # G[m][n] = sum_j Wq[m][j] Wk[n][j]
        g0 = (wk @ ab[:E]).astype(np.float32).astype(np.float64)
        wvp = (wv @ w[p + "attn.c_proj.weight"]).astype(np.float32).astype(np.float64)
        by = np.sqrt(E - 1.0) * np.abs(w[p + "ln_1.weight"]).max() + np.abs(w[p + "ln_1.bias"]).max()
        ymax = max(ymax, by)
        qmax = max(qmax, (np.abs(g0) + np.abs(G).sum(0) * by).max())
        gw = max(gw, np.abs(G).max(), np.abs(wvp).max())
        bx = np.sqrt(E - 1.0) * np.abs(w[p + "ln_2.weight"]).max() + np.abs(w[p + "ln_2.bias"]).max()
        bh = max(0.17, (np.abs(w[p + "mlp.c_fc.bias"]) + np.abs(w[p + "mlp.c_fc.weight"]).sum(0) * bx).max())
        wmax = max(wmax, np.abs(w[p + "mlp.c_fc.weight"]).max(), np.abs(w[p + "mlp.c_proj.weight"]).max())
        amax = max(amax, bx, bh)
    assert all(np.isfinite(v) for v in (wmax, amax, gw, ymax, qmax))
    raw = {k: int(np.floor(np.log2(16384.0 / b))) for k, b in
           (("mlp_ew", wmax), ("mlp_ex", amax), ("attn_ew", gw), ("attn_ey", ymax), ("attn_eq", qmax))}
    hi = dict(mlp_ew=12, mlp_ex=8, attn_ew=12, attn_ey=8, attn_eq=8)
    e = {k: min(max(v, -24), hi[k]) for k, v in raw.items()}
    return raw, e, e["mlp_ew"] + e["mlp_ex"] < -40


@pytest.mark.parametrize("level,head", HEADS)
def test_scale_derivation_refuses_neither_level(level, head):
    """Every width-32 model the GPU file hands to dpt_model_create: no exponent reaches its lower
    clamp (-24, where a bound would no longer fit fp16's range) and the MLP refusal does not trigger,
    so both levels run the fp16 split products on scales that cover their bounds."""
    models = [(f"window {env}", SM.window_weights(env, level), 4) for env in ("bandit", "darkroom")] \
        if head == 1.0 else []
    models += [(f"rollout L={L} A={A}", SM.rollout_weights(L, A, level, head), L) for L, A in SM.ROLLOUT_MODELS
               if head == 1.0 or (L, A) == (4, 5)]
    if head == 1.0:
        models.append(("darkroom", SM.darkroom_weights(level), 4))
    for label, w, L in models:
        raw, e, refused = fwd_scales_host(w, L)
        print(f"sharp-host scales {label} {level} head x{head:g}: {e}")
        assert not refused, (label, e)
        assert all(v > -24 for v in raw.values()), (label, raw)
