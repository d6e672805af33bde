"""The deployment of the image-conditioned DPT on the GPU (csrc/dpt_imageact.hip, dpt_hip.ImageActSession,
ctrls.ctrl_miniworld, envs.miniworld_env, evals.eval_miniworld).

Oracle: the scipy.ndimage restatement of skimage's anti-aliased resize (miniworld_stub.preprocess_oracle,
float64), rounded to fp32 as the reference's ``.float()`` does, fed to tests/image_oracle.forward (float64).

Bars: a preprocessed element within 2^-22 (absolute) of the oracle: normalised values lie in [-2.12, 2.64],
so one fp32 step is at most 2^-22, and an fp64 accumulation differs from the oracle by a rounding flip at
most; logits within 1e-5 max(1, |x|), the bar tests/test_gpu_image.py holds forward values to.  Shapes:
2 layers, A = 4, sd = 2, widths 32 (float4 LayerNorm rows) and 18 (the scalar LayerNorm), B in {1, 5}
(5 is no multiple of any tile), C in {0, 1, 7} (C = 0 is window 1)."""
import numpy as np
import pytest
import torch

import image_oracle as IO
import miniworld_stub as S

pytestmark = pytest.mark.gpu

SD, A, LAYERS = 2, 4, 2
PRE_BAR = 2.0 ** -22
SIZES = [(60, 80), (25, 25), (31, 47), (80, 60), (128, 25)]
# chosen on the CPU: along the trajectory the float64 oracle's top-two logit gap stays above 0.14 and the
# greedy actions vary between steps and envs (seed 0 plays one action throughout)
E2E_SEED = 3


def fwd_violation(got, ref):
    return float((np.abs(got - ref) / np.maximum(1, np.abs(ref))).max())


def make_model(E, horizon=3, seed=0, dropout=0.0):
    """an ImageTransformer (on the CPU) with every parameter moved off GPT-2's tiny initial values, so
    that the logits differ between actions by far more than fp32 rounding"""
    from models.net import ImageTransformer
    torch.manual_seed(seed)
    m = ImageTransformer(dict(horizon=horizon, state_dim=SD, action_dim=A, n_layer=LAYERS, n_embd=E, n_head=1,
                              dropout=dropout, test=True, image_size=25))
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.startswith("image_encoder") or "wte" in k:
                continue
            r = torch.randn(p.shape, generator=g)
            if k.endswith(".bias"):
                p.copy_(0.1 * r)
            elif ".ln_" in k or k.startswith("embed_ln"):
                p.copy_(1 + 0.1 * r)
            elif k.startswith("pred_actions"):
                p.copy_(0.5 * r)
            else:
                p.copy_(0.15 * r)
    return m.eval()


def weights64(m):
    return {k: v.detach().cpu().double().numpy() for k, v in m.state_dict().items() if "wte" not in k}


def make_context(B, C, seed):
    """a reference-shaped context batch (fp32 numpy): normalised images, direction vectors, one-hot actions"""
    rs = np.random.RandomState(seed)
    raw = rs.uniform(0, 1, (B, C, 25, 25, 3))
    acts = np.eye(A)[rs.randint(0, A, (B, C))]
    return {"context_images": ((raw - S.MEAN) / S.STD).transpose(0, 1, 4, 2, 3).astype(np.float32),
            "context_states": rs.normal(size=(B, C, SD)).astype(np.float32),
            "context_actions": acts.astype(np.float32),
            "context_rewards": rs.uniform(0, 1, (B, C, 1)).astype(np.float32)}


def make_frames(B, hw, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (B, *hw, 3)).astype(np.uint8), rs.normal(size=(B, SD)).astype(np.float32)


def oracle_logits(w64, obs, angle, ctx):
    """float64 logits (B, A) of the last position from fp32-representable inputs"""
    batch = dict(ctx, query_images=obs, query_states=angle)
    if ctx["context_images"].shape[1] == 0:  # window 1: the query token alone
        B = len(angle)
        images = torch.as_tensor(obs, dtype=torch.float64)[:, None]
        feats = torch.cat([torch.as_tensor(angle, dtype=torch.float64), torch.zeros((B, A + 1), dtype=torch.float64)],
                          dim=1)[:, None]
    else:
        images, feats = IO.pack(batch, A)
    with torch.no_grad():
        preds, _ = IO.forward({k: torch.tensor(v) for k, v in w64.items()}, images, feats, LAYERS)
    return preds[:, -1].numpy()


def oracle_obs(frames):
    """the oracle's preprocessing rounded to fp32 (the reference's ``.float()``)"""
    return S.preprocess_oracle(frames).astype(np.float32)


def gpu(batch):
    return {k: torch.as_tensor(v, dtype=torch.float32, device="cuda") for k, v in batch.items()}


def tables_from_dense(Ry, Rx):
    """a dpt_obs_tables struct from two dense 25 x n tables (for the control)"""
    from dpt_hip import _lib
    t = _lib.ObsTables()
    t.in_h, t.in_w = Ry.shape[1], Rx.shape[1]
    for R, first, count, w in ((Ry, t.first_y, t.count_y, t.wy), (Rx, t.first_x, t.count_x, t.wx)):
        for o in range(25):
            nz = np.nonzero(R[o])[0]
            first[o], count[o] = int(nz[0]), int(nz[-1] - nz[0] + 1)
            assert count[o] <= _lib.OBS_BAND
            for k in range(count[o]):
                w[o][k] = float(R[o, nz[0] + k])
    return t


# ----------------------------------------------------------------------------- 1. preprocessing
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("hw", SIZES)
def test_preprocess_vs_oracle(hw, n):
    from dpt_hip import act
    from dpt_hip import train as tr
    frames, _ = make_frames(n, hw, 7 * hw[0] + hw[1] + n)
    ref = S.preprocess_oracle(frames)
    got = act.obs_preprocess(frames).cpu().numpy()
    assert got.shape == (n, 3, 25, 25) and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref).max()
    unequal = int((got != ref.astype(np.float32)).sum())
    print(f"obs_preprocess {hw} n={n}: max err {err:.3e}, {unequal} of {got.size} elements differ from fp32(oracle)")
    assert err <= PRE_BAR, f"max err {err:.3e}; {unequal} of {got.size} elements unequal to fp32(oracle)"
    assert ref.min() >= -2.12 and ref.max() <= 2.65
    if hw == (25, 25):  # the identity tables: the bits of dpt_image_normalize on x / 255
        same = tr.normalize_images(frames.astype(np.float64) / 255).cpu().numpy()
        assert np.array_equal(got, same)
    # the control: tables without the half-pixel offset, through the same kernel, exceed the bound
    if hw != (25, 25):
        bad = act.upload_tables(tables_from_dense(S.tables_no_half_pixel(hw[0]), S.tables_no_half_pixel(hw[1])))
        off = act.obs_preprocess(frames, tables=bad).cpu().numpy()
        assert np.abs(off.astype(np.float64) - ref).max() > PRE_BAR


# ----------------------------------------------------------------------------- 2. the paths agree bit for bit
@pytest.mark.parametrize("C", [0, 1, 7])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("E", [32, 18])
def test_step_front_equals_the_batch_front(E, B, C):
    import dpt_hip
    from dpt_hip import act
    from dpt_hip import train as tr
    m = make_model(E, seed=1).cuda()
    s = dpt_hip.ImageActSession(m, B, (60, 80))
    ctx = gpu(make_context(B, C, 10 + C))
    s.set_context(ctx)
    frames, angle = make_frames(B, (60, 80), 20 + B)
    s.act(frames, angle, sample=False)
    obs = act.obs_preprocess(frames)
    assert torch.equal(s.obs, obs)
    front, _ = s._blobs()
    feats0 = torch.cat([torch.as_tensor(angle, device="cuda"), torch.zeros((B, A + 1), device="cuda")], dim=1)
    e0, _ = tr.front_forward(tr.image_desc(B, SD, A, E, flags=tr.FORWARD_ONLY), front, obs, feats0.contiguous())
    assert torch.equal(s.embeds[:, 0], e0)
    before = s.embeds[:, 1:].clone()
    if C:
        feats = torch.cat([ctx["context_states"], ctx["context_actions"], ctx["context_rewards"]], dim=2)
        ec, _ = tr.front_forward(tr.image_desc(B * C, SD, A, E, flags=tr.FORWARD_ONLY), front,
                                 ctx["context_images"].reshape(B * C, 3, 25, 25).contiguous(),
                                 feats.reshape(B * C, -1).contiguous())
        assert torch.equal(before, ec.reshape(B, C, E))
    frames2, angle2 = make_frames(B, (60, 80), 30 + B)
    s.act(frames2, angle2, sample=False)
    assert torch.equal(s.embeds[:, 1:], before)
    assert not torch.equal(s.embeds[:, 0], e0)


# ----------------------------------------------------------------------------- 3. logits
@pytest.mark.parametrize("C", [0, 1, 7])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("E", [32, 18])
def test_logits_vs_oracle_and_the_plain_forward(E, B, C):
    import dpt_hip
    m = make_model(E, seed=2)
    w64 = weights64(m)
    m = m.cuda()
    ctx = make_context(B, C, 40 + C)
    frames, angle = make_frames(B, (60, 80), 50 + B)
    ref = oracle_logits(w64, oracle_obs(frames), angle, ctx)
    s = dpt_hip.ImageActSession(m, B, (60, 80))
    s.set_context(gpu(ctx))
    s.act(frames, angle, sample=False)
    got = s.logits.cpu().numpy()
    with torch.no_grad():
        plain = m(dict(gpu(ctx), query_images=s.obs, query_states=torch.as_tensor(angle, device="cuda"))).cpu().numpy()
    print(f"image_act E={E} B={B} C={C}: logits vs oracle {fwd_violation(got, ref):.3e}, vs model(batch) "
          f"{fwd_violation(got, plain):.3e}, spread of the oracle's logits {np.ptp(ref, axis=1).min():.3e}")
    assert fwd_violation(got, ref) <= 1e-5
    assert fwd_violation(got, plain) <= 1e-5


def test_the_logit_bar_can_fail():
    """conv2's weights off by 1e-3: the same comparison reports a violation"""
    import dpt_hip
    E, B, C = 32, 5, 7
    m = make_model(E, seed=2)
    w64 = weights64(m)
    ctx = make_context(B, C, 40 + C)
    frames, angle = make_frames(B, (60, 80), 50 + B)
    ref = oracle_logits(w64, oracle_obs(frames), angle, ctx)
    with torch.no_grad():
        m.image_encoder[2].weight.mul_(1 + 1e-3)
    s = dpt_hip.ImageActSession(m.cuda(), B, (60, 80))
    s.set_context(gpu(ctx))
    s.act(frames, angle, sample=False)
    assert fwd_violation(s.logits.cpu().numpy(), ref) > 1e-5


# ----------------------------------------------------------------------------- 4. selection
def test_selection():
    import dpt_hip
    E, B, C = 32, 5, 1
    m = make_model(E, seed=3).cuda()
    ctx = gpu(make_context(B, C, 60))
    frames, angle = make_frames(B, (31, 47), 61)
    s = dpt_hip.ImageActSession(m, B, (31, 47))
    s.set_context(ctx)
    a = s.act(frames, angle, sample=False)
    assert a.dtype == torch.int32 and a.shape == (B,) and a.is_cuda
    assert torch.equal(a.long(), s.logits.argmax(dim=1))
    u = np.random.RandomState(62).uniform(size=B)
    a = s.act(frames, angle, sample=True, uniforms=u)
    assert torch.equal(a, dpt_hip.select_action(s.logits, True, 1.0, uniforms=u))
    a = s.act(frames, angle, sample=True, temp=0.7, seed=5, counter=3)
    assert torch.equal(a, dpt_hip.select_action(s.logits, True, 0.7, seed=5, counter=3))
    s2 = dpt_hip.ImageActSession(m, B, (31, 47))
    s2.set_context(ctx)
    assert torch.equal(a, s2.act(frames, angle, sample=True, temp=0.7, seed=5, counter=3))
    assert torch.equal(s.logits, s2.logits)


# ----------------------------------------------------------------------------- 5. weights changed in place
def test_weights_changed_in_place_are_used():
    import dpt_hip
    E, B, C = 18, 5, 7
    m = make_model(E, seed=4)
    ctx = make_context(B, C, 70)
    frames, angle = make_frames(B, (60, 80), 71)
    mg = m.cuda()
    s = dpt_hip.ImageActSession(mg, B, (60, 80))
    s.set_context(gpu(ctx))
    s.act(frames, angle, sample=False)
    old = s.logits.clone()
    with torch.no_grad():
        mg.image_encoder[0].weight.add_(0.05)
    s.act(frames, angle, sample=False)
    ref = oracle_logits(weights64(mg), oracle_obs(frames), angle, ctx)
    assert fwd_violation(s.logits.cpu().numpy(), ref) <= 1e-5
    assert fwd_violation(old.cpu().numpy(), ref) > 1e-5


# ----------------------------------------------------------------------------- 6. end to end on the stub
E2E = dict(B=3, horizon=3, H=6, Heps=3, E=32)


def e2e_envs():
    return [S.StubMiniworldEnv(env_id=8000 + i, horizon=E2E["horizon"]) for i in range(E2E["B"])]


def plain_loop(w64, model=None):
    """The evaluation written out: oracle preprocessing, the float64 oracle per step (and ``model(batch)``
    on the device when given), greedy actions, the reference's context roll.  Returns (actions (Heps, B,
    horizon), returns (B, Heps), the smallest top-two gap of the oracle's logits)."""
    B, hz, H, Heps = E2E["B"], E2E["horizon"], E2E["H"], E2E["Heps"]
    n_ctx = H // hz
    envs = e2e_envs()
    ctx = {"context_images": np.zeros((B, n_ctx, hz, 3, 25, 25), np.float32),
           "context_states": np.zeros((B, n_ctx, hz, SD), np.float32),
           "context_actions": np.zeros((B, n_ctx, hz, A), np.float32),
           "context_rewards": np.zeros((B, n_ctx, hz, 1), np.float32)}
    all_actions, returns, gap = [], [], np.inf
    for ep in range(Heps):
        filled = min(ep, n_ctx)
        batch = {k: v[:, :filled].reshape(B, filled * hz, *v.shape[3:]) for k, v in ctx.items()}
        frames = np.stack([e.reset()[0] for e in envs])
        rec = {k: np.zeros_like(v[:, 0]) for k, v in ctx.items()}
        ep_actions = np.zeros((B, hz), np.int64)
        for t in range(hz):
            angle = np.stack([e.agent.dir_vec[[0, -1]] for e in envs]).astype(np.float32)
            obs = oracle_obs(frames)
            lg = oracle_logits(w64, obs, angle, batch)
            top = np.sort(lg, axis=1)
            gap = min(gap, float((top[:, -1] - top[:, -2]).min()))
            act = lg.argmax(axis=1)
            if model is not None:
                with torch.no_grad():
                    dev = model(dict(gpu(batch), query_images=torch.as_tensor(obs, device="cuda"),
                                     query_states=torch.as_tensor(angle, device="cuda"))).cpu().numpy()
                assert fwd_violation(dev, lg) <= 1e-5
                assert np.array_equal(dev.argmax(axis=1), act), (ep, t)
            ep_actions[:, t] = act
            rec["context_images"][:, t], rec["context_states"][:, t] = obs, angle
            rec["context_actions"][:, t] = np.eye(A, dtype=np.float32)[act]
            out = [e.step(int(a)) for e, a in zip(envs, act)]
            rec["context_rewards"][:, t, 0] = [o[1] for o in out]
            frames = np.stack([o[0] for o in out])
        all_actions.append(ep_actions)
        returns.append(rec["context_rewards"][:, :, 0].sum(axis=1))
        for k in ctx:
            if ep < n_ctx:
                ctx[k][:, ep] = rec[k]
            else:
                ctx[k] = np.concatenate([ctx[k][:, 1:], rec[k][:, None]], axis=1)
    return np.stack(all_actions), np.stack(returns, axis=1), gap


def test_deploy_online_vec_equals_the_plain_loop():
    from ctrls.ctrl_miniworld import MiniworldTransformerController
    from envs.miniworld_env import MiniworldEnvVec
    from evals.eval_miniworld import deploy_online_vec
    B, hz = E2E["B"], E2E["horizon"]
    m = make_model(E2E["E"], horizon=E2E["H"], seed=E2E_SEED)
    w64 = weights64(m)
    m = m.cuda()
    ref_actions, ref_returns, gap = plain_loop(w64, m)
    assert gap > 1e-3, gap  # no step is decided by fp32 rounding: every step is compared

    episodes = []

    class Recording(MiniworldEnvVec):
        def deploy(self, ctrl):
            out = super().deploy(ctrl)
            episodes.append(out)
            return out

    vec = Recording(e2e_envs())
    ctrl = MiniworldTransformerController(m, batch_size=B, sample=False)
    got = deploy_online_vec(vec, ctrl, E2E["Heps"], E2E["H"], hz, learner=True)
    assert got.shape == (B, E2E["Heps"]) and np.array_equal(got, ref_returns)
    assert len(episodes) == E2E["Heps"]
    for ep, (obs, states, acts, next_obs, rews) in enumerate(episodes):
        assert tuple(obs.shape) == (B, hz, 3, 25, 25) and obs.dtype == torch.float32
        assert states.shape == (B, hz, SD) and acts.shape == (B, hz, A) and rews.shape == (B, hz)
        assert tuple(next_obs.shape) == (B, hz, 3, 60, 80)
        assert np.array_equal(acts.argmax(axis=-1), ref_actions[ep]), ep
        assert np.array_equal(acts.sum(axis=-1), np.ones((B, hz)))


def test_offline_returns_the_four_baselines():
    from evals.eval_miniworld import offline
    n_eval, H = 2, 6
    m = make_model(32, horizon=H, seed=E2E_SEED).cuda()
    rs = np.random.RandomState(80)
    trajs = [{"env_id": 8100 + i, "context_images": rs.uniform(0, 1, (H, 25, 25, 3)),
              "context_states": rs.normal(size=(H, SD)), "context_actions": np.eye(A)[rs.randint(0, A, H)],
              "context_rewards": rs.uniform(0, 1, H)} for i in range(n_eval)]
    np.random.seed(0)
    out = offline(trajs, m, n_eval, make_env=lambda env_id: S.StubMiniworldEnv(env_id=env_id, horizon=3))
    assert sorted(out) == ["lnr", "lnr_greedy", "opt", "rand"]
    for k, v in out.items():
        assert v.shape == (n_eval,), k
    assert np.array_equal(out["opt"], np.full(n_eval, 3.0))  # the stub pays 1 per optimal action


def test_batch_size_one_returns_one_action_row():
    from ctrls.ctrl_miniworld import MiniworldTransformerController
    m = make_model(32, seed=5).cuda()
    ctrl = MiniworldTransformerController(m, batch_size=1, sample=True)
    ctrl.set_batch(gpu(make_context(1, 2, 90)))
    env = S.StubMiniworldEnv(env_id=1)
    frame, _ = env.reset()
    a = ctrl.act(frame, env.agent.pos[[0, -1]], env.agent.dir_vec[[0, -1]])
    assert a.shape == (A,) and a.sum() == 1.0


def test_training_mode_with_dropout_takes_the_plain_forward():
    from ctrls.ctrl_miniworld import MiniworldTransformerController
    from dpt_hip import act
    m = make_model(32, seed=6, dropout=0.1).cuda().train()
    ctrl = MiniworldTransformerController(m, batch_size=2, sample=False)
    ctrl.set_batch(gpu(make_context(2, 3, 91)))
    frames, angle = make_frames(2, (60, 80), 92)
    a = ctrl.act(frames, None, angle)
    assert a.shape == (2, A) and ctrl._session is None
    assert torch.equal(ctrl.last_obs, act.obs_preprocess(frames))


# ----------------------------------------------------------------------------- 7. refusals before a launch
def test_refusals():
    import dpt_hip
    m = make_model(32, horizon=3, seed=7).cuda()  # n_positions 16
    for hw in ((24, 80), (60, 129)):
        with pytest.raises(NotImplementedError, match="sides"):
            dpt_hip.ImageActSession(m, 2, hw)
    s = dpt_hip.ImageActSession(m, 2, (60, 80))
    frames, angle = make_frames(2, (60, 80), 93)
    with pytest.raises(TypeError, match="uint8"):
        s.act(frames.astype(np.float32) / 255, angle, sample=False)
    with pytest.raises(ValueError, match="n_positions"):
        s.set_context(gpu(make_context(2, 16, 94)))
    with pytest.raises(ValueError, match="frames"):
        s.act(frames[:1], angle[:1], sample=False)
    s.set_context(gpu(make_context(2, 15, 95)))  # the longest window the model has positions for
    s.act(frames, angle, sample=False)
    with pytest.raises(ValueError, match="eval mode"):
        dpt_hip.ImageActSession(make_model(32, seed=7, dropout=0.1).cuda().train(), 2, (60, 80))
    from models.net import ImageTransformer
    train_model = ImageTransformer(dict(horizon=3, state_dim=SD, action_dim=A, n_layer=LAYERS, n_embd=32, n_head=1,
                                        dropout=0.0, test=False, image_size=25)).cuda()
    with pytest.raises(ValueError, match="test=True"):
        dpt_hip.ImageActSession(train_model, 2, (60, 80))
    torch.cuda.synchronize()
