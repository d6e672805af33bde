"""The fused rollouts' action selection against its definition on their own logits, with draws placed at
the cdf edges (tests/selection_edges.py; the conditions are shown reachable without a GPU in
tests/test_selection_edges_host.py).

Every rollout selects by one rule (include/dpt_hip.h, dpt_select_action).  The per-step kernel with
set_select_fast(False) runs it in fp64 (select_from_logits, csrc/dpt_common.h); the fused rollouts run the
fp32 shortcut (cdf_fast / select_fast: v_exp_f32, v_rcp_f32, a sequential fp32 sum; the exact fp64 cdf
within kCdfMargin = 2^-15 of an edge), the DarkRoom kernel a second copy of it in its memo tail chain.  Here
every action of a rollout must equal dpt_select_action's (fp64 path) for the logits the rollout reported
at that step and the draw it was given: no step left out, no tolerance, whatever the trajectory.

Each sampled case runs on seeded uniforms, then per delta on draws put delta inside the edge of the
interval run 1 chose.  Steady deltas 1e-6, 1e-5, 2.5e-5, 2.9e-5, 3.2e-5, 3.6e-5, 1e-4: 2^-15 = 3.05e-5 is
the band inside which select_fast hands over to the fp64 cdf, so 2.9e-5 should take the fallback and
3.2e-5 the fp32 comparison alone; both sit only 1.5e-6 from the band's edge, cdf_fast is within about 1e-6
of the exact cdf and no test observes which branch ran, hence 2.5e-5 and 3.6e-5 beside them, clear of the
edge by more than that error.  Steady runs must repeat run 1 bit for bit, and the definition on draws moved
2 delta across the edge must disagree with the rollout at every placed step (the control: the check can
fail).  Razor deltas 1e-9, 1e-8, 1e-7 are below what numpy's cdf and the device's differ by (>= 1e-8, < 1e-6
measured): the side is the device's to decide, and where it decides the other one the run leaves the
trajectory its draws were placed on.  Each razor delta is therefore run in rounds that keep every task's
draws up to its first departure and re-place the later ones on the latest run's own logits
(selection_edges.razor_runs: as many runs as steps, which surely ends with no departure, on rollouts of up
to 256 steps; 64 runs on the one longer shape, the 600 steps at 16 waves, to keep its tests to a few seconds).

Asserted per delta (all collected, raised after the case's last line): >= 0.9 of the task-steps placed, both
sides of an edge, with the DarkRoom memo on >= 1/4 of the steps served by it; >= 0.9 of the placed steps
within 2^-15 of an edge of the run's own logits at the steady deltas <= 2.9e-5, at 1e-7, and at 1e-9 and 1e-8
on every rollout of up to 256 steps.  On the 600-step shape at 1e-9 and 1e-8 the device falls the other way on
so many of the re-placed steps that 64 rounds do not reach the end (a round moves a task on by two to seven
steps; measured shares 0.26 .. 0.75 at 1e-9 and 0.68 .. 1 at 1e-8, printed and recorded), and the bound the
construction guarantees is asserted instead: every placed task-step up to and
including each task's first departure is in band, and each task has at least as many such steps as runs were
made.

Sites: DeviceModel.rollout_darkroom (finish_step and the memo tail chain; 4, 8 and 16 waves, memo and
workspace on / off, perms, temp 1 / 0.5 / 2, greedy), DeviceModel.rollout_bandit (select_rollout: the register
form at 5 and 20 arms, select_from_logits at 7), rollout_bandit_generic, rollout_darkroom_episode
(darkroom_act) and rollout_darkroom_interactive (mdp_act_kernel).  The interactive rollout returns no
logits: each step's are recomputed from its records by the two calls its chain makes (dpt_mdp_pack and the
forward-only, last-position dpt_train_forward on the same blob), which is what the act step read.

The `medium` models of tests/sharp_models.py (one DarkRoom case, one bandit case) keep the 0.9 placed
share (shown on the CPU), so they run the same construction unweakened.

Measured on an MI355X: the whole file takes 34 s; a 600-step case (64 runs per razor delta) 2.4 s, a 254-step
case (up to 168 runs for one razor delta, each a whole rollout and one select call over all its steps) 0.7 to
1.1 s, every other case under half a second.  The round limits are what keeps the cases there: the 600-step
shape would need about 250 runs per delta (some 8 s a case) to end with no departure.

The figures of every case are printed (pytest -s) and recorded in profiles/selection_edges/summary.txt."""
import numpy as np
import pytest
import torch

import selection_edges as SE
from oracle import dpt_oracle as O
from test_gpu_kernels import model_from_golden

pytestmark = pytest.mark.gpu

N_DARKROOM = 11
# (Heps, horizon, R, dim): windows 61 (4 waves), 128 (8 waves) and 301 (16 waves)
DARKROOM_SHAPES = [(3, 30, 2, 10), (2, 127, 1, 10), (2, 300, 1, 12)]
# (shape, workspace, memo).  The 16-wave kernel exists only with the workspace, and its shape's dim 12 has
# more cells (144) than the memo has rows (128): the launcher runs it without the memo whatever the switch
# says, so it gets one pass, and the memo tail chain is never reached at 16 waves.
DARKROOM_CASES = ([(s, ws, memo) for s in DARKROOM_SHAPES[:2] for ws in (True, False) for memo in (True, False)]
                  + [(DARKROOM_SHAPES[2], True, False)])
_DR_SHAPE = lambda s: "%dx%dxR%d-dim%d" % s  # noqa: E731
_DR_ID = lambda c: "%s-ws%d-memo%d" % (_DR_SHAPE(c[0]), c[1], c[2])  # noqa: E731


@pytest.fixture(autouse=True)
def _defaults():
    import dpt_hip
    dpt_hip.device()
    yield
    dpt_hip.set_select_fast(True)
    dpt_hip.set_darkroom_memo(True)
    dpt_hip.set_darkroom_workspace(True)
    dpt_hip.set_decode_tile(8)


def device_select(logits, u, sample, temp):
    """the definition: dpt_select_action on its fp64 path, every (step, task) row in one call"""
    import dpt_hip
    shape, A = logits.shape[:-1], logits.shape[-1]
    lg = np.ascontiguousarray(logits, np.float32).reshape(-1, A)
    if not sample:
        return dpt_hip.select_action(lg, False).cpu().numpy().reshape(shape)
    dpt_hip.set_select_fast(False)
    try:
        a = dpt_hip.select_action(lg, True, temp, uniforms=np.ascontiguousarray(u, np.float64).reshape(-1))
        return a.cpu().numpy().reshape(shape)
    finally:
        dpt_hip.set_select_fast(True)


def test_device_select_is_the_oracle_rule_away_from_edges():
    """the definition used here against numpy's away from the edges (nearer than 1e-5 numpy's expf may
    decide otherwise), at temp 1, 0.5 and 2 and 5, 7 and 20 arms"""
    rs = np.random.RandomState(1)
    for A in (5, 7, 20):
        lg = (rs.randn(3, 500, A) * 2).astype(np.float32)
        u = rs.uniform(size=(3, 500))
        for temp in (1.0, 0.5, 2.0):
            ok = O.boundary_margin(O.softmax_f32(lg, temp), u) > 1e-5
            assert np.array_equal(device_select(lg, u, True, temp)[ok], O.select_actions(lg, u, True, temp=temp)[ok])
        assert np.array_equal(device_select(lg, u, False, 1.0), lg.argmax(-1))


# ----------------------------------------------------------------------------- DeviceModel.rollout_darkroom
def _darkroom_rollout(m, goals, Heps, horizon, R, dim, perms, temp, sample=True):
    def rollout(u):
        o = m.rollout_darkroom(goals, Heps, horizon, R, dim=dim, perms=perms, sample=sample, temp=temp, uniforms=u,
                               want_actions=True, want_logits=True, want_forwards=True)
        return dict(logits=o["logits"].cpu().numpy(), actions=o["actions"].cpu().numpy().T,
                    forwards=o["forwards"].cpu().numpy())
    return rollout


def _darkroom_inputs(shape, permuted):
    Heps, horizon, R, dim = shape
    rs = np.random.RandomState(1000 * Heps + horizon + 7 * permuted)
    goals = rs.randint(0, dim, (N_DARKROOM, 2))
    perms = O.perm_table()[rs.randint(0, 120, N_DARKROOM)].astype(np.int32) if permuted else None
    return goals, perms, rs.uniform(size=(Heps * horizon, N_DARKROOM))


def _darkroom_settings(ws, memo):
    import dpt_hip
    dpt_hip.set_darkroom_workspace(ws)
    dpt_hip.set_darkroom_memo(memo)


@pytest.mark.parametrize("temp", [1.0, 0.5, 2.0])
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("case", DARKROOM_CASES, ids=_DR_ID)
def test_rollout_darkroom_selection(case, permuted, temp):
    shape, ws, memo = case
    Heps, horizon, R, dim = shape
    _, m, _ = model_from_golden("darkroom")
    goals, perms, u0 = _darkroom_inputs(shape, permuted)
    _darkroom_settings(ws, memo)
    label = f"darkroom {_DR_SHAPE(shape)} perms={int(permuted)} temp={temp:g} ws={int(ws)} memo={int(memo)}"
    rollout = _darkroom_rollout(m, goals, Heps, horizon, R, dim, perms, temp)
    SE.run_case(label, rollout, device_select, u0, temp=temp, seed=17, memo=memo)
    if not memo:
        assert (rollout(u0)["forwards"] == horizon).all()
    if dim * dim > 128:  # the memo switch changes nothing there
        _darkroom_settings(ws, True)
        assert (rollout(u0)["forwards"] == horizon).all()


@pytest.mark.parametrize("case", DARKROOM_CASES, ids=_DR_ID)
def test_rollout_darkroom_greedy_selection(case):
    shape, ws, memo = case
    Heps, horizon, R, dim = shape
    _, m, _ = model_from_golden("darkroom")
    goals, perms, u0 = _darkroom_inputs(shape, True)
    _darkroom_settings(ws, memo)
    SE.run_greedy(f"darkroom {_DR_SHAPE(shape)} perms=1 ws={int(ws)} memo={int(memo)}",
                  _darkroom_rollout(m, goals, Heps, horizon, R, dim, perms, 1.0, sample=False), device_select, u0)


def test_rollout_darkroom_selection_medium_model():
    import dpt_hip
    import sharp_models as SM
    m = dpt_hip.DeviceModel(SM.as_torch(SM.darkroom_weights("medium")), 4, 2, 5, 512)
    goals, perms, u0 = SM.darkroom_setup(3, 30, True)
    SE.run_case("darkroom medium 3x30xR2 perms=1 temp=1 ws=1 memo=1",
                _darkroom_rollout(m, goals, 3, 30, 2, 10, perms, 1.0), device_select, u0, seed=5, memo=True)


# ----------------------------------------------------------------------------- DeviceModel.rollout_bandit
BANDIT_L, BANDIT_H = 2, 70


def _bandit_rollout(m, means, H, g, sample=True):
    def rollout(u):
        o = m.rollout_bandit(means, H, 0.3, sample, uniforms=u, noise=g, want_logits=True)
        return dict(logits=o["logits"].cpu().numpy(), actions=o["actions"].cpu().numpy().T)
    return rollout


@pytest.mark.parametrize("A", [5, 20, 7])
@pytest.mark.parametrize("tile,N", [(8, 11), (16, 19)])
def test_rollout_bandit_selection(tile, N, A):
    import bench
    import dpt_hip
    sd, _ = bench.synthetic_state_dict(BANDIT_L, 1, A, BANDIT_H)
    m = dpt_hip.DeviceModel(sd, BANDIT_L, 1, A, 4 * (1 + BANDIT_H))
    dpt_hip.set_decode_tile(tile)
    rs = np.random.RandomState(100 * tile + A)
    means = rs.uniform(0, 1, (N, A))
    u0, g = rs.uniform(size=(BANDIT_H, N)), rs.standard_normal((BANDIT_H, N))
    label = f"bandit L={BANDIT_L} H={BANDIT_H} tile={tile} N={N} A={A}"
    SE.run_case(label, _bandit_rollout(m, means, BANDIT_H, g), device_select, u0, seed=23)
    SE.run_greedy(label, _bandit_rollout(m, means, BANDIT_H, g, sample=False), device_select, u0)


def test_rollout_bandit_selection_medium_model():
    import dpt_hip
    import sharp_models as SM
    N = 11
    m = dpt_hip.DeviceModel(SM.as_torch(SM.rollout_weights(2, 5, "medium")), 2, 1, 5, 4 * (1 + max(SM.ROLLOUT_HS)))
    u0, g = SM.bandit_draws(N, BANDIT_H)
    SE.run_case(f"bandit medium L=2 H={BANDIT_H} tile=8 N={N} A=5",
                _bandit_rollout(m, SM.bandit_means(N, 5), BANDIT_H, g), device_select, u0, seed=6)


# ----------------------------------------------------------------------------- rollout_bandit_generic
@pytest.mark.parametrize("E", [18, 64])
def test_rollout_bandit_generic_selection(E):
    from dpt_hip import train as tr
    from test_gpu_train_grads import _model
    L, A, N, H = 2, 5, 7, 40
    m, _ = _model(E, L, 1, H, 300 + E, test=True)
    m = m.cuda().eval()
    rs = np.random.RandomState(E)
    means = rs.uniform(0, 1, (N, A))
    u0, g = rs.uniform(size=(H, N)), rs.standard_normal((H, N))

    def rollout(u):
        o = tr.rollout_bandit_generic(m, means, H, 0.3, True, 0, uniforms=u, noise=g, want_logits=True)
        return dict(logits=o["logits"].cpu().numpy(), actions=o["actions"].cpu().numpy().T)

    SE.run_case(f"generic bandit E={E} A={A} N={N} H={H}", rollout, device_select, u0, seed=29)


# ----------------------------------------------------------------------------- the in-episode DarkRoom rollouts
def _episode_case(permuted):
    import interactive_mdp_oracle as MO
    m, _ = MO.model(32, MO.REC_L, MO.REC_K, 1032)  # records_case's model, without its oracle episode
    rs = np.random.RandomState(MO.REC_UNIFORM_SEED)
    u0 = rs.uniform(size=(MO.REC_K - 1, MO.REC_N))
    perm = np.stack([rs.permutation(5) for _ in range(MO.REC_N)]).astype(np.int32) if permuted else None
    return m.cuda().eval(), MO.REC_GOALS, MO.REC_K, MO.REC_DIM, perm, u0


@pytest.mark.parametrize("permuted", [False, True])
def test_rollout_darkroom_episode_selection(permuted):
    import dpt_hip
    m, goals, K, dim, perm, u0 = _episode_case(permuted)

    def rollout(u):
        rec, _, lg = dpt_hip.rollout_darkroom_episode(m, goals, K, dim, sample=True, perm=perm, uniforms=u, logits=True)
        return dict(logits=np.ascontiguousarray(lg.cpu().numpy()[:, :K - 1].transpose(1, 0, 2)),
                    actions=rec["actions"].cpu().numpy().T)

    SE.run_case(f"episode K={K} N={len(goals)} dim={dim} perm={int(permuted)}", rollout, device_select, u0, seed=31)


@pytest.mark.parametrize("permuted", [False, True])
def test_rollout_darkroom_interactive_selection(permuted):
    import ctypes

    from dpt_hip import _lib
    from dpt_hip import train as tr
    m, goals, K, dim, perm, u0 = _episode_case(permuted)
    N = len(goals)
    blob = tr.pack_params(tr.param_list(m), torch.device("cuda"))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr())

    def rollout(u):
        rec, _ = tr.rollout_darkroom_interactive(m, goals, K, dim, sample=True, perm=perm, uniforms=u, blob=blob)
        logits = np.zeros((K - 1, N, 5), np.float32)
        for t in range(K - 1):  # step t's window from the records, forwarded as the chain forwards it
            tokens = torch.empty((N, t + 1, 10), device="cuda")
            _lib.call("dpt_mdp_pack", ptr(rec["states"]), ptr(rec["actions"]), ptr(rec["rewards"]), N, K, t,
                      ptr(tokens), stream)
            d = tr.desc(m.n_layer, m.n_embd, 2, 5, m.n_positions, N, t + 1,
                        flags=_lib.TRAIN_FORWARD_ONLY | _lib.TRAIN_LAST_ONLY)
            logits[t] = tr.forward(d, blob, tokens)[0][:, -1].cpu().numpy()
        return dict(logits=logits, actions=rec["actions"].cpu().numpy().T)

    SE.run_case(f"interactive K={K} N={N} dim={dim} perm={int(permuted)}", rollout, device_select, u0, seed=37)
