"""Every training gradient path against the float64 oracle directly (csrc/dpt_train.hip,
dpt_trainstep.hip, dpt_interactive.hip, the rollout of dpt_generic.hip; oracle/dpt_oracle_torch.py).

The parameter-tracking tests (test_gpu_train_step, test_gpu_interactive) see a gradient only through
AdamW, which divides every entry by its own running magnitude: a gradient wrong by a common factor
moves the parameters the same way.  Here the gradient itself is compared, per parameter, under the
bar test_gpu_train holds widths 16 / 64 and the 501-token window to:

    max|got - ref| <= 5 * GRAD_TOL * max|ref|

at the token level (random tokens, so every column of embed_transition.weight sees a varying input,
and random dpreds that are nonzero at position 0 too).  Next to the float64 oracle the same oracle
runs once in fp32; both worst errors are printed per case (profiles/train_grads/errors.txt is the
record of one run: the kernels at 0.25-1.2e-6 of max|g|, the fp32 oracle at 0.37-3.4e-6, its
largest at the 9552-row cases), so the bar leaves 30x or more for a different summation order.

Cases: the row kernels without dropout at the widths only they serve; the window edges of the
matrix-core attention; the weight-gradient reduction at 150 chunks; the last-position top block at
windows past one 64-key lap; the gradient inside the fused supervised step (from AdamW's first
moment) and inside the fused interactive step (its dblob); and the generic rollout's decode
attention past one lap."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_train import GRAD_TOL, KEYS, model_from_fixture

pytestmark = pytest.mark.gpu

A = 5
BAR = 5 * GRAD_TOL


def _model(E, L, sd, H, seed, test=False):
    """a perturbed Transformer on the host (n_positions = 4 (1 + H)) and its float64 state_dict"""
    from models.net import Transformer
    torch.manual_seed(seed)
    m = Transformer(dict(horizon=H, state_dim=sd, action_dim=A, n_layer=L, n_embd=E, n_head=1, dropout=0.0,
                         test=test))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    w64 = {k: v.detach().numpy().astype(np.float64) for k, v in m.state_dict().items()}
    return m, w64


def _names(m):
    """the reference names of tr.param_list(m), in blob order"""
    from dpt_hip import train as tr
    name_of = {id(p): k for k, p in m.named_parameters()}
    return [name_of[id(p)] for p in tr.param_list(m)]


def _split64(vec, m):
    """a float64 blob-order vector as {name: array shaped like the parameter} (the two nn.Linear
    weights are [in][out] in the blob), without the code under test"""
    from dpt_hip import train as tr
    params, names = tr.param_list(m), _names(m)
    out, off, n = {}, 0, len(params)
    for i, (p, k) in enumerate(zip(params, names)):
        flat = vec[off:off + p.numel()]
        out[k] = flat.reshape(p.shape[1], p.shape[0]).T if i in (0, n - 2) else flat.reshape(tuple(p.shape))
        off += p.numel()
    assert off == vec.size
    return out


def _worst(got, ref):
    """(worst max|got - ref| / max|ref| over the parameters, its name); asserts nothing"""
    worst, at = 0.0, None
    for k, r in ref.items():
        r = np.asarray(r, np.float64)
        scale = np.abs(r).max()
        assert scale > 0, k  # a bar relative to a zero gradient would hold nothing
        e = float(np.abs(np.asarray(got[k], np.float64) - r).max() / scale)
        if e >= worst:
            worst, at = e, k
    return worst, at


def _assert_grads(label, got, ref, ref32=None, bars=None):
    """print the worst errors (kernel and fp32 oracle, of max|g| per parameter), then hold every
    parameter to BAR (or to its own entry of ``bars``, for callers whose models have bars of their
    own: tests/sharp_models.py)"""
    worst, at = _worst(got, ref)
    line = f"train_grads {label}: kernel {worst:.3e} of max|g| ({at})"
    if ref32 is not None:
        w32, at32 = _worst(ref32, ref)
        line += f", fp32 oracle {w32:.3e} ({at32})"
    print(line)
    for k, r in ref.items():
        e = np.abs(np.asarray(got[k], np.float64) - r).max()
        assert e <= (BAR if bars is None else bars[k]) * np.abs(r).max(), (label, k, e / np.abs(r).max())


def _oracle(w64, L, tok, dp, dtype):
    """(preds, {name: gradient}) of sum(preds * dpreds) in ``dtype`` from the fp32 tokens / dpreds"""
    from oracle import dpt_oracle_torch as OT
    P = OT.state_dict_params(w64, L, dtype=dtype)
    preds = OT.forward(P, tok.to(dtype), L)
    (preds * dp.to(dtype)).sum().backward()
    return preds.detach().numpy(), {k: v.grad.numpy() for k, v in P.items()}


def _token_inputs(E, L, sd, B, T, last=False, transform=None):
    """the model (on the host), its float64 weights, the random tokens and dpreds of one _token_level
    case; ``transform``: float64 weights -> the weights the case runs on (tests/sharp_models.py),
    loaded into the module"""
    seed = 1000 * E + 10 * T + L + sd + B
    m, w64 = _model(E, L, sd, T, seed)
    if transform is not None:
        import sharp_models as SM
        w64 = SM.as_f64(transform(w64))
        SM.load_into(m, {k: v.astype(np.float32) for k, v in w64.items()})
    gen = torch.Generator().manual_seed(seed + 1)
    tok = torch.randn(B, T, 2 * sd + A + 1, generator=gen)
    dp = torch.randn(B, T, A, generator=gen)
    if last:
        dp[:, :-1] = 0
    return m, w64, tok, dp


def _token_level(label, E, L, sd, B, T, last=False, transform=None, level=None, perturb=None):
    """The shared helper: dpt_train_forward / dpt_train_backward on random tokens and dpreds against
    the float64 oracle.  Every parameter's gradient within BAR of its largest float64 entry, preds
    within the logit bar, wpe's gradient rows at positions >= T exactly zero, a second forward +
    backward bit-identical.  ``last``: DPT_TRAIN_LAST_LOSS with dpreds zero except at the last row
    (preds are then compared at the last row, the only one that path writes).

    ``transform`` / ``level``: the case runs on a model of tests/sharp_models.py; its attention
    statistics are asserted first and its bars follow that module's rule (at ``sharp``, per parameter,
    the larger of the project's bar and twice the fp32 oracle's error).  ``perturb``: applied to the
    module after the oracle has run, so the kernels see other weights than the reference (the
    bar-can-fail control).  Returns the printed figures."""
    from dpt_hip import train as tr
    m, w64, tok, dp = _token_inputs(E, L, sd, B, T, last, transform)
    preds64, g64 = _oracle(w64, L, tok, dp, torch.float64)
    preds32, g32 = _oracle(w64, L, tok, dp, torch.float32)
    rows = slice(T - 1, T) if last else slice(None)
    bars, preds_bar = None, 1e-5
    if level is not None:
        import sharp_models as SM
        SM.assert_sharp(level, SM.token_stats(w64, L, tok.numpy()), label)
        bars = {k: SM.bar(level, BAR, float(np.abs(g32[k] - r).max() / np.abs(r).max())) for k, r in g64.items()}
        preds_bar = SM.bar(level, 1e-5, SM.rel_err(preds32[:, rows], preds64[:, rows]))
    if perturb is not None:
        perturb(m)

    m = m.cuda()
    params = tr.param_list(m)
    blob = tr.pack_params(params)
    d = tr.desc(L, E, sd, A, m.n_positions, B, T, flags=tr.LAST_LOSS if last else 0)
    tok_d, dp_d = tok.cuda().contiguous(), dp.cuda().contiguous()
    runs = []
    for _ in range(2):
        preds, ws = tr.forward(d, blob, tok_d)
        runs.append((preds, tr.backward(d, blob, tok_d, ws, dp_d)))
    got = {k: g.cpu().numpy() for k, g in zip(_names(m), tr.unpack_grads(runs[0][1], params))}
    p_got = runs[0][0].cpu().numpy()
    p_err = np.abs(p_got[:, rows] - preds64[:, rows]) / np.maximum(1, np.abs(preds64[:, rows]))
    if level is not None:
        print(f"train_grads {label}: preds kernel {p_err.max():.3e}, fp32 oracle "
              f"{np.abs((preds32[:, rows] - preds64[:, rows]) / np.maximum(1, np.abs(preds64[:, rows]))).max():.3e}")
    _assert_grads(label, got, g64, g32, bars)
    assert (np.abs(p_got[:, rows] - preds64[:, rows]) <= preds_bar * np.maximum(1, np.abs(preds64[:, rows]))).all(), \
        np.abs(p_got[:, rows] - preds64[:, rows]).max()
    assert m.n_positions > T and not got["transformer.wpe.weight"][T:].any()
    assert torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][0][:, rows], runs[1][0][:, rows])
    return dict(grad=_worst(got, g64)[0], grad32=_worst(g32, g64)[0], preds=float(p_err.max()))


# ----------------------------------------------------------------------------- 1. row kernels
@pytest.mark.parametrize("E,L,sd,B,T", [(18, 2, 1, 3, 38), (20, 2, 2, 3, 65), (48, 2, 2, 3, 103),
                                        (128, 2, 1, 3, 21), (260, 1, 1, 2, 9)])
def test_row_kernels_without_dropout(E, L, sd, B, T):
    """tr_linear / tr_attn_fwd / tr_attn_bwd_ds,dq,dkv / tr_wgrad_part / tr_linear_bwd_data with the
    residual fused (no dropout), at widths mm_fast does not take: 18 (E % 4 != 0: the scalar
    tr_layernorm), 20 (tr_layernorm_rows with 5 of 8 lanes live; T = 65: the attention's second lap
    over the keys), 48 (E / 4 not a power of two), 128 (the e += 64 laps; 63 rows: one partial
    chunk) and 260 (E > 256: tr_ln_param_part and the scalar LayerNorm)."""
    _token_level(f"rows E={E} L={L} sd={sd} B={B} T={T}", E, L, sd, B, T)


# ----------------------------------------------------------------------------- 2. matrix-core window edges
@pytest.mark.parametrize("E,T", [(32, 1), (32, 2), (32, 16), (32, 17), (32, 63), (32, 64), (32, 65), (32, 129),
                                 (16, 1), (16, 17), (16, 65), (64, 1), (64, 17), (64, 65)])
def test_matrix_core_window_edges(E, T):
    """tr_attn_fwd_mfma / tr_attn_bwd_dq_mfma / tr_attn_bwd_dkv_mfma (64 queries per workgroup, 16
    per wave, 16-key tiles, P / dS rows padded to a multiple of 4) at windows of exactly one tile
    (16) and one workgroup (64), one past them (17, 65: the second workgroup holds one live query;
    129), one short (63), and 1 and 2.  dpreds is nonzero at position 0, so the dS = 0 special case
    of query 0 meets a nonzero upstream gradient."""
    _token_level(f"mfma-edge E={E} T={T}", E, 2, 2 if E == 32 else 1, 3, T)


# ----------------------------------------------------------------------------- 3. reduction depth
@pytest.mark.parametrize("E", [32, 18])
def test_weight_gradient_reduction_depth(E):
    """tr_wgrad_reduce over 150 chunks (48 x 199 = 9552 rows): each of its 16 waves sums a run of 9
    or 10 chunks, past the unroll of 8 and into its remainder loop; partials from tr_wgrad_mfma
    (width 32) and tr_wgrad_part (width 18)."""
    _token_level(f"reduce E={E} B=48 T=199", E, 1, 1, 48, 199)


# ----------------------------------------------------------------------------- 4. last-position path
@pytest.mark.parametrize("E", [32, 18])
@pytest.mark.parametrize("T", [2, 9, 65, 130])
def test_last_position_path(T, E):
    """DPT_TRAIN_LAST_LOSS (tr_attn_last / tr_attn_last_bwd: lanes on keys with stride 64) held to
    the oracle under the same absolute bar, not relative to the full backward: windows 2 and 9, and
    65 and 130 where lanes run a second and a third lap; 5 sequences (a partial second workgroup of
    tr_attn_last)."""
    _token_level(f"last-loss E={E} T={T}", E, 2, 1, 5, T, last=True)


# ----------------------------------------------------------------------------- 5. fused supervised step
@pytest.mark.parametrize("E", [32, 18])
def test_fused_step_gradient(E):
    """The gradient inside dpt_train_step.  A fresh Trainer has m = 0, so step k's gradient is
    (m_k - beta1 m_{k-1}) / (1 - beta1), taken in float64 from the trainer's fp32 m, against
    OT.grads at the weights unpacked from the trainer's own blob as it stood before that step (no
    drift): the train_grads.npz darkroom batch, indices [0, 1, 2, 3] then [3, 1, 2] (a smaller batch
    on the larger workspace), at width 32 (the fixture's model) and 18."""
    from dpt_hip.train import DATA_KEYS, Trainer
    from oracle import dpt_oracle_torch as OT
    g = golden("train_grads.npz")
    hb = {k: g[f"darkroom/{k}"] for k in KEYS}
    hb["optimal_actions"] = g["darkroom/optimal_actions"]
    if E == 32:
        fw, m = model_from_fixture("darkroom")
        _, sd, _, L, _ = (int(x) for x in fw["cfg"])
    else:
        sd, L = hb["query_states"].shape[1], 2
        m = _model(E, L, sd, hb["context_states"].shape[1], E)[0].cuda()
    beta1 = 0.9
    trainer = Trainer(m, lr=1e-3, weight_decay=1e-4, betas=(beta1, 0.999))
    data = {k: torch.tensor(hb[k], dtype=torch.float32) for k in DATA_KEYS}
    m_prev = np.zeros(trainer.m.numel())
    for step, idx in enumerate(([0, 1, 2, 3], [3, 1, 2]), 1):
        w = _split64(trainer.blob.cpu().numpy().astype(np.float64), m)
        trainer.step(data, torch.tensor(idx))
        loss = trainer.read_loss()
        m_now = trainer.m.cpu().numpy().astype(np.float64)
        got = _split64((m_now - beta1 * m_prev) / (1 - beta1), m)
        m_prev = m_now
        loss_ref, _, ref = OT.grads(w, {k: hb[k][idx] for k in hb}, L, sd, A)
        assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref), (loss, loss_ref)
        _assert_grads(f"fused-step E={E} step {step} batch {len(idx)}", got, ref)


# ----------------------------------------------------------------------------- 6. fused interactive step
@pytest.mark.parametrize("K,E,chunk,full_width",
                         [(K, E, chunk, False) for K in (1, 2, 6, 70) for E in (32, 18) for chunk in (0, 3)]
                         + [(6, E, chunk, True) for E in (32, 18) for chunk in (0, 3)])
def test_interactive_step_gradient(K, E, chunk, full_width):
    """InteractiveTrainer.dblob after one step (8 envs; all at once, and chunks of 3, 3, 2 added with
    DPT_INTERACTIVE_ACCUMULATE: unequal, so a per-chunk scale error cannot cancel) against the
    oracle's gradient of the mean last-position cross-entropy on the window built from the step's
    own recorded actions and rewards, at the pre-step weights.  Windows 1, 2, 6 and 70 (the rollout's
    decode attention and tr_attn_last past one lap); the last block at full width too at K = 6.
    Conditioned on the records, so there are no near-tie exclusions."""
    from dpt_hip import train as tr
    from oracle import dpt_oracle_torch as OT
    from test_gpu_interactive import _tokens64
    N, L, var = 8, 2, 0.3
    m, w64 = _model(E, L, 1, max(K, 6), 100 * K + E, test=True)
    m = m.cuda()
    trainer = tr.InteractiveTrainer(m, lr=1e-3, weight_decay=1e-4, chunk=chunk, full_width=full_width)
    rs = np.random.RandomState(K * 7 + E + chunk)
    means = rs.uniform(0, 1, (N, A))
    u, gn = rs.uniform(size=(K - 1, N)), rs.normal(size=(K - 1, N))
    actions, rewards = trainer.step(means, K, var, "uniform", uniforms=u, noise=gn)
    loss = trainer.read_loss()
    got = {k: v.cpu().numpy() for k, v in zip(_names(m), tr.unpack_grads(trainer.dblob, tr.param_list(m)))}
    P = OT.state_dict_params(w64, L)
    preds = OT.forward(P, _tokens64(actions.cpu().numpy(), rewards.cpu().numpy(), A), L)[:, -1]
    ref_loss = torch.nn.functional.cross_entropy(preds, torch.from_numpy(means.argmax(1)))
    ref_loss.backward()
    assert abs(loss - ref_loss.item()) <= 1e-5 * abs(ref_loss.item()), (loss, ref_loss.item())
    _assert_grads(f"interactive K={K} E={E} chunk={chunk} full_width={int(full_width)}", got,
                  {k: v.grad.numpy() for k, v in P.items()})


# ----------------------------------------------------------------------------- 7. decode attention past one lap
# (E, L, N, H, draw seed): the seed is the first whose float64-oracle rollout keeps every selection
# uniform more than 1e-5 from a cdf edge (found on the host; asserted below)
@pytest.mark.parametrize("E,L,N,H,seed", [(16, 2, 9, 130, 0), (18, 2, 9, 130, 0), (64, 2, 9, 40, 0),
                                             (20, 2, 9, 70, 0), (128, 2, 9, 40, 0), (256, 1, 9, 20, 0)])
def test_decode_attention_past_one_lap(E, L, N, H, seed):
    """dpt_rollout_bandit_generic against the float64 oracle's re-forward-every-step rollout fed the
    same draws, at horizons past one lap of the decode attention: gen_attn_ydecode (width 18, lanes
    on keys with stride 64) at 130 keys, gen_attn_ydecode4<4> (width 16, 64 keys per iteration) into
    its second and third iteration with the running-max rescale, and width 64 at 40; width 20
    (gen_attn_ydecode4<8> with the row-kernel products), 128 (<32>, the column-split products with
    LayerNorm on load) and 256 (<64>, one key per wave instruction, row-kernel products).  Logits within
    1e-5 at every step; actions, rewards and arm values exactly, no task or step left out: the draw
    seed is chosen so that the oracle alone has no uniform within 1e-5 of a cdf edge, and that margin
    is asserted here, so a changed oracle or seed fails loudly instead of flaking."""
    from dpt_hip import train as tr
    from oracle import dpt_oracle as O
    m, w64 = _model(E, L, 1, H, E + L, test=True)
    W = O.split_weights(w64, L)
    rs = np.random.RandomState(seed)
    means = rs.uniform(0, 1, (N, A))
    u, gn = rs.uniform(size=(H, N)), rs.normal(size=(H, N))
    ref = O.bandit_online_rollout(W, means, H, 0.3, u, gn)
    margin = O.boundary_margin(O.softmax_f32(ref["logits"]), u).min()
    print(f"train_grads decode E={E} H={H}: oracle cdf margin {margin:.3e}")
    assert margin > 1e-5, margin
    out = tr.rollout_bandit_generic(m.cuda().eval(), means, H, 0.3, True, 0, uniforms=u, noise=gn, want_logits=True)
    lg = out["logits"].cpu().numpy()
    err = np.abs(lg - ref["logits"]) / np.maximum(1, np.abs(ref["logits"]))
    print(f"train_grads decode E={E} H={H}: max logit error {err.max():.3e}")
    assert (err <= 1e-5).all()
    assert np.array_equal(out["actions"].cpu().numpy(), ref["actions"])
    assert np.array_equal(out["rewards"].cpu().numpy(), ref["rewards"])
    assert np.array_equal(out["arm_value"].cpu().numpy().T, ref["cum_means"])
