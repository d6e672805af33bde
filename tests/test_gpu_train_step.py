"""The fused device training step (csrc/dpt_trainstep.hip, dpt_hip.train.Trainer, train.py).

Batch packing against Transformer._tokens on batches recorded from the reference's loader
(tests/golden/train_loader.npz); the summed cross-entropy and AdamW against float64 restatements
on the same fp32 inputs, each held to twice torch's own fp32 error plus one fp32 rounding
(2^-23); three fused steps against the float64 oracle under the bars of
test_gpu_train.test_adamw_steps_track_the_float64_oracle; the test loss against the existing
no-grad training-mode forward; and collect_data -> train -> eval from the command line."""
import ctypes
import glob
import os
import pickle

import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_train import KEYS, batch_from, model_from_fixture

pytestmark = pytest.mark.gpu

TRAJ_KEYS = ("context_states", "context_actions", "context_next_states", "context_rewards", "query_state",
             "optimal_action")
ULP = 2.0 ** -23


def _lib_call(name, *args):
    from dpt_hip import _lib
    _lib.call(name, *args)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------- pack
def _loader_model(name):
    """(fixture, our Dataset arrays as a dict of fp32 tensors, a Transformer of the fixture's dims)"""
    from models.net import Transformer
    g = golden("train_loader.npz")
    n, H, sd, A = (int(x) for x in g[f"{name}/cfg"])
    m = Transformer(dict(horizon=H, state_dim=sd, action_dim=A, n_layer=1, n_embd=32, n_head=1, dropout=0.0,
                         test=False))
    tr = {k: torch.from_numpy(g[f"{name}/traj/{k}"].astype(np.float32)) for k in TRAJ_KEYS}
    data = {"query_states": tr["query_state"], "optimal_actions": tr["optimal_action"],
            "context_states": tr["context_states"], "context_actions": tr["context_actions"],
            "context_next_states": tr["context_next_states"], "context_rewards": tr["context_rewards"][:, :, None]}
    return g, data, m, (n, H, sd, A)


def _pack(dd, m, index, perm):
    from dpt_hip import train as tr
    B, T = len(index), 1 + dd.horizon
    d = tr.desc(m.n_layer, m.n_embd, m.state_dim, m.action_dim, m.n_positions, B, T)
    idx = torch.as_tensor(index, dtype=torch.int64).cuda()
    pm = None if perm is None else torch.as_tensor(perm, dtype=torch.int64).cuda()
    tokens = torch.full((B, T, 2 * dd.state_dim + dd.action_dim + 1), float("nan"), device="cuda")
    targets = torch.full((B, dd.action_dim), float("nan"), device="cuda")
    _lib_call("dpt_train_pack_batch", ctypes.byref(d), ctypes.byref(dd.struct), _p(idx), _p(pm), B, _p(tokens),
              _p(targets), _stream())
    return tokens, targets


@pytest.mark.parametrize("name", ["bandit", "darkroom"])
@pytest.mark.parametrize("shuffle", [False, True])
def test_pack_equals_tokens_of_recorded_batches(name, shuffle, tmp_path):
    """dpt_train_pack_batch on the loader's (index, perm) plan == Transformer._tokens on the batch
    the reference's loader produced, bit for bit: every batch of the first epoch (8 samples, and
    the last batch of 4 / 3), state_dim 1 and 2, with and without the context permutation."""
    from dataset import Dataset
    from dpt_hip.train import DeviceData
    g, data, m, (n, H, sd, A) = _loader_model(name)
    trajs = [{k: g[f"{name}/traj/{k}"][i] for k in TRAJ_KEYS} for i in range(n)]
    path = tmp_path / "trajs.pkl"
    with open(path, "wb") as f:
        pickle.dump(trajs, f)
    ds = Dataset(str(path), {"shuffle": shuffle, "horizon": H, "store_gpu": True, "state_dim": sd,
                             "action_dim": A})
    dd = DeviceData(ds)
    torch.manual_seed(int(g["loader_seed"]))
    loader = torch.utils.data.DataLoader(ds.index_view(), batch_size=int(g["batch_size"]), shuffle=True)
    sizes = []
    for b, batch in enumerate(loader):
        index, perm = batch if shuffle else (batch, None)
        pre = f"{name}/shuf{int(shuffle)}/e0/b{b}/"
        rec = {k: torch.from_numpy(g[pre + k]) for k in KEYS}
        tokens, targets = _pack(dd, m, index, perm)
        assert torch.equal(tokens, m._tokens(rec)), b
        assert torch.equal(targets.cpu(), torch.from_numpy(g[pre + "optimal_actions"])), b
        sizes.append(len(index))
    assert sizes[0] == 8 and sizes[-1] == (4 if name == "bandit" else 3)


@pytest.mark.parametrize("name", ["bandit", "darkroom"])
def test_pack_repeated_and_unsorted_indices(name):
    """Batches of 3 and 8 with repeated, unsorted sample indices and arbitrary permutations; an
    index outside the dataset packs zeros instead of reading."""
    from dpt_hip.train import DeviceData
    g, data, m, (n, H, sd, A) = _loader_model(name)
    dd = DeviceData(data)
    rs = np.random.RandomState(5)
    for index in ([n - 1, 0, n - 1], [7, 7, 3, 11, 0, 3, n - 1, 2]):
        for perm in (None, np.stack([rs.permutation(H) for _ in index])):
            idx = torch.tensor(index)
            batch = {k: data[k][idx] for k in KEYS}
            if perm is not None:
                rows = torch.arange(len(idx))[:, None]
                for k in ("context_states", "context_actions", "context_next_states", "context_rewards"):
                    batch[k] = batch[k][rows, torch.from_numpy(perm)]
            tokens, targets = _pack(dd, m, idx, perm)
            assert torch.equal(tokens, m._tokens(batch))
            assert torch.equal(targets.cpu(), data["optimal_actions"][idx])
    tokens, targets = _pack(dd, m, [2, n, -1], None)
    assert torch.equal(tokens[0], m._tokens({k: data[k][[2]] for k in KEYS})[0])
    assert not tokens[1:].any() and not targets[1:].any()


# ----------------------------------------------------------------------------- cross-entropy
def _ce(preds, targets, want_grad=True):
    B, T, A = preds.shape
    dp = torch.full_like(preds, float("nan")) if want_grad else None
    partial = torch.empty(B, dtype=torch.float64, device="cuda")
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    _lib_call("dpt_train_ce_loss", _p(preds), _p(targets), B, T, A, _p(dp), _p(partial), _p(acc), _stream())
    return acc, dp


@pytest.mark.parametrize("B,T,A", [(3, 2, 5), (4, 9, 20), (2, 5, 1)])
@pytest.mark.parametrize("soft", [False, True])
def test_ce_loss_and_gradient(B, T, A, soft):
    """dpt_train_ce_loss (train.py:295-301) against a float64 restatement on the same fp32 inputs:
    logits of magnitude up to 30, one-hot and soft targets.  dpreds within twice the error of
    torch's own fp32 cross_entropy gradient plus 2^-23, the loss within 1e-5 relative (the project's
    loss bar), position 0 zero, two calls bit-identical, the loss-only call the same loss."""
    rs = np.random.RandomState(B * 100 + T * 10 + A + soft)
    x = (rs.uniform(-1, 1, (B, T, A)) * rs.choice([1.0, 5.0, 30.0], (B, T, 1))).astype(np.float32)
    if soft:
        t = rs.dirichlet(np.ones(A), B).astype(np.float32)
    else:
        t = np.eye(A, dtype=np.float32)[rs.randint(0, A, B)]
    preds, targets = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    # float64 restatement
    x64, t64 = x.astype(np.float64)[:, 1:], t.astype(np.float64)[:, None, :]
    mx = x64.max(-1, keepdims=True)
    lse = mx + np.log(np.exp(x64 - mx).sum(-1, keepdims=True))
    ref_loss = float((t64 * (lse - x64)).sum())
    ref_d = np.zeros((B, T, A))
    ref_d[:, 1:] = np.exp(x64 - lse) * t64.sum(-1, keepdims=True) - t64
    # torch's fp32 gradient of the same loss
    pt = preds.clone().requires_grad_(True)
    true = targets.unsqueeze(1).repeat(1, T - 1, 1).reshape(-1, A)
    torch.nn.CrossEntropyLoss(reduction="sum")(pt[:, 1:].reshape(-1, A), true).backward()
    torch_err = np.abs(pt.grad.cpu().numpy() - ref_d).max()

    acc, dp = _ce(preds, targets)
    acc2, dp2 = _ce(preds, targets)
    acc3, _ = _ce(preds, targets, want_grad=False)
    loss, got = acc.item(), dp.cpu().numpy()
    err = np.abs(got - ref_d).max()
    print(f"ce {B}x{T}x{A} soft={soft}: dpreds err {err:.3e} (torch {torch_err:.3e}), loss {loss!r} ref {ref_loss!r}")
    assert err <= 2 * torch_err + ULP
    assert abs(loss - ref_loss) <= 1e-5 * abs(ref_loss)
    assert not got[:, 0].any()
    assert torch.equal(acc, acc2) and torch.equal(dp, dp2) and torch.equal(acc, acc3)
    # the accumulator accumulates
    partial = torch.empty(B, dtype=torch.float64, device="cuda")
    _lib_call("dpt_train_ce_loss", _p(preds), _p(targets), B, T, A, None, _p(partial), _p(acc), _stream())
    assert acc.item() == 2 * loss


# ----------------------------------------------------------------------------- AdamW
def test_adamw_step_matches_float64_update():
    """dpt_adamw_step over 4099 entries (no multiple of 4 or of the block), gradients with exact
    zeros and entries of 1e-20, steps 1..3 with the state carried over, against a float64
    restatement of torch.optim.AdamW's documented update from the same fp32 inputs: max error
    within twice torch.optim.AdamW's own fp32 error plus 2^-23 max|p|; zero-gradient entries equal
    fl(p (1 - lr wd)) within 1 ulp.  Buffers that are not 16-byte aligned give the same bits."""
    from dpt_hip import _lib
    n, lr, wd, b1, b2, eps = 4099, 1e-3, 1e-4, 0.9, 0.999, 1e-8
    rs = np.random.RandomState(9)
    p0 = rs.normal(0, 0.5, n).astype(np.float32)
    zero = rs.rand(n) < 0.2
    tiny = (rs.rand(n) < 0.1) & ~zero
    grads = []
    for _ in range(3):
        g = (rs.normal(0, 1, n) * 10.0 ** rs.uniform(-6, 0, n)).astype(np.float32)
        g[zero], g[tiny] = 0.0, np.float32(1e-20)
        grads.append(g)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    pt = torch.from_numpy(p0).cuda().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    ours = [torch.from_numpy(p0).cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    off = [torch.zeros(n + 1, device="cuda")[1:] for _ in range(3)]  # 4 bytes past an aligned address
    off[0].copy_(ours[0])
    for step, g in enumerate(grads, 1):
        g64 = g.astype(np.float64)
        p64 = p64 * (1 - lr * wd)
        m64 = b1 * m64 + (1 - b1) * g64
        v64 = b2 * v64 + (1 - b2) * g64 * g64
        p64 = p64 - lr / (1 - b1 ** step) * m64 / (np.sqrt(v64) / np.sqrt(1 - b2 ** step) + eps)
        pt.grad = torch.from_numpy(g).cuda()
        opt.step()
        before = ours[0].cpu().numpy()
        gd = torch.from_numpy(g).cuda()
        goff = torch.zeros(n + 1, device="cuda")[1:].copy_(gd)
        args = _lib.AdamWArgs(lr, b1, b2, eps, wd, step)
        for bufs, grad in ((ours, gd), (off, goff)):
            _lib_call("dpt_adamw_step", _p(bufs[0]), _p(grad), _p(bufs[1]), _p(bufs[2]), n, ctypes.byref(args),
                      _stream())
        assert all(torch.equal(a, b) for a, b in zip(ours, off)), step
        got = ours[0].cpu().numpy()
        err = np.abs(got - p64).max()
        torch_err = np.abs(pt.detach().cpu().numpy() - p64).max()
        print(f"adamw step {step}: err {err:.3e} (torch {torch_err:.3e})")
        assert err <= 2 * torch_err + ULP * np.abs(p64).max(), step
        decayed = (before.astype(np.float64) * (1 - lr * wd)).astype(np.float32)
        assert (np.abs(got[zero] - decayed[zero]) <= np.spacing(np.abs(decayed[zero]))).all(), step
        assert not ours[1].cpu().numpy()[zero].any() and not ours[2].cpu().numpy()[zero].any()


# ----------------------------------------------------------------------------- fused step
def _fused_steps_vs_oracle(m, w64, L, sd, A, hb, plans, lr=1e-3):
    """Trainer.step over the index batches ``plans`` against the same AdamW steps on the float64
    oracle's gradients, under test_adamw_steps_track_the_float64_oracle's bars."""
    from dpt_hip.train import DATA_KEYS, Trainer
    from oracle import dpt_oracle_torch as OT
    P = OT.state_dict_params(w64, L)
    names = list(P)
    opt_ref = torch.optim.AdamW([P[k] for k in names], lr=lr, weight_decay=1e-4)
    wte = m.transformer.wte.weight.detach().clone()
    trainer = Trainer(m, lr=lr, weight_decay=1e-4)
    data = {k: torch.tensor(hb[k], dtype=torch.float32) for k in DATA_KEYS}
    for idx in plans:
        trainer.step(data, torch.tensor(idx))
        loss = trainer.read_loss()
        sub = {k: hb[k][idx] for k in hb}
        opt_ref.zero_grad()
        ref_loss = OT.train_loss(P, sub, L, sd, A)[0]
        ref_loss.backward()
        opt_ref.step()
        assert abs(loss - ref_loss.item()) <= 1e-5 * abs(ref_loss.item()), (loss, ref_loss.item())
    assert trainer.read_loss() == 0.0 and trainer.steps == len(plans)
    trainer.sync_to_model()
    params = dict(m.named_parameters())
    assert torch.equal(params["transformer.wte.weight"], wte)
    diffs = np.concatenate([np.abs(params[k].detach().cpu().numpy() - P[k].detach().numpy()).ravel()
                            for k in names])
    assert (diffs <= 1e-5).mean() >= 0.995, (diffs <= 1e-5).mean()
    assert diffs.max() <= 2 * lr * len(plans) + 1e-5


def _darkroom_setting():
    g = golden("train_grads.npz")
    fw, m = model_from_fixture("darkroom")
    _, sd, A, L, _ = (int(x) for x in fw["cfg"])
    hb = {k: g[f"darkroom/{k}"] for k in KEYS}
    hb["optimal_actions"] = g["darkroom/optimal_actions"]
    return fw, m, sd, A, L, hb


@pytest.mark.parametrize("plans", [[[0, 1, 2, 3]] * 3, [[0, 1, 2, 3], [3, 1, 2], [2, 0]]],
                         ids=["full_batches", "smaller_last_batches"])
def test_fused_steps_track_the_float64_oracle(plans):
    """Three Trainer.steps on the train_grads.npz darkroom batch (width 32: the matrix-core
    kernels), and the same with later batches smaller than the workspace's desc.batch."""
    fw, m, sd, A, L, hb = _darkroom_setting()
    w64 = {k[2:]: v for k, v in fw.items() if k.startswith("w/")}
    _fused_steps_vs_oracle(m, w64, L, sd, A, hb, plans)


def test_fused_steps_track_the_float64_oracle_width_16():
    """The same at width 16: the generic-width kernels, where only the training path runs."""
    from models.net import Transformer
    _, _, sd, A, _, hb = _darkroom_setting()
    for E in (16,):
        torch.manual_seed(E)
        m = Transformer(dict(horizon=hb["context_states"].shape[1], state_dim=sd, action_dim=A, n_layer=2, n_embd=E,
                             n_head=1, dropout=0.0, test=False))
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.05 * torch.randn_like(p))
        w64 = {k: v.detach().numpy().astype(np.float64) for k, v in m.state_dict().items()}
        _fused_steps_vs_oracle(m.cuda(), w64, 2, sd, A, hb, [[0, 1, 2, 3]] * 3)


def test_eval_loss_equals_no_grad_training_mode_forward():
    """Trainer.eval_loss (pack -> forward only -> cross-entropy) against the existing path: the
    model's no-grad forward in training mode and torch's summed cross-entropy, at dropout 0.  The
    weights, the optimizer state and the step count stay as they were."""
    from dpt_hip.train import DATA_KEYS, Trainer
    g = golden("train_grads.npz")
    fw, m, sd, A, L, hb = _darkroom_setting()
    batch, opt = batch_from(g, "darkroom")
    m.train()
    with torch.no_grad():
        pred = m(batch)
        true = opt.unsqueeze(1).repeat(1, pred.shape[1], 1).reshape(-1, A)
        ref = torch.nn.CrossEntropyLoss(reduction="sum")(pred.reshape(-1, A), true).item()
    trainer = Trainer(m, lr=1e-3)
    blob = trainer.blob.clone()
    data = {k: torch.tensor(hb[k], dtype=torch.float32) for k in DATA_KEYS}
    trainer.eval_loss(data, torch.arange(4))
    got = trainer.read_loss()
    assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
    trainer.eval_loss(data, torch.tensor([1, 3]))   # a smaller batch on the same workspace
    trainer.eval_loss(data, torch.tensor([0, 2]))
    assert abs(trainer.read_loss() - ref) <= 1e-5 * abs(ref)
    assert torch.equal(trainer.blob, blob) and trainer.steps == 0 and not trainer.m.any()


def test_trainer_dropout_draws_fresh_masks():
    """With the model's dropout > 0 every call takes a new seed from the CUDA generator (the test
    loss included: the reference evaluates in training mode); torch.manual_seed reproduces them."""
    from dpt_hip.train import DATA_KEYS, Trainer
    _, m, sd, A, L, hb = _darkroom_setting()
    m.dropout = 0.3
    trainer = Trainer(m, lr=1e-3)
    data = {k: torch.tensor(hb[k], dtype=torch.float32) for k in DATA_KEYS}
    losses = []
    for seed in (3, 3):
        torch.manual_seed(seed)
        for _ in range(2):
            trainer.eval_loss(data, torch.arange(4))
            losses.append(trainer.read_loss())
    assert losses[0] == losses[2] and losses[1] == losses[3] and losses[0] != losses[1]


# ----------------------------------------------------------------------------- command line
def test_cli_collect_train_eval(tmp_path, monkeypatch):
    """collect_data.py -> train.py (2 epochs) -> eval.py without --checkpoint, in a scratch
    directory: the log carries two finite test-loss and train-loss lines, the final checkpoint has
    the reference's key set, loads strictly, differs from the initial weights, and eval.py's figures
    are written."""
    import importlib

    import matplotlib
    matplotlib.use("Agg")
    import collect_data
    from models.net import Transformer
    train = importlib.import_module("train")
    ev = importlib.import_module("eval")
    monkeypatch.chdir(tmp_path)
    data_args = ["--env", "bandit", "--envs", "50", "--envs_eval", "8", "--H", "20", "--dim", "5", "--var", "0.3"]
    collect_data.main(data_args)
    train.main(data_args + ["--num_epochs", "2"])
    logs = glob.glob("figs/loss/*_logs.txt")
    assert len(logs) == 1
    lines = open(logs[0]).read().splitlines()
    for tag in ("\tTest loss: ", "\tTrain loss: "):
        vals = [float(ln[len(tag):]) for ln in lines if ln.startswith(tag)]
        assert len(vals) == 2 and np.isfinite(vals).all() and min(vals) > 0, (tag, vals)
    assert lines[0].startswith("Num train batches: ") and lines[1].startswith("Num test batches: ")
    ckpts = glob.glob("trained_models/*.pt")
    assert len(ckpts) == 1 and os.path.basename(ckpts[0]) == os.path.basename(logs[0])[:-len("_logs.txt")] + ".pt"
    sd = torch.load(ckpts[0], map_location="cpu", weights_only=True)
    torch.manual_seed(0)
    fresh = Transformer(dict(horizon=20, state_dim=1, action_dim=5, n_layer=3, n_embd=32, n_head=1, dropout=0.0,
                             test=True))
    init = {k: v.clone() for k, v in fresh.state_dict().items()}
    assert set(sd) == set(init)
    fresh.load_state_dict(sd, strict=True)
    assert torch.equal(sd["transformer.wte.weight"], init["transformer.wte.weight"])
    for k in ("embed_transition.weight", "transformer.h.0.attn.c_attn.weight", "pred_actions.bias",
              "transformer.wpe.weight"):
        assert not torch.equal(sd[k], init[k]), k
    ev.main(data_args + ["--n_eval", "8"])
    figs = glob.glob("figs/evals_epoch-1/*/*.png")
    assert len(figs) >= 2, figs


def test_cli_train_darkroom_shuffled_ten_epochs(tmp_path, monkeypatch):
    """train.py on a DarkRoom dataset with --shuffle (the loader yields (index, perm) batches; 80
    samples: a full batch and a smaller last one) for ten epochs: the tenth epoch writes the
    reference's summary lines and the loss plot, the loss falls, and the same seed reproduces the
    run's losses exactly (loader order, permutations and the deterministic kernels)."""
    import importlib

    import matplotlib
    matplotlib.use("Agg")
    import collect_data
    train = importlib.import_module("train")
    monkeypatch.chdir(tmp_path)
    data_args = ["--env", "darkroom_heldout", "--envs", "100", "--H", "20", "--dim", "10"]
    collect_data.main(data_args)
    runs = []
    for _ in range(2):
        train.main(data_args + ["--num_epochs", "10", "--shuffle", "--lr", "0.001"])
        logs = glob.glob("figs/loss/*_logs.txt")
        assert len(logs) == 1 and "_shufTrue_" in logs[0]
        lines = open(logs[0]).read().splitlines()
        runs.append([float(ln.split(": ")[1]) for ln in lines if ln.startswith(("\tTest loss: ", "\tTrain loss: "))])
    assert lines[0] == "Num train batches: 2" and "Train Loss:       " + str(runs[1][-1]) in lines
    assert len(runs[0]) == 20 and np.isfinite(runs[0]).all() and runs[0][-1] < runs[0][1]
    assert runs[0] == runs[1]
    assert len(glob.glob("figs/loss/*_train_loss.png")) == 1
    assert len(glob.glob("trained_models/*.pt")) == 1   # the final checkpoint only (no epoch-50 one yet)
