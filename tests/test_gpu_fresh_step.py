"""The fresh-task training step on the device (dpt_fresh_step / dpt_fresh_eval_loss,
dpt_hip.train.FreshTrainer, train_fresh.py) at width 32, 2 layers, batch 8 (bandit: 5 arms, H 12; DarkRoom:
dim 5, H 9):

- three ``FreshTrainer.step`` calls (8, 8, then 5 samples) leave blob, m, v and the loss accumulator
  bit-identical to three ``Trainer.step`` calls on ``fresh_dataset`` of the same tasks in identity index
  order, also with dropout 0.1 under equal dropout seeds, and ``eval_loss`` matches in the same way;
- ``Trainer.step`` on a resident dataset gives the bytes the parent commit's build gave
  (profiles/fresh_step/digests.txt, the cases of scripts/fresh_step_ab.py);
- 150 fresh steps lower a held-out fresh test loss, and a second run gives a bit-identical blob;
- train_fresh.py end to end at tiny flags writes the checkpoint train.py would, and eval.py's loader takes it.
"""
import copy
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

E, L, B = 32, 2, 8
SEED = 4711


def make_env(kind):
    import dpt_hip
    if kind == "bandit":
        return dpt_hip.FreshEnv.bandit(5, 12, 0.3, "uniform")
    goals = np.array([[(j, i) for i in range(5)] for j in range(5)]).reshape(-1, 2)
    return dpt_hip.FreshEnv.darkroom(5, 9, goals)


def make_model(env, dropout=0.0, n_layer=L, seed=7):
    from models.net import Transformer
    torch.manual_seed(seed)
    m = Transformer(dict(horizon=env.H, state_dim=env.state_dim, action_dim=env.action_dim, n_layer=n_layer,
                         n_embd=E, n_head=1, dropout=dropout, test=False))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return m.cuda().train()


def state_bytes(t):
    torch.cuda.synchronize()
    return {k: getattr(t, k).contiguous().view(torch.uint8).cpu() for k in ("blob", "m", "v", "loss")}


def assert_same(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["bandit", "darkroom"])
def test_fresh_steps_equal_trainer_steps_on_the_materialised_tasks(kind, dropout):
    from dpt_hip import train as tr
    env = make_env(kind)
    model = make_model(env, dropout)
    fresh = tr.FreshTrainer(copy.deepcopy(model), env, lr=1e-3, seed=SEED)
    resident = tr.Trainer(copy.deepcopy(model), lr=1e-3)
    sizes, ds = (B, B, 5), [900, 901, 902]  # the third step with a smaller batch; one dropout seed per step
    dd = resident.device_data(tr.fresh_dataset(0, sum(sizes), env, SEED))
    lo = 0
    for n, s in zip(sizes, ds):
        fresh.step(n, dropout_seed=s)
        resident._run(True, dd, torch.arange(lo, lo + n), None, seed=s)
        lo += n
        assert_same(state_bytes(fresh), state_bytes(resident))
    assert fresh.first_task == sum(sizes) and fresh.steps == resident.steps == 3
    assert float(fresh.loss.item()) > 0
    # the test loss: other tasks, another key, chunks of 8 + 8 + 5
    test_dd = resident.device_data(tr.fresh_dataset(1000, 21, env, SEED + 1))
    fresh.eval_loss(1000, 21, seed=SEED + 1, batch=B, dropout_seed=903)
    for lo in (0, 8, 16):
        resident._run(False, test_dd, torch.arange(lo, min(lo + 8, 21)), None, seed=903)
    assert_same(state_bytes(fresh), state_bytes(resident))
    assert fresh.read_loss() == resident.read_loss() > 0
    # the module's parameters after the sync
    for p, q in zip(fresh.sync_to_model().parameters(), resident.sync_to_model().parameters()):
        assert torch.equal(p, q)


def test_resident_trainer_bytes_are_the_parent_builds():
    """Trainer.step / eval_loss on a resident dataset: the digests recorded from the parent commit's build
    (first column of profiles/fresh_step/digests.txt) against this build's"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    ab = importlib.import_module("fresh_step_ab")
    want = {}
    for line in open(os.path.join(ROOT, "profiles", "fresh_step", "digests.txt")):
        if line.strip() and not line.startswith("#"):
            parent, _, name = line.rstrip("\n").split("  ", 2)
            want[name] = parent
    got = ab.resident_digests()
    assert len(want) >= 4 and set(got) == set(want)
    assert got == want


def test_fresh_steps_learn_and_repeat():
    """150 fresh steps (1 layer, 3 arms, H 8, var 0): the held-out fresh test loss falls below its value at
    step 0, and the same seed gives the same bytes"""
    import dpt_hip
    from dpt_hip import train as tr
    env = dpt_hip.FreshEnv.bandit(3, 8, 0.0, "uniform")

    def run():
        t = tr.FreshTrainer(make_model(env, n_layer=1, seed=11), env, lr=1e-3, seed=SEED)
        t.eval_loss(0, 256, seed=SEED + 1)
        before = t.read_loss()
        for _ in range(150):
            t.step()
        assert t.first_task == 150 * 64
        t.read_loss()
        t.eval_loss(0, 256, seed=SEED + 1)
        return before, t.read_loss(), t.blob.clone()

    before, after, blob = run()
    print(f"held-out test loss per position: {before / 256 / 8:.4f} -> {after / 256 / 8:.4f}")
    assert np.isfinite(after) and after < before
    before2, after2, blob2 = run()
    assert (before2, after2) == (before, after) and torch.equal(blob.view(torch.int32), blob2.view(torch.int32))


@pytest.mark.parametrize("env", ["bandit", "darkroom_heldout"])
def test_train_fresh_end_to_end(env, tmp_path, monkeypatch):
    from models.net import Transformer
    from utils import build_bandit_model_filename, build_darkroom_model_filename
    train_fresh = importlib.import_module("train_fresh")
    ev = importlib.import_module("eval")
    monkeypatch.chdir(tmp_path)
    flags = ["--env", env, "--envs", "200", "--H", "8", "--dim", "3", "--num_epochs", "2", "--layer", "2",
             "--var", "0.3", "--batch", "48"]
    train_fresh.main(flags)
    cfg = {"shuffle": False, "lr": 1e-3, "dropout": 0, "n_embd": 32, "n_layer": 2, "n_head": 1, "n_envs": 200,
           "n_hists": 1, "n_samples": 1, "horizon": 8, "dim": 3, "seed": 0}
    if env == "bandit":
        name, sd, A = build_bandit_model_filename(env, dict(cfg, var=0.3, cov=0.0)), 1, 3
    else:
        name, sd, A = build_darkroom_model_filename(env, cfg), 2, 5
    path = tmp_path / "trained_models" / f"{name}.pt"
    assert path.exists(), os.listdir(tmp_path / "trained_models")
    model = Transformer(dict(horizon=8, state_dim=sd, action_dim=A, n_layer=2, n_embd=32, n_head=1, dropout=0,
                             test=True))
    ev.load_checkpoint(model, str(path))
    log = open(tmp_path / "figs" / "loss" / f"{name}_logs.txt").read()
    assert "Num train batches: 4" in log and "Num test batches: 1" in log  # 160 train / 40 test samples at 48
    assert log.count("\tTest loss: ") == 2 and log.count("\tTrain loss: ") == 2
    losses = [float(x.split(": ")[1]) for x in log.splitlines() if "loss: " in x]
    assert all(np.isfinite(v) and v > 0 for v in losses)
