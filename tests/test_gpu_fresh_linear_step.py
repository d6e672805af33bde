"""The linear bandit's fresh-task training step on the device (dpt_fresh_linear_step /
dpt_fresh_linear_eval_loss through dpt_hip.train.FreshTrainer on ``FreshEnv.linear_bandit``; train_fresh.py
--data_type) at 5 arms, 2 features, H 9, batch 8, 2 layers, widths 32 and 18:

- three ``FreshTrainer.step`` calls (8, 8, then 5 samples: a smaller last batch on the larger workspace) leave
  blob, m, v and the loss accumulator bit-identical to three ``Trainer.step`` calls on ``fresh_dataset`` of the
  same tasks in identity index order, once under dropout 0.1 with equal dropout seeds; ``eval_loss`` matches
  in the same way and regenerates the same loss twice;
- train_fresh.py --env linear_bandit with either --data_type writes train.py's file names (with lin_d, var,
  cov), and eval.py's loader takes the checkpoint.
"""
import copy
import importlib
import os

import numpy as np
import pytest
import torch

import fresh_linear_oracle as LO
from test_gpu_fresh_step import assert_same, state_bytes

pytestmark = pytest.mark.gpu

A, D, H, B, L = 5, 2, 9, 8, 2
SEED = 4712


def make_env(rollin):
    import dpt_hip
    return dpt_hip.FreshEnv.linear_bandit(LO.arms_of(A, D), H, 0.3, rollin)


def make_model(env, E, dropout=0.0, seed=7):
    from models.net import Transformer
    torch.manual_seed(seed)
    m = Transformer(dict(horizon=env.H, state_dim=env.state_dim, action_dim=env.action_dim, n_layer=L, n_embd=E,
                         n_head=1, dropout=dropout, test=False))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return m.cuda().train()


@pytest.mark.parametrize("rollin,E,dropout", [("thompson", 32, 0.0), ("thompson", 18, 0.0), ("thompson", 32, 0.1),
                                              ("uniform", 32, 0.0), ("uniform", 18, 0.1)])
def test_fresh_steps_equal_trainer_steps_on_the_materialised_tasks(rollin, E, dropout):
    from dpt_hip import train as tr
    env = make_env(rollin)
    model = make_model(env, E, dropout)
    fresh = tr.FreshTrainer(copy.deepcopy(model), env, lr=1e-3, seed=SEED)
    resident = tr.Trainer(copy.deepcopy(model), lr=1e-3)
    sizes, ds = (B, B, 5), [900, 901, 902]  # the third step with a smaller batch; one dropout seed per step
    data = tr.fresh_dataset(0, sum(sizes), env, SEED)
    assert data["context_actions"].shape == (sum(sizes), H, A) and data["context_states"].shape == (sum(sizes), H, 1)
    dd = resident.device_data(data)
    lo = 0
    for n, s in zip(sizes, ds):
        fresh.step(n, dropout_seed=s)
        resident._run(True, dd, torch.arange(lo, lo + n), None, seed=s)
        lo += n
        assert_same(state_bytes(fresh), state_bytes(resident))
    assert fresh.first_task == sum(sizes) and fresh.steps == resident.steps == 3
    assert fresh._ws_batch == B
    assert float(fresh.loss.item()) > 0
    assert fresh.read_loss() == resident.read_loss()  # reads and clears the accumulators
    # the test loss: other tasks, another key, chunks of 8 + 8 + 5
    test_dd = resident.device_data(tr.fresh_dataset(1000, 21, env, SEED + 1))
    fresh.eval_loss(1000, 21, seed=SEED + 1, batch=B, dropout_seed=903)
    for lo in (0, 8, 16):
        resident._run(False, test_dd, torch.arange(lo, min(lo + 8, 21)), None, seed=903)
    assert_same(state_bytes(fresh), state_bytes(resident))
    first = fresh.read_loss()
    assert first == resident.read_loss() > 0
    # nothing is stored: the same arguments regenerate the same samples and the same loss
    fresh.eval_loss(1000, 21, seed=SEED + 1, batch=B, dropout_seed=903)
    assert fresh.read_loss() == first
    for p, q in zip(fresh.sync_to_model().parameters(), resident.sync_to_model().parameters()):
        assert torch.equal(p, q)


def test_the_two_rollins_train_on_different_batches():
    from dpt_hip import train as tr
    th, un = (tr.fresh_dataset(0, 4, make_env(r), SEED) for r in ("thompson", "uniform"))
    assert torch.equal(th["optimal_actions"], un["optimal_actions"])
    assert not torch.equal(th["context_actions"], un["context_actions"])


@pytest.mark.parametrize("data_type", ["thompson", "uniform"])
def test_train_fresh_end_to_end(data_type, tmp_path, monkeypatch):
    from models.net import Transformer
    from utils import build_linear_bandit_model_filename
    train_fresh = importlib.import_module("train_fresh")
    ev = importlib.import_module("eval")
    monkeypatch.chdir(tmp_path)
    train_fresh.main(["--env", "linear_bandit", "--data_type", data_type, "--envs", "40", "--H", "9", "--dim", "5",
                      "--num_epochs", "1", "--layer", "2", "--var", "0.3", "--batch", "24"])
    cfg = {"shuffle": False, "lr": 1e-3, "dropout": 0, "n_embd": 32, "n_layer": 2, "n_head": 1, "n_envs": 40,
           "n_hists": 1, "n_samples": 1, "horizon": 9, "dim": 5, "seed": 0, "lin_d": 2, "var": 0.3, "cov": 0.0}
    name = build_linear_bandit_model_filename("linear_bandit", cfg)
    assert "_lind2" in name and "_var0.3" in name
    path = tmp_path / "trained_models" / f"{name}.pt"
    assert path.exists(), os.listdir(tmp_path / "trained_models")
    model = Transformer(dict(horizon=9, state_dim=1, action_dim=5, n_layer=2, n_embd=32, n_head=1, dropout=0,
                             test=True))
    ev.load_checkpoint(model, str(path))
    log = open(tmp_path / "figs" / "loss" / f"{name}_logs.txt").read()
    assert "Num train batches: 2" in log and "Num test batches: 1" in log  # 32 train / 8 test samples at 24
    assert log.count("\tTest loss: ") == 1 and log.count("\tTrain loss: ") == 1
    losses = [float(x.split(": ")[1]) for x in log.splitlines() if "loss: " in x]
    assert all(np.isfinite(v) and v > 0 for v in losses)
