"""Pretraining on fresh tasks: train.py without collect_data.py, a dataset file or a resident dataset.

Every batch is generated on the device where the training step consumes it
(dpt_hip.train.FreshTrainer -> dpt_fresh_step): the task, the behaviour policy, the rollin with its
reward noise, the query state and the optimal-action label are Philox draws keyed by ``--seed`` and the
sample's global index, so each step sees tasks no earlier step saw and nothing is stored.

Flags: train.py's, plus ``--batch`` (default 64).  An epoch is ``int(0.8 * envs)`` fresh training samples;
the test loss is taken over ``envs - int(0.8 * envs)`` samples regenerated every epoch from a fixed key
distinct from the training key (``darkroom_heldout``: drawn from the 20 % of goals collect_data.py holds
out, the training samples from the other 80 %; any other ``darkroom*`` name: every goal for both).  The log
file, log lines, loss plot, checkpoint schedule and checkpoint names are train.py's, so eval.py with the same
flags loads the result -- and a train.py checkpoint with equal flags is overwritten.  ``--hists``,
``--samples`` and ``--shuffle`` only name the file: fresh tasks leave nothing to repeat, and the rollin
steps are i.i.d., so permuting them changes nothing in law.

``--env linear_bandit`` needs ``--data_type thompson`` or ``--data_type uniform`` (collect_data.py's two
data types; it collects 'thompson').  The two are different training distributions, hence the opt-in:
'thompson' is the adaptive Thompson-sampling rollin of collect_data.py run on the device inside the step
(equal to collect_data.py's in law, not bit for bit: the tasks are other draws), 'uniform' the bandit's i.i.d.
behaviour policy.  The arms are collect_data.py's (``RandomState(1234)``, ``--dim`` x ``--lin_d``), the file
names and the extra checkpoint every 10 epochs are train.py's, and ``--shuffle`` is refused as train.py refuses it.

``--bayes_floor`` (bandit, bandit_thompson, darkroom*, linear_bandit at lin_d 2): before epoch 1, the
irreducible floor of the printed test loss, ``E[-log P(a* | D_t)]`` averaged over t = 1 .. H of the test samples (the same every epoch) under
the exact Bayes posterior of the optimal action (dpt_hip.fresh_posterior; the DarkRoom prior is the list the
test samples are drawn from), printed and logged as one line ``\tBayes floor (test): ...``.  The test loss
minus this floor is the mean KL from the posterior to the model.  linear_bandit has it at ``--lin_d 2`` with
``--var`` > 0 (dpt_hip.linear_posterior: an angular quadrature, either ``--data_type``); otherwise it is refused:
P(arm optimal) under the Gaussian posterior over theta is a lin_d-dimensional integral with no cheap form.
Without the flag the log and every file are as before.
"""
import argparse
import hashlib
import os
import time

import numpy as np
import torch

import common_args
from dpt_hip import (FreshEnv, fresh_batch, fresh_posterior, linear_posterior_supported, posterior_compare,
                     posterior_grid)
from dpt_hip.train import FreshTrainer
from models.net import Transformer
from train_common import LossLog, set_seeds
from utils import build_bandit_model_filename, build_darkroom_model_filename, build_linear_bandit_model_filename

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")


def generator_key(seed, role):
    """The 64-bit Philox key of the ``role`` ('train' / 'test') samples of a run seeded ``seed``."""
    return int.from_bytes(hashlib.sha256(f"train_fresh/{role}/{seed}".encode()).digest()[:8], "little")


def darkroom_goals(env, dim):
    """(train goals, test goals) as (G, 2) arrays: collect_data.py's split for darkroom_heldout (the
    shuffled grid, the first 80 % for training), else the whole grid for both."""
    goals = np.array([[(j, i) for i in range(dim)] for j in range(dim)]).reshape(-1, 2)
    if env != "darkroom_heldout":
        return goals, goals
    np.random.RandomState(seed=0).shuffle(goals)
    split = int(.8 * len(goals))
    return goals[:split], goals[split:]


FLOOR_CHUNK = 2048  # test samples per posterior launch (post is (chunk, 1 + H, A) float64)


def bayes_floor(test_env, test_key, n_test, horizon):
    """sum_{t=1..H} -log P(a* | D_t) / H / n_test over the test samples 0 .. n_test - 1 of ``test_key``: the
    floor of the test loss main() prints (one host read at the end)."""
    total = torch.zeros((), dtype=torch.float64, device=device)
    for lo in range(0, n_test, FLOOR_CHUNK):
        batch = fresh_batch(test_env, test_key, lo, min(FLOOR_CHUNK, n_test - lo))
        post, targets = fresh_posterior(test_env, batch)
        nll = posterior_compare(post, torch.zeros(post.shape, dtype=torch.float32, device=post.device), targets)
        total += nll["nll_bayes"][:, 1:].sum()
    return float(total.item()) / horizon / max(n_test, 1)


def main(argv=None):
    parser = argparse.ArgumentParser()
    common_args.add_dataset_args(parser)
    common_args.add_model_args(parser)
    common_args.add_train_args(parser)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--batch", type=int, default=64)
    parser.add_argument("--data_type", choices=["thompson", "uniform"], default=None,
                        help="linear_bandit only: the rollin, collect_data.py's data types")
    parser.add_argument("--bayes_floor", action="store_true",
                        help="print the Bayes floor of the test loss before epoch 1 (bandit, bandit_thompson, darkroom*, "
                             "linear_bandit at --lin_d 2 and --var > 0)")
    args = vars(parser.parse_args(argv))
    print("Args: ", args)

    env, n_envs, horizon, dim = args["env"], args["envs"], args["H"], args["dim"]
    lr, shuffle, seed, batch = args["lr"], args["shuffle"], args["seed"], args["batch"]
    var, cov, lin_d, data_type = args["var"], args["cov"], args["lin_d"], args["data_type"]
    if env == "linear_bandit":
        if data_type is None:
            raise NotImplementedError("linear_bandit: collect_data.py's rollin is an adaptive Thompson run, not "
                                      "i.i.d. draws: a training distribution of its own.  Choose it with "
                                      "--data_type thompson (run on the device inside the step), or the i.i.d. "
                                      "--data_type uniform; or use collect_data.py and train.py")
        if shuffle:
            raise Exception("Are you sure you want to shuffle on the linear bandit? Data collected from an adaptive "
                            "algorithm in a stochastic setting can bias the learner if shuffled.")
    elif data_type is not None:
        raise ValueError(f"--data_type {data_type} belongs to --env linear_bandit, not to {env}")
    if batch < 1:
        raise ValueError(f"--batch {batch}")
    if args["bayes_floor"]:
        if env == "linear_bandit":
            why = linear_posterior_supported(lin_d, var)
            if why is not None:
                raise NotImplementedError(f"--bayes_floor: {why}; the floor also exists for bandit, bandit_thompson "
                                          "and darkroom*")
        if env in ("bandit", "bandit_thompson"):  # ValueError where the grid would under-resolve the posterior
            posterior_grid(var, horizon, "uniform" if env == "bandit" else "bernoulli")

    os.makedirs("figs/loss", exist_ok=True)
    os.makedirs("trained_models", exist_ok=True)
    set_seeds(0 if seed == -1 else seed)

    model_config = {"shuffle": shuffle, "lr": lr, "dropout": args["dropout"], "n_embd": args["embd"],
                    "n_layer": args["layer"], "n_head": args["head"], "n_envs": n_envs, "n_hists": args["hists"],
                    "n_samples": args["samples"], "horizon": horizon, "dim": dim, "seed": seed}
    if env in ("bandit", "bandit_thompson"):
        state_dim, action_dim = 1, dim
        model_config.update({"var": var, "cov": cov})
        filename = build_bandit_model_filename(env, model_config)
        train_env = test_env = FreshEnv.bandit(dim, horizon, var, "uniform" if env == "bandit" else "bernoulli")
    elif env == "linear_bandit":
        state_dim, action_dim = 1, dim
        model_config.update({"lin_d": lin_d, "var": var, "cov": cov})
        filename = build_linear_bandit_model_filename(env, model_config)
        arms = np.random.RandomState(seed=1234).normal(size=(dim, lin_d)) / np.sqrt(lin_d)  # collect_data.py's
        train_env = test_env = FreshEnv.linear_bandit(arms, horizon, var, data_type)
    elif env.startswith("darkroom"):
        state_dim, action_dim = 2, 5
        filename = build_darkroom_model_filename(env, model_config)
        train_goals, test_goals = darkroom_goals(env, dim)
        train_env = FreshEnv.darkroom(dim, horizon, train_goals)
        test_env = FreshEnv.darkroom(dim, horizon, test_goals)
    else:
        raise NotImplementedError(f"{env} (miniworld trains with train_miniworld.py)")

    config = {"horizon": horizon, "state_dim": state_dim, "action_dim": action_dim, "n_layer": args["layer"],
              "n_embd": args["embd"], "n_head": args["head"], "shuffle": shuffle, "dropout": args["dropout"],
              "test": False, "store_gpu": True}
    model = Transformer(config).to(device)

    printw = LossLog(filename)

    n_train = int(.8 * n_envs)
    n_test = n_envs - n_train
    train_key, test_key = generator_key(seed, "train"), generator_key(seed, "test")
    trainer = FreshTrainer(model, train_env, lr=lr, weight_decay=1e-4, seed=train_key)

    test_loss, train_loss = [], []
    printw("Num train batches: " + str(-(-n_train // batch)))
    printw("Num test batches: " + str(-(-n_test // batch)))
    if args["bayes_floor"]:
        printw(f"\tBayes floor (test): {bayes_floor(test_env, test_key, n_test, horizon)}")

    for epoch in range(args["num_epochs"]):
        printw(f"Epoch: {epoch + 1}")
        start_time = time.time()
        trainer.eval_loss(0, n_test, seed=test_key, env=test_env, batch=batch)
        test_loss.append(trainer.read_loss() / horizon / max(n_test, 1))
        printw(f"\tTest loss: {test_loss[-1]}")
        printw(f"\tEval time: {time.time() - start_time}")

        start_time = time.time()
        for lo in range(0, n_train, batch):
            trainer.step(min(batch, n_train - lo))
        train_loss.append(trainer.read_loss() / horizon / max(n_train, 1))
        printw(f"\tTrain loss: {train_loss[-1]}")
        printw(f"\tTrain time: {time.time() - start_time}")

        if (epoch + 1) % 50 == 0 or (env == "linear_bandit" and (epoch + 1) % 10 == 0):
            torch.save(trainer.sync_to_model().state_dict(), f"trained_models/{filename}_epoch{epoch + 1}.pt")

        printw.report(epoch, test_loss, train_loss)

    torch.save(trainer.sync_to_model().state_dict(), f"trained_models/{filename}.pt")
    print("Done.")


if __name__ == "__main__":
    main()
