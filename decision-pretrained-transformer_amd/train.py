"""Training CLI — drop-in for the reference train.py (same flags, seeding, file names, log file and
log lines, checkpoint schedule and loss plot).

The epoch loops are the reference's (train.py:261-331): a test loss over the test set in training
mode, then one AdamW step per batch of 64 from a shuffled ``DataLoader``.  Each batch is one fused
device step (dpt_hip.train.Trainer -> dpt_train_step): the loader only yields sample indices (and
the per-sample context permutations with ``--shuffle``), drawn from the CPU generator as the
reference's loader draws them, the samples are gathered on the device, and the loss is summed
there and read once per epoch.  Checkpoints are the module's state_dict after
``Trainer.sync_to_model()``; eval.py loads them as it loads the reference's.
"""
import argparse
import os
import time

import torch

import common_args
from dataset import Dataset
from dpt_hip.train import Trainer
from models.net import Transformer
from train_common import LossLog, run_epoch, set_seeds
from utils import (build_bandit_data_filename, build_bandit_model_filename,
                   build_darkroom_data_filename, build_darkroom_model_filename,
                   build_linear_bandit_data_filename, build_linear_bandit_model_filename)

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")


def main(argv=None):
    os.makedirs("figs/loss", exist_ok=True)
    os.makedirs("trained_models", exist_ok=True)

    parser = argparse.ArgumentParser()
    common_args.add_dataset_args(parser)
    common_args.add_model_args(parser)
    common_args.add_train_args(parser)
    parser.add_argument("--seed", type=int, default=0)
    args = vars(parser.parse_args(argv))
    print("Args: ", args)

    env, n_envs, horizon, dim = args["env"], args["envs"], args["H"], args["dim"]
    state_dim, action_dim = dim, dim
    lr, shuffle, seed = args["lr"], args["shuffle"], args["seed"]
    var, cov, lin_d = args["var"], args["cov"], args["lin_d"]

    set_seeds(0 if seed == -1 else seed)

    if shuffle and env == "linear_bandit":
        raise Exception("Are you sure you want to shuffle on the linear bandit? Data collected from an adaptive "
                        "algorithm in a stochastic setting can bias the learner if shuffled.")

    dataset_config = {"n_hists": args["hists"], "n_samples": args["samples"], "horizon": horizon, "dim": dim}
    model_config = {"shuffle": shuffle, "lr": lr, "dropout": args["dropout"], "n_embd": args["embd"],
                    "n_layer": args["layer"], "n_head": args["head"], "n_envs": n_envs, "n_hists": args["hists"],
                    "n_samples": args["samples"], "horizon": horizon, "dim": dim, "seed": seed}
    if env in ("bandit", "bandit_thompson"):
        state_dim = 1
        dataset_config.update({"var": var, "cov": cov, "type": "uniform" if env == "bandit" else "bernoulli"})
        data_name, model_name = build_bandit_data_filename, build_bandit_model_filename
        model_config.update({"var": var, "cov": cov})
    elif env == "linear_bandit":
        state_dim = 1
        dataset_config.update({"lin_d": lin_d, "var": var, "cov": cov})
        data_name, model_name = build_linear_bandit_data_filename, build_linear_bandit_model_filename
        model_config.update({"lin_d": lin_d, "var": var, "cov": cov})
    elif env.startswith("darkroom"):
        state_dim, action_dim = 2, 5
        dataset_config.update({"rollin_type": "uniform"})
        data_name, model_name = build_darkroom_data_filename, build_darkroom_model_filename
    else:
        raise NotImplementedError(f"{env} (miniworld trains with train_miniworld.py)")
    path_train = data_name(env, n_envs, dataset_config, mode=0)
    path_test = data_name(env, n_envs, dataset_config, mode=1)
    filename = model_name(env, model_config)

    config = {"horizon": horizon, "state_dim": state_dim, "action_dim": action_dim, "n_layer": args["layer"],
              "n_embd": args["embd"], "n_head": args["head"], "shuffle": shuffle, "dropout": args["dropout"],
              "test": False, "store_gpu": True}
    model = Transformer(config).to(device)

    printw = LossLog(filename)

    train_dataset = Dataset(path_train, config)
    test_dataset = Dataset(path_test, config)
    params = {"batch_size": 64, "shuffle": True}
    train_loader = torch.utils.data.DataLoader(train_dataset.index_view(), **params)
    test_loader = torch.utils.data.DataLoader(test_dataset.index_view(), **params)

    trainer = Trainer(model, lr=lr, weight_decay=1e-4)
    train_data, test_data = trainer.device_data(train_dataset), trainer.device_data(test_dataset)

    test_loss, train_loss = [], []
    printw("Num train batches: " + str(len(train_loader)))
    printw("Num test batches: " + str(len(test_loader)))

    for epoch in range(args["num_epochs"]):
        printw(f"Epoch: {epoch + 1}")
        start_time = time.time()
        total = run_epoch(trainer, trainer.eval_loss, test_data, test_loader)
        test_loss.append(total / horizon / len(test_dataset))
        printw(f"\tTest loss: {test_loss[-1]}")
        printw(f"\tEval time: {time.time() - start_time}")

        start_time = time.time()
        total = run_epoch(trainer, trainer.step, train_data, train_loader)
        train_loss.append(total / horizon / len(train_dataset))
        printw(f"\tTrain loss: {train_loss[-1]}")
        printw(f"\tTrain time: {time.time() - start_time}")

        if (epoch + 1) % 50 == 0 or (env == "linear_bandit" and (epoch + 1) % 10 == 0):
            torch.save(trainer.sync_to_model().state_dict(), f"trained_models/{filename}_epoch{epoch + 1}.pt")

        printw.report(epoch, test_loss, train_loss)

    torch.save(trainer.sync_to_model().state_dict(), f"trained_models/{filename}.pt")
    print("Done.")


if __name__ == "__main__":
    main()
