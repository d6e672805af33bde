"""Miniworld training CLI — the miniworld branch of the reference train.py (train.py:155-250 with the
epoch loops of :261-331): the flags of common_args, the 5000-env shard files, image_size 25, batches
of 64, ``AdamW(lr, weight_decay=1e-4)``, the same log file and log lines, checkpoint schedule and loss
plot.

The datasets are the reference's: shard pickles plus per-trajectory ``.npy`` image stacks collected
elsewhere (the Miniworld environment itself is out of scope).  The model is
``models.net.ImageTransformer`` on the autograd path: each batch runs the HIP image front end and the
trunk's training kernels forward and backward (dpt_hip.train.ImageTransformerFunction), and
``torch.optim.AdamW`` steps the module's parameters.  ``--workers`` (default 16, the reference's
``num_workers``) sets the loader's worker processes; 0 loads in the main process.

``--fused`` (opt-in) runs each batch as one fused device step instead (dpt_hip.train.ImageTrainer ->
dpt_image_train_step): both datasets are read once into device-resident, device-normalised image sets
(dpt_hip.train.DeviceImageData), the loader only yields sample indices (and the per-sample context
permutations with ``--shuffle``) drawn from the CPU generator as the default path's loader draws them,
AdamW runs on the device, and the loss is summed there and read once per epoch pass.  Checkpoints are
the module's state_dict after ``ImageTrainer.sync_to_model()``.  Log lines, file names and the
checkpoint schedule are the same.
"""
import argparse
import os
import time

import numpy as np
import torch

import common_args
from dataset import ImageDataset, image_transform
from models.net import ImageTransformer
from train_common import LossLog, run_epoch, set_seeds
from utils import build_miniworld_data_filename, build_miniworld_model_filename, worker_init_fn

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")


def _epoch_loss(model, loader, loss_fn, action_dim, horizon, optimizer=None):
    """One pass over ``loader`` (train.py:265-278 without an optimizer, :290-304 with one) -> the summed
    loss / horizon."""
    total = 0.0
    for i, batch in enumerate(loader):
        print(f"Batch {i} of {len(loader)}", end="\r")
        batch = {k: v.to(device) for k, v in batch.items()}
        pred_actions = model(batch)
        true_actions = batch["optimal_actions"].unsqueeze(1).repeat(1, pred_actions.shape[1], 1)
        true_actions = true_actions.reshape(-1, action_dim)
        pred_actions = pred_actions.reshape(-1, action_dim)
        if optimizer is not None:
            optimizer.zero_grad()
        loss = loss_fn(pred_actions, true_actions)
        if optimizer is not None:
            loss.backward()
            optimizer.step()
        total += loss.item() / horizon
    return total


def main(argv=None):
    os.makedirs("figs/loss", exist_ok=True)
    os.makedirs("trained_models", exist_ok=True)

    parser = argparse.ArgumentParser()
    common_args.add_dataset_args(parser)
    common_args.add_model_args(parser)
    common_args.add_train_args(parser)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--workers", type=int, default=16,
                        help="DataLoader worker processes (0: none); ignored with --fused, whose index loader "
                             "runs in the main process")
    parser.add_argument("--fused", action="store_true",
                        help="one fused device step per batch on a device-resident image set (dpt_image_train_step)")
    args = vars(parser.parse_args(argv))
    print("Args: ", args)

    env = args["env"]
    if env != "miniworld":
        raise NotImplementedError(f"{env}: train_miniworld.py trains --env miniworld (train.py trains the others)")
    n_envs, horizon, dim = args["envs"], args["H"], args["dim"]
    lr, shuffle, seed = args["lr"], args["shuffle"], args["seed"]
    state_dim, action_dim = 2, 4  # the direction vector (no position), four actions

    set_seeds(0 if seed == -1 else seed)

    dataset_config = {"n_hists": args["hists"], "n_samples": args["samples"], "horizon": horizon, "dim": dim,
                      "rollin_type": "uniform"}
    model_config = {"shuffle": shuffle, "lr": lr, "dropout": args["dropout"], "n_embd": args["embd"],
                    "n_layer": args["layer"], "n_head": args["head"], "n_envs": n_envs, "n_hists": args["hists"],
                    "n_samples": args["samples"], "horizon": horizon, "dim": dim, "seed": seed}
    increment = 5000
    paths_train, paths_test = [], []
    for start in np.arange(0, n_envs, increment):
        paths_train.append(build_miniworld_data_filename(env, start, start + increment - 1, dataset_config, mode=0))
        paths_test.append(build_miniworld_data_filename(env, start, start + increment - 1, dataset_config, mode=1))
    filename = build_miniworld_model_filename(env, model_config)
    print(f"Generate filename: {filename}")

    config = {"horizon": horizon, "state_dim": state_dim, "action_dim": action_dim, "n_layer": args["layer"],
              "n_embd": args["embd"], "n_head": args["head"], "shuffle": shuffle, "dropout": args["dropout"],
              "test": False, "store_gpu": False, "image_size": 25}
    model = ImageTransformer(config).to(device)

    printw = LossLog(filename)

    fused = args["fused"]
    params = {"batch_size": 64, "shuffle": True}
    if args["workers"] > 0 and not fused:
        params.update({"num_workers": args["workers"], "prefetch_factor": 2, "persistent_workers": True,
                       "pin_memory": True, "worker_init_fn": worker_init_fn})

    printw("Loading miniworld data...")
    train_dataset = ImageDataset(paths_train, config, image_transform)
    test_dataset = ImageDataset(paths_test, config, image_transform)
    printw("Done loading miniworld data")

    if fused:
        from dpt_hip.train import ImageTrainer
        trainer = ImageTrainer(model, lr=lr, weight_decay=1e-4)
        train_data, test_data = trainer.device_data(train_dataset), trainer.device_data(test_dataset)
        train_loader = torch.utils.data.DataLoader(train_dataset.index_view(), **params)
        test_loader = torch.utils.data.DataLoader(test_dataset.index_view(), **params)
    else:
        train_loader = torch.utils.data.DataLoader(train_dataset, **params)
        test_loader = torch.utils.data.DataLoader(test_dataset, **params)
        optimizer = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=1e-4)
        loss_fn = torch.nn.CrossEntropyLoss(reduction="sum")

    def state_dict():
        return (trainer.sync_to_model() if fused else model).state_dict()

    test_loss, train_loss = [], []
    printw("Num train batches: " + str(len(train_loader)))
    printw("Num test batches: " + str(len(test_loader)))

    for epoch in range(args["num_epochs"]):
        printw(f"Epoch: {epoch + 1}")
        start_time = time.time()
        if fused:
            total = run_epoch(trainer, trainer.eval_loss, test_data, test_loader) / horizon
        else:
            with torch.no_grad():
                total = _epoch_loss(model, test_loader, loss_fn, action_dim, horizon)
        test_loss.append(total / len(test_dataset))
        printw(f"\tTest loss: {test_loss[-1]}")
        printw(f"\tEval time: {time.time() - start_time}")

        start_time = time.time()
        if fused:
            total = run_epoch(trainer, trainer.step, train_data, train_loader) / horizon
        else:
            total = _epoch_loss(model, train_loader, loss_fn, action_dim, horizon, optimizer)
        train_loss.append(total / len(train_dataset))
        printw(f"\tTrain loss: {train_loss[-1]}")
        printw(f"\tTrain time: {time.time() - start_time}")

        if (epoch + 1) % 50 == 0:
            torch.save(state_dict(), f"trained_models/{filename}_epoch{epoch + 1}.pt")

        printw.report(epoch, test_loss, train_loss)

    torch.save(state_dict(), f"trained_models/{filename}.pt")
    print("Done.")


if __name__ == "__main__":
    main()
