"""What the training CLIs share: the seeding block, the index-batch epoch on a fused trainer, and the
reference's loss log (train.py:206-219 and :313-327: the log file, the every-10-epochs report and the
loss plot)."""
import random

import numpy as np
import torch


def set_seeds(seed, cudnn=False):
    """Seed torch (host and devices), numpy and random; ``cudnn``: also the two cudnn flags the bandit
    CLIs' reference scripts set (the dataset CLIs' reference does not)."""
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
    if cudnn:
        torch.backends.cudnn.deterministic = True
        torch.backends.cudnn.benchmark = False
    np.random.seed(seed)
    random.seed(seed)


def run_epoch(trainer, call, data, loader):
    """One pass over ``loader`` (index batches, or (index, perm) batches) with ``call`` = the trainer's
    ``step`` or ``eval_loss`` -> the summed loss, read once at the end."""
    for i, batch in enumerate(loader):
        print(f"Batch {i} of {len(loader)}", end="\r")
        index, perm = batch if isinstance(batch, (list, tuple)) else (batch, None)
        call(data, index, perm)
    return trainer.read_loss()


class LossLog:
    """``log(line)`` prints the line and appends it to figs/loss/<filename>_logs.txt (emptied first)."""

    def __init__(self, filename):
        import matplotlib  # here, not at the top: the bandit CLIs import this module and plot nothing
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        self.plt, self.filename = plt, filename
        self.path = f"figs/loss/{filename}_logs.txt"
        with open(self.path, "w"):
            pass

    def __call__(self, string):
        print(string)
        with open(self.path, "a") as f:
            print(string, file=f)

    def report(self, epoch, test_loss, train_loss):
        """Every 10th epoch: the report lines and figs/loss/<filename>_train_loss.png."""
        if (epoch + 1) % 10 != 0:
            return
        self(f"Epoch: {epoch + 1}")
        self(f"Test Loss:        {test_loss[-1]}")
        self(f"Train Loss:       {train_loss[-1]}")
        self("\n")

        plt = self.plt
        plt.yscale("log")
        plt.plot(train_loss[1:], label="Train Loss")
        plt.plot(test_loss[1:], label="Test Loss")
        plt.legend()
        plt.savefig(f"figs/loss/{self.filename}_train_loss.png")
        plt.clf()
