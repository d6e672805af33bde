"""Training datasets — drop-in for the reference dataset.py:11-91 ``Dataset``.

Same constructor (``path`` or list of paths of collect_data.py pickles, config keys ``shuffle``,
``horizon``, ``store_gpu``, ``state_dim``, ``action_dim``), the same ``.dataset`` dict of fp32
tensors, ``.zeros``, ``__len__`` and ``__getitem__`` (with ``shuffle`` the item's context is
permuted by one ``torch.randperm(horizon)``).

``IndexView`` is what train.py iterates: its items are the sample index alone, or
``(index, torch.randperm(horizon))`` with ``shuffle``, so a ``DataLoader`` over it draws from the
CPU generator exactly what a loader over the ``Dataset`` draws (the sampler's order, then one
permutation per item in batch order) while the samples themselves stay on the device, where
dpt_train_pack_batch gathers them.  ImageDataset (miniworld) is out of scope.
"""
import pickle

import numpy as np
import torch

from utils import convert_to_tensor

_TRAJ_KEYS = (("context_states", "context_states"), ("context_actions", "context_actions"),
              ("context_next_states", "context_next_states"), ("context_rewards", "context_rewards"),
              ("query_states", "query_state"), ("optimal_actions", "optimal_action"))
_CONTEXT = ("context_states", "context_actions", "context_next_states", "context_rewards")


class Dataset(torch.utils.data.Dataset):
    """Dataset class (dataset.py:11-91)."""

    def __init__(self, path, config):
        self.shuffle = config["shuffle"]
        self.horizon = config["horizon"]
        self.store_gpu = config["store_gpu"]
        self.config = config

        self.trajs = []
        for p in path if isinstance(path, list) else [path]:
            with open(p, "rb") as f:  # our own pickles (collect_data.py output), as in the reference
                self.trajs += pickle.load(f)

        arrays = {key: np.array([traj[field] for traj in self.trajs]) for key, field in _TRAJ_KEYS}
        if arrays["context_rewards"].ndim < 3:
            arrays["context_rewards"] = arrays["context_rewards"][:, :, None]
        order = ("query_states", "optimal_actions") + _CONTEXT
        self.dataset = {k: convert_to_tensor(arrays[k], store_gpu=self.store_gpu) for k in order}
        self.zeros = convert_to_tensor(np.zeros(config["state_dim"] ** 2 + config["action_dim"] + 1),
                                       store_gpu=self.store_gpu)

    def __len__(self):
        return len(self.dataset["query_states"])

    def __getitem__(self, index):
        res = {k: self.dataset[k][index] for k in _CONTEXT + ("query_states", "optimal_actions")}
        res["zeros"] = self.zeros
        if self.shuffle:
            perm = torch.randperm(self.horizon)
            for k in _CONTEXT:
                res[k] = res[k][perm]
        return res

    def index_view(self):
        return IndexView(self)


class IndexView(torch.utils.data.Dataset):
    """Items name a sample instead of carrying it: ``index``, or ``(index, randperm(horizon))``
    when the dataset shuffles its contexts."""

    def __init__(self, dataset):
        self.dataset = dataset

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, index):
        if self.dataset.shuffle:
            return index, torch.randperm(self.dataset.horizon)
        return index
