"""Training datasets — drop-in for the reference dataset.py:11-91 ``Dataset``.

Same constructor (``path`` or list of paths of collect_data.py pickles, config keys ``shuffle``,
``horizon``, ``store_gpu``, ``state_dim``, ``action_dim``), the same ``.dataset`` dict of fp32
tensors, ``.zeros``, ``__len__`` and ``__getitem__`` (with ``shuffle`` the item's context is
permuted by one ``torch.randperm(horizon)``).

``IndexView`` is what train.py iterates: its items are the sample index alone, or
``(index, torch.randperm(horizon))`` with ``shuffle``, so a ``DataLoader`` over it draws from the
CPU generator exactly what a loader over the ``Dataset`` draws (the sampler's order, then one
permutation per item in batch order) while the samples themselves stay on the device, where
dpt_train_pack_batch gathers them.

``ImageDataset`` is the reference's dataset.py:94-145 for image-based (miniworld) data collected
elsewhere: the same constructor and item dict, each item's ``context_images`` read from its ``.npy``
stack, and ``image_transform`` restating the reference's ``ToTensor`` + ``Normalize`` pair.
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


_IMAGE_MEAN = (0.485, 0.456, 0.406)  # train.py:224-228: the ImageNet statistics
_IMAGE_STD = (0.229, 0.224, 0.225)


def image_transform(pic):
    """train.py:224-228 ``Compose([ToTensor(), Normalize(mean, std)])`` for the float HWC arrays in
    [0, 1] the collected data holds (``skimage.resize`` output): ``ToTensor`` only permutes a float
    array to CHW, ``Normalize`` computes (x - mean) / std in the array's own dtype (float64)."""
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(pic).transpose(2, 0, 1)))
    if not t.is_floating_point():
        raise TypeError("image_transform: expected a float image in [0, 1]")
    mean = torch.as_tensor(_IMAGE_MEAN, dtype=t.dtype)[:, None, None]
    std = torch.as_tensor(_IMAGE_STD, dtype=t.dtype)[:, None, None]
    return (t - mean) / std


class ImageDataset(Dataset):
    """Dataset class for image-based data (dataset.py:94-145)."""

    def __init__(self, paths, config, transform=image_transform):
        config["store_gpu"] = False
        super().__init__(paths, config)
        self.transform = transform
        self.config = config
        self.dataset.update({
            "context_filepaths": [traj["context_images"] for traj in self.trajs],
            "query_images": torch.stack([self.transform(traj["query_image"]).float() for traj in self.trajs]),
        })

    def __getitem__(self, index):
        context_images = np.load(self.dataset["context_filepaths"][index])
        context_images = torch.stack([self.transform(images) for images in context_images]).float()
        res = {"context_images": context_images}
        res.update({k: self.dataset[k][index] for k in _CONTEXT})
        res.update({"query_images": self.dataset["query_images"][index],
                    "query_states": self.dataset["query_states"][index],
                    "optimal_actions": self.dataset["optimal_actions"][index], "zeros": self.zeros})
        if self.shuffle:
            perm = torch.randperm(self.horizon)
            for k in ("context_images",) + _CONTEXT:
                res[k] = res[k][perm]
        return res
