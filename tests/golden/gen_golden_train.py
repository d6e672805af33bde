"""Generate tests/golden/train_loader.npz by running the REFERENCE's dataset.py.

Test infrastructure only (as gen_golden.py): imports the reference checkout at generation time and
records data, never code.  Two tiny synthetic trajectory lists in collect_data.py's pickle format
are written to a temporary directory, loaded through the reference ``Dataset``, and iterated with
the reference's loader settings (train.py:201-204,249: ``DataLoader(batch_size=8, shuffle=True)``)
for two epochs under ``torch.manual_seed``, with the dataset's ``shuffle`` off and on.  Recorded:
the trajectories, every batch tensor of every epoch, and every item of one pass over
``Dataset.__getitem__`` under a second seed.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_train.py <reference checkout>
"""
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

sys.dont_write_bytecode = True  # never leave __pycache__ in the reference tree

OUT = os.path.dirname(os.path.abspath(__file__))
LOADER_SEED, ITEM_SEED, EPOCHS, BATCH = 1234, 77, 2, 8
TRAJ_KEYS = ("context_states", "context_actions", "context_next_states", "context_rewards", "query_state",
             "optimal_action")
ITEM_KEYS = ("context_states", "context_actions", "context_next_states", "context_rewards", "query_states",
             "optimal_actions", "zeros")


def bandit_like(rs, n=20, H=7, A=5):
    """bandit trajectories (collect_data.py:158-182): unit states, one-hot arms, float rewards"""
    return [{"context_states": np.ones((H, 1)), "context_actions": np.eye(A)[rs.randint(0, A, H)],
             "context_next_states": np.ones((H, 1)), "context_rewards": rs.normal(0.5, 0.3, H),
             "query_state": np.array([1.0]), "optimal_action": np.eye(A)[rs.randint(0, A)]} for _ in range(n)]


def darkroom_like(rs, n=19, H=7, A=5, dim=10):
    """darkroom trajectories (collect_data.py:189-218): integer grid states, 1-D integer rewards"""
    return [{"context_states": rs.randint(0, dim, (H, 2)), "context_actions": np.eye(A)[rs.randint(0, A, H)],
             "context_next_states": rs.randint(0, dim, (H, 2)), "context_rewards": rs.randint(0, 2, H),
             "query_state": rs.randint(0, dim, 2), "optimal_action": np.eye(A)[rs.randint(0, A)]}
            for _ in range(n)]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DPT_REFERENCE", "")
    if not os.path.isfile(os.path.join(ref, "dataset.py")):
        raise SystemExit("usage: gen_golden_train.py <reference checkout> (the directory holding dataset.py)")
    sys.path[:0] = [ref]
    from dataset import Dataset  # the reference's

    rs = np.random.RandomState(20240)
    out = {"loader_seed": np.int64(LOADER_SEED), "item_seed": np.int64(ITEM_SEED), "batch_size": np.int64(BATCH)}
    sets = {"bandit": (bandit_like(rs), 1, 5), "darkroom": (darkroom_like(rs), 2, 5)}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (trajs, sd, A) in sets.items():
            path = os.path.join(tmp, name + ".pkl")
            with open(path, "wb") as f:
                pickle.dump(trajs, f)
            H = trajs[0]["context_states"].shape[0]
            out[f"{name}/cfg"] = np.array([len(trajs), H, sd, A], np.int64)
            for k in TRAJ_KEYS:
                out[f"{name}/traj/{k}"] = np.stack([t[k] for t in trajs])
            for shuffle in (0, 1):
                ds = Dataset(path, {"shuffle": bool(shuffle), "horizon": H, "store_gpu": False, "state_dim": sd,
                                    "action_dim": A})
                torch.manual_seed(LOADER_SEED)
                loader = torch.utils.data.DataLoader(ds, batch_size=BATCH, shuffle=True)
                for e in range(EPOCHS):
                    for b, batch in enumerate(loader):
                        for k in ITEM_KEYS:
                            out[f"{name}/shuf{shuffle}/e{e}/b{b}/{k}"] = batch[k].numpy()
                out[f"{name}/shuf{shuffle}/batches"] = np.int64(len(loader))
                torch.manual_seed(ITEM_SEED)
                for i in range(len(ds)):
                    item = ds[i]
                    for k in ITEM_KEYS:
                        out[f"{name}/shuf{shuffle}/item{i}/{k}"] = item[k].numpy()
    np.savez_compressed(os.path.join(OUT, "train_loader.npz"), **out)
    print(f"train_loader.npz: {len(out)} arrays")


if __name__ == "__main__":
    main()
