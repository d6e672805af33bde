"""Generate tests/golden/image_transformer.npz by running the REFERENCE's ImageTransformer, ImageDataset
and miniworld filename builders on the CPU.

Test infrastructure only (as gen_golden.py, whose module stubs it installs): imports the reference
checkout at generation time and records data, never code.  Recorded:

* the weights of one ImageTransformer (L = 2, E = 32, H = 3, sd 2, A 4; every value fp32-representable,
  stored as fp32, without wte) and the key list of its state_dict;
* one batch of B = 2 (uniform-random images through the transform below), and the reference's float64
  preds[:, 1:], CrossEntropyLoss(sum) and every parameter's gradient (train.py:293-302);
* one ImageDataset item per trajectory of a two-trajectory synthetic pickle with ``.npy`` image stacks,
  with and without shuffle, under ``torch.manual_seed(ITEM_SEED)``, plus the trajectories themselves;
* the miniworld data / model filenames of one configuration.

torchvision is not installed where this runs, so train.py:224-228's ``ToTensor`` + ``Normalize`` pair is
restated in ``transform``: for a float HWC array ``ToTensor`` only permutes to CHW, ``Normalize``
computes (x - mean) / std in float64.  The seed of the batch is the first whose ReLU pre-activations
(tests/image_oracle.py) all lie RELU_MARGIN from zero.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_image.py <reference checkout>
"""
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

sys.dont_write_bytecode = True  # never leave __pycache__ in the reference tree

OUT = os.path.dirname(os.path.abspath(__file__))
L, E, H, B, SD, A = 2, 32, 3, 2, 2, 4
ITEM_SEED = 91
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def transform(pic):
    t = torch.from_numpy(np.ascontiguousarray(pic.transpose(2, 0, 1)))
    return (t - torch.tensor(MEAN, dtype=t.dtype)[:, None, None]) / torch.tensor(STD, dtype=t.dtype)[:, None, None]


def raw_images(rs, *lead):
    """float64 HWC images in [0, 1] whose values are fp32-representable (stored as fp32)"""
    return rs.uniform(0, 1, lead + (25, 25, 3)).astype(np.float32).astype(np.float64)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DPT_REFERENCE", "")
    if not os.path.isfile(os.path.join(ref, "models", "net.py")):
        raise SystemExit("usage: gen_golden_image.py <reference checkout> (the directory holding models/net.py)")
    sys.path[:0] = [OUT, os.path.dirname(OUT)]
    from gen_golden import _install_stubs
    import image_oracle as IO
    _install_stubs()
    sys.path[:0] = [ref, os.path.join(ref, "models")]
    from net import ImageTransformer  # the reference's
    from dataset import ImageDataset
    from utils import build_miniworld_data_filename, build_miniworld_model_filename

    out = {"cfg": np.array([L, E, H, B, SD, A], np.int64)}
    cfg = {"horizon": H, "state_dim": SD, "action_dim": A, "n_layer": L, "n_embd": E, "n_head": 1, "shuffle": False,
           "dropout": 0.0, "test": False, "store_gpu": False, "image_size": 25}
    torch.manual_seed(5)
    model = ImageTransformer(cfg)
    with torch.no_grad():  # move the GPT-2 part off its near-zero initialisation; the encoder keeps torch's
        for k, p in model.named_parameters():
            if not k.startswith("image_encoder") and not k.endswith("wte.weight"):
                p.add_(0.05 * torch.randn_like(p))
    w32 = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    out["keys"] = np.array(list(w32.keys()))
    for k, v in w32.items():
        if not k.endswith("wte.weight") and v.dtype == np.float32:
            out["w/" + k] = v
    w64 = {k[2:]: v.astype(np.float64) for k, v in out.items() if k.startswith("w/")}
    model = model.double()
    model.train()

    for seed in range(100):
        rs = np.random.RandomState(1000 + seed)
        batch = {"query_images": transform_batch(raw_images(rs, B)), "context_images": transform_batch(raw_images(rs, B, H)),
                 "query_states": rs.normal(size=(B, SD)), "context_states": rs.normal(size=(B, H, SD)),
                 "context_actions": np.eye(A)[rs.randint(0, A, (B, H))],
                 "context_rewards": rs.normal(0.2, 0.5, (B, H, 1)),
                 "optimal_actions": np.eye(A)[rs.randint(0, A, B)]}
        batch = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in batch.items()}
        loss_o, preds_o, grads_o, pre = IO.grads(w64, batch, L, A)
        if IO.relu_margin(pre) >= IO.RELU_MARGIN:
            break
    else:
        raise SystemExit("no seed with the ReLU margin")
    out["batch_seed"] = np.int64(1000 + seed)
    for k, v in batch.items():
        out["batch/" + k] = v.astype(np.float32)

    tb = {k: torch.tensor(v, dtype=torch.float64) for k, v in batch.items()}
    pred = model(tb)  # train.py:294
    true = tb["optimal_actions"].unsqueeze(1).repeat(1, pred.shape[1], 1)
    loss = torch.nn.CrossEntropyLoss(reduction="sum")(pred.reshape(-1, A), true.reshape(-1, A))
    loss.backward()
    out["loss"] = np.float64(loss.item())
    out["preds"] = pred.detach().numpy()
    for k, p in model.named_parameters():
        if p.grad is not None and not k.endswith("wte.weight"):
            out["grad/" + k] = p.grad.detach().numpy()
    assert set(k[5:] for k in out if k.startswith("grad/")) == set(w64), "a parameter without a gradient"
    print(f"reference loss {loss.item():.6f}; oracle loss {loss_o:.6f}; margin {IO.relu_margin(pre):.2e}")

    # ImageDataset items from a two-trajectory pickle
    rs = np.random.RandomState(77)
    with tempfile.TemporaryDirectory() as tmp:
        trajs = []
        for i in range(2):
            stack = raw_images(rs, H)
            path = os.path.join(tmp, f"traj{i}.npy")
            np.save(path, stack)
            trajs.append({"query_image": raw_images(rs), "query_state": rs.normal(size=SD), "context_images": path,
                          "context_states": rs.normal(size=(H, SD)), "context_actions": np.eye(A)[rs.randint(0, A, H)],
                          "context_next_states": rs.normal(size=(H, SD)), "context_rewards": rs.normal(size=H),
                          "optimal_action": np.eye(A)[rs.randint(0, A)]})
            out[f"data/{i}/context_images"] = stack.astype(np.float32)
            for k, v in trajs[-1].items():
                if k != "context_images":
                    out[f"data/{i}/{k}"] = np.asarray(v, np.float32 if k == "query_image" else np.float64)
        pkl = os.path.join(tmp, "trajs.pkl")
        with open(pkl, "wb") as f:
            pickle.dump(trajs, f)
        for shuffle in (0, 1):
            ds = ImageDataset([pkl], {"shuffle": bool(shuffle), "horizon": H, "store_gpu": False, "state_dim": SD,
                                      "action_dim": A}, transform)
            torch.manual_seed(ITEM_SEED)
            for i in range(len(ds)):
                for k, v in ds[i].items():
                    out[f"item/shuf{shuffle}/{i}/{k}"] = v.numpy()
    out["item_seed"] = np.int64(ITEM_SEED)

    dcfg = {"n_hists": 1, "n_samples": 1, "horizon": 50, "dim": 10, "rollin_type": "uniform"}
    mcfg = {"shuffle": True, "lr": 0.001, "dropout": 0.1, "n_embd": 32, "n_layer": 4, "n_head": 4, "n_envs": 60000,
            "n_hists": 1, "n_samples": 1, "horizon": 50, "dim": 10, "seed": 3}
    out["names/data"] = np.array([build_miniworld_data_filename("miniworld", 5000, 9999, dcfg, mode=m)
                                  for m in (0, 1, 2)])
    out["names/model"] = np.array(build_miniworld_model_filename("miniworld", mcfg))

    path = os.path.join(OUT, "image_transformer.npz")
    np.savez_compressed(path, **out)
    print(f"image_transformer.npz: {len(out)} arrays, {os.path.getsize(path)} bytes")


def transform_batch(raw):
    """``transform`` over the leading dims of (..., 25, 25, 3) -> (..., 3, 25, 25) float64"""
    flat = raw.reshape(-1, 25, 25, 3)
    return torch.stack([transform(x) for x in flat]).numpy().reshape(raw.shape[:-3] + (3, 25, 25))


if __name__ == "__main__":
    main()
