#!/usr/bin/env python3
"""A/B of one miniworld training step: today's loader-fed autograd path, the same step on a batch that
already sits on the device, and the fused device step, in one process.

Arm "loader": what train_miniworld.py runs without --fused -- ``_epoch_loss`` over a shuffled
``DataLoader`` on the ``ImageDataset`` (each item loads its ``.npy`` stack and runs ``image_transform``
per image; ``--workers`` worker processes, pinned batches), the batch copied to the device, the module's
forward, torch's summed cross-entropy, ``backward()``, ``torch.optim.AdamW`` and ``loss.item()`` every
batch.  One round is ``--epochs`` passes over the set.
Arm "device_batch": the same step without the loader, on a batch already on the device.
Arm "fused": ``ImageTrainer.step`` (dpt_image_train_step on the ``DeviceImageData`` set) with a fresh host
index batch and context permutations uploaded every step, the loss read once per round.

Shape: batch 64, window 51, width 32, four layers, state_dim 2, action_dim 4, on a synthetic set of
``--samples`` trajectories written to a temporary directory.  The arms warm up, then alternate over
``--rounds`` rounds; every round starts and ends in a device synchronise and is timed with the host
clock.  The spread of an arm is (max - min) / median of its round times; a difference between two arms
counts only where it exceeds the spread of both.

Writes one JSON document (default profiles/image_step/ab.json).  Needs the GPU: there is no CPU fallback.
"""
import argparse
import contextlib
import copy
import io
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "decision-pretrained-transformer_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SD, A = 2, 4


def write_dataset(root, n, H, seed=0):
    """``n`` synthetic trajectories as train_miniworld.py reads them: one pickle plus a float64 .npy stack
    of (H, 25, 25, 3) raw images in [0, 1] per trajectory"""
    rs = np.random.RandomState(seed)
    trajs = []
    for i in range(n):
        path = os.path.join(root, f"img_{i}.npy")
        np.save(path, rs.uniform(0, 1, (H, 25, 25, 3)))
        trajs.append({"query_image": rs.uniform(0, 1, (25, 25, 3)), "query_state": rs.normal(size=SD),
                      "context_images": path, "context_states": rs.normal(size=(H, SD)),
                      "context_actions": np.eye(A)[rs.randint(0, A, H)],
                      "context_next_states": rs.normal(size=(H, SD)), "context_rewards": rs.normal(size=H),
                      "optimal_action": np.eye(A)[rs.randint(0, A)]})
    pkl = os.path.join(root, "trajs.pkl")
    with open(pkl, "wb") as f:
        pickle.dump(trajs, f)
    return pkl


def summary(times, steps):
    per_step = [t / steps * 1e3 for t in times]
    med = statistics.median(per_step)
    return {"ms_per_step_rounds": [round(x, 3) for x in per_step], "ms_per_step_median": round(med, 3),
            "spread": round((max(per_step) - min(per_step)) / med, 4), "timed_steps": steps * len(times)}


def compare(res, slow, fast):
    """ratio fast / slow of the medians, and whether the difference exceeds both arms' spreads"""
    s, f = res[slow]["ms_per_step_median"], res[fast]["ms_per_step_median"]
    gap = abs(s - f) / min(s, f)
    exceeds = bool(gap > res[slow]["spread"] and gap > res[fast]["spread"])
    return {"ratio": round(f / s, 4), "difference_exceeds_both_spreads": exceeds,
            f"{fast}_is_faster": bool(f < s and exceeds)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed round of the two device arms")
    ap.add_argument("--epochs", type=int, default=6, help="passes over the set per timed round of the loader arm")
    ap.add_argument("--rounds", type=int, default=4, help="alternating rounds per arm")
    ap.add_argument("--warmup", type=int, default=300,
                    help="untimed steps per device arm first (the loader arm: one pass); with 30 the autograd arm was "
                         "still speeding up over the timed rounds")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--workers", type=int, default=8,
                    help="the loader arm's worker processes (at most 8: they are forked from a process that holds "
                         "the GPU)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--layer", type=int, default=4)
    ap.add_argument("--embd", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_step", "ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_step_ab.py measures on the GPU; none is visible")
    if not 0 <= args.workers <= 8:
        raise SystemExit("--workers must be within 0..8")
    import dpt_hip
    import train_miniworld
    from dataset import ImageDataset, image_transform
    from dpt_hip.train import DeviceImageData, ImageTrainer
    from models.net import ImageTransformer
    from utils import worker_init_fn
    dev = dpt_hip.device()
    B, H, n = args.batch, args.H, args.samples
    cfg = dict(horizon=H, state_dim=SD, action_dim=A, n_layer=args.layer, n_embd=args.embd, n_head=4, shuffle=True,
               dropout=0.0, test=False, store_gpu=False, image_size=25)
    torch.manual_seed(0)
    loader_model = ImageTransformer(cfg).to(dev).train()
    batch_model, fused_model = copy.deepcopy(loader_model), copy.deepcopy(loader_model)
    loss_fn = torch.nn.CrossEntropyLoss(reduction="sum")

    with tempfile.TemporaryDirectory() as tmp:
        dataset = ImageDataset([write_dataset(tmp, n, H)], dict(cfg), image_transform)
        params = {"batch_size": B, "shuffle": True}
        if args.workers > 0:
            params.update({"num_workers": args.workers, "prefetch_factor": 2, "persistent_workers": True,
                           "pin_memory": True, "worker_init_fn": worker_init_fn})
        loader = torch.utils.data.DataLoader(dataset, **params)
        opt_a = torch.optim.AdamW(loader_model.parameters(), lr=1e-3, weight_decay=1e-4)

        def arm_loader(epochs):
            with contextlib.redirect_stdout(io.StringIO()):  # _epoch_loss's per-batch progress line
                for _ in range(epochs):
                    train_miniworld._epoch_loss(loader_model, loader, loss_fn, A, H, opt_a)
            return epochs * len(loader)

        dataset.shuffle = False  # the device batch: samples 0..B-1 in their stored order (compared with the fused arm below)
        batch = {k: v.to(dev) for k, v in next(iter(torch.utils.data.DataLoader(dataset, batch_size=B))).items()}
        dataset.shuffle = True
        true = batch["optimal_actions"].unsqueeze(1).repeat(1, H, 1).reshape(-1, A)
        opt_b = torch.optim.AdamW(batch_model.parameters(), lr=1e-3, weight_decay=1e-4)

        def arm_device_batch(k):
            for _ in range(k):
                pred = batch_model(batch)
                opt_b.zero_grad()
                loss = loss_fn(pred.reshape(-1, A), true)
                loss.backward()
                opt_b.step()
                loss.item()  # the per-batch synchronisation of _epoch_loss
            return k

        t0 = time.perf_counter()
        dd = DeviceImageData(dataset)
        torch.cuda.synchronize()
        load_s = time.perf_counter() - t0
        trainer = ImageTrainer(fused_model, lr=1e-3, weight_decay=1e-4)
        rs = np.random.RandomState(1)
        plans = [(torch.from_numpy(rs.randint(0, n, B)), torch.stack([torch.randperm(H) for _ in range(B)]))
                 for _ in range(args.steps)]  # host index batches and permutations, uploaded by every step

        def arm_fused(k):
            for i in range(k):
                trainer.step(dd, *plans[i % len(plans)])
            trainer.read_loss()
            return k

        # the device-batch arm and the fused arm compute the same step: compare one loss before timing
        with torch.no_grad():
            ref = loss_fn(batch_model(batch).reshape(-1, A), true).item()
        trainer.eval_loss(dd, torch.arange(B), torch.arange(H).repeat(B, 1))
        agree = abs(trainer.read_loss() - ref) / abs(ref)

        arms = {"loader": (arm_loader, args.epochs), "device_batch": (arm_device_batch, args.steps),
                "fused": (arm_fused, args.steps)}
        arm_loader(1)
        arm_device_batch(args.warmup)
        arm_fused(args.warmup)
        torch.cuda.synchronize()
        times, steps = {a: [] for a in arms}, {}
        for _ in range(args.rounds):
            for a, (fn, k) in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps[a] = fn(k)
                torch.cuda.synchronize()
                times[a].append(time.perf_counter() - t0)
        del loader  # ends the persistent workers before the temporary directory goes

    res = {"device": torch.cuda.get_device_name(0), "batch": B, "window": H + 1, "images_per_step": B * (H + 1),
           "n_embd": args.embd, "n_layer": args.layer, "state_dim": SD, "action_dim": A, "samples": n,
           "loader_workers": args.workers, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "host clock around each round, device synchronise before and after; rounds alternate arms",
           "arms": {"loader": "train_miniworld._epoch_loss over the DataLoader (npy loads, image_transform, collate, "
                              "pinned copy, module forward, torch CE, backward, torch.optim.AdamW, loss.item())",
                    "device_batch": "the same step on a batch already on the device",
                    "fused": "ImageTrainer.step with the index and permutation upload; loss read once per round"},
           "resident_set_load_seconds": round(load_s, 3), "resident_set_bytes": dd.image_bytes,
           "eval_loss_disagreement_fused_vs_module": agree}
    res.update({a: summary(t, steps[a]) for a, t in times.items()})
    res["fused_over_loader"] = compare(res, "loader", "fused")
    res["fused_over_device_batch"] = compare(res, "device_batch", "fused")
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
