#!/usr/bin/env python3
"""A/B of one training step: the autograd path against the fused device step, in one process.

Arm "parent": what train.py's step cost before the fused step existed -- Transformer.forward in
training mode (dpt_train_forward through TransformerFunction), torch's summed cross-entropy,
``loss.backward()`` (dpt_train_backward + the per-parameter gradient views),
``torch.optim.AdamW.step()`` and ``loss.item()`` every batch, on a batch that already sits on the
device.  Arm "fused": ``Trainer.step`` (dpt_train_step: device-side packing from the resident
dataset by a fresh index batch, forward, cross-entropy, backward, AdamW on the blob) with the loss
read once per timed round.

Shapes: the training shapes of BASELINE configs 2, 3 and 4 (batch 64, window 1 + H, width 32, four
layers).  Per shape both arms warm up, then run ``--rounds`` alternating rounds of ``--steps``
steps each (4 x 200 timed steps per arm by default); every round ends in a device synchronise and
is timed with the host clock.  The spread of an arm is (max - min) / median of its round times:
the difference between runs of the same code, which any difference between the arms has to exceed.

Writes one JSON document (default profiles/train_step/ab.json).  Needs the GPU: there is no CPU
fallback.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "decision-pretrained-transformer_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [  # name, state_dim, action_dim, horizon
    ("config2_bandit_H500", 1, 5, 500),
    ("config3_darkroom_H100", 2, 5, 100),
    ("config4_linear_bandit_H1000", 1, 20, 1000),
]
KEYS = ("query_states", "context_states", "context_actions", "context_next_states", "context_rewards")


def make_data(rs, n, H, sd, A):
    return {"query_states": torch.tensor(rs.randint(0, 10, (n, sd)), dtype=torch.float32),
            "context_states": torch.tensor(rs.randint(0, 10, (n, H, sd)), dtype=torch.float32),
            "context_actions": torch.tensor(np.eye(A)[rs.randint(0, A, (n, H))], dtype=torch.float32),
            "context_next_states": torch.tensor(rs.randint(0, 10, (n, H, sd)), dtype=torch.float32),
            "context_rewards": torch.tensor(rs.normal(0.5, 0.5, (n, H, 1)), dtype=torch.float32),
            "optimal_actions": torch.tensor(np.eye(A)[rs.randint(0, A, n)], dtype=torch.float32)}


def summary(times, steps):
    per_step = [t / steps * 1e3 for t in times]
    med = statistics.median(per_step)
    return {"ms_per_step_rounds": [round(x, 4) for x in per_step], "ms_per_step_median": round(med, 4),
            "spread": round((max(per_step) - min(per_step)) / med, 4), "timed_steps": steps * len(times)}


def run_shape(name, sd, A, H, args):
    from dpt_hip.train import Trainer
    from models.net import Transformer
    B = args.batch
    rs = np.random.RandomState(H)
    torch.manual_seed(H)
    model = Transformer(dict(horizon=H, state_dim=sd, action_dim=A, n_layer=args.layer, n_embd=args.embd, n_head=1,
                             dropout=0.0, test=False)).cuda().train()
    fused_model = copy.deepcopy(model)
    data = {k: v.cuda() for k, v in make_data(rs, 4 * B, H, sd, A).items()}
    batch = {k: data[k][:B].contiguous() for k in KEYS}
    true = data["optimal_actions"][:B].unsqueeze(1).repeat(1, H, 1).reshape(-1, A)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    loss_fn = torch.nn.CrossEntropyLoss(reduction="sum")
    trainer = Trainer(fused_model, lr=1e-3, weight_decay=1e-4)
    dd = trainer.device_data(data)
    plans = [torch.from_numpy(rs.randint(0, 4 * B, B)) for _ in range(args.steps)]  # host index batches

    def parent(k):
        total = 0.0
        for _ in range(k):
            pred = model(batch)
            opt.zero_grad()
            loss = loss_fn(pred.reshape(-1, A), true)
            loss.backward()
            opt.step()
            total += loss.item() / H
        return total

    def fused(k):
        for i in range(k):
            trainer.step(dd, plans[i % len(plans)])
        return trainer.read_loss() / H

    arms = {"parent": parent, "fused": fused}
    times = {a: [] for a in arms}
    for fn in arms.values():
        fn(args.warmup)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for a, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.steps)
            torch.cuda.synchronize()
            times[a].append(time.perf_counter() - t0)
    out = {a: summary(t, args.steps) for a, t in times.items()}
    out["window"] = 1 + H
    out["fused_over_parent"] = round(out["fused"]["ms_per_step_median"] / out["parent"]["ms_per_step_median"], 4)
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per timed round")
    ap.add_argument("--rounds", type=int, default=4, help="alternating rounds per arm")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--layer", type=int, default=4)
    ap.add_argument("--embd", type=int, default=32)
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step", "ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_step_ab.py measures on the GPU; none is visible")
    want = set(filter(None, args.shapes.split(",")))
    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "n_layer": args.layer, "n_embd": args.embd,
           "steps_per_round": args.steps, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "host clock around each round, device synchronise before and after; rounds alternate arms",
           "shapes": {}}
    for name, sd, A, H in SHAPES:
        if not want or name in want:
            res["shapes"][name] = run_shape(name, sd, A, H, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
