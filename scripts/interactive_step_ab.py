#!/usr/bin/env python3
"""A/B of one interactive training episode: the plain per-step loop against the fused step, in one
process.

Arm "plain": ``train_interactive.interactive_step_plain`` -- a fresh GPUBanditEnv, K forwards of the
module over the growing window (the fused inference kernels without a graph for the K - 1 steps that
only sample, the training forward for the last), torch's Categorical sampling, the env kernel,
torch's CrossEntropyLoss, ``loss.backward()`` and ``torch.optim.AdamW.step()``.  Arm "fused": a
fresh GPUBanditEnv and ``InteractiveTrainer.step`` (dpt_interactive_grad: the y-cache rollout from
the blob, the window packed from its records, forward, last-position cross-entropy, backward; then
dpt_adamw_step) with the last block's c_proj, ln_2, MLP, then ln_f and the head run for the last row
of each sequence alone (DPT_TRAIN_LAST_LOSS).  Arm "fused_full_width": the same step with the last
block at full width (DPT_INTERACTIVE_FULL_WIDTH).  No arm reads the loss inside a timed round.

Shapes: 5 arms, width 32, four layers, 1024 envs, at K = 100 (the reference's default horizon) and
K = 500.  Per shape both arms warm up, then run ``--rounds`` alternating rounds of ``--steps``
episodes each; every round starts and ends in a device synchronise and is timed with the host
clock.  The spread of an arm is (max - min) / median of its round times: the difference between
runs of the same code, which any difference between the arms has to exceed.

Writes one JSON document (default profiles/interactive_step/ab.json).  Needs the GPU: there is no
CPU fallback.
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

import torch  # noqa: E402

SHAPES = [("K100", 100, 5), ("K500", 500, 2)]  # name, K, default episodes per timed round


def summary(times, steps):
    per_step = [t / steps * 1e3 for t in times]
    med = statistics.median(per_step)
    return {"ms_per_episode_rounds": [round(x, 3) for x in per_step], "ms_per_episode_median": round(med, 3),
            "spread": round((max(per_step) - min(per_step)) / med, 4), "timed_episodes": steps * len(times)}


def run_shape(name, K, steps, args):
    import dpt_hip
    from dpt_hip.train import InteractiveTrainer
    from models.net import Transformer
    from train_interactive import build_bandit_env, interactive_step_plain
    dev = dpt_hip.device()
    torch.manual_seed(K)
    model = Transformer(dict(horizon=K, state_dim=1, action_dim=args.dim, n_layer=args.layer, n_embd=args.embd,
                             n_head=1, dropout=0.0, test=True)).to(dev)
    fused_model = copy.deepcopy(model)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    loss_fn = torch.nn.CrossEntropyLoss()
    trainer = InteractiveTrainer(fused_model, lr=1e-3, weight_decay=1e-4, chunk=args.chunk)
    wide = InteractiveTrainer(copy.deepcopy(fused_model), lr=1e-3, weight_decay=1e-4, chunk=args.chunk,
                              full_width=True)

    def plain(k):
        for _ in range(k):
            env = build_bandit_env(args.dim, args.envs, K, args.var, "bandit", dev)
            interactive_step_plain(model, opt, loss_fn, env, K)

    def fused_with(tr):
        def run(k):
            for _ in range(k):
                env = build_bandit_env(args.dim, args.envs, K, args.var, "bandit", dev)
                tr.step(env.means, K, args.var, env.type, targets=env.opt_a_index)
        return run

    arms = {"plain": plain, "fused_full_width": fused_with(wide), "fused": fused_with(trainer)}
    times = {a: [] for a in arms}
    for fn in arms.values():
        fn(args.warmup)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for a, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(steps)
            torch.cuda.synchronize()
            times[a].append(time.perf_counter() - t0)
    out = {a: summary(t, steps) for a, t in times.items()}
    out["K"] = K
    out["fused_mean_loss"] = trainer.read_loss() / (args.warmup + steps * args.rounds)
    out["fused_over_plain"] = round(out["fused"]["ms_per_episode_median"] / out["plain"]["ms_per_episode_median"], 4)
    out["fused_over_fused_full_width"] = round(out["fused"]["ms_per_episode_median"] /
                                               out["fused_full_width"]["ms_per_episode_median"], 4)
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="episodes per timed round (0: the shape's default)")
    ap.add_argument("--rounds", type=int, default=4, help="alternating rounds per arm")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=5)
    ap.add_argument("--layer", type=int, default=4)
    ap.add_argument("--embd", type=int, default=32)
    ap.add_argument("--var", type=float, default=0.3)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interactive_step", "ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("interactive_step_ab.py measures on the GPU; none is visible")
    want = set(filter(None, args.shapes.split(",")))
    res = {"device": torch.cuda.get_device_name(0), "envs": args.envs, "dim": args.dim, "n_layer": args.layer,
           "n_embd": args.embd, "var": args.var, "chunk": args.chunk, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "host clock around each round, device synchronise before and after; rounds alternate arms",
           "shapes": {}}
    for name, K, steps in SHAPES:
        if not want or name in want:
            res["shapes"][name] = run_shape(name, K, args.steps or steps, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
