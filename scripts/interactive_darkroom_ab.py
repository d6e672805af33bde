#!/usr/bin/env python3
"""A/B of one interactive DarkRoom training episode: the plain per-step loop against the fused step, in
one process.

Arm "plain": ``train_interactive_darkroom.interactive_mdp_step_plain`` -- a fresh GPUDarkroomEnv, K
forwards of the module over the growing window (a training forward with ``backward()`` where the loss
reads the step, the inference kernels without a graph elsewhere), the selection and env kernels one call
each, torch's cross-entropy and ``torch.optim.AdamW.step()``.  Arm "fused": a fresh GPUDarkroomEnv and
``InteractiveMDPTrainer.step`` (dpt_interactive_mdp_grad: per step the pack, the forward from the master
blob -- with the last block on the last row alone --, on a loss-bearing step the last-position
cross-entropy and the backward, and one act-step launch; then dpt_adamw_step).  Neither arm reads the loss
inside a timed round.

Shapes: dim 10, width 32, four layers, 1024 envs in one chunk, K = 25 and K = 100, both loss modes.  Per
shape both arms warm up, then run ``--rounds`` alternating rounds of ``--steps`` episodes each; every round
starts and ends in a device synchronise and is timed with the host clock.  The spread of an arm is
(max - min) / median of its round times: the difference between runs of the same code, which any
difference between the arms has to exceed.  The fused step's workspace bytes are recorded per shape.

Writes one JSON document (default profiles/interactive_darkroom/ab.json).  Needs the GPU: there is no
CPU fallback.
"""
import argparse
import copy
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "decision-pretrained-transformer_amd"))

import torch  # noqa: E402

# name, K, loss mode, default episodes per timed round (each round runs for about half a second or more)
SHAPES = [("K25_every", 25, "every", 15), ("K25_last", 25, "last", 60), ("K100_every", 100, "every", 3),
          ("K100_last", 100, "last", 20)]


def summary(times, steps):
    per_step = [t / steps * 1e3 for t in times]
    med = statistics.median(per_step)
    return {"ms_per_episode_rounds": [round(x, 3) for x in per_step], "ms_per_episode_median": round(med, 3),
            "spread": round((max(per_step) - min(per_step)) / med, 4), "timed_episodes": steps * len(times)}


def run_shape(name, K, mode, steps, args):
    import dpt_hip
    from dpt_hip import _lib
    from dpt_hip.train import MDP_LOSS, InteractiveMDPTrainer
    from envs.gpu_darkroom_env import GPUDarkroomEnv
    from models.net import Transformer
    from train_interactive_darkroom import interactive_mdp_step_plain
    dev = dpt_hip.device()
    torch.manual_seed(K)
    model = Transformer(dict(horizon=K, state_dim=2, action_dim=5, n_layer=args.layer, n_embd=args.embd, n_head=1,
                             dropout=0.0, test=True)).to(dev)
    trainer = InteractiveMDPTrainer(copy.deepcopy(model), lr=1e-3, weight_decay=1e-4, chunk=args.chunk, loss=mode)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)

    def plain(k):
        for _ in range(k):
            interactive_mdp_step_plain(model, opt, GPUDarkroomEnv(args.dim, args.envs, K, dev), K, mode, seed=1)

    def fused(k):
        for _ in range(k):
            trainer.step(GPUDarkroomEnv(args.dim, args.envs, K, dev).goals, K, args.dim, seed=1)

    arms = {"plain": plain, "fused": fused}
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
    need = ctypes.c_int64()
    n_chunk = args.envs if args.chunk == 0 else min(args.chunk, args.envs)
    _lib.call("dpt_interactive_mdp_workspace_numel", ctypes.byref(trainer._d), n_chunk, K, MDP_LOSS[mode],
              ctypes.byref(need))
    out.update(K=K, loss=mode, fused_workspace_bytes=4 * need.value,
               fused_mean_loss=trainer.read_loss() / (args.warmup + steps * args.rounds))
    ratio = out["fused"]["ms_per_episode_median"] / out["plain"]["ms_per_episode_median"]
    out["fused_over_plain"] = round(ratio, 4)
    out["gain_exceeds_both_spreads"] = bool(1.0 - ratio > max(out["fused"]["spread"], out["plain"]["spread"]))
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=0, help="episodes per timed round (0: the shape's default)")
    ap.add_argument("--rounds", type=int, default=4, help="alternating rounds per arm")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=10)
    ap.add_argument("--layer", type=int, default=4)
    ap.add_argument("--embd", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interactive_darkroom", "ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("interactive_darkroom_ab.py measures on the GPU; none is visible")
    want = set(filter(None, args.shapes.split(",")))
    res = {"device": torch.cuda.get_device_name(0), "envs": args.envs, "dim": args.dim, "n_layer": args.layer,
           "n_embd": args.embd, "chunk": args.chunk, "rounds": args.rounds, "warmup": args.warmup,
           "timing": "host clock around each round, device synchronise before and after; rounds alternate arms",
           "shapes": {}}
    for name, K, mode, steps in SHAPES:
        if not want or name in want:
            res["shapes"][name] = run_shape(name, K, mode, args.steps or steps, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
