#!/usr/bin/env python3
"""A/B/C of one in-episode DarkRoom evaluation rollout, three arms alternating in one process.

Arm "chain": ``dpt_hip.train.rollout_darkroom_interactive`` -- dpt_interactive_mdp_grad with
DPT_MDP_LOSS_NONE: per step a pack launch, the generic training forward in its forward-only last-position
form, and the act step.  This is what the training script's closing evaluation line runs, the baseline.
Arm "loop": the per-step host loop -- ``model(batch)`` under ``no_grad`` (dpt_forward_window: the width-32
prefill), ``dpt_hip.select_action``, ``GPUDarkroomEnv.step`` -- the sampling part of
``train_interactive_darkroom.interactive_mdp_step_plain``.
Arm "episode": ``dpt_hip.rollout_darkroom_episode`` -- dpt_rollout_darkroom_episode, the whole episode of
every env in one launch.

Shapes: dim 10, 1024 envs, width 32, four layers, K = 25 and K = 100, greedy and sampled.  Per shape every
arm warms up, its episodes per round are chosen so that a round runs about ``--round_seconds``, then the
arms run ``--rounds`` alternating rounds; every round starts and ends in a device synchronise and is timed
with the host clock.  The spread of an arm is (max - min) / median of its round times: the difference
between runs of the same code, which any difference between two arms has to exceed.

Writes one JSON document (default profiles/episode_rollout/ab.json).  Needs the GPU: there is no CPU
fallback.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "decision-pretrained-transformer_amd"))

import torch  # noqa: E402

SHAPES = [("K25_greedy", 25, False), ("K25_sampled", 25, True), ("K100_greedy", 100, False),
          ("K100_sampled", 100, True)]


def summary(times, steps):
    per = [t / steps * 1e3 for t in times]
    med = statistics.median(per)
    return {"ms_per_episode_rounds": [round(x, 3) for x in per], "ms_per_episode_median": round(med, 3),
            "spread": round((max(per) - min(per)) / med, 4), "episodes_per_round": steps}


def run_shape(name, K, sample, args):
    import dpt_hip
    from dpt_hip.train import rollout_darkroom_interactive
    from envs.gpu_darkroom_env import GPUDarkroomEnv
    from models.net import Transformer
    dev = dpt_hip.device()
    torch.manual_seed(K)
    model = Transformer(dict(horizon=K, state_dim=2, action_dim=5, n_layer=args.layer, n_embd=args.embd, n_head=1,
                             dropout=0.0, test=True)).to(dev).eval()
    goals = GPUDarkroomEnv(args.dim, args.envs, K, dev).goals
    n, A = args.envs, 5

    def chain(k):
        for _ in range(k):
            rollout_darkroom_interactive(model, goals, K, args.dim, sample=sample, seed=1)

    def loop(k):
        for _ in range(k):
            env = GPUDarkroomEnv(args.dim, n, K, dev)
            env.goals = goals
            state = env.reset()
            states = torch.zeros((n, K, 2), device=dev)
            acts = torch.zeros((n, K, A), device=dev)
            nexts = torch.zeros((n, K, 2), device=dev)
            rews = torch.zeros((n, K, 1), device=dev)
            with torch.no_grad():
                for t in range(K):
                    logits = model({"context_states": states[:, :t], "context_actions": acts[:, :t],
                                    "context_next_states": nexts[:, :t], "context_rewards": rews[:, :t],
                                    "query_states": state})
                    if t < K - 1:
                        a = dpt_hip.select_action(logits, sample, 1.0, None, seed=1, counter=t)
                        states[:, t] = state
                        acts[:, t] = torch.nn.functional.one_hot(a.long(), num_classes=A).float()
                        state, r, _, _ = env.step(acts[:, t])
                        nexts[:, t], rews[:, t, 0] = state, r

    def episode(k):
        for _ in range(k):
            dpt_hip.rollout_darkroom_episode(model, goals, K, args.dim, sample=sample, seed=1)

    arms = {"chain": chain, "loop": loop, "episode": episode}
    steps = {}
    for a, fn in arms.items():  # warm up, then size the rounds from a short timed run
        fn(args.warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(2)
        torch.cuda.synchronize()
        steps[a] = max(2, math.ceil(args.round_seconds / ((time.perf_counter() - t0) / 2)))
    times = {a: [] for a in arms}
    for _ in range(args.rounds):
        for a, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(steps[a])
            torch.cuda.synchronize()
            times[a].append(time.perf_counter() - t0)
    out = {a: summary(t, steps[a]) for a, t in times.items()}
    out.update(K=K, sample=sample)
    # the same seed and the same goals: the chain and the episode kernel draw the same Philox uniforms
    rec_c, ret_c = rollout_darkroom_interactive(model, goals, K, args.dim, sample=sample, seed=1)
    rec_e, ret_e = dpt_hip.rollout_darkroom_episode(model, goals, K, args.dim, sample=sample, seed=1)
    out["envs_with_equal_records_chain_vs_episode"] = int((rec_c["actions"] == rec_e["actions"]).all(1).sum().item())
    out["mean_return_chain"] = float(ret_c.double().mean().item())
    out["mean_return_episode"] = float(ret_e.double().mean().item())
    for other in ("chain", "loop"):
        ratio = out["episode"]["ms_per_episode_median"] / out[other]["ms_per_episode_median"]
        out[f"episode_over_{other}"] = round(ratio, 4)
        out[f"difference_from_{other}_exceeds_both_spreads"] = bool(
            abs(1.0 - ratio) > max(out["episode"]["spread"], out[other]["spread"]))
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4, help="alternating rounds per arm")
    ap.add_argument("--round_seconds", type=float, default=0.5, help="target length of one timed round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=10)
    ap.add_argument("--layer", type=int, default=4)
    ap.add_argument("--embd", type=int, default=32)
    ap.add_argument("--shapes", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_rollout", "ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("episode_rollout_ab.py measures on the GPU; none is visible")
    want = set(filter(None, args.shapes.split(",")))
    res = {"device": torch.cuda.get_device_name(0), "envs": args.envs, "dim": args.dim, "n_layer": args.layer,
           "n_embd": args.embd, "rounds": args.rounds, "warmup": args.warmup, "round_seconds": args.round_seconds,
           "timing": "host clock around each round, device synchronise before and after; rounds alternate arms",
           "arms": {"chain": "rollout_darkroom_interactive (dpt_interactive_mdp_grad, DPT_MDP_LOSS_NONE)",
                    "loop": "model(batch) under no_grad + select_action + GPUDarkroomEnv.step per step",
                    "episode": "rollout_darkroom_episode (dpt_rollout_darkroom_episode, one launch)"},
           "shapes": {}}
    for name, K, sample in SHAPES:
        if not want or name in want:
            res["shapes"][name] = run_shape(name, K, sample, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
