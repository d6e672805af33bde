"""In-episode evaluation of the interactive DarkRoom model (train_interactive_darkroom.py's checkpoint),
the DarkRoom sibling of evals/eval_interactive_bandit.py.

The protocol is the one the model was trained in: every env starts at (0, 0) with an empty context, the
context is the episode's own transitions (it grows by one token per step) and the current state is the
query at position 0.  On ``--n_eval`` random goals it runs

* the model -- all K steps of every env in one launch (``dpt_hip.rollout_darkroom_episode``:
  dpt_rollout_darkroom_episode, one workgroup per env) --,
* the expert (``dpt_hip.rollin_darkroom`` in its expert mode),
* a uniformly random walk (``GPUDarkroomEnv`` stepped with ``torch.randint`` actions), and
* optionally a second checkpoint of the same architecture (``--baseline_path``: for example an offline
  ``train.py --env darkroom`` model), in the same protocol,

and reports per policy the reward per step and the cumulative return (mean and SEM over the goals), the
final return, the share of goals reached and the mean first-hit step; for the model also the share of
visited states at which its action is the expert's.  ``online.png`` plots the two curves.
"""
import argparse
import os
import random

import matplotlib

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

if __package__ in (None, ""):  # `python evals/eval_interactive_darkroom.py` from the package directory
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import common_args  # noqa: E402
import dpt_hip  # noqa: E402
from envs.gpu_darkroom_env import GPUDarkroomEnv  # noqa: E402
from models.net import Transformer  # noqa: E402

EXPERT, MODEL, RANDOM, BASELINE = "opt", "Interactive", "Random", "Baseline"


def _sem(v):
    """standard error of the mean over axis 0 (ddof 1, as scipy.stats.sem in evals.eval_bandit.regret_stats);
    0 for a single row"""
    v = np.asarray(v, np.float64)
    n = v.shape[0]
    return v.std(axis=0, ddof=1) / np.sqrt(n) if n > 1 else np.zeros(v.shape[1:])


def episode_stats(rewards, actions=None, targets=None):
    """The statistics of one policy from its rewards (N, K - 1) (0 / 1 per env and step): the reward per
    step and the cumulative return, mean and SEM over the N envs; the final return (mean over envs); the
    share of envs whose goal was reached; and the mean first-hit step (the index of the first reward, K - 1
    where there is none).  With ``actions`` (N, K - 1) and ``targets`` (N, >= K - 1) also the share of
    visited states at which the action equals the target (NaN with no action)."""
    r = np.asarray(rewards, np.float64)
    n, steps = r.shape
    cum = np.cumsum(r, axis=1)
    hit = r > 0
    first = np.where(hit.any(axis=1), hit.argmax(axis=1), steps) if steps else np.zeros(n)
    out = dict(reward_mean=r.mean(axis=0), reward_sem=_sem(r), return_mean=cum.mean(axis=0), return_sem=_sem(cum),
               final_return=float(r.sum(axis=1).mean()) if steps else 0.0,
               reached=float(hit.any(axis=1).mean()), first_hit=float(first.mean()))
    if actions is not None:
        a, t = np.asarray(actions), np.asarray(targets)[:, :steps]
        out["agreement"] = float((a == t).mean()) if a.size else float("nan")
    return out


def _model_episode(model, goals, K, dim, sample, name):
    """(rewards, actions, targets) of ``model`` in the protocol: the one-launch rollout, or, where it is not
    built (another width, K above the prefill window), the chain of dpt_interactive_mdp_grad"""
    try:
        rec, _ = dpt_hip.rollout_darkroom_episode(model, goals, K, dim, sample=sample)
    except NotImplementedError as e:
        from dpt_hip.train import rollout_darkroom_interactive
        print(f"{name}: the one-launch episode rollout does not take this shape ({e}); running "
              f"rollout_darkroom_interactive instead")
        rec, _ = rollout_darkroom_interactive(model, goals, K, dim, sample=sample)
    return tuple(rec[k].cpu().numpy() for k in ("rewards", "actions", "targets"))


def random_walk(goals, K, dim):
    """rewards (N, K - 1) of uniformly random actions (torch's device generator) from (0, 0)"""
    n, dev = int(goals.shape[0]), goals.device
    env = GPUDarkroomEnv(dim, n, max(K - 1, 1), dev)
    env.goals = goals.to(torch.int32)
    env.reset()
    rews = torch.zeros((n, K - 1), device=dev)
    for t in range(K - 1):
        a = torch.randint(0, env.action_dim, (n,), device=dev)
        _, rews[:, t], _, _ = env.step(torch.nn.functional.one_hot(a, num_classes=env.action_dim).float())
    return rews.cpu().numpy()


def run_online_eval(model, goals, K, dim, sample, baseline=None):
    """The model, the expert, a random walk and optionally ``baseline`` on the same ``goals`` (N, 2) for K
    steps each (K - 1 transitions); {policy: ``episode_stats``} plus ``goals`` and ``K``."""
    goals = dpt_hip._dev(goals, torch.int32)
    K = int(K)
    if K < 1:
        raise ValueError(f"K={K} (at least 1)")
    n = int(goals.shape[0])
    results = {}
    r, a, tg = _model_episode(model, goals, K, dim, sample, MODEL)
    results[MODEL] = episode_stats(r, a, tg)
    if K > 1:
        expert = dpt_hip.rollin_darkroom(goals, K - 1, dim, mode=1)["rewards"].cpu().numpy()
    else:
        expert = np.zeros((n, 0))
    results[EXPERT] = episode_stats(expert)
    results[RANDOM] = episode_stats(random_walk(goals, K, dim))
    if baseline is not None:
        r, a, tg = _model_episode(baseline, goals, K, dim, sample, BASELINE)
        results[BASELINE] = episode_stats(r, a, tg)
    results["goals"] = goals.cpu().numpy()
    results["K"] = K
    return results


def plot_results(results, save_path=None):
    """Reward per step and cumulative return against the step, one curve per policy, the expert dashed black."""
    fig, (ax1, ax2) = plt.subplots(1, 2, figsize=(14, 5))
    for key in (EXPERT, MODEL, BASELINE, RANDOM):
        if key not in results:
            continue
        st = results[key]
        steps = np.arange(len(st["reward_mean"]))
        style = dict(linestyle="--", color="black", linewidth=2) if key == EXPERT else {}
        fill = {"color": "black"} if key == EXPERT else {}
        for ax, mean, sem in ((ax1, st["reward_mean"], st["reward_sem"]), (ax2, st["return_mean"], st["return_sem"])):
            ax.plot(steps, mean, label=key, **style)
            ax.fill_between(steps, mean - sem, mean + sem, alpha=0.2, **fill)
    ax1.set_xlabel("Steps")
    ax1.set_ylabel("Reward per step")
    ax1.set_title("In-episode Evaluation (Interactive DarkRoom)")
    ax1.legend()
    ax2.set_xlabel("Steps")
    ax2.set_ylabel("Cumulative return")
    ax2.set_title("Cumulative Return Over the Episode")
    ax2.legend()
    plt.tight_layout()
    if save_path:
        os.makedirs(os.path.dirname(save_path) or ".", exist_ok=True)
        plt.savefig(save_path)
        plt.close(fig)
    else:
        plt.show()


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Evaluate interactive DarkRoom model", conflict_handler="resolve")
    common_args.add_dataset_args(parser)
    common_args.add_model_args(parser)
    parser.add_argument("--n_eval", type=int, default=100, help="Number of eval goals")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--model_path", type=str, default="trained_models/interactive_darkroom.pt",
                        help="Path to saved model state dict")
    parser.add_argument("--baseline_path", type=str, default=None,
                        help="A second checkpoint of the same architecture, run in the same protocol")
    parser.add_argument("--sample", action="store_true", help="Sample actions from model policy (default: greedy)")
    parser.add_argument("--K", type=int, default=-1, help="Steps per episode (default: --H)")
    parser.add_argument("--save", type=str, default="figs/eval_interactive_darkroom",
                        help="Directory or path prefix for saving plots")
    parser.add_argument("--env", type=str, default="darkroom", help="Unused, for CLI compat")
    return vars(parser.parse_args(argv))


def load_model(path, args, K, device):
    """The checkpoint at ``path`` as a Transformer in eval mode; its horizon is read off its position table
    (n_positions = 4 (1 + horizon)), so an offline checkpoint with a longer horizon loads as it is."""
    sd = torch.load(path, map_location=device)
    npos = int(sd["transformer.wpe.weight"].shape[0])
    if npos % 4 or K > npos:
        raise ValueError(f"{path}: {npos} positions cannot run K={K} steps")
    config = {"horizon": npos // 4 - 1, "state_dim": 2, "action_dim": 5, "n_layer": args["layer"],
              "n_embd": args["embd"], "n_head": args["head"], "dropout": args["dropout"], "test": True}
    model = Transformer(config).to(device)
    model.load_state_dict(sd)
    model.eval()
    return model


def main(argv=None):
    args = parse_args(argv)
    K = args["K"] if args["K"] > 0 else args["H"]
    n_eval, dim, seed, save = args["n_eval"], args["dim"], args["seed"], args["save"]

    if seed >= 0:
        torch.manual_seed(seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(seed)
        np.random.seed(seed)
        random.seed(seed)

    device = dpt_hip.device()
    print(f"Loading model from {args['model_path']}")
    model = load_model(args["model_path"], args, K, device)
    baseline = None
    if args["baseline_path"]:
        print(f"Loading baseline from {args['baseline_path']}")
        baseline = load_model(args["baseline_path"], args, K, device)

    print(f"Generating {n_eval} eval goals (dim={dim}, K={K})")
    goals = GPUDarkroomEnv(dim, n_eval, K, device).goals

    print("Running in-episode evaluation...")
    results = run_online_eval(model, goals, K, dim, args["sample"], baseline=baseline)
    for key in (EXPERT, MODEL, BASELINE, RANDOM):
        if key in results:
            st = results[key]
            extra = f" - expert-action agreement: {st['agreement']:.4f}" if "agreement" in st else ""
            print(f"{key}: return {st['final_return']:.4f} - reached {st['reached']:.4f} - first hit "
                  f"{st['first_hit']:.2f}{extra}")

    save_path = save if save.endswith(".png") else os.path.join(save, "online.png")
    plot_results(results, save_path=save_path)
    print(f"Plots saved to {save_path}")
    return results


if __name__ == "__main__":
    main()
