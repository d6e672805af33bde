"""Online evaluation of the interactive bandit model (train_interactive.py's checkpoint) -- drop-in
for the reference evals/eval_interactive_bandit.py: same flags, same result keys (``opt``,
``Interactive``, ``Emp``, ``UCB1.0``, ``Thomp``) and the same plot file.

The model and the classical policies are deployed on ``--n_eval`` random bandits through
``evals.eval_bandit.deploy_online_vec``, so each of the five rollouts is one fused device launch
(dpt_rollout_bandit / dpt_rollout_bandit_generic for the model, dpt_rollout_policy for the rest);
the suboptimality and cumulative-regret statistics are ``evals.eval_bandit.regret_stats``.
"""
import argparse
import os
import random

import matplotlib

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

if __package__ in (None, ""):  # `python evals/eval_interactive_bandit.py` from the package directory
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import common_args  # noqa: E402
import dpt_hip  # noqa: E402
from ctrls.ctrl_bandit import (BanditTransformerController, EmpMeanPolicy, OptPolicy,  # noqa: E402
                               ThompsonSamplingPolicy, UCBPolicy)
from envs.bandit_env import BanditEnv, BanditEnvVec  # noqa: E402
from evals.eval_bandit import deploy_online_vec, regret_stats  # noqa: E402
from models.net import Transformer  # noqa: E402


def generate_eval_trajs(n_eval, dim, bandit_type="uniform"):
    """``n_eval`` bandit instances (arm means only), drawn from numpy's global RNG."""
    draw = {"uniform": lambda: np.random.uniform(0, 1, dim), "bernoulli": lambda: np.random.beta(1, 1, dim)}
    if bandit_type not in draw:
        raise ValueError(f"Unknown bandit_type: {bandit_type}")
    return [{"means": draw[bandit_type]()} for _ in range(n_eval)]


def run_online_eval(eval_trajs, model, n_eval, horizon, var, bandit_type, sample_model=False):
    """Opt, the interactive transformer, empirical mean, UCB and Thompson sampling on the same
    bandits; per-step suboptimality and cumulative regret (mean and SEM over the bandits)."""
    envs = [BanditEnv(eval_trajs[i]["means"], horizon, var=var, type=bandit_type) for i in range(n_eval)]
    vec_env = BanditEnvVec(envs)
    n = len(envs)
    controllers = [
        ("opt", OptPolicy(envs, batch_size=n)),
        ("Interactive", BanditTransformerController(model, sample=sample_model, batch_size=n)),
        ("Emp", EmpMeanPolicy(envs[0], online=True, batch_size=n)),
        ("UCB1.0", UCBPolicy(envs[0], const=1.0, batch_size=n)),
        ("Thomp", ThompsonSamplingPolicy(envs[0], std=var if var > 0 else 0.3, sample=True, prior_mean=0.5,
                                         prior_var=1 / 12.0, warm_start=False, batch_size=n)),
    ]
    all_means = {}
    for name, ctrl in controllers:
        all_means[name] = deploy_online_vec(vec_env, ctrl, horizon).T
        assert all_means[name].shape[0] == n_eval
    results = regret_stats(all_means)
    results["all_means"] = {k: np.array(v) for k, v in all_means.items()}
    results["all_means_diff"] = {k: results["all_means"]["opt"] - v for k, v in results["all_means"].items()}
    return results


def plot_results(results, horizon, save_path=None):
    """Suboptimality (log scale) and cumulative regret against the step, one curve per policy."""
    steps = np.arange(horizon)
    fig, (ax1, ax2) = plt.subplots(1, 2, figsize=(14, 5))
    for key, m in results["means"].items():
        s = results["sems"][key]
        style = dict(linestyle="--", color="black", linewidth=2) if key == "opt" else {}
        ax1.plot(m, label=key, **style)
        ax1.fill_between(steps, m - s, m + s, alpha=0.2, **({"color": "black"} if key == "opt" else {}))
    ax1.set_yscale("log")
    ax1.set_xlabel("Steps")
    ax1.set_ylabel("Suboptimality")
    ax1.set_title("Online Evaluation (Interactive Bandit)")
    ax1.legend()
    for key, m in results["regret_means"].items():
        if key == "opt":
            continue
        s = results["regret_sems"][key]
        ax2.plot(m, label=key)
        ax2.fill_between(steps, m - s, m + s, alpha=0.2)
    ax2.set_xlabel("Steps")
    ax2.set_ylabel("Cumulative Regret")
    ax2.set_title("Cumulative Regret Over Time")
    ax2.legend()
    plt.tight_layout()
    if save_path:
        os.makedirs(os.path.dirname(save_path) or ".", exist_ok=True)
        plt.savefig(save_path)
        plt.close(fig)
    else:
        plt.show()


def main(argv=None):
    # the reference re-declares --var and --env after the common groups: the later declaration rules
    parser = argparse.ArgumentParser(description="Evaluate interactive bandit model", conflict_handler="resolve")
    common_args.add_dataset_args(parser)
    common_args.add_model_args(parser)
    parser.add_argument("--n_eval", type=int, default=100, help="Number of eval envs")
    parser.add_argument("--var", type=float, default=0.3, help="Reward variance")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--model_path", type=str, default="trained_models/interactive_bandit.pt",
                        help="Path to saved model state dict")
    parser.add_argument("--bandit_type", type=str, default="uniform", choices=["uniform", "bernoulli"],
                        help="Bandit arm means distribution")
    parser.add_argument("--sample", action="store_true", help="Sample actions from model policy (default: greedy)")
    parser.add_argument("--save", type=str, default="figs/eval_interactive_bandit",
                        help="Directory or path prefix for saving plots")
    parser.add_argument("--env", type=str, default="bandit", help="Unused, for CLI compat")
    args = vars(parser.parse_args(argv))

    n_eval, dim, horizon, var, seed = args["n_eval"], args["dim"], args["H"], args["var"], args["seed"]
    bandit_type, save = args["bandit_type"], args["save"]
    config = {"horizon": horizon, "state_dim": 1, "action_dim": dim, "n_layer": args["layer"],
              "n_embd": args["embd"], "n_head": args["head"], "dropout": args["dropout"], "test": True}

    if seed >= 0:
        torch.manual_seed(seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(seed)
        np.random.seed(seed)
        random.seed(seed)

    device = dpt_hip.device()
    print(f"Loading model from {args['model_path']}")
    model = Transformer(config).to(device)
    model.load_state_dict(torch.load(args["model_path"], map_location=device))
    model.eval()

    print(f"Generating {n_eval} eval bandits (dim={dim}, horizon={horizon}, type={bandit_type})")
    eval_trajs = generate_eval_trajs(n_eval, dim, bandit_type)

    print("Running online evaluation...")
    results = run_online_eval(eval_trajs, model, n_eval, horizon, var, bandit_type, sample_model=args["sample"])

    save_path = save if save.endswith(".png") else os.path.join(save, "online.png")
    plot_results(results, horizon, save_path=save_path)
    print(f"Plots saved to {save_path}")
    return results


if __name__ == "__main__":
    main()
