"""Is the model's action distribution the Bayes posterior of the optimal action?  Prefix by prefix.

The minimiser of the pretraining cross-entropy is P(a* | D_t), the posterior of the optimal action given the
first t transitions of the context, and for the bandits, the linear bandit in the plane and DarkRoom it is
computable (dpt_hip.bandit_posterior / dpt_hip.linear_posterior / dpt_hip.darkroom_posterior; include/dpt_hip.h,
"Bayes posterior of the optimal action" and "Linear bandit, lin_d = 2").  This script puts
a checkpoint's softmax beside it on ``--n_eval`` tasks and reports, per t = 0 .. H as mean +- SEM over the
tasks: ``kl`` = KL(posterior || model), ``nll_model`` and ``nll_bayes`` (-log of the optimal action's
probability under each; their gap is the KL in expectation), the posterior's ``entropy`` (which ``nll_bayes``
equals in expectation), and the optimal action's probability under both.  A regret curve cannot show this.

Flags: evals/eval_interactive_bandit.py's, plus ``--env {bandit,bandit_thompson,linear_bandit,darkroom,
darkroom_heldout}`` (bandit_thompson: Bernoulli rewards; linear_bandit: collect_data.py's arms at ``--lin_d`` 2,
the generator's rollin chosen by ``--data_type {thompson,uniform}``), ``--context {fresh,online}``, ``--grid``
(the posterior's grid size; default dpt_hip.posterior_grid, for linear_bandit dpt_hip.linear_posterior_grid) and
``--chunk`` (tasks per launch).  ``fresh``: the contexts are the fresh-task
generator's samples under train_fresh.py's test key for ``--seed`` (its held-out goals for darkroom_heldout).
``online`` (bandits): the model's own sampled rollout, its records the context -- the distribution the model
meets when deployed (linear_bandit: on ``means = arms @ theta``, theta ~ N(0, I / 2)).  The model's row t is one forward over the whole window (the query token sits at position
0 and attention is causal): dpt_hip.train.exploit_curve for the bandits, one forward-only every-position
training forward on the generator's tokens for DarkRoom.  Writes ``<save>/posterior_gap.png`` and
``<save>/posterior_gap.json``.
"""
import argparse
import json
import os
import random

import matplotlib

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

if __package__ in (None, ""):  # `python evals/eval_posterior.py` from the package directory
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import common_args  # noqa: E402
import dpt_hip  # noqa: E402
from dpt_hip import train as tr  # noqa: E402
from models.net import Transformer  # noqa: E402
from train_fresh import darkroom_goals, generator_key  # noqa: E402

KEYS = ("kl", "nll_model", "nll_bayes", "entropy", "p_opt_model", "p_opt_bayes")


def bandit_records(model, context, n_eval, dim, horizon, var, bandit_type, seed):
    """(actions (n, H) int32, rewards (n, H) float64, targets (n) int64) on the device"""
    if context == "fresh":
        env = dpt_hip.FreshEnv.bandit(dim, horizon, var, bandit_type)
        tok = dpt_hip.fresh_batch(env, generator_key(seed, "test"), 0, n_eval)
        acts = tok["tokens"][:, 1:, 1:1 + dim].argmax(dim=-1).to(torch.int32)
        # the rewards as the float32 the tokens hold: the context the model is given
        return acts, tok["tokens"][:, 1:, 2 + dim].to(torch.float64), tok["opt_action"].to(torch.int64)
    means = np.random.uniform(0, 1, (n_eval, dim))  # the prior of the posterior (both reward types)
    code = dpt_hip.BANDIT_BERNOULLI if bandit_type == "bernoulli" else dpt_hip.BANDIT_GAUSSIAN
    out = tr.rollout_bandit_generic(model, means, horizon, var, True, code, seed=dpt_hip.next_seed())
    return out["actions"], out["rewards"], torch.as_tensor(means.argmax(1), device=out["actions"].device)


def linear_arms(dim, lin_d):
    """collect_data.py's arms"""
    return np.random.RandomState(seed=1234).normal(size=(dim, lin_d)) / np.sqrt(lin_d)


def linear_records(model, context, n_eval, arms, horizon, var, data_type, seed):
    """(actions (n, H) int32, rewards (n, H) float64, targets (n) int64) on the device"""
    dim = len(arms)
    if context == "fresh":
        env = dpt_hip.FreshEnv.linear_bandit(arms, horizon, var, data_type)
        tok = dpt_hip.fresh_batch(env, generator_key(seed, "test"), 0, n_eval)
        acts = tok["tokens"][:, 1:, 1:1 + dim].argmax(dim=-1).to(torch.int32)
        return acts, tok["tokens"][:, 1:, 2 + dim].to(torch.float64), tok["opt_action"].to(torch.int64)
    theta = np.random.normal(size=(n_eval, arms.shape[1])) / np.sqrt(arms.shape[1])  # sample_linear's prior
    means = theta @ arms.T
    out = tr.rollout_bandit_generic(model, means, horizon, var, True, dpt_hip.BANDIT_GAUSSIAN, seed=dpt_hip.next_seed())
    return out["actions"], out["rewards"], torch.as_tensor(means.argmax(1), device=out["actions"].device)


def darkroom_logits(model, tokens, chunk):
    """(n, 1 + H, 5) float32: row t = the model after t transitions (forward-only, every position)"""
    dev = tokens.device
    blob = tr.pack_params(tr.param_list(model), dev)
    n, T = int(tokens.shape[0]), int(tokens.shape[1])
    out = []
    for off, k in tr.chunk_plan(n, chunk):
        d = tr.desc(model.n_layer, model.n_embd, 2, 5, model.n_positions, k, T, tr.FORWARD_ONLY)
        out.append(tr.forward(d, blob, tokens[off:off + k].contiguous())[0])
    return torch.cat(out)


def run(model, env, context, n_eval, dim, horizon, var, bandit_type, seed, grid=None, chunk=0, lin_d=2,
        data_type="thompson"):
    """dict key -> (n_eval, H + 1) float64 numpy arrays of KEYS"""
    if env == "linear_bandit":
        why = dpt_hip.linear_posterior_supported(lin_d, var)
        if why is not None:
            raise NotImplementedError(why)
        arms = linear_arms(dim, lin_d)
        acts, rews, targets = linear_records(model, context, n_eval, arms, horizon, var, data_type, seed)
        post = dpt_hip.linear_posterior(arms, acts, rews, var, grid, chunk)
        means = torch.zeros((n_eval, dim), dtype=torch.float64, device=post.device)  # values are not read here
        logits = tr.exploit_curve(model, acts, rews, means, targets=targets, chunk=chunk, want_logits=True)["logits"]
    elif env.startswith("darkroom"):
        if context != "fresh":
            raise NotImplementedError("--context online is for the bandits: a DarkRoom rollout's context is the "
                                      "episode's own transitions, whose query state moves with it")
        fenv = dpt_hip.FreshEnv.darkroom(dim, horizon, darkroom_goals(env, dim)[1])
        batch = dpt_hip.fresh_batch(fenv, generator_key(seed, "test"), 0, n_eval)
        post, targets = dpt_hip.fresh_posterior(fenv, batch)
        logits = darkroom_logits(model, batch["tokens"], chunk)
    else:
        acts, rews, targets = bandit_records(model, context, n_eval, dim, horizon, var, bandit_type, seed)
        post = dpt_hip.bandit_posterior(acts, rews, dim, var, bandit_type, grid, chunk)
        means = torch.zeros((n_eval, dim), dtype=torch.float64, device=post.device)  # values are not read here
        logits = tr.exploit_curve(model, acts, rews, means, targets=targets, chunk=chunk, want_logits=True)["logits"]
    c = dpt_hip.posterior_compare(post, logits, targets)
    res = {k: c[k].cpu().numpy() for k in ("kl", "nll_model", "nll_bayes", "entropy")}
    res["p_opt_model"], res["p_opt_bayes"] = np.exp(-res["nll_model"]), np.exp(-res["nll_bayes"])
    return res


def summarise(res):
    n = len(res["kl"])
    return {k: {"mean": res[k].mean(0).tolist(),
                "sem": (res[k].std(0, ddof=1) / np.sqrt(n) if n > 1 else np.zeros(res[k].shape[1])).tolist()} for k in KEYS}


def plot_results(summary, save_path):
    fig, axes = plt.subplots(1, 3, figsize=(18, 5))
    steps = np.arange(len(summary["kl"]["mean"]))

    def band(ax, key, **kw):
        m, s = np.array(summary[key]["mean"]), np.array(summary[key]["sem"])
        ax.plot(steps, m, label=key, **kw)
        ax.fill_between(steps, m - s, m + s, alpha=0.2)
    band(axes[0], "kl")
    axes[0].set_title("KL(posterior || model)")
    for key in ("nll_model", "nll_bayes", "entropy"):
        band(axes[1], key)
    axes[1].set_title("-log P(optimal action): model, posterior (floor), posterior entropy")
    for key in ("p_opt_model", "p_opt_bayes"):
        band(axes[2], key)
    axes[2].set_title("P(optimal action)")
    for ax in axes:
        ax.set_xlabel("transitions in the context")
        ax.legend()
    plt.tight_layout()
    os.makedirs(os.path.dirname(save_path) or ".", exist_ok=True)
    plt.savefig(save_path)
    plt.close(fig)


def main(argv=None):
    parser = argparse.ArgumentParser(description="The model's action distribution against the Bayes posterior",
                                     conflict_handler="resolve")
    common_args.add_dataset_args(parser)
    common_args.add_model_args(parser)
    parser.add_argument("--n_eval", type=int, default=100, help="Number of eval tasks")
    parser.add_argument("--var", type=float, default=0.3, help="Reward std")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--model_path", type=str, default="trained_models/interactive_bandit.pt",
                        help="Path to saved model state dict")
    parser.add_argument("--bandit_type", type=str, default="uniform", choices=["uniform", "bernoulli"],
                        help="Reward type of --env bandit (bandit_thompson is bernoulli)")
    parser.add_argument("--sample", action="store_true", help="Unused (the online context is always sampled)")
    parser.add_argument("--save", type=str, default="figs/eval_posterior", help="Directory for the plot and the JSON")
    parser.add_argument("--env", type=str, default="bandit",
                        choices=["bandit", "bandit_thompson", "linear_bandit", "darkroom", "darkroom_heldout"])
    parser.add_argument("--data_type", choices=["thompson", "uniform"], default="thompson",
                        help="linear_bandit, --context fresh: the generator's rollin")
    parser.add_argument("--context", type=str, default="fresh", choices=["fresh", "online"])
    parser.add_argument("--grid", type=int, default=None, help="Posterior grid size (default: posterior_grid)")
    parser.add_argument("--chunk", type=int, default=0, help="Tasks per launch (0: all at once)")
    args = vars(parser.parse_args(argv))

    env, n_eval, dim, horizon, var, seed = args["env"], args["n_eval"], args["dim"], args["H"], args["var"], args["seed"]
    bandit_type = "bernoulli" if env == "bandit_thompson" else args["bandit_type"]
    darkroom = env.startswith("darkroom")
    if darkroom and args["context"] == "online":
        parser.error("--context online is for the bandits")
    config = {"horizon": horizon, "state_dim": 2 if darkroom else 1, "action_dim": 5 if darkroom else dim,
              "n_layer": args["layer"], "n_embd": args["embd"], "n_head": args["head"], "dropout": args["dropout"],
              "test": True}
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

    res = run(model, env, args["context"], n_eval, dim, horizon, var, bandit_type, max(seed, 0), args["grid"],
              args["chunk"], args["lin_d"], args["data_type"])
    summary = summarise(res)
    save = args["save"]
    plot_results(summary, os.path.join(save, "posterior_gap.png"))
    meta = {k: args[k] for k in ("env", "context", "n_eval", "H", "dim", "var", "seed", "grid")}
    meta["bandit_type"] = None if darkroom or env == "linear_bandit" else bandit_type
    if env == "linear_bandit":
        meta.update(lin_d=args["lin_d"], data_type=args["data_type"])
    with open(os.path.join(save, "posterior_gap.json"), "w") as f:
        json.dump({"args": meta, **summary}, f)
    last = {k: summary[k]["mean"][-1] for k in KEYS}
    print(f"t = {horizon}: " + ", ".join(f"{k} {v:.4f}" for k, v in last.items()))
    print(f"Saved {os.path.join(save, 'posterior_gap.png')} and posterior_gap.json")
    return summary


if __name__ == "__main__":
    main()
