"""Interactive (on-policy) bandit training CLI -- drop-in for the reference train_interactive.py
(same flags, seeding, log lines and checkpoint name), plus ``--chunk``.

Every episode samples ``--envs`` fresh bandits on the device (GPUBanditEnv: the means come from the
torch device generator as in the reference), rolls the model out with sampling, takes one
CrossEntropyLoss() on the last step's logits against the optimal arm and one AdamW step
(train_interactive.py:92-143).  Without dropout an episode is one fused device step
(dpt_hip.train.InteractiveTrainer -> dpt_interactive_grad per chunk of envs, then dpt_adamw_step):
the rollout decodes through an exact y-cache straight from the master blob, the window is packed
from its records, and the loss is summed on the device and read once per epoch.  With
``--dropout > 0`` every step needs fresh masks over the whole window, so no cached decode exists
and ``interactive_step_plain`` runs instead: a per-step loop on the module with torch.optim.AdamW.
"""
import argparse
import os
import time

import torch

import common_args
import dpt_hip
from dpt_hip.train import InteractiveTrainer
from envs.gpu_bandit_env import GPUBanditEnv
from models.net import Transformer
from train_common import set_seeds


def build_bandit_env(dim, n_envs, horizon, var, env_name, device=None):
    kinds = {"bandit": "uniform", "bandit_thompson": "bernoulli"}
    if env_name not in kinds:
        raise ValueError(f"Unsupported env: {env_name}")
    return GPUBanditEnv(dim, n_envs, horizon, var=var, type=kinds[env_name], device=device)


def interactive_step_plain(model, optimizer, loss_fn, env, K):
    """One episode as a plain per-step loop on the module: step t forwards the window of the t
    transitions so far, samples an action from the logits and steps ``env``; the loss is taken on
    step K - 1's logits.  Only that last forward reaches the loss, so the earlier ones run without
    a graph (in training mode: dropout, if any, stays active, as in the reference).  Returns the
    loss tensor (no synchronisation)."""
    dev = env.means.device
    n, A = env.means.shape
    state = env.reset().float().view(n, 1)
    ones = torch.ones((n, K, 1), device=dev)  # a bandit's state and next state are always 1
    acts = torch.zeros((n, K, A), device=dev)
    rews = torch.zeros((n, K, 1), device=dev)
    model.train()
    logits = None
    for t in range(K):
        batch = {"context_states": ones[:, :t], "context_actions": acts[:, :t], "context_next_states": ones[:, :t],
                 "context_rewards": rews[:, :t], "query_states": state}
        if t < K - 1:
            with torch.no_grad():
                logits = model(batch)
            a = torch.distributions.Categorical(logits=logits).sample()
            acts[:, t] = torch.nn.functional.one_hot(a, num_classes=A).float()
            rews[:, t, 0] = env.step(acts[:, t])[1].float()
        else:
            logits = model(batch)
    loss = loss_fn(logits, env.opt_a_index)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.detach()


def main(argv=None):
    os.makedirs("trained_models", exist_ok=True)

    parser = argparse.ArgumentParser()
    common_args.add_dataset_args(parser)
    common_args.add_model_args(parser)
    common_args.add_train_args(parser)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--K", type=int, default=-1, help="Interactive rollout steps")
    parser.add_argument("--episodes_per_epoch", type=int, default=1000)
    parser.add_argument("--chunk", type=int, default=0,
                        help="Envs per fused gradient chunk (0: all at once); bounds the workspace")
    args = vars(parser.parse_args(argv))
    print("Args: ", args)

    env_name = args["env"]
    if env_name not in ("bandit", "bandit_thompson"):
        raise ValueError("train_interactive.py currently supports bandit envs only.")

    K = args["K"] if args["K"] > 0 else args["H"]
    dim, var, n_envs = args["dim"], args["var"], args["envs"]
    num_epochs, episodes = args["num_epochs"], args["episodes_per_epoch"]
    set_seeds(0 if args["seed"] == -1 else args["seed"], cudnn=True)

    device = dpt_hip.device()
    config = {"horizon": K, "state_dim": 1, "action_dim": dim, "n_layer": args["layer"], "n_embd": args["embd"],
              "n_head": args["head"], "dropout": args["dropout"], "test": True}
    model = Transformer(config).to(device)

    fused = args["dropout"] == 0
    if fused:
        trainer = InteractiveTrainer(model, lr=args["lr"], weight_decay=1e-4, chunk=args["chunk"])
    else:
        optimizer = torch.optim.AdamW(model.parameters(), lr=args["lr"], weight_decay=1e-4)
        loss_fn = torch.nn.CrossEntropyLoss()

    for epoch in range(num_epochs):
        start_time = time.time()
        total = torch.zeros((), device=device)
        for _ in range(episodes):
            env = build_bandit_env(dim, n_envs, K, var, env_name, device)
            if fused:
                trainer.step(env.means, K, var, env.type, targets=env.opt_a_index)
            else:
                total += interactive_step_plain(model, optimizer, loss_fn, env, K)
        epoch_loss = trainer.read_loss() if fused else float(total.item())  # the epoch's one synchronisation
        avg_loss = epoch_loss / max(1, episodes)
        print(f"Epoch {epoch + 1}/{num_epochs} - loss: {avg_loss:.6f} - time: {time.time() - start_time:.2f}s")

    if fused:
        trainer.sync_to_model()
    torch.save(model.state_dict(), "trained_models/interactive_bandit.pt")
    print("Done.")


if __name__ == "__main__":
    main()
