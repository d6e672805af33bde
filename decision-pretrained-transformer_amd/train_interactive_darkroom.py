"""Interactive (on-policy) DarkRoom training CLI: train_interactive.py's episode for the DarkRoom MDP
(the reference's script runs bandits only, train_interactive.py:54-55), with its flags, seeding, epoch
line and checkpoint naming, plus ``--chunk``, ``--loss`` and ``--n_eval``.

Every episode samples ``--envs`` fresh goals on the device (GPUDarkroomEnv), starts every env at (0, 0)
and rolls the model out for K steps in its own episode: step t forwards the window of the t transitions so
far with the current state as the query, samples an action from the logits and moves the env.  The loss is
the cross-entropy against the expert action at the states the model itself visits -- at every step
(``--loss every``, the default) or at the last one (``--loss last``, train_interactive.py:134-135
transliterated) -- followed by one AdamW step.  Without dropout an episode is one fused device step
(dpt_hip.train.InteractiveMDPTrainer -> dpt_interactive_mdp_grad per chunk of envs, then dpt_adamw_step)
with the loss and the return summed on the device and read once per epoch.  With ``--dropout > 0`` every
forward needs fresh masks, which the fused chain does not draw, and ``interactive_mdp_step_plain`` runs
instead: the per-step loop on the module with torch.optim.AdamW.  At the end the model plays ``--n_eval``
fresh goals greedily and its mean return is printed beside the expert's.
"""
import argparse
import os
import time

import torch

import common_args
import dpt_hip
from dpt_hip.train import InteractiveMDPTrainer, rollout_darkroom_interactive
from envs.gpu_darkroom_env import GPUDarkroomEnv
from models.net import Transformer
from train_common import set_seeds


def interactive_mdp_step_plain(model, optimizer, env, K, loss="every", sample=True, uniforms=None, seed=None):
    """One episode as a plain per-step loop on the module: step t forwards the window of the t
    transitions so far with the current state as the query, takes the cross-entropy against the expert
    action where the loss reads the step (every step, or the last one; the other forwards run without a
    graph, in training mode: dropout, if any, stays active), selects an action with the library's rule
    (``uniforms`` (K - 1, N), or Philox keyed by ``seed`` and the step) and steps ``env``; then one
    optimizer step.  Returns (the loss, the mean return) as tensors (no synchronisation)."""
    if loss not in ("every", "last"):
        raise ValueError(f"loss={loss!r} ('every' or 'last')")
    dev, n, A = env.goals.device, env.n_envs, env.action_dim
    state = env.reset()
    states = torch.zeros((n, K, 2), device=dev)
    acts = torch.zeros((n, K, A), device=dev)
    nexts = torch.zeros((n, K, 2), device=dev)
    rews = torch.zeros((n, K, 1), device=dev)
    seed = dpt_hip.next_seed() if seed is None and uniforms is None else seed
    model.train()
    optimizer.zero_grad()
    total = torch.zeros((), device=dev)
    for t in range(K):
        batch = {"context_states": states[:, :t], "context_actions": acts[:, :t], "context_next_states": nexts[:, :t],
                 "context_rewards": rews[:, :t], "query_states": state}
        if loss == "every" or t == K - 1:
            logits = model(batch)
            step_loss = torch.nn.functional.cross_entropy(logits, env.opt_action()) / (K if loss == "every" else 1)
            step_loss.backward()
            total += step_loss.detach()
            logits = logits.detach()
        else:
            with torch.no_grad():
                logits = model(batch)
        if t < K - 1:
            a = dpt_hip.select_action(logits, sample, 1.0, None if uniforms is None else uniforms[t], seed=seed or 0,
                                      counter=t)
            states[:, t] = state
            acts[:, t] = torch.nn.functional.one_hot(a.long(), num_classes=A).float()
            state, r, _, _ = env.step(acts[:, t])
            nexts[:, t], rews[:, t, 0] = state, r
    optimizer.step()
    return total, rews.sum() / n


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    common_args.add_dataset_args(parser)
    common_args.add_model_args(parser)
    common_args.add_train_args(parser)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--K", type=int, default=-1, help="Interactive rollout steps")
    parser.add_argument("--episodes_per_epoch", type=int, default=1000)
    parser.add_argument("--chunk", type=int, default=0,
                        help="Envs per fused gradient chunk (0: all at once); bounds the workspace")
    parser.add_argument("--loss", choices=("every", "last"), default="every",
                        help="Cross-entropy at every visited state, or at the last one only")
    parser.add_argument("--n_eval", type=int, default=100, help="Fresh goals of the final greedy evaluation")
    return vars(parser.parse_args(argv))


def main(argv=None):
    args = parse_args(argv)
    print("Args: ", args)
    if args["env"] != "darkroom":
        raise ValueError("train_interactive_darkroom.py supports --env darkroom only.")
    os.makedirs("trained_models", exist_ok=True)

    K = args["K"] if args["K"] > 0 else args["H"]
    dim, n_envs, n_eval = args["dim"], args["envs"], args["n_eval"]
    num_epochs, episodes = args["num_epochs"], args["episodes_per_epoch"]
    set_seeds(0 if args["seed"] == -1 else args["seed"], cudnn=True)

    device = dpt_hip.device()
    config = {"horizon": K, "state_dim": 2, "action_dim": 5, "n_layer": args["layer"], "n_embd": args["embd"],
              "n_head": args["head"], "dropout": args["dropout"], "test": True}
    model = Transformer(config).to(device)

    fused = args["dropout"] == 0
    if fused:
        trainer = InteractiveMDPTrainer(model, lr=args["lr"], weight_decay=1e-4, chunk=args["chunk"], loss=args["loss"])
    else:
        optimizer = torch.optim.AdamW(model.parameters(), lr=args["lr"], weight_decay=1e-4)

    for epoch in range(num_epochs):
        start_time = time.time()
        total = torch.zeros((), device=device)
        returns = torch.zeros((), device=device)
        for _ in range(episodes):
            env = GPUDarkroomEnv(dim, n_envs, K, device)
            if fused:
                rec = trainer.step(env.goals, K, dim)
                returns += rec["rewards"].sum() / n_envs
            else:
                loss, ret = interactive_mdp_step_plain(model, optimizer, env, K, args["loss"])
                total += loss
                returns += ret
        epoch_loss = trainer.read_loss() if fused else float(total.item())  # the epoch's one synchronisation
        avg_loss, avg_return = epoch_loss / max(1, episodes), float(returns.item()) / max(1, episodes)
        print(f"Epoch {epoch + 1}/{num_epochs} - loss: {avg_loss:.6f} - return: {avg_return:.4f} - "
              f"time: {time.time() - start_time:.2f}s")

    if fused:
        trainer.sync_to_model()
    torch.save(model.state_dict(), "trained_models/interactive_darkroom.pt")

    if n_eval > 0:
        model.eval()
        goals = GPUDarkroomEnv(dim, n_eval, K, device).goals
        _, ret = rollout_darkroom_interactive(model, goals, K, dim, sample=False, chunk=args["chunk"])
        value = float(ret.double().mean().item())
        expert = 0.0
        if K > 1:
            expert = float(dpt_hip.rollin_darkroom(goals, K - 1, dim, mode=1)["rewards"].double().sum(1).mean().item())
        print(f"Eval ({n_eval} goals, greedy, K={K}) - return: {value:.4f} - expert: {expert:.4f}")
    print("Done.")


if __name__ == "__main__":
    main()
