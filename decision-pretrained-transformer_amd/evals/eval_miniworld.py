"""Miniworld evaluation — drop-in for the reference evals/eval_miniworld.py.

``deploy_online_vec``, ``online`` and ``offline`` keep the reference's arguments; ``online`` and
``offline`` take one more keyword, ``make_env``: a callable ``env_id -> env`` used where the reference
calls ``gym.make(...)`` and ``env.set_task(env_id=...)``.  The default factory imports ``gymnasium`` and
``miniworld`` when it is first called, so everything else here (the controllers, the vectorised
wrapper, the episode loop, the model's device act step) works without the environment package.

The context lives on the device for the whole evaluation: an episode's record (the frames the
controller normalised for its own steps, the direction vectors, the one-hot actions, the rewards)
is written straight into the context buffers.
"""
import os
from functools import partial

import matplotlib.pyplot as plt
import numpy as np
import scipy
import scipy.stats
import torch

from ctrls.ctrl_miniworld import MiniworldOptPolicy, MiniworldRandPolicy, MiniworldTransformerController
from envs.miniworld_env import MiniworldEnvVec
from utils import convert_to_tensor

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
ENV_NAME = "MiniWorld-OneRoomS6FastMultiFourBoxesFixedInit-v0"
OBS_DIM, STATE_DIM, ACTION_DIM = (3, 25, 25), 2, 4


def default_make_env(env_id):
    """The reference's environment for task ``env_id``; needs the packages this project leaves out."""
    try:
        import gymnasium as gym
        import miniworld  # noqa: F401  (registers the MiniWorld ids)
    except ImportError as e:
        raise ImportError(f"evals.eval_miniworld builds {ENV_NAME} with the `gymnasium` and `miniworld` packages, "
                          "which are not installed (the environment and its 3-D renderer are not part of this "
                          "project); install them or pass make_env=<callable env_id -> env>") from e
    env = gym.make(ENV_NAME)
    env.set_task(env_id=env_id)
    return env


def deploy_online_vec(vec_env, controller, Heps, H, horizon, filename_template="", learner=False):
    """evals/eval_miniworld.py:23-108: ``Heps`` episodes; the context grows by one episode until it
    holds ``H // horizon`` of them, then rolls.  Returns the episode returns (num_envs, Heps)."""
    assert H % horizon == 0
    n_ctx = H // horizon
    n = vec_env.num_envs
    ctx = {"context_images": torch.zeros((n, n_ctx, horizon, *OBS_DIM), dtype=torch.float32, device=device),
           "context_states": torch.zeros((n, n_ctx, horizon, STATE_DIM), dtype=torch.float32, device=device),
           "context_actions": torch.zeros((n, n_ctx, horizon, ACTION_DIM), dtype=torch.float32, device=device),
           "context_rewards": torch.zeros((n, n_ctx, horizon, 1), dtype=torch.float32, device=device)}
    returns = []
    for ep in range(max(Heps, n_ctx)):  # the reference always fills the context once
        filled = min(ep, n_ctx)  # episodes the controller may see
        controller.set_batch({k: v[:, :filled].reshape(n, filled * horizon, *v.shape[3:]) for k, v in ctx.items()})
        if controller.save_video:
            controller.filename_template = partial(filename_template, ep=ep)
        images, states, actions, _, rewards = vec_env.deploy_eval(controller)
        returns.append(np.sum(rewards, axis=-1))
        if not learner:
            continue
        record = {"context_images": images.float().to(device), "context_states": convert_to_tensor(states),
                  "context_actions": convert_to_tensor(actions),
                  "context_rewards": convert_to_tensor(np.asarray(rewards)[:, :, None])}
        for k, v in record.items():
            if ep < n_ctx:
                ctx[k][:, ep] = v
            else:  # shift out the oldest episode
                ctx[k] = torch.cat((ctx[k][:, 1:], v[:, None]), dim=1)
    return np.stack(returns, axis=1)


def _make_vec(env_ids, make_env):
    make_env = make_env or default_make_env
    return MiniworldEnvVec([make_env(i) for i in env_ids])


def online(eval_trajs, model, Heps, horizon, H, n_eval, save_video=False, filename_template="", make_env=None):
    """evals/eval_miniworld.py:111-194: learner, optimal and random policies on envs 8000 .. 8000 + n_eval."""
    assert H % horizon == 0
    vec_env = _make_vec([8000 + i for i in range(n_eval)], make_env)
    curves = {}

    print("Evaluating learner")
    tmpl = partial(filename_template.format, controller="lnr")
    lnr = MiniworldTransformerController(model, batch_size=n_eval, sample=True, save_video=save_video,
                                         filename_template=tmpl)
    curves["lnr"] = np.array(deploy_online_vec(vec_env, lnr, Heps, H, horizon, tmpl, learner=True))

    print("Evaluating optimal policy")
    tmpl = partial(filename_template.format, controller="opt")
    opt = MiniworldOptPolicy(vec_env, batch_size=n_eval, save_video=save_video, filename_template=tmpl)
    curves["opt"] = np.repeat(deploy_online_vec(vec_env, opt, 1, H, horizon, tmpl), Heps, axis=-1)

    print("Evaluating random policy")
    rand = MiniworldRandPolicy(vec_env, batch_size=n_eval)
    curves["rand"] = np.array(deploy_online_vec(vec_env, rand, Heps, H, horizon))

    colors = {"lnr": ("blue", "LNR"), "opt": ("green", "Optimal"), "rand": ("orange", "Rand")}
    for k, (color, label) in colors.items():
        for row in curves[k]:
            plt.plot(row, color=color, alpha=0.2)
    for k, (color, label) in colors.items():
        mean = np.mean(curves[k], axis=0)
        sem = scipy.stats.sem(curves[k], axis=0) if n_eval > 1 else np.zeros_like(mean)
        plt.plot(mean, color=color, label=label)
        plt.fill_between(np.arange(Heps), mean - sem, mean + sem, color=color, alpha=0.2)
    plt.legend()
    plt.xlabel("t")
    plt.ylabel("Average Reward")
    plt.title(f"Online Evaluation on {n_eval} envs")
    return curves


def _context_images(traj):
    """a trajectory's (H, 25, 25, 3) float images in [0, 1] (an array, or the .npy path the collection
    wrote) -> (H, 3, 25, 25) normalised fp32 on the device"""
    from dpt_hip import train as tr
    raw = traj["context_images"]
    if isinstance(raw, (str, os.PathLike)):
        raw = np.load(raw)
    return tr.normalize_images(np.asarray(raw))


def offline(eval_trajs, model, n_eval, save_video=False, filename_template="", make_env=None):
    """evals/eval_miniworld.py:197-277: the sampled and the greedy learner on each trajectory's context,
    the optimal and the random policy; returns the four return arrays (n_eval,)."""
    trajs = [eval_trajs[i] for i in range(n_eval)]
    for traj in trajs:
        print(f"Eval traj id: {traj['env_id']}")
    vec_env = _make_vec([traj["env_id"] for traj in trajs], make_env)
    tmpl = lambda name: partial(filename_template.format, controller=name)  # noqa: E731
    ctrls = {
        "lnr": MiniworldTransformerController(model, batch_size=n_eval, sample=True, save_video=save_video,
                                              filename_template=tmpl("lnr")),
        "lnr_greedy": MiniworldTransformerController(model, batch_size=n_eval, sample=False, save_video=save_video,
                                                     filename_template=tmpl("lnr_greedy")),
        "opt": MiniworldOptPolicy(vec_env, batch_size=n_eval, save_video=False, filename_template=tmpl("opt")),
        "rand": MiniworldRandPolicy(vec_env, batch_size=n_eval),
    }
    batch = {
        "context_images": torch.stack([_context_images(traj) for traj in trajs]),
        "context_states": convert_to_tensor([traj["context_states"] for traj in trajs]),
        "context_actions": convert_to_tensor([traj["context_actions"] for traj in trajs]),
        "context_rewards": convert_to_tensor([np.asarray(traj["context_rewards"])[:, None] for traj in trajs]),
    }
    baselines = {}
    for name in ("opt", "lnr", "lnr_greedy", "rand"):
        ctrls[name].set_batch(batch)
    for name in ("lnr", "lnr_greedy", "opt", "rand"):
        rewards = vec_env.deploy_eval(ctrls[name])[4]
        baselines[name] = np.sum(rewards, axis=-1)
    baselines = {k: np.array(baselines[k]) for k in ("opt", "lnr", "lnr_greedy", "rand")}
    means = {k: np.mean(v) for k, v in baselines.items()}
    plt.bar(means.keys(), means.values(), color=plt.cm.viridis(np.linspace(0, 1, len(means))))
    plt.title(f"Mean Reward on {n_eval} Trajectories")
    return baselines
