"""Vectorised Miniworld wrapper — drop-in for the reference envs/miniworld_env.py.

The wrapped envs are gymnasium-style objects (``reset() -> (obs, info)``, ``step(a) -> (obs, rew, done,
trunc, info)``, ``agent.pos`` / ``agent.dir_vec``, ``action_space``, ``opt_a``); nothing here needs the
Miniworld package or its renderer.  ``deploy`` records as ``obs`` the frames the controller already
resized and normalised on the device for its own step (``ctrl.last_obs``) where the reference resizes
every frame a second time; a policy that never looked at the frames has them preprocessed here by the
same kernel.  ``imageio`` is imported only to write a video.
"""
import numpy as np
import torch

import dpt_hip
from envs.darkroom_env import DarkroomEnvVec

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
target_shape = (25, 25, 3)

_MEAN = torch.tensor([0.485, 0.456, 0.406])[:, None, None]
_STD = torch.tensor([0.229, 0.224, 0.225])[:, None, None]


def _normalize_raw(frames):
    """(B, h, w, 3) uint8 -> (B, 3, h, w) fp32: ToTensor + Normalize of the raw frames (torch ops)"""
    x = torch.from_numpy(np.ascontiguousarray(np.stack(frames))).permute(0, 3, 1, 2).float() / 255
    return (x - _MEAN) / _STD


class MiniworldEnvVec(DarkroomEnvVec):
    """Vectorized environment for MiniWorld (envs/miniworld_env.py:12-91)."""

    def __init__(self, envs):
        super().__init__(envs)
        self.action_space = envs[0].action_space

    def reset(self):
        return [env.reset()[0] for env in self._envs]

    def step(self, actions):
        next_obs, rews, dones = [], [], []
        for action, env in zip(actions, self._envs):
            ob, rew, done, _, _ = env.step(action)
            next_obs.append(ob)
            rews.append(rew)
            dones.append(done)
        return next_obs, rews, dones, False, {}

    def opt_a(self, x):
        return [env.opt_a(x) for env in self._envs]

    def _pose_angle(self):
        return ([env.agent.pos[[0, -1]] for env in self._envs], [env.agent.dir_vec[[0, -1]] for env in self._envs])

    def deploy(self, ctrl):
        """One episode: (obs (B, T, 3, 25, 25) normalised on the device, states (B, T, 2) the agents'
        direction vectors, actions (B, T, A) one-hot, next_obs (B, T, 3, h, w) the raw next frames
        normalised, rewards (B, T))."""
        images = self.reset()
        pose, angle = self._pose_angle()
        obs, states, acts, next_obs, rews = [], [], [], [], []
        videos = [[] for _ in range(self.num_envs)] if ctrl.save_video else None
        done = False
        while not done:
            action = np.atleast_2d(ctrl.act(images, pose, angle))
            seen = getattr(ctrl, "last_obs", None)
            obs.append(seen if seen is not None else dpt_hip.obs_preprocess(np.stack(images)))
            states.append(angle)
            acts.append(action)
            chosen = np.argmax(action, axis=-1)
            images, rew, dones, _, _ = self.step(chosen)
            pose, angle = self._pose_angle()
            done = all(dones)
            rews.append(rew)
            next_obs.append(_normalize_raw(images))
            if videos is not None:
                for i, (env, ac) in enumerate(zip(self._envs, chosen)):
                    videos[i].append(env.unwrapped.render(goal_text=True, action=ac))
        if videos is not None:
            import imageio
            for i in range(self.num_envs):
                imageio.mimsave(ctrl.filename_template(env_id=i), np.array(videos[i]))
        return (torch.stack(obs, dim=1), np.stack(states, axis=1), np.stack(acts, axis=1),
                torch.stack(next_obs, dim=1), np.stack(rews, axis=1))
