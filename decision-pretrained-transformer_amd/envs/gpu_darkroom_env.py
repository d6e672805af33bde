"""GPUDarkroomEnv -- N DarkRoom tasks on one device, modelled on GPUBanditEnv.

The reference has no device-resident DarkRoom env (its DarkroomEnvVec steps numpy envs one by one);
this is the env of the interactive DarkRoom training (train_interactive_darkroom.py).  Goals come from
``torch.randint`` on the device generator (so ``torch.manual_seed`` governs them, as it governs
GPUBanditEnv's means); transitions, rewards and the expert action are the gfx950 integer kernels
``dpt_darkroom_step`` / ``dpt_darkroom_opt_action`` for all envs at once.
"""
import torch

import dpt_hip
from envs.base_env import BaseEnv, spaces


class GPUDarkroomEnv(BaseEnv):
    def __init__(self, dim, n_envs, H, device=None):
        self.dim = dim
        self.n_envs = n_envs
        self._device = device if device is not None else dpt_hip.device()
        self.goals = torch.randint(0, dim, (n_envs, 2), device=self._device, dtype=torch.int32)
        self.perm = None
        self.H = H
        self.horizon = H
        self.state_dim = 2
        self.action_dim = 5
        self.dx = 2
        self.du = 5
        self.observation_space = spaces.Box(low=0, high=dim - 1, shape=(self.state_dim,))
        self.action_space = spaces.Discrete(self.action_dim)
        self.reset()

    def reset(self):
        self.current_step = 0
        self.state = torch.zeros((self.n_envs, 2), dtype=torch.int32, device=self._device)
        return self.state.float()

    def transit(self, state, actions):
        """(next states (n_envs, 2) int32, rewards (n_envs) int32) of one-hot (or logit) ``actions``."""
        a = torch.argmax(actions.to(self._device), dim=1).to(torch.int32)
        return dpt_hip.darkroom_step(state.to(torch.int32), a, self.goals, self.perm, self.dim)

    def step(self, actions):
        if self.current_step >= self.H:
            raise ValueError("Episode has already ended")
        self.state, r = self.transit(self.state, actions)
        self.current_step += 1
        done = torch.full((self.n_envs,), self.current_step >= self.H, dtype=torch.bool, device=self._device)
        return self.state.float(), r.float(), done, {}

    def opt_action(self, state=None):
        """The expert action index (n_envs) int64 at ``state`` (default: the current states)."""
        s = self.state if state is None else state.to(self._device, torch.int32)
        return dpt_hip.darkroom_opt_action(s, self.goals, self.perm).long()

    def deploy(self, ctrl):
        ob = self.reset()
        obs, acts, next_obs, rews = [], [], [], []
        done = False
        while not done:
            act = ctrl.act(ob)
            obs.append(ob)
            acts.append(act)
            ob, rew, d, _ = self.step(act)
            done = bool(d.all())
            rews.append(rew)
            next_obs.append(ob)
        return torch.stack(obs, 1), torch.stack(acts, 1), torch.stack(next_obs, 1), torch.stack(rews, 1)
