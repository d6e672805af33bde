"""Miniworld controllers — drop-in for the reference ctrls/ctrl_miniworld.py.

``MiniworldTransformerController`` keeps the reference protocol (``set_batch`` once per episode,
``act(image, pose, angle)`` returning one-hot numpy actions) on a ``dpt_hip.ImageActSession``: the raw
uint8 frames go to the device as they are, one fused kernel resizes, normalises, encodes and embeds
them, and the context rows are encoded once per ``set_batch`` instead of once per step.  Neither
``skimage`` nor ``torchvision`` is needed: the resize is the device kernel (``dpt_image_obs_preprocess``'s
arithmetic) and ``transform`` is ``dataset.image_transform``.

Sampling draws from the controller's own Philox stream through ``dpt_select_action`` (scipy-softmax +
numpy-choice semantics), as ``BanditTransformerController`` does: the reference's distribution, not
numpy's random stream.

``last_obs`` is the (batch, 3, 25, 25) normalised frames of the latest ``act`` on the device, which
``MiniworldEnvVec.deploy`` records (the reference resizes every frame a second time there); the
policies that never look at a frame leave it ``None``.
"""
import numpy as np
import torch

import dpt_hip
from ctrls.ctrl_bandit import Controller, _SelectStream, _onehot
from dataset import image_transform

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
target_shape = (25, 25, 3)


class MiniworldOptPolicy(Controller):
    """Asks every env for its optimal action (ctrls/ctrl_miniworld.py:13-37)."""

    def __init__(self, env, batch_size=1, save_video=False, filename_template=""):
        super().__init__()
        self.env = env
        self.batch_size = batch_size
        self.save_video = save_video
        self.filename_template = filename_template
        self.transform = image_transform
        self.last_obs = None

    def reset(self):
        return

    def act(self, state, pose, angle):
        idx = np.array([self.env.envs[i].opt_a(state[i], pose[i], angle[i]) for i in range(self.batch_size)])
        return _onehot(idx, self.env.action_space.n)


class MiniworldRandPolicy(MiniworldOptPolicy):
    """Uniformly random actions from numpy's global stream (ctrls/ctrl_miniworld.py:40-49)."""

    def __init__(self, env, batch_size=1):
        super().__init__(env, batch_size=batch_size)

    def act(self, state, pose, angle):
        idx = np.random.randint(self.env.action_space.n, size=self.batch_size)
        return _onehot(idx, self.env.action_space.n)


class MiniworldTransformerController(Controller):
    """DPT policy on raw frames (ctrls/ctrl_miniworld.py:52-113)."""

    def __init__(self, model, batch_size=1, sample=False, save_video=False, filename_template=""):
        self.model = model
        self.action_dim = 4
        self.horizon = model.horizon
        self.transform = image_transform
        self.sample = sample
        self.temp = 1.0
        self.batch_size = batch_size
        self.save_video = save_video
        self.filename_template = filename_template
        self.last_obs = None
        self._stream = _SelectStream()
        self._session = None
        self._fresh = False  # the session holds the current batch's context

    def set_batch(self, batch):
        self.batch = batch
        self._fresh = False

    def _fused(self):
        return not (self.model.training and self.model.dropout > 0)

    def _logits_unfused(self, frames, angle):
        """training mode with dropout: the stand-alone preprocessing kernel, then a plain model(batch)"""
        obs = dpt_hip.obs_preprocess(frames)
        self.batch["query_images"] = obs
        self.batch["query_states"] = torch.as_tensor(angle, dtype=torch.float32, device=obs.device)
        return obs, self.model(self.batch)

    def act(self, image, pose, angle):
        frames = np.asarray(image)
        angle = np.asarray(angle, dtype=np.float32)
        if self.batch_size == 1 and frames.ndim == 3:
            frames, angle = frames[None], angle[None]
        if frames.ndim != 4 or frames.shape[0] != self.batch_size:
            raise ValueError(f"images {frames.shape}: expected ({self.batch_size}, h, w, 3)")
        angle = angle.reshape(self.batch_size, -1)
        seed, ctr = self._stream.next()
        if self._fused():
            s = self._session
            if s is None or (s.in_h, s.in_w) != frames.shape[1:3]:
                s = self._session = dpt_hip.ImageActSession(self.model, self.batch_size, frames.shape[1:3])
                self._fresh = False
            if not self._fresh:
                s.set_context(self.batch)
                self._fresh = True
            idx = s.act(frames, angle, self.sample, self.temp, seed=seed, counter=ctr)
            self.last_obs = s.obs.clone()
        else:
            if frames.dtype != np.uint8:
                raise TypeError(f"frames must be uint8 (got {frames.dtype})")
            self.last_obs, logits = self._logits_unfused(frames, angle)
            idx = dpt_hip.select_action(logits, self.sample, self.temp, seed=seed, counter=ctr)
        actions = _onehot(idx.cpu().numpy(), self.action_dim)
        return actions[0] if self.batch_size == 1 else actions
