"""A deterministic fake of the Miniworld env (test helper, not a conftest) with the surface
envs.miniworld_env.MiniworldEnvVec and ctrls.ctrl_miniworld touch: ``reset() -> (obs, info)``,
``step(a) -> (obs, rew, done, trunc, info)``, ``agent.pos`` / ``agent.dir_vec``, ``action_space.n == 4``,
``opt_a``, ``set_task(env_id=...)``, ``unwrapped``.

The uint8 frame after a sequence of actions comes from ``numpy.random.default_rng((env_id, step, *actions
so far))``, so the trajectory depends on every action taken; the agent turns by the action, and the
reward is 1 when the action equals ``opt_a``.  ``done`` after ``horizon`` steps.

Also the float64 oracle of the observation preprocessing: the ``scipy.ndimage`` restatement of
``skimage.transform.resize(frame, (25, 25, 3), anti_aliasing=True)`` followed by the ImageNet
normalisation.
"""
import numpy as np

MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
OUT = 25


class _Space:
    n = 4


class _Agent:
    def __init__(self):
        self.pos = np.zeros(3)
        self.dir_vec = np.array([1.0, 0.0, 0.0])


class StubMiniworldEnv:
    def __init__(self, env_id=0, horizon=3, frame_hw=(60, 80)):
        self.action_space = _Space()
        self.horizon = horizon
        self.frame_hw = tuple(frame_hw)
        self.agent = _Agent()
        self.set_task(env_id=env_id)
        self.reset()

    @property
    def unwrapped(self):
        return self

    def set_task(self, env_id):
        self.env_id = int(env_id)

    def _frame(self):
        rng = np.random.default_rng((self.env_id, len(self.actions), *self.actions))
        return rng.integers(0, 256, (*self.frame_hw, 3), dtype=np.uint8)

    def _place(self):
        k = sum(self.actions) + self.env_id
        th = 0.25 * np.pi * k
        self.agent.dir_vec = np.array([np.cos(th), 0.0, np.sin(th)])
        self.agent.pos = np.array([0.5 * len(self.actions), 0.0, 0.25 * k])

    def reset(self):
        self.actions = []
        self._place()
        return self._frame(), {}

    def opt_a(self, obs=None, pose=None, angle=None):
        return (self.env_id + len(self.actions)) % self.action_space.n

    def step(self, action):
        if len(self.actions) >= self.horizon:
            raise ValueError("Episode has already ended")
        rew = 1.0 if int(action) == self.opt_a() else 0.0
        self.actions.append(int(action))
        self._place()
        return self._frame(), rew, len(self.actions) >= self.horizon, False, {}

    def render(self, goal_text=True, action=None):
        return self._frame()


def resize_oracle(frame):
    """skimage 0.21's resize(frame, (25, 25, 3), anti_aliasing=True) restated on scipy.ndimage, float64:
    (h, w, 3) uint8 -> (25, 25, 3) in [0, 1]"""
    from scipy import ndimage
    x = frame.astype(np.float64) / 255
    factors = np.array(x.shape[:2]) / OUT
    sigma = np.maximum(0, (factors - 1) / 2)
    blurred = ndimage.gaussian_filter(x, (sigma[0], sigma[1], 0), mode="mirror", truncate=4.0)
    out = ndimage.zoom(blurred, (OUT / x.shape[0], OUT / x.shape[1], 1), order=1, mode="mirror", grid_mode=True)
    return np.clip(out, x.min(), x.max())


def preprocess_oracle(frames):
    """(n, h, w, 3) uint8 -> (n, 3, 25, 25) float64: the resize, then (x - mean) / std"""
    return np.stack([((resize_oracle(f) - MEAN) / STD).transpose(2, 0, 1) for f in frames])


def tables_no_half_pixel(n_in):
    """the control: the 25 x n_in table with zoom coordinates x = o f (no half-pixel offset)"""
    f = n_in / OUT
    sigma = max(0.0, (f - 1) / 2)
    r = int(4 * sigma + 0.5)
    G = np.eye(n_in)
    if sigma > 0:
        k = np.exp(-0.5 / sigma ** 2 * np.arange(-r, r + 1) ** 2)
        k /= k.sum()
        G = np.zeros((n_in, n_in))
        period = 2 * (n_in - 1)
        for i in range(n_in):
            for t in range(-r, r + 1):
                j = abs(i + t) % period
                G[i, period - j if j > n_in - 1 else j] += k[t + r]
    Z = np.zeros((OUT, n_in))
    for o in range(OUT):
        x = min(o * f, n_in - 1)
        i0 = int(np.floor(x))
        t = x - i0
        Z[o, i0] += 1 - t
        if t > 0:
            Z[o, i0 + 1] += t
    return Z @ G
