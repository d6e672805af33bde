"""Deployment of the image-conditioned DPT through libdpt_hip (include/dpt_hip.h, "image act step").

``obs_tables`` / ``obs_preprocess`` are the reference's per-step observation preprocessing
(``skimage.transform.resize(frame, (25, 25, 3), anti_aliasing=True)`` then ``dataset.image_transform``)
as one device kernel on raw uint8 frames.

``ImageActSession`` is the model's part of ``MiniworldTransformerController.act`` for a fixed number of
envs: the context rows are encoded once per episode (``set_context``), and a step (``act``) resizes,
normalises, encodes and embeds only the new query frame in one fused kernel, runs the trunk on the
window and chooses the action with ``dpt_select_action``.  Everything stays on the device; the library
owns no memory (the tables, ``embeds`` and the workspace are torch tensors held here).
"""
import ctypes

import numpy as np
import torch

from . import _dev, _lib, _p, _stream, device, select_action
from . import train as tr

IMAGE_SIZE = tr.IMAGE_SIZE


def obs_tables(in_h, in_w):
    """The resize tables of (in_h, in_w) frames (``_lib.ObsTables``), built on the host in double
    precision; no device is needed.  A side outside 25..128 raises NotImplementedError."""
    t = _lib.ObsTables()
    _lib.call("dpt_image_obs_tables", int(in_h), int(in_w), ctypes.byref(t))
    return t


def obs_tables_dense(t):
    """(R_y (25, in_h), R_x (25, in_w)) float64: the banded rows of ``obs_tables`` written out."""
    out = []
    for n, first, count, w in ((t.in_h, t.first_y, t.count_y, t.wy), (t.in_w, t.first_x, t.count_x, t.wx)):
        R = np.zeros((_lib.OBS_OUT, n))
        for o in range(_lib.OBS_OUT):
            R[o, first[o]:first[o] + count[o]] = np.ctypeslib.as_array(w[o])[:count[o]]
        out.append(R)
    return tuple(out)


def upload_tables(t, dev=None):
    """The table struct's bytes on the device (what the kernels take)."""
    return torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(dev or device())


def _frames(frames, in_hw=None):
    """uint8 (n, h, w, 3) frames as a contiguous device tensor; anything but uint8 is a TypeError."""
    if isinstance(frames, torch.Tensor):
        if frames.dtype != torch.uint8:
            raise TypeError(f"frames must be uint8 (got {frames.dtype})")
    else:
        frames = np.asarray(frames)
        if frames.dtype != np.uint8:
            raise TypeError(f"frames must be uint8 (got {frames.dtype})")
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if frames.dim() != 4 or frames.shape[3] != 3 or (in_hw is not None and tuple(frames.shape[1:3]) != tuple(in_hw)):
        raise ValueError(f"frames {tuple(frames.shape)}: expected (n, {'h, w' if in_hw is None else in_hw}, 3)")
    return frames.to(device()).contiguous()


def obs_preprocess(frames, tables=None, out=None):
    """frames (n, h, w, 3) uint8 -> (n, 3, 25, 25) fp32 on the device: resized and normalised
    (dpt_image_obs_preprocess).  ``tables``: the uploaded tables of (h, w) (``upload_tables``)."""
    fr = _frames(frames)
    n, h, w = (int(v) for v in fr.shape[:3])
    if tables is None:
        tables = upload_tables(obs_tables(h, w), fr.device)
    if out is None:
        out = torch.empty((n, 3, IMAGE_SIZE, IMAGE_SIZE), dtype=torch.float32, device=fr.device)
    _lib.call("dpt_image_obs_preprocess", _p(fr), n, h, w, _p(tables), _p(out), _stream())
    return out


def act_desc(n_layer, n_embd, state_dim, action_dim, n_positions, batch, max_context, in_h, in_w, dropout=0.0,
             image_size=IMAGE_SIZE):
    return _lib.ImageActDesc(n_layer, n_embd, state_dim, action_dim, n_positions, batch, max_context, image_size, in_h,
                             in_w, dropout, 0)


def workspace_numel(d):
    n = ctypes.c_int64()
    _lib.call("dpt_image_act_workspace_numel", ctypes.byref(d), ctypes.byref(n))
    return n.value


class ImageActSession:
    """The act step of an ``ImageTransformer`` for ``batch_size`` envs with raw frames of ``frame_hw``.

    ``set_context(batch)`` once per episode, ``act(frames, query_states, sample)`` per step.  The packed
    weights follow the model: they are repacked when a parameter's version, storage or identity changes
    (the signature ``Transformer.device_model`` uses)."""

    def __init__(self, model, batch_size, frame_hw):
        if not getattr(model, "test", False):
            raise ValueError("ImageActSession needs a model built with test=True (it reads the last position)")
        if model.training and model.dropout > 0:
            raise ValueError("ImageActSession is inference: put the model in eval mode (or build it with dropout 0)")
        self.model = model
        self.B = int(batch_size)
        self.in_h, self.in_w = (int(v) for v in frame_hw)
        tables = obs_tables(self.in_h, self.in_w)  # refuses unsupported sides before the device is touched
        dev = device()
        self.tables = upload_tables(tables, dev)
        self.sd, self.A, self.E = model.state_dim, model.action_dim, model.n_embd
        self.obs = torch.empty((self.B, 3, IMAGE_SIZE, IMAGE_SIZE), dtype=torch.float32, device=dev)
        self.logits = torch.empty((self.B, self.A), dtype=torch.float32, device=dev)
        self._sig = None
        self._cap = -1
        self.set_context(None)

    def _desc(self, max_context):
        m = self.model
        return act_desc(m.n_layer, m.n_embd, m.state_dim, m.action_dim, m.n_positions, self.B, max_context, self.in_h,
                        self.in_w)

    def _blobs(self):
        params = tr.image_param_list(self.model)
        sig = tuple((id(p), p._version, p.data_ptr()) for p in params)
        if sig != self._sig:
            emb_numel = (2 * self.sd + self.A + 1) * self.E + self.E
            self.front, self.trunk = tr.pack_image_params(params, emb_numel, device())
            self._sig = sig
        return self.front, self.trunk

    def set_context(self, batch):
        """The reference's context of an episode: ``context_images`` (B, C, 3, 25, 25) normalised,
        ``context_states`` (B, C, sd), ``context_actions`` (B, C, A), ``context_rewards`` (B, C) or
        (B, C, 1).  ``None`` or C = 0: no context."""
        dev = device()
        B = self.B
        C = 0 if batch is None else int(batch["context_images"].shape[1])
        if C > self._cap:  # the library checks the window against n_positions before anything is allocated
            self.ws = torch.empty(max(workspace_numel(self._desc(C)), 4), dtype=torch.float32, device=dev)
            self._cap = C
        d = self.desc = self._desc(self._cap)
        self.C = C
        self.embeds = torch.empty((B, 1 + C, self.E), dtype=torch.float32, device=dev)
        images = feats = None
        if C > 0:
            f32 = lambda k: _dev(batch[k], torch.float32, dev)  # noqa: E731
            images = f32("context_images").reshape(B * C, 3, IMAGE_SIZE, IMAGE_SIZE).contiguous()
            feats = torch.cat([f32("context_states").reshape(B, C, self.sd), f32("context_actions").reshape(B, C, self.A),
                               f32("context_rewards").reshape(B, C, 1)], dim=2).reshape(B * C, -1).contiguous()
        front, _ = self._blobs()
        _lib.call("dpt_image_act_set_context", ctypes.byref(d), C, _p(front), _p(images), _p(feats), _p(self.ws),
                  _p(self.embeds), _stream())
        self._ctx_sig = self._sig
        self._ctx = batch

    def act(self, frames_uint8, query_states, sample, temp=1.0, uniforms=None, seed=0, counter=0):
        """One step: actions (B,) int32 on the device; ``.logits`` (B, A) and ``.obs`` (B, 3, 25, 25, the
        normalised frames) stay readable until the next call."""
        fr = _frames(frames_uint8, (self.in_h, self.in_w))
        if fr.shape[0] != self.B:
            raise ValueError(f"{fr.shape[0]} frames for a session of {self.B} envs")
        qs = _dev(query_states, torch.float32, fr.device).reshape(self.B, self.sd)
        front, trunk = self._blobs()
        if self._sig != self._ctx_sig:  # the weights changed since the context rows were encoded
            self.set_context(self._ctx)
        _lib.call("dpt_image_act_step", ctypes.byref(self.desc), self.C, _p(trunk), _p(front), _p(fr), _p(self.tables),
                  _p(qs), _p(self.ws), _p(self.embeds), _p(self.obs), _p(self.logits), _stream())
        return select_action(self.logits, sample, temp, uniforms=uniforms, seed=seed, counter=counter)
