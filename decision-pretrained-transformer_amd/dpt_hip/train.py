"""Training forward / backward through libdpt_hip (dpt_train_forward / dpt_train_backward).

``TransformerFunction`` is the autograd node of ``models.net.Transformer.forward`` when autograd
needs it (train.py:286-331: ``loss.backward()`` then ``AdamW.step()``) and the forward of models
whose width the fused kernels are not built for (any ``n_embd``).  The parameters enter in the
packed blob order of include/dpt_hip.h; the gradients come back in that order and are mapped to
the reference's parameter shapes (nn.Linear weights are stored [out][in] by torch and [in][out]
in the blob).  Everything runs on the device; the library owns no memory here (the workspace
holding the forward's saved activations is a torch tensor kept on the autograd context).

``ImageTransformerFunction`` is the autograd node of ``models.net.ImageTransformer.forward``: the HIP
image front end (dpt_image_front_forward / _backward: conv encoder, embed_transition, embed_ln) chained
into the trunk through dpt_train_forward_embeds / dpt_train_backward_embeds.

``Trainer`` is the fused training step that train.py runs (dpt_train_step: batch packing from a
device-resident dataset, forward, summed cross-entropy, backward, AdamW on the packed blob) with
the master weights, the optimizer state and the loss accumulator kept on the device.

``InteractiveTrainer`` is the fused on-policy bandit step that train_interactive.py runs
(dpt_interactive_grad per chunk of envs: the y-cache rollout straight from the master blob, the
window packed from its records, forward, last-position cross-entropy, backward; then dpt_adamw_step).

``ExploreExploitTrainer`` is the fused two-model step that train_explorer_exploiter.py runs
(dpt_explore_grad per chunk of envs: the explorer's rollout with the env stepped apart, one pack, the
exploiter's and the explorer's forward / every-position cross-entropy / backward with the advantage
weights in between; then dpt_adamw_step for each model).

``DeviceImageData`` / ``ImageTrainer`` are the fused step that train_miniworld.py --fused runs
(dpt_image_train_step: the batch gathered from a device-resident, device-normalised image set, the
image front end, the trunk, summed cross-entropy, both backwards, dpt_adamw_step on the trunk blob and
on the front blob).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import _dev, _p, _stream, device

GRAD_BACKWARD = "dpt_train_backward"


def param_list(model):
    """The Transformer's parameters in blob order (pack_weights): embed_transition, wpe, the
    blocks' [ln_1, c_attn, c_proj, ln_2, c_fc, mlp.c_proj] weight/bias pairs, ln_f, pred_actions."""
    t = model.transformer
    ps = [model.embed_transition.weight, model.embed_transition.bias, t.wpe.weight]
    for blk in t.h:
        ps += [blk.ln_1.weight, blk.ln_1.bias, blk.attn.c_attn.weight, blk.attn.c_attn.bias,
               blk.attn.c_proj.weight, blk.attn.c_proj.bias, blk.ln_2.weight, blk.ln_2.bias,
               blk.mlp.c_fc.weight, blk.mlp.c_fc.bias, blk.mlp.c_proj.weight, blk.mlp.c_proj.bias]
    ps += [t.ln_f.weight, t.ln_f.bias, model.pred_actions.weight, model.pred_actions.bias]
    return ps


def pack_params(params, dev=None):
    """Flatten the parameters (blob order) into one fp32 vector on ``dev`` (default: the
    parameters' own device).  The nn.Linear weights (the first and the second-to-last
    parameter) are stored [out][in] by torch and [in][out] in the blob.  Called on every
    training forward, so the common case (fp32, already on ``dev``) is one C++ flatten plus
    the two transposed copies."""
    n = len(params)
    dev = dev or params[0].device
    with torch.no_grad():
        if all(p.dtype == torch.float32 and p.device == dev for p in params):
            blob = torch._C._nn.flatten_dense_tensors([p.detach() for p in params])
        else:
            blob = torch.cat([p.detach().to(device=dev, dtype=torch.float32).reshape(-1) for p in params])
        off = 0
        for i, p in enumerate(params):
            k = p.numel()
            if i == 0 or i == n - 2:
                blob[off:off + k].view(p.shape[1], p.shape[0]).copy_(p.detach().t())
            off += k
    return blob


def _on_device(*tensors):
    """Every pointer handed to the library must be device memory (a host pointer would fault)."""
    for t in tensors:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise ValueError("dpt_hip.train: expected contiguous fp32 device tensors")


def unpack_grads(dblob, params):
    """Split a gradient blob into per-parameter gradients shaped like ``params`` (views of the
    blob; the two nn.Linear weights come back transposed to torch's [out][in])."""
    return _unpack(dblob, [p.shape for p in params], [p.dtype for p in params])


_META = {}


def _unpack(dblob, shapes, dtypes):
    key = tuple(shapes)
    metas = _META.get(key)
    if metas is None:  # shape templates for the C++ unflatten (no storage)
        metas = _META[key] = [torch.empty(sh, device="meta") for sh in shapes]
    total = sum(m.numel() for m in metas)
    if total != dblob.numel():
        raise ValueError(f"gradient blob {dblob.numel()} != parameters {total}")
    out = list(torch._C._nn.unflatten_dense_tensors(dblob, metas))
    n = len(shapes)
    off = 0
    for i, sh in enumerate(shapes):
        k = metas[i].numel()
        if i == 0 or i == n - 2:
            out[i] = dblob[off:off + k].view(sh[1], sh[0]).t()
        off += k
    return [g if dt == g.dtype else g.to(dt) for g, dt in zip(out, dtypes)]


FORWARD_ONLY = _lib.TRAIN_FORWARD_ONLY  # inference workspace, no backward
LAST_ONLY = _lib.TRAIN_LAST_ONLY  # with FORWARD_ONLY: preds at the last position only (test mode)
LAST_LOSS = _lib.TRAIN_LAST_LOSS  # training forward / backward whose loss reads the last position only


def desc(n_layer, n_embd, state_dim, action_dim, n_positions, batch, window, flags=0, dropout=0.0, seed=0):
    """dpt_train_desc; dropout > 0: GPT2Model's embd/attn/resid dropout with masks drawn from
    Philox(seed) (include/dpt_hip.h), regenerated by the backward from the same desc."""
    return _lib.TrainDesc(n_layer, n_embd, state_dim, action_dim, n_positions, batch, window, flags, dropout, 0,
                          seed)


def _numel(fn, d):
    n = ctypes.c_int64()
    _lib.call(fn, ctypes.byref(d), ctypes.byref(n))
    return n.value


def forward(d, blob, tokens):
    """preds (batch, window, A) at every position + the workspace the backward needs."""
    dev = device()
    _on_device(blob, tokens)
    if tokens.shape != (d.batch, d.window, 2 * d.state_dim + d.action_dim + 1):
        raise ValueError(f"tokens {tuple(tokens.shape)} do not match the description")
    ws = torch.empty(_numel("dpt_train_workspace_numel", d), dtype=torch.float32, device=dev)
    preds = torch.empty((d.batch, d.window, d.action_dim), dtype=torch.float32, device=dev)
    _lib.call("dpt_train_forward", ctypes.byref(d), _p(blob), _p(tokens), _p(ws), _p(preds), _stream())
    return preds, ws


def backward(d, blob, tokens, ws, dpreds):
    """dL/dblob (packed order) from dL/dpreds (batch, window, A)."""
    dblob = torch.empty(_numel("dpt_train_blob_numel", d), dtype=torch.float32, device=blob.device)
    dp = dpreds.to(torch.float32).contiguous()
    _on_device(blob, tokens, ws, dp)
    if dp.shape != (d.batch, d.window, d.action_dim):
        raise ValueError(f"dpreds {tuple(dp.shape)} do not match the description")
    _lib.call(GRAD_BACKWARD, ctypes.byref(d), _p(blob), _p(tokens), _p(ws), _p(dp), _p(dblob), _stream())
    return dblob


class TransformerFunction(torch.autograd.Function):
    """preds (B, T, A) = Transformer(tokens) at every position, with the HIP backward."""

    @staticmethod
    def forward(ctx, tokens, dims, *params):
        # dims[7] (optional) = FORWARD_ONLY when the caller runs without autograd (no_grad, or
        # no parameter requires grad): the forward-only workspace (one layer's activations, no
        # attention probabilities, no backward scratch) -- and nothing saved for a backward
        # dims[8:10] (optional) = (dropout p, Philox seed of this forward's masks)
        flags = dims[7] if len(dims) > 7 else 0
        p, seed = (float(dims[8]), int(dims[9])) if len(dims) > 9 else (0.0, 0)
        # | LAST_ONLY (with FORWARD_ONLY, no dropout): only preds[:, -1] is written (the caller reads no other row)
        need = any(ctx.needs_input_grad[2:]) and not flags & FORWARD_ONLY
        last = bool(flags & LAST_ONLY) and p == 0.0
        d = desc(*dims[:7], flags=0 if need else FORWARD_ONLY | (LAST_ONLY if last else 0), dropout=p, seed=seed)
        dev = device()
        blob = pack_params(params, dev)
        if blob.numel() != _numel("dpt_train_blob_numel", d):
            raise ValueError("parameter shapes do not match the model description")
        tok = tokens.to(device=dev, dtype=torch.float32).contiguous()
        preds, ws = forward(d, blob, tok)
        if need:
            ctx.d, ctx.blob, ctx.tok, ctx.ws = d, blob, tok, ws
            ctx.params_meta = ([p.shape for p in params], [p.dtype for p in params], [p.device for p in params])
        # forward-only requested although a parameter requires grad: nothing is saved, so a
        # backward through this node must say so (not the retain_graph message below)
        ctx.forward_only = bool(flags & FORWARD_ONLY) and any(ctx.needs_input_grad[2:])
        return preds

    @staticmethod
    def backward(ctx, dpreds):
        if getattr(ctx, "forward_only", False):
            raise RuntimeError("dpt_hip.train: this forward ran with FORWARD_ONLY (no activations saved) while "
                               "parameters require grad; drop the FORWARD_ONLY flag to train through it")
        if getattr(ctx, "ws", None) is None:
            raise RuntimeError("dpt_hip.train: the saved activations were released by the first backward; "
                               "a second backward through the same graph (retain_graph=True) is not supported")
        dblob = backward(ctx.d, ctx.blob, ctx.tok, ctx.ws, dpreds)
        shapes, dtypes, devs = ctx.params_meta
        grads = [g if g.device == dv else g.to(dv) for g, dv in zip(_unpack(dblob, shapes, dtypes), devs)]
        ctx.ws = None  # the saved activations are not needed again
        return (None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))


# ----------------------------------------------------------------------------- image-conditioned DPT
IMAGE_SIZE = 25  # the only image size the front end is built for


def image_desc(rows, state_dim, action_dim, n_embd, flags=0, dropout=0.0, seed=0, image_size=IMAGE_SIZE):
    """dpt_image_desc of the image front end (encoder -> embed_transition -> embed_ln) over ``rows``
    images; ``dropout`` / ``seed`` as in the step's dpt_train_desc (the encoder's nn.Dropout)."""
    return _lib.ImageDesc(image_size, rows, state_dim, action_dim, n_embd, flags, dropout, 0, seed)


def front_forward(d, blob, images, feats):
    """embeds (rows, E) = embed_ln(embed_transition([encoder(images) | feats])) + the workspace the
    backward needs.  images (rows, 3, 25, 25) normalised fp32, feats (rows, sd + A + 1)."""
    _on_device(blob, images, feats)
    if tuple(images.shape) != (d.rows, 3, d.image_size, d.image_size) or \
            tuple(feats.shape) != (d.rows, d.state_dim + d.action_dim + 1):
        raise ValueError(f"images {tuple(images.shape)} / feats {tuple(feats.shape)} do not match the description")
    if blob.numel() != _numel("dpt_image_front_blob_numel", d):
        raise ValueError("front parameter shapes do not match the description")
    ws = torch.empty(_numel("dpt_image_front_workspace_numel", d), dtype=torch.float32, device=blob.device)
    embeds = torch.empty((d.rows, d.n_embd), dtype=torch.float32, device=blob.device)
    _lib.call("dpt_image_front_forward", ctypes.byref(d), _p(blob), _p(images), _p(feats), _p(ws), _p(embeds),
              _stream())
    return embeds, ws


def front_backward(d, blob, images, feats, ws, dembeds):
    """dL/d(front blob) (front blob order) from dL/dembeds (rows, E)."""
    de = dembeds.to(torch.float32).contiguous()
    _on_device(blob, images, feats, ws, de)
    if tuple(de.shape) != (d.rows, d.n_embd):
        raise ValueError(f"dembeds {tuple(de.shape)} do not match the description")
    dblob = torch.empty(_numel("dpt_image_front_blob_numel", d), dtype=torch.float32, device=blob.device)
    _lib.call("dpt_image_front_backward", ctypes.byref(d), _p(blob), _p(images), _p(feats), _p(ws), _p(de),
              _p(dblob), _stream())
    return dblob


def forward_embeds(d, blob, embeds):
    """``forward`` with the token embedding skipped (dpt_train_forward_embeds): embeds (batch, window, E)
    enter as x0 = drop(embeds + wpe); the blob keeps its layout and its emb_w / emb_b region is not read."""
    _on_device(blob, embeds)
    if embeds.numel() != d.batch * d.window * d.n_embd:
        raise ValueError(f"embeds {tuple(embeds.shape)} do not match the description")
    ws = torch.empty(_numel("dpt_train_workspace_numel", d), dtype=torch.float32, device=blob.device)
    preds = torch.empty((d.batch, d.window, d.action_dim), dtype=torch.float32, device=blob.device)
    _lib.call("dpt_train_forward_embeds", ctypes.byref(d), _p(blob), _p(embeds), _p(ws), _p(preds), _stream())
    return preds, ws


def backward_embeds(d, blob, ws, dpreds):
    """(dL/dblob with an exactly zero emb_w / emb_b region, dL/dembeds (batch, window, E))."""
    dp = dpreds.to(torch.float32).contiguous()
    _on_device(blob, ws, dp)
    if dp.shape != (d.batch, d.window, d.action_dim):
        raise ValueError(f"dpreds {tuple(dp.shape)} do not match the description")
    dblob = torch.empty(_numel("dpt_train_blob_numel", d), dtype=torch.float32, device=blob.device)
    dembeds = torch.empty((d.batch, d.window, d.n_embd), dtype=torch.float32, device=blob.device)
    _lib.call("dpt_train_backward_embeds", ctypes.byref(d), _p(blob), _p(ws), _p(dp), _p(dblob), _p(dembeds),
              _stream())
    return dblob, dembeds


def image_param_list(model):
    """An ImageTransformer's parameters as the image function takes them: the front end in front-blob
    order (dpt_hip.FRONT_KEYS), then the trunk in blob order without embed_transition."""
    from . import FRONT_KEYS
    named = dict(model.named_parameters())
    return [named[k] for k in FRONT_KEYS] + param_list(model)[2:]


N_FRONT = 10  # parameters of the front end (dpt_hip.FRONT_KEYS)


def pack_image_params(params, emb_numel, dev):
    """(front blob, trunk blob) of ``image_param_list``'s parameters; the trunk blob keeps the
    dpt_train_desc layout with a zero emb_w / emb_b region of ``emb_numel`` floats (never read)."""
    from . import FRONT_KEYS, pack_front
    with torch.no_grad():
        ps = [p.detach().to(device=dev, dtype=torch.float32) for p in params]
        front = pack_front(dict(zip(FRONT_KEYS, ps[:N_FRONT])))
        trunk = ps[N_FRONT:]
        trunk[-2] = trunk[-2].t()  # pred_actions.weight: [out][in] -> [in][out]
        tblob = torch.cat([torch.zeros(emb_numel, dtype=torch.float32, device=dev)] + [p.reshape(-1) for p in trunk])
    return front, tblob


def unpack_image_grads(dfront, dtrunk, emb_numel, shapes):
    """Per-parameter gradients (``image_param_list`` order, shaped like the parameters) from the two
    gradient blobs."""
    out, off = [], 0
    for i, sh in enumerate(shapes[:N_FRONT]):
        n = int(torch.Size(sh).numel())
        flat = dfront[off:off + n]
        out.append(flat.view(sh[1], sh[0]).t() if i in (4, 6) else flat.view(sh))  # fc / embed_transition weights
        off += n
    if off != dfront.numel():
        raise ValueError(f"front gradient blob {dfront.numel()} != parameters {off}")
    off, n_all = emb_numel, len(shapes)
    for i, sh in enumerate(shapes[N_FRONT:], N_FRONT):
        n = int(torch.Size(sh).numel())
        flat = dtrunk[off:off + n]
        out.append(flat.view(sh[1], sh[0]).t() if i == n_all - 2 else flat.view(sh))
        off += n
    if off != dtrunk.numel():
        raise ValueError(f"gradient blob {dtrunk.numel()} != parameters {off}")
    return out


class ImageTransformerFunction(torch.autograd.Function):
    """preds (B, T, A) = ImageTransformer(images, feats) at every position: the HIP image front end
    chained into the trunk (front forward -> dpt_train_forward_embeds) and, in ``backward``, the
    trunk's backward handing dL/dembeds to the front end's.  ``dims`` as TransformerFunction's:
    (n_layer, n_embd, state_dim, action_dim, n_positions, batch, window, flags, dropout p, seed);
    ``params`` = ``image_param_list(model)``."""

    @staticmethod
    def forward(ctx, images, feats, dims, *params):
        L, E, sd, A, npos, B, T = (int(v) for v in dims[:7])
        flags = dims[7] if len(dims) > 7 else 0
        p, seed = (float(dims[8]), int(dims[9])) if len(dims) > 9 else (0.0, 0)
        need = any(ctx.needs_input_grad[3:]) and not flags & FORWARD_ONLY
        last = bool(flags & LAST_ONLY) and p == 0.0
        td = desc(L, E, sd, A, npos, B, T, flags=0 if need else FORWARD_ONLY | (LAST_ONLY if last else 0), dropout=p,
                  seed=seed)
        fd = image_desc(B * T, sd, A, E, flags=0 if need else FORWARD_ONLY, dropout=p, seed=seed)
        dev = device()
        emb_numel = (2 * sd + A + 1) * E + E
        fblob, tblob = pack_image_params(params, emb_numel, dev)
        if tblob.numel() != _numel("dpt_train_blob_numel", td):
            raise ValueError("parameter shapes do not match the model description")
        img = images.to(device=dev, dtype=torch.float32).reshape(B * T, 3, IMAGE_SIZE, IMAGE_SIZE).contiguous()
        ft = feats.to(device=dev, dtype=torch.float32).reshape(B * T, sd + A + 1).contiguous()
        embeds, fws = front_forward(fd, fblob, img, ft)
        preds, tws = forward_embeds(td, tblob, embeds)
        if need:
            ctx.saved = (td, fd, fblob, tblob, img, ft, fws, tws, emb_numel)
            ctx.params_meta = ([tuple(q.shape) for q in params], [q.dtype for q in params], [q.device for q in params])
        ctx.forward_only = bool(flags & FORWARD_ONLY) and any(ctx.needs_input_grad[3:])
        return preds

    @staticmethod
    def backward(ctx, dpreds):
        if getattr(ctx, "forward_only", False):
            raise RuntimeError("dpt_hip.train: this forward ran with FORWARD_ONLY (no activations saved) while "
                               "parameters require grad; drop the FORWARD_ONLY flag to train through it")
        if getattr(ctx, "saved", None) is None:
            raise RuntimeError("dpt_hip.train: the saved activations were released by the first backward; "
                               "a second backward through the same graph (retain_graph=True) is not supported")
        td, fd, fblob, tblob, img, ft, fws, tws, emb_numel = ctx.saved
        dtrunk, dembeds = backward_embeds(td, tblob, tws, dpreds)
        dfront = front_backward(fd, fblob, img, ft, fws, dembeds.view(fd.rows, fd.n_embd))
        shapes, dtypes, devs = ctx.params_meta
        grads = unpack_image_grads(dfront, dtrunk, emb_numel, shapes)
        grads = [g.to(device=dv, dtype=dt) for g, dt, dv in zip(grads, dtypes, devs)]
        ctx.saved = None  # the saved activations are not needed again
        return (None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:]))


DATA_KEYS = ("query_states", "context_states", "context_actions", "context_next_states", "context_rewards",
             "optimal_actions")


class DeviceData:
    """The training set as dpt_train_data: contiguous fp32 device tensors (dataset.py's
    ``Dataset.dataset`` dict, or the ``Dataset`` itself) and the struct that points at them."""

    def __init__(self, dataset):
        src = getattr(dataset, "dataset", dataset)
        dev = device()
        self.tensors = {k: _dev(src[k], torch.float32, dev) for k in DATA_KEYS}
        q, cs, ca, opt = (self.tensors[k] for k in ("query_states", "context_states", "context_actions",
                                                    "optimal_actions"))
        if q.dim() != 2 or cs.dim() != 3 or ca.dim() != 3 or opt.dim() != 2:
            raise ValueError("dpt_hip.train: expected query (n, sd), context (n, H, .), optimal_actions (n, A)")
        self.n, self.horizon, self.state_dim = int(cs.shape[0]), int(cs.shape[1]), int(cs.shape[2])
        self.action_dim = int(ca.shape[2])
        want = {"query_states": (self.n, self.state_dim), "context_states": (self.n, self.horizon, self.state_dim),
                "context_actions": (self.n, self.horizon, self.action_dim),
                "context_next_states": (self.n, self.horizon, self.state_dim),
                "optimal_actions": (self.n, self.action_dim)}
        for k, shape in want.items():
            if tuple(self.tensors[k].shape) != shape:
                raise ValueError(f"dpt_hip.train: {k} {tuple(self.tensors[k].shape)} != {shape}")
        if self.tensors["context_rewards"].numel() != self.n * self.horizon:  # (n, H) or (n, H, 1)
            raise ValueError("dpt_hip.train: context_rewards must hold one reward per transition")
        self.struct = _lib.TrainData(self.n, self.horizon, 0, *(_p(self.tensors[k]).value for k in DATA_KEYS))

    def __len__(self):
        return self.n


def _index_tensors(data, index, perm, dev):
    idx = torch.as_tensor(index, dtype=torch.int64).reshape(-1).to(dev).contiguous()
    pm = None
    if perm is not None:
        pm = torch.as_tensor(perm, dtype=torch.int64).to(dev).contiguous()
        if tuple(pm.shape) != (idx.numel(), data.horizon):
            raise ValueError(f"perm {tuple(pm.shape)} != (batch {idx.numel()}, horizon {data.horizon})")
    if idx.numel() < 1:
        raise ValueError("empty batch")
    return idx, pm


class Trainer:
    """The fused device training step of train.py:286-310 for a models.net.Transformer.

    Holds the fp32 master weights as one packed blob (include/dpt_hip.h layout), AdamW's ``m`` and
    ``v`` in the same layout, the step count, the workspace and a float64 loss accumulator, all on
    the device.  ``step`` is one dpt_train_step: batch packing, forward, summed cross-entropy,
    backward and the AdamW update as a chain of launches on the current stream, with no host
    synchronisation; ``read_loss`` is the only call that waits for the device.  The module's own
    parameters are not touched until ``sync_to_model``."""

    def __init__(self, model, lr, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8):
        self.model = model
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), tuple(betas), float(eps)
        dev = device()
        self.blob = pack_params(param_list(model), dev)
        self.m = torch.zeros_like(self.blob)
        self.v = torch.zeros_like(self.blob)
        self.steps = 0
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self._ws = None
        self._ws_batch = self._ws_window = 0  # the workspace grows to the largest batch seen
        self._data = {}

    def device_data(self, data):
        """``data`` as DeviceData (a Dataset / dict is converted once and kept)."""
        if isinstance(data, DeviceData):
            return data
        dd = self._data.get(id(data))
        if dd is None or dd[0] is not data:
            dd = self._data[id(data)] = (data, DeviceData(data))
        return dd[1]

    def _desc(self, data, batch):
        m = self.model
        if (data.state_dim, data.action_dim) != (m.state_dim, m.action_dim):
            raise ValueError(f"dataset (sd {data.state_dim}, A {data.action_dim}) does not match the model "
                             f"(sd {m.state_dim}, A {m.action_dim})")
        p, seed = 0.0, 0
        if m.dropout > 0:  # fresh masks per call; the reference's test loss runs in training mode too
            from models.net import _dropout_seed
            p, seed = float(m.dropout), _dropout_seed()
        cap = max(batch, self._ws_batch)
        d = desc(m.n_layer, m.n_embd, m.state_dim, m.action_dim, m.n_positions, cap, 1 + data.horizon, dropout=p,
                 seed=seed)
        if self._ws is None or cap > self._ws_batch or self._ws_window != d.window:
            self._ws = torch.empty(_numel("dpt_train_step_workspace_numel", d), dtype=torch.float32,
                                   device=self.blob.device)
            self._ws_batch, self._ws_window = cap, d.window
        return d

    def step(self, data, index, perm=None):
        """One training step on the samples ``index`` (int64; ``perm`` (batch, horizon): each
        sample's context permutation, dataset.py:84-89).  Adds the batch's summed loss to the
        accumulator."""
        data = self.device_data(data)
        idx, pm = _index_tensors(data, index, perm, self.blob.device)
        d = self._desc(data, idx.numel())
        self.steps += 1
        args = _lib.AdamWArgs(self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.steps)
        try:
            _lib.call("dpt_train_step", ctypes.byref(d), ctypes.byref(data.struct), _p(idx), _p(pm), idx.numel(),
                      _p(self.blob), _p(self.m), _p(self.v), ctypes.byref(args), _p(self._ws), _p(self.loss),
                      _stream())
        except Exception:
            self.steps -= 1  # rejected on the host before any launch
            raise

    def eval_loss(self, data, index, perm=None):
        """The test loss of train.py:265-278 on the samples ``index`` (forward only, the model's
        dropout active); adds the batch's summed loss to the accumulator."""
        data = self.device_data(data)
        idx, pm = _index_tensors(data, index, perm, self.blob.device)
        d = self._desc(data, idx.numel())
        _lib.call("dpt_train_eval_loss", ctypes.byref(d), ctypes.byref(data.struct), _p(idx), _p(pm), idx.numel(),
                  _p(self.blob), _p(self._ws), _p(self.loss), _stream())

    def read_loss(self):
        """The accumulated loss sum (one device synchronisation), then reset to zero."""
        val = float(self.loss.item())
        self.loss.zero_()
        return val

    def sync_to_model(self):
        """Unpack the master blob into the module's parameters (wte, which the model never reads,
        is untouched)."""
        params = param_list(self.model)
        with torch.no_grad():
            for p, w in zip(params, _unpack(self.blob, [p.shape for p in params], [p.dtype for p in params])):
                p.copy_(w)
        return self.model


IMAGE_DATA_KEYS = ("query_states", "context_states", "context_actions", "context_rewards", "optimal_actions")


def normalize_images(raw, out=None):
    """``raw`` (n, 25, 25, 3) float64 / float32 HWC in [0, 1] (numpy or torch, host or device) ->
    (n, 3, 25, 25) fp32 on the device, bit-equal to ``dataset.image_transform(x).float()`` per image
    (dpt_image_normalize).  ``out``: write into this contiguous fp32 device tensor of n * 1875 floats."""
    dev = device()
    t = raw if isinstance(raw, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(raw))
    code = _lib.IMAGE_RAW_DTYPES.get(str(t.dtype).replace("torch.", ""))
    if code is None:
        raise TypeError(f"normalize_images: expected float64 or float32 images in [0, 1], got {t.dtype}")
    if t.dim() != 4 or tuple(t.shape[1:]) != (IMAGE_SIZE, IMAGE_SIZE, 3):
        raise ValueError(f"normalize_images: raw {tuple(t.shape)} != (n, {IMAGE_SIZE}, {IMAGE_SIZE}, 3)")
    t = t.to(dev).contiguous()
    n = int(t.shape[0])
    if out is None:
        out = torch.empty((n, 3, IMAGE_SIZE, IMAGE_SIZE), dtype=torch.float32, device=dev)
    if not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == n * 1875):
        raise ValueError("normalize_images: `out` must be a contiguous fp32 device tensor of n * 1875 floats")
    _lib.call("dpt_image_normalize", _p(t), code, n, _p(out), _stream())
    return out


class DeviceImageData:
    """The image training set as dpt_image_data: dataset.py's ``ImageDataset`` with every image resident
    on the device, normalised, in fp32.  Each trajectory's ``.npy`` stack is read once (and every
    ``query_image``), the raw stacks are uploaded in chunks of at most ``chunk_bytes`` and normalised
    there by dpt_image_normalize: no per-image host work.  The images take n (1 + horizon) 7,500 bytes.
    ``from_arrays`` takes a collated batch dict whose images are normalised already."""

    def __init__(self, image_dataset, chunk_bytes=256 << 20):
        dev = device()
        src = image_dataset.dataset
        self._states(src, dev)
        paths, trajs = src["context_filepaths"], image_dataset.trajs
        if len(paths) != self.n or len(trajs) != self.n:
            raise ValueError(f"dpt_hip.train: {len(paths)} image stacks for {self.n} samples")
        try:
            qi = torch.empty((self.n, 3, IMAGE_SIZE, IMAGE_SIZE), dtype=torch.float32, device=dev)
            ci = torch.empty((self.n, self.horizon, 3, IMAGE_SIZE, IMAGE_SIZE), dtype=torch.float32, device=dev)
        except torch.cuda.OutOfMemoryError as e:
            raise MemoryError(f"DeviceImageData: {self.n} samples at horizon {self.horizon} need "
                              f"{self.image_bytes} bytes of device memory for their images") from e
        self.chunks = 0  # uploads made (one normalise launch each)
        self._fill(qi, (np.asarray(t["query_image"])[None] for t in trajs), 1, chunk_bytes)
        self._fill(ci, (np.load(p) for p in paths), self.horizon, chunk_bytes)
        self._images(qi, ci)

    @classmethod
    def from_arrays(cls, arrays):
        """The resident set of a batch dict as ``ImageDataset``'s items collate to (``query_images`` (n, 3,
        25, 25) and ``context_images`` (n, H, 3, 25, 25) normalised already, plus IMAGE_DATA_KEYS)."""
        self, dev = cls.__new__(cls), device()
        self._states(arrays, dev)
        self.chunks = 0
        self._images(*(_dev(arrays[k], torch.float32, dev) for k in ("query_images", "context_images")))
        return self

    def _images(self, qi, ci):
        want = {"query_images": (self.n, 3, IMAGE_SIZE, IMAGE_SIZE),
                "context_images": (self.n, self.horizon, 3, IMAGE_SIZE, IMAGE_SIZE)}
        for k, t in (("query_images", qi), ("context_images", ci)):
            if tuple(t.shape) != want[k]:
                raise ValueError(f"dpt_hip.train: {k} {tuple(t.shape)} != {want[k]}")
            self.tensors[k] = t
        self.struct = _lib.ImageData(self.n, self.horizon, IMAGE_SIZE,
                                     *(_p(self.tensors[k]).value for k in IMAGE_DATA_KEYS + ("query_images",
                                                                                            "context_images")))

    def _states(self, src, dev):
        self.tensors = {k: _dev(src[k], torch.float32, dev) for k in IMAGE_DATA_KEYS}
        cs, ca = self.tensors["context_states"], self.tensors["context_actions"]
        if cs.dim() != 3 or ca.dim() != 3:
            raise ValueError("dpt_hip.train: expected context (n, H, .) arrays")
        self.n, self.horizon, self.state_dim = int(cs.shape[0]), int(cs.shape[1]), int(cs.shape[2])
        self.action_dim = int(ca.shape[2])
        want = {"query_states": (self.n, self.state_dim), "context_actions": (self.n, self.horizon, self.action_dim),
                "optimal_actions": (self.n, self.action_dim)}
        for k, shape in want.items():
            if tuple(self.tensors[k].shape) != shape:
                raise ValueError(f"dpt_hip.train: {k} {tuple(self.tensors[k].shape)} != {shape}")
        if self.tensors["context_rewards"].numel() != self.n * self.horizon:  # (n, H) or (n, H, 1)
            raise ValueError("dpt_hip.train: context_rewards must hold one reward per transition")
        self.image_bytes = self.n * (1 + self.horizon) * 4 * 3 * IMAGE_SIZE * IMAGE_SIZE

    def _fill(self, out, stacks, per_item, chunk_bytes):
        """normalise the items' raw stacks ((per_item, 25, 25, 3) each) into ``out`` in item order: one
        upload and one launch per chunk of items of one dtype holding at most ``chunk_bytes``"""
        flat = out.view(-1, 3, IMAGE_SIZE, IMAGE_SIZE)
        pending, held, done = [], 0, 0

        def flush():
            nonlocal pending, held, done
            if pending:
                raw = np.concatenate(pending)
                normalize_images(raw, flat[done:done + raw.shape[0]])
                done += raw.shape[0]
                self.chunks += 1
            pending, held = [], 0
        for stack in stacks:
            if stack.shape != (per_item, IMAGE_SIZE, IMAGE_SIZE, 3):
                raise ValueError(f"dpt_hip.train: image stack {stack.shape} != "
                                 f"{(per_item, IMAGE_SIZE, IMAGE_SIZE, 3)}")
            if pending and (stack.dtype != pending[0].dtype or held + stack.nbytes > chunk_bytes):
                flush()
            pending.append(stack)
            held += stack.nbytes
        flush()
        if done != flat.shape[0]:
            raise ValueError(f"dpt_hip.train: {done} images read for {flat.shape[0]} slots")

    def __len__(self):
        return self.n


class ImageTrainer:
    """The fused device training step of train_miniworld.py for a models.net.ImageTransformer.

    Built like ``Trainer``: the fp32 master weights as two packed blobs (the trunk in the
    dpt_train_desc layout with a zero emb_w / emb_b region, the front end in the front-blob layout),
    AdamW's ``m`` and ``v`` for each, the step count, the workspace and a float64 loss accumulator, all
    on the device.  ``step`` is one dpt_image_train_step: the batch gathered from the resident image
    set, the image front end, the trunk, the summed cross-entropy, both backwards and the two AdamW
    updates as a chain of launches on the current stream, with no host synchronisation; ``read_loss``
    is the only call that waits for the device.  The module's own parameters are not touched until
    ``sync_to_model``."""

    def __init__(self, model, lr, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8):
        self.model = model
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), tuple(betas), float(eps)
        dev = device()
        self.emb_numel = (2 * model.state_dim + model.action_dim + 1) * model.n_embd + model.n_embd
        self.front_blob, self.blob = pack_image_params(image_param_list(model), self.emb_numel, dev)
        self.m, self.v = torch.zeros_like(self.blob), torch.zeros_like(self.blob)
        self.front_m, self.front_v = torch.zeros_like(self.front_blob), torch.zeros_like(self.front_blob)
        self.steps = 0
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self._ws = None
        self._ws_batch = self._ws_window = 0  # the workspace grows to the largest batch seen
        self._data = {}

    def device_data(self, data, **kw):
        """``data`` as DeviceImageData (an ImageDataset is converted once and kept)."""
        if isinstance(data, DeviceImageData):
            return data
        dd = self._data.get(id(data))
        if dd is None or dd[0] is not data:
            dd = self._data[id(data)] = (data, DeviceImageData(data, **kw))
        return dd[1]

    def _desc(self, data, batch, seed):
        m = self.model
        if (data.state_dim, data.action_dim) != (m.state_dim, m.action_dim):
            raise ValueError(f"dataset (sd {data.state_dim}, A {data.action_dim}) does not match the model "
                             f"(sd {m.state_dim}, A {m.action_dim})")
        p = 0.0
        if m.dropout > 0:  # fresh masks per call; the reference's test loss runs in training mode too
            p = float(m.dropout)
            if seed is None:
                from models.net import _dropout_seed
                seed = _dropout_seed()
        cap = max(batch, self._ws_batch)
        d = desc(m.n_layer, m.n_embd, m.state_dim, m.action_dim, m.n_positions, cap, 1 + data.horizon, dropout=p,
                 seed=(int(seed) & (2 ** 64 - 1)) if p > 0 else 0)
        if self._ws is None or cap > self._ws_batch or self._ws_window != d.window:
            self._ws = torch.empty(_numel("dpt_image_train_step_workspace_numel", d), dtype=torch.float32,
                                   device=self.blob.device)
            self._ws_batch, self._ws_window = cap, d.window
        return d

    def step(self, data, index, perm=None, seed=None):
        """One training step on the samples ``index`` (int64; ``perm`` (batch, horizon): each sample's
        context permutation).  ``seed``: the Philox seed of this step's dropout masks (default: a fresh
        one from the CUDA generator, as ``Trainer`` draws it).  Adds the batch's summed loss to the
        accumulator."""
        data = self.device_data(data)
        idx, pm = _index_tensors(data, index, perm, self.blob.device)
        d = self._desc(data, idx.numel(), seed)
        self.steps += 1
        args = _lib.AdamWArgs(self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.steps)
        try:
            _lib.call("dpt_image_train_step", ctypes.byref(d), ctypes.byref(data.struct), _p(idx), _p(pm),
                      idx.numel(), _p(self.blob), _p(self.m), _p(self.v), _p(self.front_blob), _p(self.front_m),
                      _p(self.front_v), ctypes.byref(args), _p(self._ws), _p(self.loss), _stream())
        except Exception:
            self.steps -= 1  # rejected on the host before any launch
            raise

    def eval_loss(self, data, index, perm=None, seed=None):
        """The test loss on the samples ``index`` (both forwards only, the model's dropout active); adds
        the batch's summed loss to the accumulator."""
        data = self.device_data(data)
        idx, pm = _index_tensors(data, index, perm, self.blob.device)
        d = self._desc(data, idx.numel(), seed)
        _lib.call("dpt_image_train_eval_loss", ctypes.byref(d), ctypes.byref(data.struct), _p(idx), _p(pm),
                  idx.numel(), _p(self.blob), _p(self.front_blob), _p(self._ws), _p(self.loss), _stream())

    read_loss = Trainer.read_loss

    def sync_to_model(self):
        """Unpack both master blobs into the module's parameters (wte, which the model never reads, is
        untouched)."""
        params = image_param_list(self.model)
        views = unpack_image_grads(self.front_blob, self.blob, self.emb_numel, [tuple(p.shape) for p in params])
        with torch.no_grad():
            for p, w in zip(params, views):
                p.copy_(w)
        return self.model


def rollout_bandit_generic(model, means, H, var, sample=True, bandit_type=0, seed=0, first_task=0, uniforms=None,
                           noise=None, want_logits=False, counter=0, f32=False, blob=None, env_actions=None,
                           random_env=None):
    """The fused online bandit rollout (evals/eval_bandit.py:56-103) for a Transformer of any width
    (dpt_rollout_bandit_generic: exact K/V-cache decode, one step for all tasks at a time, the
    draws / selection / env step of DeviceModel.rollout_bandit).  Same arguments and result dict
    as DeviceModel.rollout_bandit: actions (N,H) int32, rewards (N,H) f64, arm_value (N,H) f64,
    logits (H,N,A) f32 if requested.  ``f32``: GPUBanditEnv's fp32 reward arithmetic (DPT_BANDIT_F32);
    ``blob``: run on this packed blob (a trainer's master weights) instead of the module's parameters.
    ``env_actions`` (H, N) int32 / ``random_env=True``: step the env with these arms (clamped to
    [0, A)) or with uniformly random ones (Philox stream STREAM_ENVACT) instead of the selected action,
    which still goes into ``actions`` and the context (dpt_rollout_bandit_generic_env; ``random_env=False``
    takes that entry point with the option off); the result then also holds ``env_actions`` (N, H)
    int32, the arms the env was stepped with."""
    dev = device()
    means_d = _dev(means, torch.float64, dev)
    N, A = means_d.shape
    if f32:
        bandit_type = int(bandit_type) | _lib.BANDIT_F32
    H = int(H)
    out = dict(actions=torch.empty((N, H), dtype=torch.int32, device=dev),
               rewards=torch.empty((N, H), dtype=torch.float64, device=dev),
               arm_value=torch.empty((N, H), dtype=torch.float64, device=dev))
    out["logits"] = torch.empty((H, N, A), dtype=torch.float32, device=dev) if want_logits else None
    separate = env_actions is not None or random_env is not None
    ea_d = None
    if separate:
        out["env_actions"] = torch.empty((N, H), dtype=torch.int32, device=dev)
        if env_actions is not None:
            ea_d = _dev(env_actions, torch.int32, dev)
            if tuple(ea_d.shape) != (H, N):
                raise ValueError(f"env_actions {tuple(ea_d.shape)} != (H = {H}, N = {N})")
    if N == 0 or H == 0:
        return out
    d = desc(model.n_layer, model.n_embd, model.state_dim, model.action_dim, model.n_positions, 1, 1)
    n = ctypes.c_int64()
    _lib.call("dpt_rollout_bandit_generic_workspace_numel", ctypes.byref(d), N, H, ctypes.byref(n))
    ws = torch.empty(n.value, dtype=torch.float32, device=dev)
    if blob is None:
        blob = pack_params(param_list(model), dev)
    _on_device(blob)
    u_d = None if uniforms is None else _dev(uniforms, torch.float64, dev)
    g_d = None if noise is None else _dev(noise, torch.float64, dev)
    args = _lib.BanditRolloutArgs(
        N, H, A, int(bandit_type), int(bool(sample)), 0, int(first_task), float(var), int(seed) & (2 ** 64 - 1),
        _p(means_d).value, None if u_d is None else _p(u_d).value, None if g_d is None else _p(g_d).value,
        _p(ws).value, _p(out["actions"]).value, _p(out["rewards"]).value, _p(out["arm_value"]).value,
        None if out["logits"] is None else _p(out["logits"]).value, int(counter) & (2 ** 64 - 1))
    if separate:
        _lib.call("dpt_rollout_bandit_generic_env", ctypes.byref(d), _p(blob), ctypes.byref(args), _p(ea_d),
                  int(bool(random_env)), _p(out["env_actions"]), _stream())
    else:
        _lib.call("dpt_rollout_bandit_generic", ctypes.byref(d), _p(blob), ctypes.byref(args), _stream())
    out["_keep"] = (ws, blob, means_d, u_d, g_d, ea_d)
    return out


def chunk_plan(n, chunk):
    """[(offset, size), ...] covering ``n`` envs in chunks of ``chunk`` (0: all at once)."""
    n, chunk = int(n), int(chunk)
    if n < 1 or chunk < 0:
        raise ValueError(f"chunk_plan: n={n} chunk={chunk}")
    size = n if chunk == 0 else min(chunk, n)
    return [(off, min(size, n - off)) for off in range(0, n, size)]


class InteractiveTrainer:
    """The fused interactive (on-policy) bandit step of train_interactive.py:92-143 for a
    models.net.Transformer with state_dim 1 and no dropout.

    Built like ``Trainer``: the fp32 master blob, AdamW's ``m`` and ``v``, the gradient blob, the
    step count, the workspace and a float64 loss accumulator live on the device.  ``step`` runs one
    dpt_interactive_grad per chunk of envs (K - 1 sampled rollout steps from the blob, the window
    packed from the records, forward, last-position cross-entropy scaled by 1 / N, backward), the
    chunks' gradients added in chunk order, then one dpt_adamw_step -- all on the current stream
    with no host synchronisation; ``read_loss`` is the only call that waits for the device."""

    def __init__(self, model, lr, weight_decay=1e-4, chunk=0, betas=(0.9, 0.999), eps=1e-8, full_width=False):
        # full_width: the last block for every row instead of the last one (DPT_INTERACTIVE_FULL_WIDTH; A/B runs)
        self.full_width = bool(full_width)
        if model.state_dim != 1:
            raise ValueError(f"InteractiveTrainer: state_dim={model.state_dim} (bandits have state_dim 1)")
        if model.dropout != 0:
            raise ValueError("InteractiveTrainer: dropout must be 0 (the cached decode has no dropout masks)")
        if int(chunk) < 0:
            raise ValueError(f"InteractiveTrainer: chunk={chunk}")
        self.model, self.chunk = model, int(chunk)
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), tuple(betas), float(eps)
        dev = device()
        self.blob = pack_params(param_list(model), dev)
        self.m = torch.zeros_like(self.blob)
        self.v = torch.zeros_like(self.blob)
        self.dblob = torch.empty_like(self.blob)
        self.steps = 0
        self.loss = torch.zeros(1, dtype=torch.float64, device=dev)
        self._ws = None
        self._ws_shape = (0, 0)  # (chunk envs, K) the workspace was sized for

    def _desc(self):
        m = self.model
        return desc(m.n_layer, m.n_embd, m.state_dim, m.action_dim, m.n_positions, 1, 1)

    def _workspace(self, d, n, K):
        if self._ws is not None and self._ws_shape == (n, K):
            return self._ws
        need = ctypes.c_int64()
        _lib.call("dpt_interactive_workspace_numel", ctypes.byref(d), n, K, ctypes.byref(need))
        self._ws = None  # release the old one first
        try:
            self._ws = torch.empty(need.value, dtype=torch.float32, device=self.blob.device)
        except torch.cuda.OutOfMemoryError as e:
            raise MemoryError(f"InteractiveTrainer: one chunk of {n} envs at K={K} needs a workspace of "
                              f"{4 * need.value} bytes; pass a smaller `chunk` (now {self.chunk}; 0 = all envs at "
                              f"once)") from e
        self._ws_shape = (n, K)
        return self._ws

    def step(self, means, K, var, bandit_type, uniforms=None, noise=None, seed=None, targets=None):
        """One episode: ``means`` (N, A) arm means, ``K`` the window (K - 1 rolled-out steps),
        ``bandit_type`` 'uniform' / 'bernoulli' (or a DPT_BANDIT_* code), ``targets`` (N) int64 the
        optimal arms (default: argmax of means, GPUBanditEnv.opt_a_index).  ``uniforms`` / ``noise``
        (K - 1, N) inject the selection uniforms / reward draws; otherwise Philox keyed by ``seed``
        (default: dpt_hip.next_seed()) and the env's global index.  Adds the step's mean loss to the
        accumulator and returns the recorded (actions (N, K-1) int32, rewards (N, K-1) float64)."""
        from . import next_seed
        dev = self.blob.device
        K = int(K)
        means_d = _dev(means, torch.float64, dev)
        if means_d.dim() != 2 or means_d.shape[1] != self.model.action_dim or means_d.shape[0] < 1:
            raise ValueError(f"means {tuple(means_d.shape)} != (N >= 1, action_dim {self.model.action_dim})")
        N = int(means_d.shape[0])
        code = {"uniform": _lib.BANDIT_GAUSSIAN, "bernoulli": _lib.BANDIT_BERNOULLI}.get(bandit_type, bandit_type)
        tg = means_d.argmax(dim=1) if targets is None else _dev(targets, torch.int64, dev).reshape(-1)
        if tg.numel() != N:
            raise ValueError(f"targets {tg.numel()} != envs {N}")
        draws = []
        for name, x in (("uniforms", uniforms), ("noise", noise)):
            x = None if x is None else _dev(x, torch.float64, dev)
            if x is not None and tuple(x.shape) != (K - 1, N):
                raise ValueError(f"{name} {tuple(x.shape)} != (K - 1 = {K - 1}, N = {N})")
            draws.append(x)
        seed = (next_seed() if seed is None else int(seed)) & (2 ** 64 - 1)
        actions = torch.empty((N, max(K - 1, 0)), dtype=torch.int32, device=dev)
        rewards = torch.empty((N, max(K - 1, 0)), dtype=torch.float64, device=dev)
        d = self._desc()
        plan = chunk_plan(N, self.chunk)
        ws = self._workspace(d, plan[0][1], K)
        base_flags = _lib.INTERACTIVE_FULL_WIDTH if self.full_width else 0
        for i, (off, n) in enumerate(plan):
            # rows off..off+n of the (N, K-1) records are one contiguous block; the draws' columns are copied
            u_c, g_c = (None if x is None else x[:, off:off + n].contiguous() for x in draws)
            args = _lib.InteractiveArgs(
                n, K, int(code), base_flags | (_lib.INTERACTIVE_ACCUMULATE if i > 0 else 0), off, float(var), 1.0 / N, seed, 0, _p(means_d[off:off + n]).value,
                _p(tg[off:off + n]).value, None if u_c is None else _p(u_c).value,
                None if g_c is None else _p(g_c).value, _p(actions[off:off + n]).value,
                _p(rewards[off:off + n]).value, _p(ws).value, _p(self.dblob).value, _p(self.loss).value)
            _lib.call("dpt_interactive_grad", ctypes.byref(d), _p(self.blob), ctypes.byref(args), _stream())
        self.steps += 1
        opt = _lib.AdamWArgs(self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.steps)
        _lib.call("dpt_adamw_step", _p(self.blob), _p(self.dblob), _p(self.m), _p(self.v), self.blob.numel(),
                  ctypes.byref(opt), _stream())
        return actions, rewards

    read_loss = Trainer.read_loss
    sync_to_model = Trainer.sync_to_model


class ExploreExploitTrainer:
    """The fused explorer/exploiter bandit step of train_explorer_exploiter.py:102-192 for two
    models.net.Transformers of one config (state_dim 1, no dropout).

    Built like ``InteractiveTrainer``, twice over: each model's fp32 master blob, AdamW ``m`` / ``v``
    and gradient blob, one step count, ONE workspace shared by the two models and two float64 loss
    accumulators live on the device.  ``step`` runs one dpt_explore_grad per chunk of envs (the
    explorer's K - 1 sampled rollout steps with the env stepped by a separate arm, the window packed
    once, the exploiter's forward / every-position cross-entropy / backward, the advantage weights
    from its row losses, the explorer's forward / weighted cross-entropy / backward), the chunks'
    gradients added in chunk order, then one dpt_adamw_step per model -- all on the current stream
    with no host synchronisation; ``read_losses`` is the only call that waits for the device.  The
    advantages use the exploiter's weights from before its update."""

    def __init__(self, explorer, exploiter, lr, weight_decay=1e-4, chunk=0, betas=(0.9, 0.999), eps=1e-8):
        if explorer is exploiter:
            raise ValueError("ExploreExploitTrainer: the explorer and the exploiter are one module")
        cfg = [(m.n_layer, m.n_embd, m.state_dim, m.action_dim, m.n_positions) for m in (explorer, exploiter)]
        if cfg[0] != cfg[1]:
            raise ValueError(f"ExploreExploitTrainer: the two models differ in shape ({cfg[0]} != {cfg[1]})")
        for m in (explorer, exploiter):
            if m.state_dim != 1:
                raise ValueError(f"ExploreExploitTrainer: state_dim={m.state_dim} (bandits have state_dim 1)")
            if m.dropout != 0:
                raise ValueError("ExploreExploitTrainer: dropout must be 0 (the cached decode has no dropout masks)")
        if int(chunk) < 0:
            raise ValueError(f"ExploreExploitTrainer: chunk={chunk}")
        self.explorer, self.exploiter, self.chunk = explorer, exploiter, int(chunk)
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), tuple(betas), float(eps)
        dev = device()
        # per model: [blob, m, v, dblob]
        self.explorer_blob, self.exploiter_blob = (pack_params(param_list(m), dev) for m in (explorer, exploiter))
        self._state = {}
        for name, blob in (("explorer", self.explorer_blob), ("exploiter", self.exploiter_blob)):
            self._state[name] = (blob, torch.zeros_like(blob), torch.zeros_like(blob), torch.empty_like(blob))
        self.explorer_dblob, self.exploiter_dblob = self._state["explorer"][3], self._state["exploiter"][3]
        self.steps = 0
        self.loss_explorer = torch.zeros(1, dtype=torch.float64, device=dev)
        self.loss_exploiter = torch.zeros(1, dtype=torch.float64, device=dev)
        self._ws = None
        self._ws_shape = (0, 0)  # (chunk envs, K) the workspace was sized for

    def _desc(self):
        m = self.explorer
        return desc(m.n_layer, m.n_embd, m.state_dim, m.action_dim, m.n_positions, 1, 1)

    def _workspace(self, d, n, K):
        if self._ws is not None and self._ws_shape == (n, K):
            return self._ws
        need = ctypes.c_int64()
        _lib.call("dpt_explore_workspace_numel", ctypes.byref(d), n, K, ctypes.byref(need))
        self._ws = None  # release the old one first
        try:
            self._ws = torch.empty(need.value, dtype=torch.float32, device=self.explorer_blob.device)
        except torch.cuda.OutOfMemoryError as e:
            raise MemoryError(f"ExploreExploitTrainer: one chunk of {n} envs at K={K} needs a workspace of "
                              f"{4 * need.value} bytes; pass a smaller `chunk` (now {self.chunk}; 0 = all envs at "
                              f"once)") from e
        self._ws_shape = (n, K)
        return self._ws

    def step(self, means, K, var, bandit_type, beta, uniforms=None, noise=None, env_actions=None, seed=None,
             targets=None):
        """One episode: ``means`` (N, A) arm means, ``K`` >= 2 the window (K - 1 rolled-out steps),
        ``bandit_type`` 'uniform' / 'bernoulli' (or a DPT_BANDIT_* code), ``beta`` the advantage
        temperature, ``targets`` (N) int64 the optimal arms (default: argmax of means).  ``uniforms`` /
        ``noise`` (K - 1, N) inject the explorer's selection uniforms / the reward draws and
        ``env_actions`` (K - 1, N) int32 the arms the env is stepped with; otherwise Philox keyed by
        ``seed`` (default: dpt_hip.next_seed()) and the env's global index.  Adds the step's two mean
        losses to the accumulators and returns the records (context actions (N, K-1) int32, env
        actions (N, K-1) int32, rewards (N, K-1) float64)."""
        from . import next_seed
        dev = self.explorer_blob.device
        K, beta = int(K), float(beta)
        A = self.explorer.action_dim
        if K < 2:
            raise ValueError(f"ExploreExploitTrainer: K={K} (the explorer's loss is a mean over K - 1 positions: "
                             f"K >= 2)")
        means_d = _dev(means, torch.float64, dev)
        if means_d.dim() != 2 or means_d.shape[1] != A or means_d.shape[0] < 1:
            raise ValueError(f"means {tuple(means_d.shape)} != (N >= 1, action_dim {A})")
        N = int(means_d.shape[0])
        code = {"uniform": _lib.BANDIT_GAUSSIAN, "bernoulli": _lib.BANDIT_BERNOULLI}.get(bandit_type, bandit_type)
        tg = means_d.argmax(dim=1) if targets is None else _dev(targets, torch.int64, dev).reshape(-1)
        if tg.numel() != N:
            raise ValueError(f"targets {tg.numel()} != envs {N}")
        draws = []
        for name, x, dt in (("uniforms", uniforms, torch.float64), ("noise", noise, torch.float64),
                            ("env_actions", env_actions, torch.int32)):
            x = None if x is None else _dev(x, dt, dev)
            if x is not None and tuple(x.shape) != (K - 1, N):
                raise ValueError(f"{name} {tuple(x.shape)} != (K - 1 = {K - 1}, N = {N})")
            draws.append(x)
        seed = (next_seed() if seed is None else int(seed)) & (2 ** 64 - 1)
        actions = torch.empty((N, K - 1), dtype=torch.int32, device=dev)
        env_acts = torch.empty((N, K - 1), dtype=torch.int32, device=dev)
        rewards = torch.empty((N, K - 1), dtype=torch.float64, device=dev)
        d = self._desc()
        plan = chunk_plan(N, self.chunk)
        ws = self._workspace(d, plan[0][1], K)
        for i, (off, n) in enumerate(plan):
            # rows off..off+n of the (N, K-1) records are one contiguous block; the draws' columns are copied
            u_c, g_c, e_c = (None if x is None else x[:, off:off + n].contiguous() for x in draws)
            args = _lib.ExploreArgs(
                n, K, int(code), _lib.EXPLORE_ACCUMULATE if i > 0 else 0, off, float(var), beta, 1.0 / (N * K),
                1.0 / (N * (K - 1)), seed, 0, _p(means_d[off:off + n]).value, _p(tg[off:off + n]).value,
                *(None if x is None else _p(x).value for x in (u_c, g_c, e_c)), _p(actions[off:off + n]).value,
                _p(env_acts[off:off + n]).value, _p(rewards[off:off + n]).value, _p(ws).value,
                _p(self.explorer_dblob).value, _p(self.exploiter_dblob).value, _p(self.loss_explorer).value,
                _p(self.loss_exploiter).value)
            _lib.call("dpt_explore_grad", ctypes.byref(d), _p(self.explorer_blob), _p(self.exploiter_blob),
                      ctypes.byref(args), _stream())
        self.steps += 1
        opt = _lib.AdamWArgs(self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.steps)
        for blob, m, v, dblob in (self._state["exploiter"], self._state["explorer"]):
            _lib.call("dpt_adamw_step", _p(blob), _p(dblob), _p(m), _p(v), blob.numel(), ctypes.byref(opt), _stream())
        return actions, env_acts, rewards

    def read_losses(self):
        """The accumulated (explorer, exploiter) loss sums (one device synchronisation), then reset."""
        both = torch.cat([self.loss_explorer, self.loss_exploiter]).cpu()
        self.loss_explorer.zero_()
        self.loss_exploiter.zero_()
        return float(both[0]), float(both[1])

    def sync_to_models(self):
        """Unpack the two master blobs into the modules' parameters (wte is untouched)."""
        with torch.no_grad():
            for model, blob in ((self.explorer, self.explorer_blob), (self.exploiter, self.exploiter_blob)):
                params = param_list(model)
                for p, w in zip(params, _unpack(blob, [p.shape for p in params], [p.dtype for p in params])):
                    p.copy_(w)
        return self.explorer, self.exploiter
