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

The fused trainers keep everything on the device.  ``ModelState`` is one model's master blob with
AdamW's ``m`` / ``v`` (and a gradient blob); ``_TrainerCore`` holds the hyper-parameters, the step count
and the loss accumulator(s).  Under it, ``_DatasetTrainer`` is the one-call step on a device-resident
dataset: ``Trainer`` (train.py; dpt_train_step on a ``DeviceData``: batch packing, forward, summed
cross-entropy, backward, AdamW) and ``ImageTrainer`` (train_miniworld.py --fused; dpt_image_train_step on
a ``DeviceImageData``: the image front end and the trunk, two blobs).  ``FreshTrainer`` (train_fresh.py;
dpt_fresh_step) is ``Trainer``'s step without a dataset: each batch is generated on the device from Philox
(``dpt_hip.FreshEnv``), and ``fresh_dataset`` materialises such samples in the ``DeviceData`` layout.
``_BanditTrainer`` is the on-policy
bandit episode, a gradient call per chunk of envs and then dpt_adamw_step per model:
``InteractiveTrainer`` (train_interactive.py; dpt_interactive_grad: the y-cache rollout straight from the
master blob, the window packed from its records, forward, last-position cross-entropy, backward) and
``ExploreExploitTrainer`` (train_explorer_exploiter.py; dpt_explore_grad: the explorer's rollout with the
env stepped apart, one pack, both models' forward / every-position cross-entropy / backward with the
advantage weights in between).  ``InteractiveMDPTrainer`` is the on-policy DarkRoom episode
(train_interactive_darkroom.py; dpt_interactive_mdp_grad per chunk of envs: per step the window packed from
the records, the forward from the master blob, where the loss reads the step the cross-entropy against the
expert action and the backward, and the act step), and ``rollout_darkroom_interactive`` its loss-free rollout.

``exploit_curve`` is the evaluation of that last stage (dpt_exploit_eval): the exploiter's recommendation
after every budget of someone's recorded pulls, from one forward over the final window.
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


class ModelState:
    """One model's training state on the device: the fp32 master weights as one packed blob, AdamW's
    ``m`` and ``v`` in the same layout and, for a trainer that calls dpt_adamw_step itself, the
    gradient blob ``dblob``."""

    def __init__(self, blob, grad=False):
        self.blob, self.m, self.v = blob, torch.zeros_like(blob), torch.zeros_like(blob)
        self.dblob = torch.empty_like(blob) if grad else None

    def ptrs(self):
        """(blob, m, v) for the fused entry points that run AdamW inside the library."""
        return _p(self.blob), _p(self.m), _p(self.v)

    def adamw(self, opt):
        """One dpt_adamw_step from the gradient blob; ``opt``: the AdamWArgs (hyper-parameters, step number)."""
        _lib.call("dpt_adamw_step", _p(self.blob), _p(self.dblob), _p(self.m), _p(self.v), self.blob.numel(),
                  ctypes.byref(opt), _stream())

    def copy_to(self, params, transposed, skip=0):
        """Copy the master blob from float ``skip`` on into the module parameters ``params`` (blob order);
        ``transposed``: the indices of the nn.Linear weights, [in][out] in the blob and [out][in] in torch."""
        total = skip + sum(p.numel() for p in params)
        if total != self.blob.numel():
            raise ValueError(f"gradient blob {self.blob.numel()} != parameters {total}")
        off = skip
        with torch.no_grad():
            for i, p in enumerate(params):
                w = self.blob[off:off + p.numel()]
                p.copy_(w.view(p.shape[1], p.shape[0]).t() if i in transposed else w.view(p.shape))
                off += p.numel()


def _sync(state, model):
    """Unpack a Transformer's master blob into the module's parameters (wte, which the model never reads,
    is untouched)."""
    params = param_list(model)
    state.copy_to(params, (0, len(params) - 2))
    return model


def _of(state, field):
    """A trainer's public name for one tensor of its ModelState attribute ``state``."""
    return property(lambda self: getattr(getattr(self, state), field))


class _TrainerCore:
    """What every fused trainer keeps besides its ModelStates: AdamW's hyper-parameters, the step count,
    one float64 loss accumulator per loss (``loss``, on the device) and the workspace slot.  The trainers
    launch on the current stream with no host synchronisation; ``read_loss`` (``read_losses``) is the only
    call that waits for the device.  The modules' own parameters are not touched until ``sync_to_model``
    (``sync_to_models``)."""

    def __init__(self, lr, weight_decay, betas, eps, n_losses=1):
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), tuple(betas), float(eps)
        self.steps = 0
        self.loss = torch.zeros(n_losses, dtype=torch.float64, device=device())
        self._ws = None

    def _adamw_args(self):
        return _lib.AdamWArgs(self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.steps)

    def _read_losses(self):
        vals = self.loss.tolist()  # the one device synchronisation
        self.loss.zero_()
        return vals

    def read_loss(self):
        """The accumulated loss sum (one device synchronisation), then reset to zero."""
        return self._read_losses()[0]


class _DatasetTrainer(_TrainerCore):
    """The fused step on a device-resident dataset, one library call per batch: ``step`` packs or gathers
    the batch, runs forward, summed cross-entropy, backward and AdamW; ``eval_loss`` runs the forwards and
    the loss.  A subclass names its dataset wrapper and its three entry points and lists its ModelStates
    in ``_states``: their (blob, m, v) go between the batch and the AdamW args, their blobs between the batch
    and the workspace of ``eval_loss``."""
    _DATA = _WS_NUMEL = _STEP = _EVAL = None

    def __init__(self, model, lr, weight_decay, betas, eps):
        super().__init__(lr, weight_decay, betas, eps)
        self.model = model
        self._ws_batch = self._ws_window = 0  # the workspace grows to the largest batch seen
        self._data = {}

    def device_data(self, data, **kw):
        """``data`` as the device-resident set (a dataset / dict is converted once and kept)."""
        if isinstance(data, self._DATA):
            return data
        dd = self._data.get(id(data))
        if dd is None or dd[0] is not data:
            dd = self._data[id(data)] = (data, self._DATA(data, **kw))
        return dd[1]

    def _desc(self, data, batch, seed=None):
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
            self._ws = torch.empty(_numel(self._WS_NUMEL, d), dtype=torch.float32, device=self.loss.device)
            self._ws_batch, self._ws_window = cap, d.window
        return d

    def _run(self, train, data, index, perm, seed=None):
        data = self.device_data(data)
        idx, pm = _index_tensors(data, index, perm, self.loss.device)
        d = self._desc(data, idx.numel(), seed)
        batch = (ctypes.byref(d), ctypes.byref(data.struct), _p(idx), _p(pm), idx.numel())
        if not train:
            return _lib.call(self._EVAL, *batch, *(_p(s.blob) for s in self._states), _p(self._ws), _p(self.loss),
                             _stream())
        self.steps += 1
        try:
            _lib.call(self._STEP, *batch, *(p for s in self._states for p in s.ptrs()),
                      ctypes.byref(self._adamw_args()), _p(self._ws), _p(self.loss), _stream())
        except Exception:
            self.steps -= 1  # rejected on the host before any launch
            raise

    def step(self, data, index, perm=None):
        """One training step on the samples ``index`` (int64; ``perm`` (batch, horizon): each
        sample's context permutation, dataset.py:84-89).  Adds the batch's summed loss to the
        accumulator."""
        self._run(True, data, index, perm)

    def eval_loss(self, data, index, perm=None):
        """The test loss of train.py:265-278 on the samples ``index`` (forward only, the model's
        dropout active); adds the batch's summed loss to the accumulator."""
        self._run(False, data, index, perm)


class Trainer(_DatasetTrainer):
    """The fused device training step of train.py:286-310 for a models.net.Transformer (dpt_train_step on
    a ``DeviceData``): one ModelState in the include/dpt_hip.h blob layout."""
    _DATA, _WS_NUMEL, _STEP, _EVAL = DeviceData, "dpt_train_step_workspace_numel", "dpt_train_step", \
        "dpt_train_eval_loss"
    blob, m, v = _of("state", "blob"), _of("state", "m"), _of("state", "v")

    def __init__(self, model, lr, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(model, lr, weight_decay, betas, eps)
        self.state = ModelState(pack_params(param_list(model), self.loss.device))
        self._states = (self.state,)

    def sync_to_model(self):
        """Unpack the master blob into the module's parameters."""
        return _sync(self.state, self.model)


def fresh_dataset(first_task, n, env, seed):
    """Samples ``first_task`` .. ``first_task + n - 1`` of the fresh-task generator (``dpt_hip.fresh_batch``)
    materialised in the ``DeviceData`` / dpt_train_data layout: a dict of contiguous fp32 device tensors
    (query_states, context_states, context_actions, context_next_states, context_rewards,
    optimal_actions).  ``Trainer.step`` on it with index ``arange`` consumes what ``FreshTrainer.step``
    generates in place; ``{k: v.cpu() ...}`` dumps a dataset."""
    from . import fresh_batch
    o = fresh_batch(env, seed, first_task, n, outputs=False)
    tok, sd, A = o["tokens"], env.state_dim, env.action_dim
    ctx = tok[:, 1:]
    return {"query_states": tok[:, 0, :sd].contiguous(), "context_states": ctx[:, :, :sd].contiguous(),
            "context_actions": ctx[:, :, sd:sd + A].contiguous(),
            "context_next_states": ctx[:, :, sd + A:2 * sd + A].contiguous(),
            "context_rewards": ctx[:, :, 2 * sd + A].contiguous(), "optimal_actions": o["targets"]}


class FreshTrainer(_TrainerCore):
    """The pretraining step on fresh tasks (train_fresh.py; dpt_fresh_step, or dpt_fresh_linear_step for
    ``FreshEnv.linear_bandit``: the env names its entry points): no dataset -- each step
    generates its batch on the device (``dpt_hip.FreshEnv``: the task, the behaviour policy, the rollin,
    the query and the label, all from Philox(``seed``) and the sample's global index), then forward, summed
    cross-entropy, backward and AdamW, the launches of ``Trainer.step`` after its pack.  ``step`` takes the
    next ``batch`` samples from ``first_task`` on, so a run sees every task once whatever its batch sizes."""
    blob, m, v = _of("state", "blob"), _of("state", "m"), _of("state", "v")

    def __init__(self, model, env, lr, weight_decay=1e-4, seed=0, first_task=0, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(lr, weight_decay, betas, eps)
        if (env.state_dim, env.action_dim, env.H) != (model.state_dim, model.action_dim, model.horizon):
            raise ValueError(f"env (sd {env.state_dim}, A {env.action_dim}, H {env.H}) does not match the model "
                             f"(sd {model.state_dim}, A {model.action_dim}, H {model.horizon})")
        self.model, self.env, self.seed, self.first_task = model, env, int(seed), int(first_task)
        self.state = ModelState(pack_params(param_list(model), self.loss.device))
        self._ws_batch = 0  # the workspace grows to the largest batch seen

    def _desc(self, batch, dropout_seed):
        m = self.model
        p = float(m.dropout) if m.dropout > 0 else 0.0
        if p > 0 and dropout_seed is None:  # fresh masks per call; the test loss runs in training mode too
            from models.net import _dropout_seed
            dropout_seed = _dropout_seed()
        cap = max(batch, self._ws_batch)
        d = desc(m.n_layer, m.n_embd, m.state_dim, m.action_dim, m.n_positions, cap, 1 + self.env.H, dropout=p,
                 seed=(int(dropout_seed) & (2 ** 64 - 1)) if p > 0 else 0)
        if self._ws is None or cap > self._ws_batch:
            self._ws = torch.empty(_numel("dpt_train_step_workspace_numel", d), dtype=torch.float32,
                                   device=self.loss.device)
            self._ws_batch = cap
        return d

    def step(self, batch=64, dropout_seed=None):
        """One training step on the next ``batch`` fresh samples; adds their summed loss to the accumulator."""
        batch = int(batch)
        if batch < 1:
            raise ValueError("empty batch")
        d = self._desc(batch, dropout_seed)
        args = self.env.args(self.seed, self.first_task)
        self.steps += 1
        try:
            _lib.call(self.env.calls["step"], ctypes.byref(d), ctypes.byref(args), batch, *self.state.ptrs(),
                      ctypes.byref(self._adamw_args()), _p(self._ws), _p(self.loss), _stream())
        except Exception:
            self.steps -= 1  # rejected on the host before any launch
            raise
        self.first_task += batch

    def eval_loss(self, first_task, n, seed=None, env=None, batch=64, dropout_seed=None):
        """The test loss on samples ``first_task`` .. ``first_task + n - 1`` of ``env`` (default: the training
        env) under the key ``seed`` (default: the training key), ``batch`` at a time: forward only, the model's
        dropout active; adds the summed loss to the accumulator.  Nothing is stored: the same arguments
        regenerate the same samples."""
        env = env or self.env
        if (env.state_dim, env.action_dim, env.H) != (self.env.state_dim, self.env.action_dim, self.env.H):
            raise ValueError("eval_loss: the env's shapes differ from the training env's")
        seed = self.seed if seed is None else int(seed)
        for lo in range(0, int(n), int(batch)):
            b = min(int(batch), int(n) - lo)
            d = self._desc(b, dropout_seed)
            args = env.args(seed, int(first_task) + lo)
            _lib.call(env.calls["eval_loss"], ctypes.byref(d), ctypes.byref(args), b, _p(self.state.blob),
                      _p(self._ws), _p(self.loss), _stream())

    def sync_to_model(self):
        """Unpack the master blob into the module's parameters."""
        return _sync(self.state, self.model)


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


class ImageTrainer(_DatasetTrainer):
    """The fused device training step of train_miniworld.py for a models.net.ImageTransformer
    (dpt_image_train_step on a ``DeviceImageData``: the image front end, the trunk, the summed
    cross-entropy, both backwards and the two AdamW updates).  Two ModelStates: the trunk in the
    dpt_train_desc layout with a zero emb_w / emb_b region of ``emb_numel`` floats, the front end in the
    front-blob layout."""
    _DATA, _WS_NUMEL, _STEP, _EVAL = DeviceImageData, "dpt_image_train_step_workspace_numel", \
        "dpt_image_train_step", "dpt_image_train_eval_loss"
    blob, m, v = _of("trunk", "blob"), _of("trunk", "m"), _of("trunk", "v")
    front_blob, front_m, front_v = _of("front", "blob"), _of("front", "m"), _of("front", "v")

    def __init__(self, model, lr, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8):
        super().__init__(model, lr, weight_decay, betas, eps)
        self.emb_numel = (2 * model.state_dim + model.action_dim + 1) * model.n_embd + model.n_embd
        front, trunk = pack_image_params(image_param_list(model), self.emb_numel, self.loss.device)
        self._states = self.trunk, self.front = ModelState(trunk), ModelState(front)

    def step(self, data, index, perm=None, seed=None):
        """``_DatasetTrainer.step``; ``seed``: the Philox seed of this step's dropout masks (default: a
        fresh one from the CUDA generator)."""
        self._run(True, data, index, perm, seed)

    def eval_loss(self, data, index, perm=None, seed=None):
        """The test loss on the samples ``index`` (both forwards only, the model's dropout active); adds
        the batch's summed loss to the accumulator."""
        self._run(False, data, index, perm, seed)

    def sync_to_model(self):
        """Unpack both master blobs into the module's parameters (wte, which the model never reads, is
        untouched)."""
        params = image_param_list(self.model)
        self.front.copy_to(params[:N_FRONT], (4, 6))  # fc / embed_transition weights
        self.trunk.copy_to(params[N_FRONT:], (len(params) - N_FRONT - 2,), skip=self.emb_numel)
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


def exploit_curve(model, actions, rewards, means, targets=None, chunk=0, blob=None, want_logits=False):
    """The explore-then-exploit curve of ``model`` (the exploiter) on someone's records: what it
    recommends after every budget t = 0 .. H of the pulls actions (N, H) int32 / rewards (N, H), for the
    bandits means (N, A) with optimal arms ``targets`` (default: ``means.argmax(1)``).  One
    dpt_exploit_eval per chunk of tasks (``chunk_plan(N, chunk)``: the pack, ONE forward-only forward at
    every position of the (1 + H)-token window -- row t is the model after t transitions -- and
    dpt_recommend_curve), on one workspace sized for the first chunk, with no host synchronisation.
    ``blob``: run on this packed blob (a trainer's master weights) instead of the module's parameters.
    Returns a dict of device tensors: greedy_arm (N, H + 1) int32, greedy_value / expected_value / p_opt
    (N, H + 1) float64 and, with ``want_logits``, logits (N, H + 1, A) float32."""
    if model.state_dim != 1:
        raise ValueError(f"exploit_curve: state_dim={model.state_dim} (bandits have state_dim 1)")
    if model.dropout > 0 and model.training:
        raise ValueError("exploit_curve: the model is in training mode with dropout > 0 (call model.eval(): the "
                         "evaluation forward has no dropout masks)")
    if int(chunk) < 0:
        raise ValueError(f"exploit_curve: chunk={chunk}")
    dev, A = device(), model.action_dim
    means_d = _dev(means, torch.float64, dev)
    if means_d.dim() != 2 or means_d.shape[1] != A or means_d.shape[0] < 1:
        raise ValueError(f"means {tuple(means_d.shape)} != (N >= 1, action_dim {A})")
    N = int(means_d.shape[0])
    acts, rews = _dev(actions, torch.int32, dev), _dev(rewards, torch.float64, dev)
    if acts.dim() != 2 or acts.shape[0] != N or acts.shape != rews.shape:
        raise ValueError(f"actions {tuple(acts.shape)} / rewards {tuple(rews.shape)} != (N = {N}, H) each")
    H = int(acts.shape[1])
    tg = means_d.argmax(dim=1) if targets is None else _dev(targets, torch.int64, dev).reshape(-1)
    if tg.numel() != N:
        raise ValueError(f"targets {tg.numel()} != tasks {N}")
    if blob is None:
        blob = pack_params(param_list(model), dev)
    _on_device(blob)
    d = desc(model.n_layer, model.n_embd, model.state_dim, A, model.n_positions, 1, 1)
    plan = chunk_plan(N, chunk)
    need = ctypes.c_int64()
    _lib.call("dpt_exploit_eval_workspace_numel", ctypes.byref(d), plan[0][1], H, ctypes.byref(need))
    try:
        ws = torch.empty(need.value, dtype=torch.float32, device=dev)
    except torch.cuda.OutOfMemoryError as e:
        raise MemoryError(f"exploit_curve: one chunk of {plan[0][1]} envs at K={H + 1} needs a workspace of "
                          f"{4 * need.value} bytes; pass a smaller `chunk` (now {int(chunk)}; 0 = all envs at "
                          f"once)") from e
    out = dict(greedy_arm=torch.empty((N, H + 1), dtype=torch.int32, device=dev),
               **{k: torch.empty((N, H + 1), dtype=torch.float64, device=dev)
                  for k in ("greedy_value", "expected_value", "p_opt")})
    out["logits"] = torch.empty((N, H + 1, A), dtype=torch.float32, device=dev) if want_logits else None
    for off, n in plan:
        rows = slice(off, off + n)  # rows of every (N, ...) array: one contiguous block
        args = _lib.ExploitEvalArgs(
            n, H, 0, 0, _ptr(acts[rows]) if H else None, _ptr(rews[rows]) if H else None, _ptr(means_d[rows]),
            _ptr(tg[rows]), _ptr(ws), None if out["logits"] is None else _ptr(out["logits"][rows]),
            _ptr(out["greedy_arm"][rows]), _ptr(out["greedy_value"][rows]), _ptr(out["expected_value"][rows]),
            _ptr(out["p_opt"][rows]))
        _lib.call("dpt_exploit_eval", ctypes.byref(d), _p(blob), ctypes.byref(args), _stream())
    out["_keep"] = (ws, blob, means_d, acts, rews, tg)
    return out


class _BanditTrainer(_TrainerCore):
    """The fused on-policy bandit episode for models.net.Transformers with state_dim 1 and no dropout: one
    ModelState with a gradient blob per model (``_states``, in the order AdamW updates them).  ``step``
    validates the episode (``_episode``), then ``_train`` runs the subclass's gradient entry point once per
    chunk of envs -- the K - 1 sampled rollout steps from the master blob, the window packed from the
    records, forward, cross-entropy, backward; chunk 0 writes the gradient blobs, later chunks add to them
    in chunk order -- and one dpt_adamw_step per model."""
    _WS_NUMEL = None

    def __init__(self, models, lr, weight_decay, chunk, betas, eps, n_losses=1):
        name = type(self).__name__
        for m in models:
            if m.state_dim != 1:
                raise ValueError(f"{name}: state_dim={m.state_dim} (bandits have state_dim 1)")
            if m.dropout != 0:
                raise ValueError(f"{name}: dropout must be 0 (the cached decode has no dropout masks)")
        if int(chunk) < 0:
            raise ValueError(f"{name}: chunk={chunk}")
        super().__init__(lr, weight_decay, betas, eps, n_losses)
        self.chunk = int(chunk)
        self._states = tuple(ModelState(pack_params(param_list(m), self.loss.device), grad=True) for m in models)
        m = models[0]
        self._d = desc(m.n_layer, m.n_embd, m.state_dim, m.action_dim, m.n_positions, 1, 1)
        self._ws_shape = (0, 0)  # (chunk envs, K) the workspace was sized for

    def _workspace(self, n, K):
        if self._ws is not None and self._ws_shape == (n, K):
            return self._ws
        need = ctypes.c_int64()
        _lib.call(self._WS_NUMEL, ctypes.byref(self._d), n, K, ctypes.byref(need))
        self._ws = None  # release the old one first
        try:
            self._ws = torch.empty(need.value, dtype=torch.float32, device=self.loss.device)
        except torch.cuda.OutOfMemoryError as e:
            raise MemoryError(f"{type(self).__name__}: one chunk of {n} envs at K={K} needs a workspace of "
                              f"{4 * need.value} bytes; pass a smaller `chunk` (now {self.chunk}; 0 = all envs at "
                              f"once)") from e
        self._ws_shape = (n, K)
        return self._ws

    def _episode(self, means, K, bandit_type, targets, seed, **draws):
        """The episode's inputs on the device, validated: (means (N, A) float64, the DPT_BANDIT_* code,
        targets (N) int64, the 64-bit seed, the injected ``draws`` in the order given -- each None or a
        (K - 1, N) tensor, int32 for ``env_actions`` and float64 otherwise)."""
        from . import next_seed
        dev, A = self.loss.device, self._d.action_dim
        means_d = _dev(means, torch.float64, dev)
        if means_d.dim() != 2 or means_d.shape[1] != A or means_d.shape[0] < 1:
            raise ValueError(f"means {tuple(means_d.shape)} != (N >= 1, action_dim {A})")
        N = int(means_d.shape[0])
        code = {"uniform": _lib.BANDIT_GAUSSIAN, "bernoulli": _lib.BANDIT_BERNOULLI}.get(bandit_type, bandit_type)
        tg = means_d.argmax(dim=1) if targets is None else _dev(targets, torch.int64, dev).reshape(-1)
        if tg.numel() != N:
            raise ValueError(f"targets {tg.numel()} != envs {N}")
        out = []
        for name, x in draws.items():
            x = None if x is None else _dev(x, torch.int32 if name == "env_actions" else torch.float64, dev)
            if x is not None and tuple(x.shape) != (K - 1, N):
                raise ValueError(f"{name} {tuple(x.shape)} != (K - 1 = {K - 1}, N = {N})")
            out.append(x)
        return means_d, int(code), tg, (next_seed() if seed is None else int(seed)) & (2 ** 64 - 1), out

    def _train(self, N, K, draws, grad):
        """``grad(ws, i, off, n, *chunk draws)`` for chunk ``i`` = envs off..off+n, then the AdamW updates."""
        plan = chunk_plan(N, self.chunk)
        ws = self._workspace(plan[0][1], K)
        for i, (off, n) in enumerate(plan):
            # rows off..off+n of the (N, K-1) records are one contiguous block; the draws' columns are copied
            grad(ws, i, off, n, *(None if x is None else x[:, off:off + n].contiguous() for x in draws))
        self.steps += 1
        opt = self._adamw_args()
        for s in self._states:
            s.adamw(opt)


def _ptr(t):
    return None if t is None else t.data_ptr()  # a c_void_p field of an args struct


class InteractiveTrainer(_BanditTrainer):
    """The fused interactive (on-policy) bandit step of train_interactive.py:92-143: one
    dpt_interactive_grad per chunk of envs with the last-position cross-entropy scaled by 1 / N, then one
    dpt_adamw_step."""
    _WS_NUMEL = "dpt_interactive_workspace_numel"
    blob, m, v, dblob = _of("state", "blob"), _of("state", "m"), _of("state", "v"), _of("state", "dblob")

    def __init__(self, model, lr, weight_decay=1e-4, chunk=0, betas=(0.9, 0.999), eps=1e-8, full_width=False):
        # full_width: the last block for every row instead of the last one (DPT_INTERACTIVE_FULL_WIDTH; A/B runs)
        self.full_width = bool(full_width)
        super().__init__((model,), lr, weight_decay, chunk, betas, eps)
        self.model, (self.state,) = model, self._states

    def step(self, means, K, var, bandit_type, uniforms=None, noise=None, seed=None, targets=None):
        """One episode: ``means`` (N, A) arm means, ``K`` the window (K - 1 rolled-out steps),
        ``bandit_type`` 'uniform' / 'bernoulli' (or a DPT_BANDIT_* code), ``targets`` (N) int64 the
        optimal arms (default: argmax of means, GPUBanditEnv.opt_a_index).  ``uniforms`` / ``noise``
        (K - 1, N) inject the selection uniforms / reward draws; otherwise Philox keyed by ``seed``
        (default: dpt_hip.next_seed()) and the env's global index.  Adds the step's mean loss to the
        accumulator and returns the recorded (actions (N, K-1) int32, rewards (N, K-1) float64)."""
        K = int(K)
        means_d, code, tg, seed, draws = self._episode(means, K, bandit_type, targets, seed, uniforms=uniforms,
                                                       noise=noise)
        N, s = int(means_d.shape[0]), self.state
        actions = torch.empty((N, max(K - 1, 0)), dtype=torch.int32, device=means_d.device)
        rewards = torch.empty((N, max(K - 1, 0)), dtype=torch.float64, device=means_d.device)
        base_flags = _lib.INTERACTIVE_FULL_WIDTH if self.full_width else 0

        def grad(ws, i, off, n, u_c, g_c):
            args = _lib.InteractiveArgs(
                n, K, code, base_flags | (_lib.INTERACTIVE_ACCUMULATE if i > 0 else 0), off, float(var), 1.0 / N,
                seed, 0, _ptr(means_d[off:off + n]), _ptr(tg[off:off + n]), _ptr(u_c), _ptr(g_c),
                _ptr(actions[off:off + n]), _ptr(rewards[off:off + n]), _ptr(ws), _ptr(s.dblob), _ptr(self.loss))
            _lib.call("dpt_interactive_grad", ctypes.byref(self._d), _p(s.blob), ctypes.byref(args), _stream())
        self._train(N, K, draws, grad)
        return actions, rewards

    def sync_to_model(self):
        """Unpack the master blob into the module's parameters."""
        return _sync(self.state, self.model)


MDP_LOSS = {"none": _lib.MDP_LOSS_NONE, "last": _lib.MDP_LOSS_LAST, "every": _lib.MDP_LOSS_EVERY}


def _mdp_check_model(model, who):
    if (model.state_dim, model.action_dim) != (2, 5):
        raise ValueError(f"{who}: state_dim={model.state_dim} action_dim={model.action_dim} (DarkRoom has state_dim 2, "
                         f"action_dim 5)")
    return desc(model.n_layer, model.n_embd, model.state_dim, model.action_dim, model.n_positions, 1, 1)


def _mdp_workspace(d, n, K, mode, dev, who, chunk):
    """The workspace of one chunk of ``n`` envs over ``K`` steps (dpt_interactive_mdp_workspace_numel floats)."""
    need = ctypes.c_int64()
    _lib.call("dpt_interactive_mdp_workspace_numel", ctypes.byref(d), n, K, mode, ctypes.byref(need))
    try:
        return torch.empty(need.value, dtype=torch.float32, device=dev)
    except torch.cuda.OutOfMemoryError as e:
        raise MemoryError(f"{who}: one chunk of {n} envs at K={K} needs a workspace of {4 * need.value} bytes; pass "
                          f"a smaller `chunk` (now {chunk}; 0 = all envs at once)") from e


def _mdp_episode(goals, K, perm, uniforms, seed, dev):
    """The episode's inputs on the device, validated: (goals (N, 2) int32, perm (N, 5) int32 or None,
    uniforms (K - 1, N) float64 or None, the 64-bit seed)."""
    from . import next_seed
    if K < 1:
        raise ValueError(f"K={K} (at least 1)")
    g = _dev(goals, torch.int32, dev)
    if g.dim() != 2 or g.shape[1] != 2 or g.shape[0] < 1:
        raise ValueError(f"goals {tuple(g.shape)} != (N >= 1, 2)")
    N = int(g.shape[0])
    pm = None if perm is None else _dev(perm, torch.int32, dev)
    if pm is not None and tuple(pm.shape) != (N, 5):
        raise ValueError(f"perm {tuple(pm.shape)} != (N = {N}, 5)")
    u = None if uniforms is None else _dev(uniforms, torch.float64, dev)
    if u is not None and tuple(u.shape) != (K - 1, N):
        raise ValueError(f"uniforms {tuple(u.shape)} != (K - 1 = {K - 1}, N = {N})")
    return g, pm, u, (next_seed() if seed is None else int(seed)) & (2 ** 64 - 1)


def _mdp_run(d, blob, ws_for, chunk, mode, goals, K, dim, sample, perm, uniforms, seed, dblob=None, loss=None):
    """dpt_interactive_mdp_grad once per chunk of envs (``chunk_plan``; first_task = the chunk's offset, so
    the Philox records do not depend on the chunking; chunk 0 writes ``dblob``, later chunks add to it) on the
    workspace ``ws_for(chunk 0's envs)``.  Returns the records: states (N, K, 2), actions (N, K - 1), rewards
    (N, K - 1), targets (N, K), int32 device tensors."""
    N, dev = int(goals.shape[0]), goals.device
    rec = dict(states=torch.empty((N, K, 2), dtype=torch.int32, device=dev),
               actions=torch.empty((N, K - 1), dtype=torch.int32, device=dev),
               rewards=torch.empty((N, K - 1), dtype=torch.int32, device=dev),
               targets=torch.empty((N, K), dtype=torch.int32, device=dev))
    plan = chunk_plan(N, chunk)
    ws = ws_for(plan[0][1])
    scale = 1.0 / (N * K) if mode == _lib.MDP_LOSS_EVERY else 1.0 / N
    for i, (off, n) in enumerate(plan):
        rows = slice(off, off + n)  # rows of every (N, ...) array: one contiguous block; the uniforms' columns are copied
        u_c = None if uniforms is None else uniforms[:, rows].contiguous()
        args = _lib.InteractiveMDPArgs(
            n, K, int(dim), mode, _lib.INTERACTIVE_ACCUMULATE if i > 0 else 0, int(bool(sample)), off, scale, seed, 0,
            _ptr(goals[rows]), None if perm is None else _ptr(perm[rows]), _ptr(u_c), _ptr(rec["states"][rows]),
            _ptr(rec["actions"][rows]) if K > 1 else None, _ptr(rec["rewards"][rows]) if K > 1 else None,
            _ptr(rec["targets"][rows]), _ptr(ws), _ptr(dblob), _ptr(loss))
        _lib.call("dpt_interactive_mdp_grad", ctypes.byref(d), _p(blob), ctypes.byref(args), _stream())
    return rec


class InteractiveMDPTrainer(_TrainerCore):
    """The fused interactive (on-policy) DarkRoom step for a models.net.Transformer with state_dim 2,
    action_dim 5 and no dropout: one dpt_interactive_mdp_grad per chunk of envs -- for each of the K steps
    the window packed from the records so far, the forward from the master blob, on a loss-bearing step the
    cross-entropy against the expert action at the visited state and the backward, and the act step -- then
    one dpt_adamw_step.  ``loss``: 'every' (the mean over all N K visited states) or 'last' (the mean over
    the N last states: train_interactive.py:134-135 transliterated)."""
    blob, m, v, dblob = _of("state", "blob"), _of("state", "m"), _of("state", "v"), _of("state", "dblob")

    def __init__(self, model, lr, weight_decay=1e-4, chunk=0, loss="every", betas=(0.9, 0.999), eps=1e-8):
        name = type(self).__name__
        d = _mdp_check_model(model, name)
        if model.dropout != 0:
            raise ValueError(f"{name}: dropout must be 0 (the fused path draws no dropout masks)")
        if int(chunk) < 0:
            raise ValueError(f"{name}: chunk={chunk}")
        if loss not in ("every", "last"):
            raise ValueError(f"{name}: loss={loss!r} ('every' or 'last')")
        super().__init__(lr, weight_decay, betas, eps)
        self.model, self.chunk, self.loss_mode, self._d = model, int(chunk), MDP_LOSS[loss], d
        self.state = ModelState(pack_params(param_list(model), self.loss.device), grad=True)
        self._ws_shape = (0, 0)  # (chunk envs, K) the workspace was sized for

    def _workspace(self, n, K):
        if self._ws is None or self._ws_shape != (n, K):
            self._ws = None  # release the old one first
            self._ws = _mdp_workspace(self._d, n, K, self.loss_mode, self.loss.device, type(self).__name__, self.chunk)
            self._ws_shape = (n, K)
        return self._ws

    def step(self, goals, K, dim, sample=True, perm=None, uniforms=None, seed=None):
        """One episode of K steps from s_0 = (0, 0): ``goals`` (N, 2) int32 in [0, dim), ``perm`` (N, 5) the
        action permutations dpt_darkroom_step takes, ``sample`` False for greedy actions.  ``uniforms``
        (K - 1, N) inject the selection uniforms; otherwise Philox keyed by ``seed`` (default:
        dpt_hip.next_seed()) and the env's global index.  Adds the step's mean loss to the accumulator and
        returns the records: a dict of int32 device tensors states (N, K, 2), actions (N, K - 1), rewards
        (N, K - 1) and targets (N, K)."""
        K = int(K)
        g, pm, u, seed = _mdp_episode(goals, K, perm, uniforms, seed, self.loss.device)
        rec = _mdp_run(self._d, self.state.blob, lambda n: self._workspace(n, K), self.chunk, self.loss_mode, g, K, dim,
                       sample, pm, u, seed, self.state.dblob, self.loss)
        self.steps += 1
        self.state.adamw(self._adamw_args())
        return rec

    def rollout(self, goals, K, dim, sample=False, perm=None, uniforms=None, seed=None):
        """``rollout_darkroom_interactive`` of the master blob as it stands (no ``sync_to_model`` needed)."""
        return rollout_darkroom_interactive(self.model, goals, K, dim, sample, perm=perm, uniforms=uniforms, seed=seed,
                                            chunk=self.chunk, blob=self.state.blob)

    def sync_to_model(self):
        """Unpack the master blob into the module's parameters."""
        return _sync(self.state, self.model)


def rollout_darkroom_interactive(model, goals, K, dim, sample=True, perm=None, uniforms=None, seed=None, chunk=0,
                                 blob=None):
    """The in-episode DarkRoom rollout of ``InteractiveMDPTrainer.step`` without a loss
    (dpt_interactive_mdp_grad, DPT_MDP_LOSS_NONE: K forward-only forwards and K - 1 act steps per chunk of
    envs, no host synchronisation).  ``blob``: run on this packed blob (a trainer's master weights) instead
    of the module's parameters.  Returns (the records dict of ``step``, the per-env return (N) int64 = the
    sum of the K - 1 rewards)."""
    who = "rollout_darkroom_interactive"
    d = _mdp_check_model(model, who)
    if model.dropout > 0 and model.training:
        raise ValueError(f"{who}: the model is in training mode with dropout > 0 (call model.eval(): the rollout's "
                         f"forwards have no dropout masks)")
    if int(chunk) < 0:
        raise ValueError(f"{who}: chunk={chunk}")
    dev, K = device(), int(K)
    g, pm, u, seed = _mdp_episode(goals, K, perm, uniforms, seed, dev)
    if blob is None:
        blob = pack_params(param_list(model), dev)
    _on_device(blob)
    rec = _mdp_run(d, blob, lambda n: _mdp_workspace(d, n, K, _lib.MDP_LOSS_NONE, dev, who, int(chunk)), int(chunk),
                   _lib.MDP_LOSS_NONE, g, K, dim, sample, pm, u, seed)
    return rec, rec["rewards"].sum(dim=1)


class ExploreExploitTrainer(_BanditTrainer):
    """The fused explorer/exploiter bandit step of train_explorer_exploiter.py:102-192 for two
    models.net.Transformers of one config: ONE workspace shared by the two models, two loss accumulators.
    One dpt_explore_grad per chunk of envs (the explorer's K - 1 sampled rollout steps with the env stepped
    by a separate arm, the window packed once, the exploiter's forward / every-position cross-entropy /
    backward, the advantage weights from its row losses, the explorer's forward / weighted cross-entropy /
    backward), then one dpt_adamw_step per model, the exploiter's first.  The advantages use the
    exploiter's weights from before its update."""
    _WS_NUMEL = "dpt_explore_workspace_numel"
    explorer_blob, explorer_dblob = _of("explorer_state", "blob"), _of("explorer_state", "dblob")
    exploiter_blob, exploiter_dblob = _of("exploiter_state", "blob"), _of("exploiter_state", "dblob")

    def __init__(self, explorer, exploiter, lr, weight_decay=1e-4, chunk=0, betas=(0.9, 0.999), eps=1e-8):
        if explorer is exploiter:
            raise ValueError("ExploreExploitTrainer: the explorer and the exploiter are one module")
        cfg = [(m.n_layer, m.n_embd, m.state_dim, m.action_dim, m.n_positions) for m in (explorer, exploiter)]
        if cfg[0] != cfg[1]:
            raise ValueError(f"ExploreExploitTrainer: the two models differ in shape ({cfg[0]} != {cfg[1]})")
        super().__init__((exploiter, explorer), lr, weight_decay, chunk, betas, eps, n_losses=2)
        self.explorer, self.exploiter = explorer, exploiter
        self.exploiter_state, self.explorer_state = self._states
        self.loss_explorer, self.loss_exploiter = self.loss[:1], self.loss[1:]

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
        K, beta = int(K), float(beta)
        if K < 2:
            raise ValueError(f"ExploreExploitTrainer: K={K} (the explorer's loss is a mean over K - 1 positions: "
                             f"K >= 2)")
        means_d, code, tg, seed, draws = self._episode(means, K, bandit_type, targets, seed, uniforms=uniforms,
                                                       noise=noise, env_actions=env_actions)
        N, ex, xp = int(means_d.shape[0]), self.explorer_state, self.exploiter_state
        actions = torch.empty((N, K - 1), dtype=torch.int32, device=means_d.device)
        env_acts = torch.empty((N, K - 1), dtype=torch.int32, device=means_d.device)
        rewards = torch.empty((N, K - 1), dtype=torch.float64, device=means_d.device)

        def grad(ws, i, off, n, u_c, g_c, e_c):
            args = _lib.ExploreArgs(
                n, K, code, _lib.EXPLORE_ACCUMULATE if i > 0 else 0, off, float(var), beta, 1.0 / (N * K),
                1.0 / (N * (K - 1)), seed, 0, _ptr(means_d[off:off + n]), _ptr(tg[off:off + n]), _ptr(u_c),
                _ptr(g_c), _ptr(e_c), _ptr(actions[off:off + n]), _ptr(env_acts[off:off + n]),
                _ptr(rewards[off:off + n]), _ptr(ws), _ptr(ex.dblob), _ptr(xp.dblob), _ptr(self.loss_explorer),
                _ptr(self.loss_exploiter))
            _lib.call("dpt_explore_grad", ctypes.byref(self._d), _p(ex.blob), _p(xp.blob), ctypes.byref(args),
                      _stream())
        self._train(N, K, draws, grad)
        return actions, env_acts, rewards

    def read_losses(self):
        """The accumulated (explorer, exploiter) loss sums (one device synchronisation), then reset."""
        return tuple(self._read_losses())

    def exploit_curve(self, actions, rewards, means, targets=None, chunk=None, want_logits=False):
        """``exploit_curve`` of the exploiter's master blob as it stands (no ``sync_to_models`` needed) on the
        records actions / rewards (N, H) of the bandits ``means``; ``chunk`` defaults to the trainer's."""
        return exploit_curve(self.exploiter, actions, rewards, means, targets=targets,
                             chunk=self.chunk if chunk is None else chunk, blob=self.exploiter_blob,
                             want_logits=want_logits)

    def sync_to_models(self):
        """Unpack the two master blobs into the modules' parameters (wte is untouched)."""
        return _sync(self.explorer_state, self.explorer), _sync(self.exploiter_state, self.exploiter)
