"""Float64 torch restatement of the reference ImageTransformer and train.py's loss (test helper).

models/net.py:63-132: image (3, 25, 25) -> Conv2d(3,16,k3,s2) -> ReLU -> Conv2d(16,16,k3,s1) -> ReLU ->
Dropout -> flatten (c, y, x) -> Linear(1600, 8) -> ReLU; [enc | state | action | reward] ->
embed_transition -> embed_ln (eps 1e-5) -> the GPT-2 stack of oracle/dpt_oracle_torch.py on input
embeddings -> pred_actions.  Pinned against the reference's own float64 run by
tests/golden/image_transformer.npz (tests/test_image_host.py).

``drop``: a callable site -> keep factors shaped like the site's tensor, as
oracle/dpt_oracle_torch.forward takes it; the encoder's site is SITE_IMAGE_ENC with the tensor shaped
(rows, 16, 10, 10).  ``front`` also returns the three ReLU pre-activations, whose distance from zero
the gradient tests assert first (a ReLU that flips between fp32 and float64 changes a conv gradient
by about 1 / sqrt(terms), which no tolerance absorbs).
"""
import math

import torch
import torch.nn.functional as Fn

SITE_IMAGE_ENC = 1 << 20
FRONT_KEYS = ("image_encoder.0.weight", "image_encoder.0.bias", "image_encoder.2.weight", "image_encoder.2.bias",
              "image_encoder.6.weight", "image_encoder.6.bias", "embed_transition.weight", "embed_transition.bias",
              "embed_ln.weight", "embed_ln.bias")
RELU_MARGIN = 1e-5


def params(w, dtype=torch.float64):
    """Leaf tensors (requires_grad) of a state_dict-like mapping, without wte."""
    return {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in w.items() if not k.endswith("wte.weight")}


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def front(P, images, feats, drop=None):
    """embeds (rows, E) and the ReLU pre-activations (z1 (rows,16,12,12), z2 (rows,16,10,10), z3 (rows,8))
    from images (rows, 3, 25, 25) and feats (rows, sd + A + 1)."""
    z1 = Fn.conv2d(images, P["image_encoder.0.weight"], P["image_encoder.0.bias"], stride=2)
    z2 = Fn.conv2d(torch.relu(z1), P["image_encoder.2.weight"], P["image_encoder.2.bias"])
    a2 = torch.relu(z2)
    if drop is not None:
        a2 = a2 * drop(SITE_IMAGE_ENC)
    z3 = a2.flatten(1) @ P["image_encoder.6.weight"].t() + P["image_encoder.6.bias"]
    tok = torch.cat([torch.relu(z3), feats], dim=1)
    h = tok @ P["embed_transition.weight"].t() + P["embed_transition.bias"]
    E = h.shape[1]
    return Fn.layer_norm(h, (E,), P["embed_ln.weight"], P["embed_ln.bias"], 1e-5), (z1, z2, z3)


def trunk(P, embeds, n_layer, drop=None):
    """GPT2Model(inputs_embeds=embeds (B, T, E)) -> pred_actions at every position (the layer loop of
    oracle/dpt_oracle_torch.forward, entered after the token embedding)."""
    E = P["transformer.wpe.weight"].shape[1]
    T = embeds.shape[1]
    keep = (lambda site, v: v) if drop is None else (lambda site, v: v * drop(site))  # noqa: E731
    x = keep(0, embeds + P["transformer.wpe.weight"][:T])
    mask = torch.triu(torch.ones((T, T), dtype=torch.bool), 1)
    ln = lambda v, g, b: Fn.layer_norm(v, (E,), g, b, 1e-5)  # noqa: E731
    for i in range(n_layer):
        p = f"transformer.h.{i}."
        h = ln(x, P[p + "ln_1.weight"], P[p + "ln_1.bias"])
        qkv = h @ P[p + "attn.c_attn.weight"] + P[p + "attn.c_attn.bias"]
        q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
        s = (q @ k.transpose(1, 2)) / math.sqrt(E)
        a = keep(1 + 3 * i, torch.softmax(s.masked_fill(mask, float("-inf")), dim=-1)) @ v
        x = x + keep(2 + 3 * i, a @ P[p + "attn.c_proj.weight"] + P[p + "attn.c_proj.bias"])
        h = ln(x, P[p + "ln_2.weight"], P[p + "ln_2.bias"])
        x = x + keep(3 + 3 * i, gelu_new(h @ P[p + "mlp.c_fc.weight"] + P[p + "mlp.c_fc.bias"])
                     @ P[p + "mlp.c_proj.weight"] + P[p + "mlp.c_proj.bias"])
    x = ln(x, P["transformer.ln_f.weight"], P["transformer.ln_f.bias"])
    return x @ P["pred_actions.weight"].t() + P["pred_actions.bias"]


def pack(batch, action_dim, dtype=torch.float64):
    """models/net.py:90-123: images (B, T, 3, S, S) and feats (B, T, sd + A + 1) = [state | action | reward],
    the query token first with zero action and reward; context_rewards with 2 or 3 dims."""
    t = lambda k: torch.as_tensor(batch[k], dtype=dtype)  # noqa: E731
    B = t("query_states").shape[0]
    images = torch.cat([t("query_images")[:, None], t("context_images")], dim=1)
    states = torch.cat([t("query_states")[:, None, :], t("context_states")], dim=1)
    actions = torch.cat([torch.zeros((B, 1, action_dim), dtype=dtype), t("context_actions")], dim=1)
    rewards = torch.cat([torch.zeros((B, 1, 1), dtype=dtype), t("context_rewards").reshape(B, -1, 1)], dim=1)
    return images, torch.cat([states, actions, rewards], dim=2)


def forward(P, images, feats, n_layer, drop=None):
    """(preds (B, T, A) at every position, the three ReLU pre-activations)."""
    B, T = images.shape[:2]
    embeds, pre = front(P, images.reshape(B * T, *images.shape[2:]), feats.reshape(B * T, -1), drop)
    return trunk(P, embeds.reshape(B, T, -1), n_layer, drop), pre


def train_loss(P, batch, n_layer, action_dim, drop=None):
    """train.py:293-301: CrossEntropyLoss(sum) of preds[:, 1:] against the repeated optimal action ->
    (loss, preds[:, 1:], pre-activations)."""
    dtype = P["pred_actions.bias"].dtype
    images, feats = pack(batch, action_dim, dtype)
    preds, pre = forward(P, images, feats, n_layer, drop)
    preds = preds[:, 1:, :]
    true = torch.as_tensor(batch["optimal_actions"], dtype=dtype)[:, None, :].expand_as(preds)
    loss = Fn.cross_entropy(preds.reshape(-1, action_dim), true.reshape(-1, action_dim), reduction="sum")
    return loss, preds, pre


def grads(w, batch, n_layer, action_dim, drop=None, dtype=torch.float64):
    """(loss, preds[:, 1:], {name: gradient}, pre-activations) of train.py's loss at the weights ``w``."""
    P = params(w, dtype)
    loss, preds, pre = train_loss(P, batch, n_layer, action_dim, drop)
    loss.backward()
    return loss.item(), preds.detach().numpy(), {k: v.grad.numpy() for k, v in P.items()}, \
        tuple(z.detach().numpy() for z in pre)


def relu_margin(pre):
    """the smallest |pre-activation| over the three ReLUs"""
    return min(float(abs(z).min()) for z in pre)
