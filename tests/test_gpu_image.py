"""The image-conditioned DPT on the GPU (csrc/dpt_image.hip, dpt_train_*_embeds, models.net.ImageTransformer,
train_miniworld.py) against the float64 oracle of tests/image_oracle.py and the reference-recorded
fixture tests/golden/image_transformer.npz.

Bars: forward values within 1e-5 max(1, |x|); every gradient within 5 GRAD_TOL of the largest entry of
its float64 gradient (GRAD_TOL = 2e-5, the project's fp32 bar).  Every gradient test first asserts ON THE
ORACLE that each pre-activation of the three ReLUs lies RELU_MARGIN = 1e-5 from zero: a ReLU that flips
between fp32 and float64 changes a conv gradient by about 1 / sqrt(terms), which no tolerance absorbs
(fp32 conv2 pre-activations differ from float64 by about 4e-7).  The seeds below were chosen on the CPU
so that the assertion holds.  Each case prints its worst errors next to the fp32 errors of the same
oracle on the same inputs (profiles/image_front/errors.txt is the record of one run)."""
import os

import numpy as np
import pytest
import torch

import image_oracle as IO
from conftest import golden
from test_gpu_train import GRAD_TOL

pytestmark = pytest.mark.gpu

BAR = 5 * GRAD_TOL
SD, A = 2, 4
G = SD + A + 1
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
# (rows, E) -> seed of the front-end case: the first whose oracle margin is at least 2e-5
FRONT_SEEDS = {(1, 32): 0, (5, 32): 2, (21, 32): 2, (1, 18): 0, (5, 18): 2, (21, 18): 2}


def front_weights(E, seed):
    """float64 front weights: torch's default initialisation for the encoder, embed_transition and
    embed_ln moved off their initial values (every value fp32-representable)"""
    torch.manual_seed(seed)
    enc = [torch.nn.Conv2d(3, 16, 3, stride=2), torch.nn.Conv2d(16, 16, 3), torch.nn.Linear(1600, 8)]
    w = {}
    for idx, mod in zip((0, 2, 6), enc):
        w[f"image_encoder.{idx}.weight"], w[f"image_encoder.{idx}.bias"] = mod.weight, mod.bias
    w["embed_transition.weight"] = 0.3 * torch.randn(E, 8 + G)
    w["embed_transition.bias"] = 0.1 * torch.randn(E)
    w["embed_ln.weight"] = 1 + 0.1 * torch.randn(E)
    w["embed_ln.bias"] = 0.1 * torch.randn(E)
    return {k: v.detach().numpy().astype(np.float64) for k, v in w.items()}


def front_inputs(rows, E, seed):
    """(images (rows, 3, 25, 25) uniform-random then normalised, feats, dembeds), fp32-representable float64"""
    rs = np.random.RandomState(seed)
    raw = rs.uniform(0, 1, (rows, 25, 25, 3))
    images = ((raw - MEAN) / STD).transpose(0, 3, 1, 2)
    feats, dembeds = rs.normal(size=(rows, G)), rs.normal(size=(rows, E))
    return tuple(np.ascontiguousarray(x, np.float32).astype(np.float64) for x in (images, feats, dembeds))


def front_oracle(w, images, feats, dembeds, dtype=torch.float64, drop=None):
    """(embeds, {name: gradient of sum(embeds * dembeds)}, pre-activations) in ``dtype``"""
    P = IO.params(w, dtype)
    embeds, pre = IO.front(P, torch.tensor(images, dtype=dtype), torch.tensor(feats, dtype=dtype), drop)
    (embeds * torch.tensor(dembeds, dtype=dtype)).sum().backward()
    return embeds.detach().numpy(), {k: P[k].grad.numpy() for k in IO.FRONT_KEYS}, \
        tuple(z.detach().numpy() for z in pre)


def violations(got, ref, bar=BAR):
    """[(name, max|got - ref| / max|ref|)] of the entries past the bar; the worst ratio"""
    bad, worst = [], 0.0
    for k, r in ref.items():
        r = np.asarray(r, np.float64)
        scale = np.abs(r).max()
        assert scale > 0, k
        e = float(np.abs(np.asarray(got[k], np.float64) - r).max() / scale)
        worst = max(worst, e)
        if not e <= bar:
            bad.append((k, e))
    return bad, worst


def fwd_violation(got, ref):
    return float((np.abs(got - ref) / np.maximum(1, np.abs(ref))).max())


def run_front(w, images, feats, dembeds, E, p=0.0, seed=0, backward=True):
    """the kernels: (embeds, {name: gradient} or None, raw gradient blob or None)"""
    import dpt_hip
    from dpt_hip import train as tr
    rows = images.shape[0]
    blob = dpt_hip.pack_front({k: torch.tensor(v, dtype=torch.float32, device="cuda") for k, v in w.items()})
    img = torch.tensor(images, dtype=torch.float32, device="cuda").contiguous()
    ft = torch.tensor(feats, dtype=torch.float32, device="cuda").contiguous()
    d = tr.image_desc(rows, SD, A, E, flags=0 if backward else tr.FORWARD_ONLY, dropout=p, seed=seed)
    embeds, ws = tr.front_forward(d, blob, img, ft)
    if not backward:
        return embeds.cpu().numpy(), None, None
    dblob = tr.front_backward(d, blob, img, ft, ws, torch.tensor(dembeds, dtype=torch.float32, device="cuda"))
    grads = {k: v.cpu().numpy() for k, v in dpt_hip.unpack_front(dblob, SD, A, E).items()}
    return embeds.cpu().numpy(), grads, dblob


# ----------------------------------------------------------------------------- 1. the front end alone
@pytest.mark.parametrize("rows,E", sorted(FRONT_SEEDS))
def test_front_end_vs_oracle(rows, E):
    """one image, a partial image tile (5 of the forward's 4-image and the backward's 8-image tiles)
    and several tiles (21); E = 32 (float4 LayerNorm rows) and 18 (the scalar LayerNorm)"""
    seed = FRONT_SEEDS[(rows, E)]
    w = front_weights(E, 100 + seed)
    images, feats, dembeds = front_inputs(rows, E, 200 + seed)
    ref_e, ref_g, pre = front_oracle(w, images, feats, dembeds)
    assert IO.relu_margin(pre) >= IO.RELU_MARGIN, IO.relu_margin(pre)
    e32, g32, _ = front_oracle(w, images, feats, dembeds, torch.float32)
    got_e, got_g, dblob = run_front(w, images, feats, dembeds, E)
    bad, worst = violations(got_g, ref_g)
    _, worst32 = violations(g32, ref_g)
    print(f"image_front rows={rows} E={E}: embeds {fwd_violation(got_e, ref_e):.3e} (torch fp32 "
          f"{fwd_violation(e32, ref_e):.3e}), gradients {worst:.3e} of max|g| (torch fp32 {worst32:.3e})")
    assert fwd_violation(got_e, ref_e) <= 1e-5
    assert not bad, bad
    # forward-only: the same embeds bit for bit; a second backward: the same gradient blob bit for bit
    fo_e, _, _ = run_front(w, images, feats, dembeds, E, backward=False)
    assert np.array_equal(fo_e, got_e)
    _, _, dblob2 = run_front(w, images, feats, dembeds, E)
    assert torch.equal(dblob, dblob2)


def test_the_bar_can_fail():
    """conv2's weights off by 1e-3: the same comparison reports a violation"""
    rows, E = 5, 32
    seed = FRONT_SEEDS[(rows, E)]
    w = front_weights(E, 100 + seed)
    images, feats, dembeds = front_inputs(rows, E, 200 + seed)
    ref_e, ref_g, pre = front_oracle(w, images, feats, dembeds)
    assert IO.relu_margin(pre) >= IO.RELU_MARGIN
    off = dict(w)
    off["image_encoder.2.weight"] = (w["image_encoder.2.weight"] * (1 + 1e-3)).astype(np.float32).astype(np.float64)
    got_e, got_g, _ = run_front(off, images, feats, dembeds, E)
    bad, worst = violations(got_g, ref_g)
    assert bad and fwd_violation(got_e, ref_e) > 1e-5, (bad, worst, fwd_violation(got_e, ref_e))


# ----------------------------------------------------------------------------- 2. the trunk on embeds
def _trunk_model(E, T, seed):
    from models.net import Transformer
    torch.manual_seed(seed)
    m = Transformer(dict(horizon=T, state_dim=SD, action_dim=A, n_layer=2, n_embd=E, n_head=1, dropout=0.0,
                         test=False))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return m, {k: v.detach().numpy().astype(np.float64) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("E", [32, 18])
@pytest.mark.parametrize("T", [1, 2, 7])
def test_trunk_on_embeds_vs_oracle(E, T):
    """dpt_train_forward_embeds / dpt_train_backward_embeds at a matrix-core width and a row-kernel width:
    preds, every trunk gradient and dembeds under the bars, dembeds nonzero on every row (position 0
    included), the emb_w / emb_b gradient exactly zero, LAST_ONLY's last row, two backwards bit-identical"""
    from dpt_hip import train as tr
    B, L = 3, 2
    m, w = _trunk_model(E, T, 7 * E + T)
    gen = torch.Generator().manual_seed(E + T)
    embeds = torch.randn(B, T, E, generator=gen)
    dp = torch.randn(B, T, A, generator=gen)

    def oracle(dtype):
        P = IO.params(w, dtype)
        x = embeds.to(dtype).requires_grad_(True)
        preds = IO.trunk(P, x, L)
        (preds * dp.to(dtype)).sum().backward()
        g = {k: v.grad.numpy() for k, v in P.items() if v.grad is not None}
        g["dembeds"] = x.grad.numpy()
        return preds.detach().numpy(), g
    preds64, g64 = oracle(torch.float64)
    preds32, g32 = oracle(torch.float32)
    assert "embed_transition.weight" not in g64  # the oracle's trunk never reads it either

    m = m.cuda()
    params = tr.param_list(m)
    blob = tr.pack_params(params)
    d = tr.desc(L, E, SD, A, m.n_positions, B, T)
    emb_d, dp_d = embeds.cuda().contiguous(), dp.cuda().contiguous()
    runs = []
    for _ in range(2):
        preds, ws = tr.forward_embeds(d, blob, emb_d)
        runs.append((preds,) + tr.backward_embeds(d, blob, ws, dp_d))
    preds, dblob, dembeds = runs[0]
    name_of = {id(p): k for k, p in m.named_parameters()}
    got = {name_of[id(p)]: g.cpu().numpy() for p, g in zip(params, tr.unpack_grads(dblob, params))}
    assert not got.pop("embed_transition.weight").any() and not got.pop("embed_transition.bias").any()
    got["dembeds"] = dembeds.cpu().numpy()
    bad, worst = violations(got, g64)
    _, worst32 = violations(g32, g64)
    pe = fwd_violation(preds.cpu().numpy(), preds64)
    print(f"image_trunk E={E} T={T}: preds {pe:.3e} (torch fp32 {fwd_violation(preds32, preds64):.3e}), "
          f"gradients {worst:.3e} of max|g| (torch fp32 {worst32:.3e})")
    assert pe <= 1e-5 and not bad, (pe, bad)
    assert np.abs(got["dembeds"]).reshape(B * T, E).max(axis=1).min() > 0
    assert not got["transformer.wpe.weight"][T:].any()
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    # test mode: the last position alone
    dl = tr.desc(L, E, SD, A, m.n_positions, B, T, flags=tr.FORWARD_ONLY | tr.LAST_ONLY)
    last, _ = tr.forward_embeds(dl, blob, emb_d)
    assert fwd_violation(last[:, -1].cpu().numpy(), preds64[:, -1]) <= 1e-5
    assert fwd_violation(last[:, -1].cpu().numpy(), preds[:, -1].cpu().numpy().astype(np.float64)) <= 1e-5
    dfo = tr.desc(L, E, SD, A, m.n_positions, B, T, flags=tr.FORWARD_ONLY)
    full, _ = tr.forward_embeds(dfo, blob, emb_d)
    assert fwd_violation(full.cpu().numpy(), preds64) <= 1e-5


# ----------------------------------------------------------------------------- 3. the module
@pytest.fixture(scope="module")
def fx():
    return golden("image_transformer.npz")


def _module(fx, dropout=0.0, test=False):
    from models.net import ImageTransformer
    Ln, E, H, B, sd, A_ = (int(v) for v in fx["cfg"])
    m = ImageTransformer(dict(horizon=H, state_dim=sd, action_dim=A_, n_layer=Ln, n_embd=E, n_head=1, shuffle=False,
                              dropout=dropout, test=test, store_gpu=False, image_size=25))
    sd_ = {str(k): torch.from_numpy(fx["w/" + str(k)]) if "w/" + str(k) in fx else m.state_dict()[str(k)]
           for k in fx["keys"]}
    m.load_state_dict(sd_, strict=True)
    return m.cuda()


def _gpu_batch(fx):
    return {k[6:]: torch.tensor(v, dtype=torch.float32, device="cuda") for k, v in fx.items() if k.startswith("batch/")}


def _loss(pred, batch, A_):
    true = batch["optimal_actions"].unsqueeze(1).repeat(1, pred.shape[1], 1)
    return torch.nn.CrossEntropyLoss(reduction="sum")(pred.reshape(-1, A_), true.reshape(-1, A_))


def test_module_reproduces_the_reference_gradients(fx):
    """train.py:293-302 on the fixture: loss.backward() fills every parameter's .grad with the
    reference's float64 gradient under the bar; test mode returns the last position"""
    Ln, E, H, B, sd, A_ = (int(v) for v in fx["cfg"])
    w = {k[2:]: v.astype(np.float64) for k, v in fx.items() if k.startswith("w/")}
    hb = {k[6:]: v.astype(np.float64) for k, v in fx.items() if k.startswith("batch/")}
    _, _, _, pre = IO.grads(w, hb, Ln, A_)
    assert IO.relu_margin(pre) >= IO.RELU_MARGIN
    m = _module(fx)
    m.train()
    batch = _gpu_batch(fx)
    pred = m(batch)
    loss = _loss(pred, batch, A_)
    loss.backward()
    assert abs(loss.item() - float(fx["loss"])) <= 1e-5 * abs(float(fx["loss"]))
    assert fwd_violation(pred.detach().cpu().numpy(), fx["preds"]) <= 1e-5
    ref = {k[5:]: v for k, v in fx.items() if k.startswith("grad/")}
    got = {k: p.grad.cpu().numpy() for k, p in m.named_parameters() if k != "transformer.wte.weight"}
    assert set(got) == set(ref) and m.transformer.wte.weight.grad is None
    bad, worst = violations(got, ref)
    print(f"image_module fixture: gradients {worst:.3e} of max|g|")
    assert not bad, bad
    # a second forward + backward: bit-identical gradients
    first = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    m.zero_grad()
    _loss(m(batch), batch, A_).backward()
    assert all(torch.equal(first[k], p.grad) for k, p in m.named_parameters() if p.grad is not None)
    # test mode (LAST_ONLY under no_grad) = the last position; 2-dim rewards are accepted
    m.eval()
    m.test = True
    flat = dict(batch, context_rewards=batch["context_rewards"].reshape(B, H))
    with torch.no_grad():
        last, last2 = m(batch), m(flat)
    assert tuple(last.shape) == (B, A_) and torch.equal(last, last2)
    assert fwd_violation(last.cpu().numpy(), fx["preds"][:, -1]) <= 1e-5


# ----------------------------------------------------------------------------- 4. dropout
DROP_SEED = 4


def test_dropout_masks_vs_oracle(fx):
    """p = 0.1 through the autograd function: site 0, the trunk's sites and the encoder's site
    (row 1600 + c 100 + y 10 + x) regenerated by tests/philox_np.py"""
    from dpt_hip import train as tr
    from philox_np import dropout_keep
    Ln, E, H, B, sd, A_ = (int(v) for v in fx["cfg"])
    T, p, seed = H + 1, 0.1, DROP_SEED
    w = {k[2:]: v.astype(np.float64) for k, v in fx.items() if k.startswith("w/")}
    hb = {k[6:]: v.astype(np.float64) for k, v in fx.items() if k.startswith("batch/")}

    def drop(site):
        shape = (B * T, 16, 10, 10) if site == IO.SITE_IMAGE_ENC else (B, T, T) if site % 3 == 1 else (B, T, E)
        return torch.from_numpy(dropout_keep(seed, p, site, shape))
    loss_ref, preds_ref, ref, pre = IO.grads(w, hb, Ln, A_, drop=drop)
    assert IO.relu_margin(pre) >= IO.RELU_MARGIN, IO.relu_margin(pre)
    m = _module(fx, dropout=p)
    m.train()
    batch = _gpu_batch(fx)
    images, feats = IO.pack({k: v.cpu() for k, v in batch.items()}, A_, torch.float32)
    dims = (Ln, E, sd, A_, m.n_positions, B, T, 0, p, seed)
    pred = tr.ImageTransformerFunction.apply(images.cuda(), feats.cuda(), dims, *tr.image_param_list(m))[:, 1:]
    loss = _loss(pred, batch, A_)
    loss.backward()
    assert abs(loss.item() - loss_ref) <= 1e-5 * abs(loss_ref)
    assert fwd_violation(pred.detach().cpu().numpy(), preds_ref) <= 1e-5
    got = {k: q.grad.cpu().numpy() for k, q in m.named_parameters() if k != "transformer.wte.weight"}
    bad, worst = violations(got, ref)
    print(f"image_module dropout p={p}: gradients {worst:.3e} of max|g|")
    assert not bad, bad
    # the masks matter: without them the same comparison fails
    _, preds_nodrop, _, _ = IO.grads(w, hb, Ln, A_)
    assert fwd_violation(pred.detach().cpu().numpy(), preds_nodrop) > 1e-3


def test_module_dropout_seeds_from_the_cuda_generator(fx):
    """training mode with dropout > 0: the same manual_seed, the same preds; a second call, new masks;
    eval mode applies none"""
    m = _module(fx, dropout=0.3)
    batch = _gpu_batch(fx)
    m.train()
    with torch.no_grad():
        torch.manual_seed(3)
        a, b = m(batch), m(batch)
        torch.manual_seed(3)
        c = m(batch)
        assert torch.equal(a, c) and not torch.equal(a, b)
        m.eval()
        e = m(batch)
    with torch.no_grad():
        f = _module(fx).eval()(batch)
    assert torch.equal(e, f)


# ----------------------------------------------------------------------------- 5. train_miniworld.py
def test_train_miniworld_one_epoch(fx, tmp_path, monkeypatch, capsys):
    """one epoch on a synthetic dataset (2 shard pickles per split plus .npy stacks, H = 3): finite
    losses, the reference's log lines, and a checkpoint with the reference's keys"""
    import importlib
    import pickle
    H = 3
    rs = np.random.RandomState(5)
    monkeypatch.chdir(tmp_path)
    os.makedirs("datasets")
    for start in (0, 5000):
        for split, n in (("train", 3), ("test", 2)):
            trajs = []
            for i in range(n):
                path = str(tmp_path / "datasets" / f"img_{start}_{split}_{i}.npy")
                np.save(path, rs.uniform(0, 1, (H, 25, 25, 3)))
                trajs.append({"query_image": rs.uniform(0, 1, (25, 25, 3)), "query_state": rs.normal(size=2),
                              "context_images": path, "context_states": rs.normal(size=(H, 2)),
                              "context_actions": np.eye(4)[rs.randint(0, 4, H)],
                              "context_next_states": rs.normal(size=(H, 2)), "context_rewards": rs.normal(size=H),
                              "optimal_action": np.eye(4)[rs.randint(0, 4)]})
            name = f"datasets/trajs_miniworld_start{start}_end{start + 4999}_hists1_samples1_H{H}_{split}.pkl"
            with open(name, "wb") as f:
                pickle.dump(trajs, f)
    tm = importlib.import_module("train_miniworld")
    tm.main(["--env", "miniworld", "--envs", "10000", "--H", str(H), "--layer", "2", "--embd", "32", "--head", "1",
             "--num_epochs", "1", "--shuffle", "--workers", "0"])
    name = "miniworld_shufTrue_lr0.001_do0_embd32_layer2_head1_envs10000_hists1_samples1_H3_seed0"
    log = open(f"figs/loss/{name}_logs.txt").read().splitlines()
    assert log[:5] == ["Loading miniworld data...", "Done loading miniworld data", "Num train batches: 1",
                       "Num test batches: 1", "Epoch: 1"]
    vals = {}
    for line in log[5:]:
        key, val = line.strip().split(": ")
        vals[key] = float(val)
    assert list(vals) == ["Test loss", "Eval time", "Train loss", "Train time"]
    assert np.isfinite(vals["Test loss"]) and np.isfinite(vals["Train loss"]) and vals["Train loss"] > 0
    ck = torch.load(f"trained_models/{name}.pt", map_location="cpu")
    assert list(ck.keys()) == [str(k) for k in fx["keys"]]
    assert all(torch.isfinite(v).all() for v in ck.values())
