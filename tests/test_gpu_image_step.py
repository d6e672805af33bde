"""The fused image training step on the GPU (csrc/dpt_imagestep.hip, dpt_hip.train.DeviceImageData /
ImageTrainer, train_miniworld.py --fused) against dataset.image_transform, the reference-recorded fixture
tests/golden/image_transformer.npz and the float64 oracle of tests/image_oracle.py.

Shapes: 5 samples, H = 3 (window 4), 2 layers, widths 32 (the matrix-core trunk) and 18 (the row kernels).
Sample 1 of the context set starts 22,500 B in (4-byte aligned only), and a batch is 16 to 20 images, past
the front end's own row counts of 1, 5 and 21.

Bars: the normalisation and the gather are bit-exact; a gradient within 5 GRAD_TOL of the largest entry of
its float64 gradient (test_gpu_image's bar), after asserting ON THE ORACLE that every ReLU pre-activation
lies RELU_MARGIN from zero (the seeds in GRAD_SEEDS were chosen on the CPU so that it does); losses within
1e-5 relative; parameters after three steps under test_gpu_train_step._fused_steps_vs_oracle's bars."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import image_oracle as IO
from conftest import golden
from test_gpu_image import BAR, _gpu_batch, _loss, _module, violations

pytestmark = pytest.mark.gpu

SD, A, H, L, N = 2, 4, 3, 2, 5
T = H + 1
BETA1 = 0.9
# E -> seed of the gradient case's model: the first whose oracle margin is at least 2e-5 (the encoder sees
# each image by itself, so the margin does not depend on the permutation)
GRAD_SEEDS = {32: 4, 18: 2}
DATA_SEED = 11
GRAD_INDEX = [1, 4, 0, 2, 3]
GRAD_PERM = [[2, 0, 1], [1, 2, 0], [0, 2, 1], [2, 1, 0], [1, 0, 2]]
DROP_SEED = 4


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------- datasets
def _write_dataset(fx, tmp_path):
    """the fixture's two recorded trajectories as a pickle plus .npy stacks (float64, as collected)"""
    trajs = []
    for i in range(2):
        path = str(tmp_path / f"traj{i}.npy")
        np.save(path, fx[f"data/{i}/context_images"].astype(np.float64))
        t = {k: fx[f"data/{i}/{k}"].astype(np.float64) for k in ("query_image", "query_state", "context_states",
                                                                  "context_actions", "context_next_states",
                                                                  "context_rewards", "optimal_action")}
        t["context_images"] = path
        trajs.append(t)
    pkl = str(tmp_path / "trajs.pkl")
    with open(pkl, "wb") as f:
        pickle.dump(trajs, f)
    return pkl


def write_synthetic(tmp_path, seed=DATA_SEED, n=N, dtype=np.float64):
    """n random trajectories (H = 3) with raw images uniform in [0, 1]"""
    rs = np.random.RandomState(seed)
    trajs = []
    for i in range(n):
        path = str(tmp_path / f"syn{i}.npy")
        np.save(path, rs.uniform(0, 1, (H, 25, 25, 3)).astype(dtype))
        trajs.append({"query_image": rs.uniform(0, 1, (25, 25, 3)).astype(dtype), "query_state": rs.normal(size=SD),
                      "context_images": path, "context_states": rs.normal(size=(H, SD)),
                      "context_actions": np.eye(A)[rs.randint(0, A, H)],
                      "context_next_states": rs.normal(size=(H, SD)), "context_rewards": rs.normal(size=H),
                      "optimal_action": np.eye(A)[rs.randint(0, A)]})
    pkl = str(tmp_path / "syn.pkl")
    with open(pkl, "wb") as f:
        pickle.dump(trajs, f)
    return pkl


def image_dataset(pkl, horizon=H):
    from dataset import ImageDataset, image_transform
    return ImageDataset([pkl], {"shuffle": False, "horizon": horizon, "store_gpu": False, "state_dim": SD,
                                "action_dim": A}, image_transform)


def host_batch(ds, index, perm=None, dtype=torch.float64):
    """the batch ImageDataset's items collate to for the samples ``index`` with the context permuted by
    ``perm``, built on the host from the dataset's own items (image_transform per image)"""
    items = []
    for b, i in enumerate(index):
        it = {k: v for k, v in ds[int(i)].items() if k != "zeros"}
        if perm is not None:
            p = torch.as_tensor(perm[b])
            for k in ("context_images", "context_states", "context_actions", "context_next_states", "context_rewards"):
                it[k] = it[k][p]
        items.append(it)
    return {k: torch.stack([it[k] for it in items]).to(dtype) for k in items[0]}


@pytest.fixture(scope="module")
def fx():
    return golden("image_transformer.npz")


@pytest.fixture(scope="module")
def fixture_data(fx, tmp_path_factory):
    """(host ImageDataset, DeviceImageData) of the fixture's two trajectories"""
    from dpt_hip.train import DeviceImageData
    ds = image_dataset(_write_dataset(fx, tmp_path_factory.mktemp("fixture")))
    return ds, DeviceImageData(ds)


@pytest.fixture(scope="module")
def batch_data(fx):
    """the fixture's recorded batch (the one its loss and gradients were taken on; its images are
    normalised already) as a resident set of two samples"""
    from dpt_hip.train import DeviceImageData
    return DeviceImageData.from_arrays({k[6:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("batch/")})


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """(host ImageDataset, DeviceImageData) of the 5 synthetic trajectories; chunks of two stacks"""
    from dpt_hip.train import DeviceImageData
    ds = image_dataset(write_synthetic(tmp_path_factory.mktemp("synthetic")))
    dd = DeviceImageData(ds, chunk_bytes=2 * H * 25 * 25 * 3 * 8)
    assert dd.chunks == 3 + 1 and dd.image_bytes == N * T * 7500  # 5 stacks in chunks of 2, 2, 1; the queries in one
    return ds, dd


def make_model(E, seed, dropout=0.0):
    """a perturbed ImageTransformer on the host and its float64 state_dict"""
    from models.net import ImageTransformer
    torch.manual_seed(seed)
    m = ImageTransformer(dict(horizon=H, state_dim=SD, action_dim=A, n_layer=L, n_embd=E, n_head=1, shuffle=False,
                              dropout=dropout, test=False, store_gpu=False, image_size=25))
    with torch.no_grad():
        for q in m.parameters():
            q.add_(0.05 * torch.randn_like(q))
    return m, {k: v.detach().numpy().astype(np.float64) for k, v in m.state_dict().items()}


# ----------------------------------------------------------------------------- 1. normalise
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 7])
def test_normalize_is_bit_equal_to_image_transform(n, dtype):
    """dpt_image_normalize == image_transform(x).float() bit for bit, float64 and float32 raw input with
    exact 0.0 and 1.0 among the values; the same bits with ``out`` 4 bytes past an aligned address"""
    from dataset import image_transform
    from dpt_hip import train as tr
    rs = np.random.RandomState(10 * n + (dtype == np.float32))
    raw = rs.uniform(0, 1, (n, 25, 25, 3)).astype(dtype)
    raw[0, 0, 0], raw[0, 0, 1], raw[-1, 24, 24] = 0.0, 1.0, (1.0, 0.0, 1.0)
    want = torch.stack([image_transform(x).float() for x in raw])
    assert image_transform(raw[0]).dtype == (torch.float64 if dtype == np.float64 else torch.float32)
    got = tr.normalize_images(raw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3, 25, 25)
    assert torch.equal(got.cpu(), want)
    off = torch.full((n * 1875 + 1,), float("nan"), device="cuda")[1:]
    assert off.data_ptr() % 16 == 4
    tr.normalize_images(raw, off)
    assert torch.equal(off.cpu().view(n, 3, 25, 25), want)
    with pytest.raises(TypeError):
        tr.normalize_images(raw.astype(np.float16))


# ----------------------------------------------------------------------------- 2. pack
def _pack(dd, index, perm, E=32):
    from dpt_hip import _lib
    from dpt_hip import train as tr
    B = len(index)
    d = tr.desc(L, E, SD, A, 4 * (1 + dd.horizon), B, 1 + dd.horizon)
    idx = torch.as_tensor(index, dtype=torch.int64).cuda()
    pm = None if perm is None else torch.as_tensor(perm, dtype=torch.int64).cuda().contiguous()
    images = torch.full((B, 1 + dd.horizon, 3, 25, 25), float("nan"), device="cuda")
    feats = torch.full((B, 1 + dd.horizon, SD + A + 1), float("nan"), device="cuda")
    targets = torch.full((B, A), float("nan"), device="cuda")
    _lib.call("dpt_image_pack_batch", ctypes.byref(d), ctypes.byref(dd.struct), _p(idx), _p(pm), B, _p(images),
              _p(feats), _p(targets), _stream())
    return images.cpu(), feats.cpu(), targets.cpu()


@pytest.mark.parametrize("shuffle", [0, 1])
def test_pack_equals_the_reference_items(fx, fixture_data, shuffle):
    """index [0, 1] with the permutations the fixture's item_seed yields: the packed images are the
    reference's recorded items bit for bit, feats the oracle's pack of them"""
    ds, dd = fixture_data
    torch.manual_seed(int(fx["item_seed"]))
    perm = torch.stack([torch.randperm(H), torch.randperm(H)]) if shuffle else None
    images, feats, targets = _pack(dd, [0, 1], perm)
    items = {k: np.stack([fx[f"item/shuf{shuffle}/{i}/{k}"] for i in range(2)])
             for k in ("query_images", "context_images", "query_states", "context_states", "context_actions",
                       "context_rewards", "optimal_actions")}
    assert np.array_equal(images[:, 0].numpy(), items["query_images"])
    assert np.array_equal(images[:, 1:].numpy(), items["context_images"])
    ref_images, ref_feats = IO.pack(items, A, torch.float32)
    assert torch.equal(images, ref_images) and torch.equal(feats, ref_feats)
    assert np.array_equal(targets.numpy(), items["optimal_actions"])
    assert not feats[:, 0, SD:].any()  # the query row: zero action and reward


def test_pack_repeats_order_and_out_of_range(fixture_data, synthetic):
    """repeated, unsorted indices with and without permutations on both sets (the synthetic set's
    sample 1 starts 22,500 B in); an index outside [0, n) or a perm entry outside [0, H) packs zeros"""
    rs = np.random.RandomState(3)
    for (ds, dd), index in ((fixture_data, [1, 1, 0]), (synthetic, [4, 1, 1, 0, 3, 2])):
        for perm in (None, np.stack([rs.permutation(H) for _ in index])):
            images, feats, targets = _pack(dd, index, perm)
            ref = host_batch(ds, index, perm, torch.float32)
            ref_images, ref_feats = IO.pack(ref, A, torch.float32)
            assert torch.equal(images, ref_images) and torch.equal(feats, ref_feats)
            assert torch.equal(targets, ref["optimal_actions"])
    ds, dd = synthetic
    images, feats, targets = _pack(dd, [2, N, -1, 1], [[0, 1, 2], [0, 1, 2], [0, 1, 2], [1, H, -1]])
    ref_images, ref_feats = IO.pack(host_batch(ds, [2, 1], [[0, 1, 2], [1, 1, 1]], torch.float32), A, torch.float32)
    assert torch.equal(images[0], ref_images[0]) and torch.equal(feats[0], ref_feats[0])
    assert not images[1:3].any() and not feats[1:3].any() and not targets[1:3].any()
    # sample 1 with perm [1, H, -1]: the query row and transition 1, then two rows of zeros
    assert torch.equal(images[3, :2], ref_images[1, :2]) and torch.equal(feats[3, :2], ref_feats[1, :2])
    assert not images[3, 2:].any() and not feats[3, 2:].any()
    assert torch.equal(targets[3], ds.dataset["optimal_actions"][1])
    assert not torch.isnan(images).any() and not torch.isnan(feats).any() and not torch.isnan(targets).any()


def test_resident_set_allocation_failure_names_the_bytes(synthetic, monkeypatch):
    """an out-of-memory error while allocating the resident images becomes a MemoryError with the bytes they need"""
    from dpt_hip import train as tr
    ds, _ = synthetic

    def out_of_memory(*args, **kw):
        raise torch.cuda.OutOfMemoryError("HIP out of memory")
    monkeypatch.setattr(tr.torch, "empty", out_of_memory)
    with pytest.raises(MemoryError, match=f"{N * T * 7500} bytes"):
        tr.DeviceImageData(ds)


# ----------------------------------------------------------------------------- 3. the gradient
def split_blobs(front, trunk, m):
    """float64 front-blob and trunk-blob vectors as {name: array shaped like the parameter} (nn.Linear
    weights are [in][out] in the blobs), without the code under test; the trunk's emb region is returned
    apart"""
    named = dict(m.named_parameters())
    out, off = {}, 0
    for k in IO.FRONT_KEYS:
        q = named[k]
        flat = front[off:off + q.numel()]
        linear = k in ("image_encoder.6.weight", "embed_transition.weight")
        out[k] = flat.reshape(q.shape[1], q.shape[0]).T if linear else flat.reshape(tuple(q.shape))
        off += q.numel()
    assert off == front.size
    emb_numel = (2 * SD + A + 1) * m.n_embd + m.n_embd
    off = emb_numel
    keys = ["transformer.wpe.weight"]
    for i in range(m.n_layer):
        keys += [f"transformer.h.{i}.{s}.{wb}" for s in ("ln_1", "attn.c_attn", "attn.c_proj", "ln_2", "mlp.c_fc",
                                                         "mlp.c_proj") for wb in ("weight", "bias")]
    keys += ["transformer.ln_f.weight", "transformer.ln_f.bias", "pred_actions.weight", "pred_actions.bias"]
    for k in keys:
        q = named[k]
        flat = trunk[off:off + q.numel()]
        out[k] = flat.reshape(q.shape[1], q.shape[0]).T if k == "pred_actions.weight" else flat.reshape(tuple(q.shape))
        off += q.numel()
    assert off == trunk.size and set(out) == set(named) - {"transformer.wte.weight"}
    return out, trunk[:emb_numel]


def step_gradient(trainer):
    """the gradient of a fresh trainer's first step from AdamW's first moment: m_1 = (1 - beta1) g"""
    front = trainer.front_m.cpu().numpy().astype(np.float64) / (1 - BETA1)
    trunk = trainer.m.cpu().numpy().astype(np.float64) / (1 - BETA1)
    return split_blobs(front, trunk, trainer.model)


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("E", [32, 18])
def test_fused_image_step_gradient(synthetic, E, permuted):
    """The gradient inside dpt_image_train_step, per parameter of both blobs, against image_oracle.grads in
    float64 on the same samples and permutation; the trunk's emb region and its m and v stay exactly zero.
    Control: a step that used a non-identity perm violates the same bar against the unpermuted oracle."""
    from dpt_hip.train import ImageTrainer
    ds, dd = synthetic
    perm = GRAD_PERM if permuted else None
    m, w64 = make_model(E, GRAD_SEEDS[E])
    hb = {k: v.numpy() for k, v in host_batch(ds, GRAD_INDEX, perm).items()}
    loss_ref, _, ref, pre = IO.grads(w64, hb, L, A)
    assert IO.relu_margin(pre) >= IO.RELU_MARGIN, IO.relu_margin(pre)
    trainer = ImageTrainer(m.cuda(), lr=1e-3, weight_decay=1e-4, betas=(BETA1, 0.999))
    trainer.step(dd, GRAD_INDEX, perm)
    loss = trainer.read_loss()
    got, emb_grad = step_gradient(trainer)
    bad, worst = violations(got, ref)
    print(f"image_step gradient E={E} perm={permuted}: loss {loss!r} ref {loss_ref!r}, gradients {worst:.3e} of max|g|")
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref), (loss, loss_ref)
    assert not bad, bad
    n_emb = trainer.emb_numel
    assert not emb_grad.any() and not trainer.blob[:n_emb].any() and not trainer.m[:n_emb].any() \
        and not trainer.v[:n_emb].any()
    if permuted:
        _, _, plain, _ = IO.grads(w64, {k: v.numpy() for k, v in host_batch(ds, GRAD_INDEX).items()}, L, A)
        bad, worst = violations(got, plain)
        assert bad, worst


# ----------------------------------------------------------------------------- 4. steps
def steps_vs_oracle(m, w64, ds, dd, plans, lr=1e-3):
    """ImageTrainer.step over the index batches ``plans`` against the same AdamW steps on the float64
    oracle's gradients, under test_gpu_train_step._fused_steps_vs_oracle's bars"""
    from dpt_hip.train import ImageTrainer
    P = IO.params(w64)
    names = list(P)
    opt_ref = torch.optim.AdamW([P[k] for k in names], lr=lr, weight_decay=1e-4)
    wte = m.transformer.wte.weight.detach().clone()
    trainer = ImageTrainer(m, lr=lr, weight_decay=1e-4)
    for idx in plans:
        trainer.step(dd, torch.tensor(idx))
        loss = trainer.read_loss()
        opt_ref.zero_grad()
        ref_loss = IO.train_loss(P, host_batch(ds, idx), L, A)[0]
        ref_loss.backward()
        opt_ref.step()
        assert abs(loss - ref_loss.item()) <= 1e-5 * abs(ref_loss.item()), (loss, ref_loss.item())
    assert trainer.read_loss() == 0.0 and trainer.steps == len(plans)
    trainer.sync_to_model()
    params = dict(m.named_parameters())
    assert torch.equal(params["transformer.wte.weight"], wte)
    diffs = np.concatenate([np.abs(params[k].detach().cpu().numpy() - P[k].detach().numpy()).ravel() for k in names])
    assert (diffs <= 1e-5).mean() >= 0.995, (diffs <= 1e-5).mean()
    assert diffs.max() <= 2 * lr * len(plans) + 1e-5
    return trainer


@pytest.mark.parametrize("plans", [[[0, 1, 2, 3]] * 3, [[0, 1, 2, 3], [3, 1, 2], [2, 0]]],
                         ids=["full_batches", "smaller_last_batches"])
@pytest.mark.parametrize("E", [32, 18])
def test_fused_image_steps_track_the_float64_oracle(synthetic, E, plans):
    ds, dd = synthetic
    m, w64 = make_model(E, 40 + E)
    steps_vs_oracle(m.cuda(), w64, ds, dd, plans)


# ----------------------------------------------------------------------------- 5. eval loss
def test_eval_loss_equals_the_module_and_the_fixture(fx, batch_data):
    """ImageTrainer.eval_loss against the module's no-grad training-mode forward with torch's summed
    cross-entropy and against the reference's recorded loss; nothing of the trainer's state moves"""
    from dpt_hip.train import ImageTrainer
    dd = batch_data
    A_ = int(fx["cfg"][5])
    m = _module(fx)
    m.train()
    batch = _gpu_batch(fx)
    with torch.no_grad():
        ref = _loss(m(batch), batch, A_).item()
    trainer = ImageTrainer(m, lr=1e-3)
    state = [t.clone() for t in (trainer.blob, trainer.front_blob, trainer.m, trainer.v, trainer.front_m,
                                 trainer.front_v)]
    trainer.eval_loss(dd, [0, 1])
    got = trainer.read_loss()
    assert abs(got - ref) <= 1e-5 * abs(ref), (got, ref)
    assert abs(got - float(fx["loss"])) <= 1e-5 * abs(float(fx["loss"])), (got, float(fx["loss"]))
    trainer.eval_loss(dd, [1])   # smaller batches on the same workspace
    trainer.eval_loss(dd, [0])
    assert abs(trainer.read_loss() - ref) <= 1e-5 * abs(ref)
    now = (trainer.blob, trainer.front_blob, trainer.m, trainer.v, trainer.front_m, trainer.front_v)
    assert all(torch.equal(a, b) for a, b in zip(state, now)) and trainer.steps == 0


# ----------------------------------------------------------------------------- 6. dropout
def test_dropout_masks_of_the_fused_step(fx, batch_data):
    """p = 0.1 with an injected seed: the first step's loss is the oracle's with the masks regenerated by
    tests/philox_np.py (the encoder's site, site 0 and the trunk's); seed=None draws fresh masks from the
    CUDA generator, reproduced by torch.manual_seed"""
    from dpt_hip.train import ImageTrainer
    from philox_np import dropout_keep
    dd = batch_data
    Ln, E, H_, B, sd, A_ = (int(v) for v in fx["cfg"])
    T_, p = H_ + 1, 0.1
    w = {k[2:]: v.astype(np.float64) for k, v in fx.items() if k.startswith("w/")}
    hb = {k[6:]: v.astype(np.float64) for k, v in fx.items() if k.startswith("batch/")}

    def drop(site):
        shape = (B * T_, 16, 10, 10) if site == IO.SITE_IMAGE_ENC else (B, T_, T_) if site % 3 == 1 else (B, T_, E)
        return torch.from_numpy(dropout_keep(DROP_SEED, p, site, shape))
    with torch.no_grad():
        loss_ref = IO.train_loss(IO.params(w), hb, Ln, A_, drop)[0].item()
    trainer = ImageTrainer(_module(fx, dropout=p), lr=1e-3)
    trainer.step(dd, [0, 1], seed=DROP_SEED)
    loss = trainer.read_loss()
    plain = float(fx["loss"])
    print(f"image_step dropout p={p}: loss {loss!r} ref {loss_ref!r} (no dropout {plain!r})")
    assert abs(loss - loss_ref) <= 1e-5 * abs(loss_ref), (loss, loss_ref)
    assert abs(loss - plain) > 1e-3 * abs(plain)
    # seed=None: fresh masks per call (on the same weights: eval_loss), the same ones after the same manual_seed
    trainer = ImageTrainer(_module(fx, dropout=p), lr=1e-3)
    losses = []
    for seed in (3, 3):
        torch.manual_seed(seed)
        for _ in range(2):
            trainer.eval_loss(dd, [0, 1])
            losses.append(trainer.read_loss())
    assert losses[0] == losses[2] and losses[1] == losses[3] and losses[0] != losses[1]
    # and through step: two runs of two seed=None steps under one manual_seed end in the same bits
    ends = []
    for _ in range(2):
        torch.manual_seed(5)
        trainer = ImageTrainer(_module(fx, dropout=p), lr=1e-3)
        first = []
        for _ in range(2):
            trainer.step(dd, [0, 1])
            first.append(trainer.read_loss())
        ends.append((trainer.blob.clone(), trainer.front_blob.clone(), first))
    assert torch.equal(ends[0][0], ends[1][0]) and torch.equal(ends[0][1], ends[1][1]) and ends[0][2] == ends[1][2]
    assert ends[0][2][0] != loss  # another seed than DROP_SEED, other masks on the same weights


# ----------------------------------------------------------------------------- 7. determinism
def test_two_trainers_end_bit_identical(synthetic):
    from dpt_hip.train import ImageTrainer
    _, dd = synthetic
    ends = []
    for _ in range(2):
        m, _ = make_model(32, 9)
        trainer = ImageTrainer(m.cuda(), lr=1e-3)
        for idx, perm in (([0, 1, 2, 3, 4], GRAD_PERM), ([3, 1, 2], None), ([2, 0, 2, 4], GRAD_PERM[:4])):
            trainer.step(dd, idx, perm)
        ends.append((trainer.blob, trainer.front_blob, trainer.m, trainer.v, trainer.front_m, trainer.front_v,
                     trainer.loss.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*ends))
    assert ends[0][6].item() > 0


# ----------------------------------------------------------------------------- 8. train_miniworld.py --fused
def test_train_miniworld_fused_one_epoch(fx, tmp_path, monkeypatch):
    """test_gpu_image.test_train_miniworld_one_epoch's synthetic dataset through --fused: the same log
    lines and checkpoint keys, and under the same --seed the default path's epoch-1 test loss and train
    loss (one batch: the pre-update loss) within 1e-5 relative"""
    import importlib
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
    args = ["--env", "miniworld", "--envs", "10000", "--H", str(H), "--layer", "2", "--embd", "32", "--head", "1",
            "--num_epochs", "1", "--shuffle", "--workers", "0", "--seed", "3"]
    name = "miniworld_shufTrue_lr0.001_do0_embd32_layer2_head1_envs10000_hists1_samples1_H3_seed3"
    runs = []
    for extra in ([], ["--fused"]):
        tm.main(args + extra)
        log = open(f"figs/loss/{name}_logs.txt").read().splitlines()
        assert log[:5] == ["Loading miniworld data...", "Done loading miniworld data", "Num train batches: 1",
                           "Num test batches: 1", "Epoch: 1"]
        vals = {}
        for line in log[5:]:
            key, val = line.strip().split(": ")
            vals[key] = float(val)
        assert list(vals) == ["Test loss", "Eval time", "Train loss", "Train time"]
        ck = torch.load(f"trained_models/{name}.pt", map_location="cpu")
        assert list(ck.keys()) == [str(k) for k in fx["keys"]]
        assert all(torch.isfinite(v).all() for v in ck.values())
        runs.append((vals, ck))
    (plain, ck_plain), (fused, ck_fused) = runs
    print(f"train_miniworld: default {plain['Test loss']!r} / {plain['Train loss']!r}, "
          f"--fused {fused['Test loss']!r} / {fused['Train loss']!r}")
    assert fused["Train loss"] > 0
    for key in ("Test loss", "Train loss"):
        assert abs(fused[key] - plain[key]) <= 1e-5 * abs(plain[key]), (key, fused[key], plain[key])
    # both runs took one AdamW step from one initialisation: the checkpoints agree to the step's size
    assert torch.equal(ck_fused["transformer.wte.weight"], ck_plain["transformer.wte.weight"])
    worst = max(float((ck_fused[k] - ck_plain[k]).abs().max()) for k in ck_plain)
    assert worst <= 2 * 1e-3 + 1e-5, worst
