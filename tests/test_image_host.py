"""CPU checks of the image-conditioned DPT (include/dpt_hip.h "image-conditioned DPT", csrc/dpt_image.hip,
models.net.ImageTransformer, dataset.ImageDataset, train_miniworld.py): the new symbols and
dpt_image_desc's layout, every host check failing before a launch with a message, the numel functions
against a Python restatement, the float64 oracle helper against the reference-recorded fixture
(tests/golden/image_transformer.npz), ImageDataset items and the filename builders against it, the
module's parameter names, and the new source under the ISA hazard scan and without scratch.  No device
work is launched."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import image_oracle as IO
from conftest import ROOT, golden
from test_isa_hazards import HIPCC, test_no_short_mfma_hazard_paths as hazard_scan
from test_resource_budget import remarks

NEW_SYMBOLS = ("dpt_image_front_blob_numel", "dpt_image_front_workspace_numel", "dpt_image_front_forward",
               "dpt_image_front_backward", "dpt_train_forward_embeds", "dpt_train_backward_embeds")


@pytest.fixture(scope="module")
def fx():
    return golden("image_transformer.npz")


def _lib():
    from dpt_hip import _lib
    return _lib, _lib.load()


def test_new_symbols_and_abi_version():
    L, lib = _lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert lib.dpt_abi_version() == 8 == L.ABI_VERSION
    assert L.SITE_IMAGE_ENC == 1 << 20 == IO.SITE_IMAGE_ENC


def test_image_desc_layout_matches_header(tmp_path):
    L, _ = _lib()
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dpt_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(dpt_image_desc));']
    for fname, _t in L.ImageDesc._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(dpt_image_desc, {fname}));')
    lines.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(tmp_path / "layout")], check=True,
                                                              capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.ImageDesc) == 40
    for fname, _t in L.ImageDesc._fields_:
        assert int(got[fname]) == getattr(L.ImageDesc, fname).offset, fname


def _desc(**kw):
    from dpt_hip import train as tr
    args = dict(rows=6, state_dim=2, action_dim=4, n_embd=32, flags=0, dropout=0.0, seed=0, image_size=25)
    args.update(kw)
    return tr.image_desc(**args)


def _numel_py(rows, sd, A, E, fwd_only):
    """the workspace of csrc/dpt_image.hip ImgWs restated: the token rows, embed_transition's rows and
    embed_ln's statistics; then the dropped conv2 activations, the three gradient rows and the partials
    (64-row chunks of the row kernels' weight gradients, 8-image groups of the conv gradients)"""
    r4 = lambda n: (n + 3) & ~3  # noqa: E731
    F = 8 + sd + A + 1
    n = r4(rows * F) + r4(rows * E) + r4(rows * 2)
    if fwd_only:
        return n
    nch, groups = (rows + 63) // 64, (rows + 7) // 8
    part = max(nch * (F + 1) * E, nch * 2 * E, nch * 1601 * 8, groups * (432 + 16 + 2304 + 16))
    return n + rows * 1600 + r4(rows * E) + r4(rows * F) + rows * 8 + r4(part)


@pytest.mark.parametrize("rows,sd,A,E", [(1, 2, 4, 32), (5, 2, 4, 18), (21, 0, 1, 7), (3264, 2, 4, 32)])
def test_numel_functions(rows, sd, A, E):
    from dpt_hip import train as tr
    L, lib = _lib()
    F = 8 + sd + A + 1
    for flags in (0, L.TRAIN_FORWARD_ONLY):
        d = _desc(rows=rows, state_dim=sd, action_dim=A, n_embd=E, flags=flags)
        assert tr._numel("dpt_image_front_blob_numel", d) == 432 + 16 + 2304 + 16 + 1600 * 8 + 8 + F * E + 3 * E
        assert tr._numel("dpt_image_front_workspace_numel", d) == _numel_py(rows, sd, A, E, bool(flags))


BAD_DESCS = [(dict(rows=0), ValueError, "rows"), (dict(image_size=24), NotImplementedError, "image_size"),
             (dict(n_embd=0), ValueError, "n_embd"), (dict(state_dim=-1), ValueError, "state_dim"),
             (dict(action_dim=0), ValueError, "action_dim"), (dict(dropout=1.0), ValueError, "dropout"),
             (dict(dropout=-0.1), ValueError, "dropout"), (dict(dropout=float("nan")), ValueError, "dropout"),
             (dict(flags=2), ValueError, "flags")]


@pytest.mark.parametrize("kw,exc,word", BAD_DESCS)
def test_host_checks_reject_the_desc_before_a_launch(kw, exc, word):
    """no device is needed: every entry point refuses the desc on the host, with a message"""
    L, lib = _lib()
    d = _desc(**kw)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    n = ctypes.c_int64()
    calls = [("dpt_image_front_blob_numel", (ctypes.byref(d), ctypes.byref(n))),
             ("dpt_image_front_workspace_numel", (ctypes.byref(d), ctypes.byref(n))),
             ("dpt_image_front_forward", (ctypes.byref(d), p, p, p, p, p, None)),
             ("dpt_image_front_backward", (ctypes.byref(d), p, p, p, p, p, p, None))]
    for name, args in calls:
        with pytest.raises(exc):
            L.call(name, *args)
        assert word in lib.dpt_last_error().decode(), (name, lib.dpt_last_error())


def test_host_checks_reserved_pointers_alignment_and_forward_only():
    L, lib = _lib()
    buf = ctypes.create_string_buffer(64)
    base = (ctypes.addressof(buf) + 15) & ~15
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    n = ctypes.c_int64()
    d = _desc()
    d.reserved = 1
    with pytest.raises(ValueError, match="reserved"):
        L.call("dpt_image_front_workspace_numel", ctypes.byref(d), ctypes.byref(n))
    with pytest.raises(ValueError, match="reserved"):
        L.call("dpt_image_front_forward", ctypes.byref(d), p, p, p, p, p, None)
    d = _desc()
    with pytest.raises(ValueError, match="null"):
        L.call("dpt_image_front_blob_numel", None, ctypes.byref(n))
    with pytest.raises(ValueError, match="null"):
        L.call("dpt_image_front_blob_numel", ctypes.byref(d), None)
    with pytest.raises(ValueError, match="null"):
        L.call("dpt_image_front_workspace_numel", ctypes.byref(d), None)
    for hole in range(5):  # each pointer of the forward in turn
        args = [p] * 5
        args[hole] = None
        with pytest.raises(ValueError, match="null pointer"):
            L.call("dpt_image_front_forward", ctypes.byref(d), *args, None)
    for hole in range(6):
        args = [p] * 6
        args[hole] = None
        with pytest.raises(ValueError, match="null pointer"):
            L.call("dpt_image_front_backward", ctypes.byref(d), *args, None)
    with pytest.raises(ValueError, match="16-byte aligned"):
        L.call("dpt_image_front_forward", ctypes.byref(d), p, p, p, odd, p, None)
    with pytest.raises(ValueError, match="16-byte aligned"):
        L.call("dpt_image_front_backward", ctypes.byref(d), p, p, p, odd, p, p, None)
    fo = _desc(flags=L.TRAIN_FORWARD_ONLY)
    with pytest.raises(ValueError, match="forward-only"):
        L.call("dpt_image_front_backward", ctypes.byref(fo), p, p, p, p, p, p, None)


def test_embeds_entry_points_check_on_the_host():
    from dpt_hip import train as tr
    L, lib = _lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    d = tr.desc(2, 32, 2, 4, 16, 2, 4)
    for hole in range(4):
        args = [p] * 4
        args[hole] = None
        with pytest.raises(ValueError, match="null pointer"):
            L.call("dpt_train_forward_embeds", ctypes.byref(d), *args, None)
    for hole in range(5):
        args = [p] * 5
        args[hole] = None
        with pytest.raises(ValueError, match="null pointer"):
            L.call("dpt_train_backward_embeds", ctypes.byref(d), *args, None)
    fo = tr.desc(2, 32, 2, 4, 16, 2, 4, flags=tr.FORWARD_ONLY)
    with pytest.raises(ValueError, match="forward-only"):
        L.call("dpt_train_backward_embeds", ctypes.byref(fo), p, p, p, p, p, None)
    bad = tr.desc(2, 32, 2, 4, 16, 2, 17)  # window past n_positions
    with pytest.raises(ValueError):
        L.call("dpt_train_forward_embeds", ctypes.byref(bad), p, p, p, p, None)


# ----------------------------------------------------------------------------- oracle helper and fixture
def _weights(fx):
    return {k[2:]: v.astype(np.float64) for k, v in fx.items() if k.startswith("w/")}


def _batch(fx):
    return {k[6:]: v.astype(np.float64) for k, v in fx.items() if k.startswith("batch/")}


def test_oracle_helper_equals_the_reference_fixture(fx):
    Ln, E, H, B, sd, A = (int(v) for v in fx["cfg"])
    loss, preds, grads, pre = IO.grads(_weights(fx), _batch(fx), Ln, A)
    assert IO.relu_margin(pre) >= IO.RELU_MARGIN
    assert abs(loss - float(fx["loss"])) <= 1e-10 * abs(float(fx["loss"]))
    assert np.abs(preds - fx["preds"]).max() <= 1e-10 * np.abs(fx["preds"]).max()
    keys = [k[5:] for k in fx if k.startswith("grad/")]
    assert set(keys) == set(grads) and len(keys) == 10 + 1 + 12 * Ln + 4
    for k in keys:
        ref = fx["grad/" + k]
        assert np.abs(grads[k] - ref).max() <= 1e-10 * np.abs(ref).max(), k
    assert not fx["grad/transformer.wpe.weight"][H + 1:].any()


def test_oracle_dropout_sites_and_pre_activation_shapes(fx):
    """the drop callable reaches the encoder site with the (rows, 16, 10, 10) tensor and the trunk's"""
    Ln, E, H, B, sd, A = (int(v) for v in fx["cfg"])
    seen = {}

    def drop(site):
        shape = {IO.SITE_IMAGE_ENC: (B * (H + 1), 16, 10, 10), 0: (B, H + 1, E)}.get(site)
        if shape is None:
            shape = (B, H + 1, H + 1) if site % 3 == 1 else (B, H + 1, E)
        seen[site] = shape
        return torch.ones(shape, dtype=torch.float64)

    P = IO.params(_weights(fx))
    images, feats = IO.pack(_batch(fx), A)
    preds, pre = IO.forward(P, images, feats, Ln, drop)
    assert set(seen) == {IO.SITE_IMAGE_ENC, 0} | {1 + 3 * i + j for i in range(Ln) for j in range(3)}
    assert [tuple(z.shape) for z in pre] == [(B * (H + 1), 16, 12, 12), (B * (H + 1), 16, 10, 10), (B * (H + 1), 8)]
    assert np.abs(preds[:, 1:].detach().numpy() - fx["preds"]).max() <= 1e-10 * np.abs(fx["preds"]).max()


# ----------------------------------------------------------------------------- module, dataset, names
def _config(fx, **kw):
    Ln, E, H, B, sd, A = (int(v) for v in fx["cfg"])
    cfg = dict(horizon=H, state_dim=sd, action_dim=A, n_layer=Ln, n_embd=E, n_head=1, shuffle=False, dropout=0.0,
               test=False, store_gpu=False, image_size=25)
    cfg.update(kw)
    return cfg


def test_module_keeps_the_reference_parameter_names(fx):
    from models.net import ImageTransformer
    m = ImageTransformer(_config(fx))
    assert list(m.state_dict().keys()) == [str(k) for k in fx["keys"]]
    sd = {k: torch.from_numpy(fx["w/" + k]) if "w/" + k in fx else v for k, v in m.state_dict().items()}
    assert set(sd) - {"transformer.wte.weight"} == {k[2:] for k in fx if k.startswith("w/")}
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        if k != "transformer.wte.weight":
            assert np.array_equal(v.numpy(), fx["w/" + k]), k
    with pytest.raises(NotImplementedError, match="image_size"):
        ImageTransformer(_config(fx, image_size=32))


def test_module_initialisation():
    """torch's defaults for the encoder (uniform within 1 / sqrt(fan_in)), GPT-2's for embed_transition"""
    from models.net import ImageTransformer
    m = ImageTransformer(dict(horizon=3, state_dim=2, action_dim=4, n_layer=1, n_embd=64, n_head=1, shuffle=False,
                              dropout=0.0, test=False, image_size=25))
    for idx, fan in ((0, 27), (2, 144), (6, 1600)):
        w = m.image_encoder[idx].weight.detach()
        assert w.abs().max() <= fan ** -0.5 and w.abs().max() > 0.8 * fan ** -0.5 and w.std() > 0.4 * fan ** -0.5
        assert m.image_encoder[idx].bias.detach().abs().max() > 0
    assert tuple(m.embed_transition.weight.shape) == (64, 15)
    assert abs(float(m.embed_transition.weight.detach().std()) - 0.02) < 0.004 and not m.embed_transition.bias.any()
    assert bool((m.embed_ln.weight == 1).all()) and not m.embed_ln.bias.any()


def test_pack_front_roundtrip(fx):
    import dpt_hip
    Ln, E, H, B, sd, A = (int(v) for v in fx["cfg"])
    w = {k: torch.from_numpy(fx["w/" + k]) for k in dpt_hip.FRONT_KEYS}
    blob = dpt_hip.pack_front(w)
    assert blob.numel() == 2768 + 12808 + 15 * E + 3 * E and blob.dtype == torch.float32
    assert np.array_equal(blob[:432].numpy(), fx["w/image_encoder.0.weight"].reshape(-1))
    assert np.array_equal(blob[448:448 + 2304].numpy(), fx["w/image_encoder.2.weight"].reshape(-1))
    assert np.array_equal(blob[2768:2768 + 12800].view(1600, 8).numpy(), fx["w/image_encoder.6.weight"].T)
    assert np.array_equal(blob[15576:15576 + 15 * E].view(15, E).numpy(), fx["w/embed_transition.weight"].T)
    back = dpt_hip.unpack_front(blob, sd, A, E)
    assert tuple(back) == dpt_hip.FRONT_KEYS
    for k in dpt_hip.FRONT_KEYS:
        assert np.array_equal(back[k].numpy(), fx["w/" + k]), k


def _write_dataset(fx, tmp_path):
    import pickle
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


@pytest.mark.parametrize("shuffle", [0, 1])
def test_image_dataset_items_equal_the_reference(fx, tmp_path, shuffle):
    from dataset import ImageDataset, image_transform
    Ln, E, H, B, sd, A = (int(v) for v in fx["cfg"])
    ds = ImageDataset([_write_dataset(fx, tmp_path)], {"shuffle": bool(shuffle), "horizon": H, "store_gpu": True,
                                                       "state_dim": sd, "action_dim": A}, image_transform)
    assert len(ds) == 2 and ds.store_gpu is False
    torch.manual_seed(int(fx["item_seed"]))
    keys = [k.split("/")[-1] for k in fx if k.startswith(f"item/shuf{shuffle}/0/")]
    for i in range(2):
        item = ds[i]
        assert list(item.keys()) == keys
        for k in keys:
            ref = fx[f"item/shuf{shuffle}/{i}/{k}"]
            assert item[k].dtype == torch.float32 and np.array_equal(item[k].numpy(), ref), (i, k)
    # one randperm per item and nothing else: the generator stands where two draws leave it
    torch.manual_seed(int(fx["item_seed"]))
    if shuffle:
        torch.randperm(H), torch.randperm(H)
    after = torch.rand(1)
    torch.manual_seed(int(fx["item_seed"]))
    ds[0], ds[1]
    assert torch.equal(torch.rand(1), after)


def test_image_transform_is_float64_then_chw():
    from dataset import image_transform
    x = np.random.RandomState(0).uniform(0, 1, (25, 25, 3))
    t = image_transform(x)
    assert t.dtype == torch.float64 and tuple(t.shape) == (3, 25, 25)
    mean, std = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
    assert np.array_equal(t.numpy(), ((x - mean) / std).transpose(2, 0, 1))


def test_filename_builders_equal_the_reference(fx):
    from utils import build_miniworld_data_filename, build_miniworld_model_filename
    dcfg = {"n_hists": 1, "n_samples": 1, "horizon": 50, "dim": 10, "rollin_type": "uniform"}
    mcfg = {"shuffle": True, "lr": 0.001, "dropout": 0.1, "n_embd": 32, "n_layer": 4, "n_head": 4, "n_envs": 60000,
            "n_hists": 1, "n_samples": 1, "horizon": 50, "dim": 10, "seed": 3}
    got = [build_miniworld_data_filename("miniworld", 5000, 9999, dcfg, mode=m) for m in (0, 1, 2)]
    assert got == [str(s) for s in fx["names/data"]]
    assert build_miniworld_model_filename("miniworld", mcfg) == str(fx["names/model"])


def test_train_cli_still_refuses_miniworld_and_names_the_script(tmp_path, monkeypatch):
    import importlib
    train = importlib.import_module("train")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match="train_miniworld.py"):
        train.main(["--env", "miniworld"])
    assert not os.path.exists(tmp_path / "datasets")
    tm = importlib.import_module("train_miniworld")
    with pytest.raises(NotImplementedError, match="miniworld"):
        tm.main(["--env", "bandit"])


# ----------------------------------------------------------------------------- the new source
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_image_source_passes_the_hazard_scan(tmp_path):
    hazard_scan("dpt_image.hip", tmp_path)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_image_kernels_use_no_scratch(tmp_path):
    r = remarks("dpt_image.hip", tmp_path)
    names = [n for n in r if "img_enc" in n]
    assert len(names) == 3, list(r)
    for n in names:
        assert r[n]["scratch"] == 0 and r[n]["occ"] >= 2, (n, r[n])
