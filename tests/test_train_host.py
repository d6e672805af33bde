"""CPU checks of the training stage: dataset.py / the index view against batches recorded from the
reference's Dataset and DataLoader (tests/golden/train_loader.npz, gen_golden_train.py), the
training-step C ABI (symbols, struct layouts, host-side validation with no device present), the
ISA hazard scan of the new source, and train.py's argument errors.  No device work is launched."""
import ctypes
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden

CSRC = os.path.join(ROOT, "decision-pretrained-transformer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
TRAJ_KEYS = ("context_states", "context_actions", "context_next_states", "context_rewards", "query_state",
             "optimal_action")
CONTEXT = ("context_states", "context_actions", "context_next_states", "context_rewards")
NEW_SYMBOLS = ("dpt_train_pack_batch", "dpt_train_ce_loss", "dpt_adamw_step", "dpt_train_step_workspace_numel",
               "dpt_train_step", "dpt_train_eval_loss")


@pytest.fixture(scope="module")
def fixture():
    return golden("train_loader.npz")


def _our_dataset(g, name, shuffle, tmp_path):
    from dataset import Dataset
    n, H, sd, A = (int(x) for x in g[f"{name}/cfg"])
    trajs = [{k: g[f"{name}/traj/{k}"][i] for k in TRAJ_KEYS} for i in range(n)]
    path = tmp_path / f"{name}.pkl"
    with open(path, "wb") as f:
        pickle.dump(trajs, f)
    return Dataset(str(path), {"shuffle": shuffle, "horizon": H, "store_gpu": False, "state_dim": sd,
                               "action_dim": A})


def _gather(g, name, index, perm):
    """the (index, perm) plan applied to the recorded trajectories with numpy -> the batch dict"""
    tr = {k: g[f"{name}/traj/{k}"].astype(np.float32) for k in TRAJ_KEYS}
    B = len(index)
    out = {"query_states": tr["query_state"][index], "optimal_actions": tr["optimal_action"][index]}
    for k in CONTEXT:
        rows = tr[k][index]
        if perm is not None:
            rows = rows[np.arange(B)[:, None], perm]
        out[k] = rows.reshape(B, rows.shape[1], -1)
    return out


@pytest.mark.parametrize("name", ["bandit", "darkroom"])
@pytest.mark.parametrize("shuffle", [False, True])
def test_loader_reproduces_reference_batches(fixture, name, shuffle, tmp_path):
    """Our Dataset's index view under the reference's DataLoader settings and seed yields the
    reference's batches: every tensor of every batch of two epochs, exactly."""
    g = fixture
    ds = _our_dataset(g, name, shuffle, tmp_path)
    n, H, sd, A = (int(x) for x in g[f"{name}/cfg"])
    assert len(ds) == n and tuple(ds.zeros.shape) == (sd * sd + A + 1,)
    torch.manual_seed(int(g["loader_seed"]))
    loader = torch.utils.data.DataLoader(ds.index_view(), batch_size=int(g["batch_size"]), shuffle=True)
    pre = f"{name}/shuf{int(shuffle)}"
    assert len(loader) == int(g[f"{pre}/batches"])
    for e in range(2):
        for b, batch in enumerate(loader):
            if shuffle:
                index, perm = (t.numpy() for t in batch)
                assert perm.shape == (len(index), H) and perm.dtype == np.int64
            else:
                index, perm = batch.numpy(), None
            assert index.dtype == np.int64
            got = _gather(g, name, index, perm)
            for k, v in got.items():
                ref = g[f"{pre}/e{e}/b{b}/{k}"]
                assert ref.dtype == np.float32 and np.array_equal(v, ref), (e, b, k)
            assert np.array_equal(np.broadcast_to(ds.zeros.numpy(), (len(index), sd * sd + A + 1)),
                                  g[f"{pre}/e{e}/b{b}/zeros"])
        assert b + 1 == len(loader)


@pytest.mark.parametrize("name", ["bandit", "darkroom"])
@pytest.mark.parametrize("shuffle", [False, True])
def test_dataset_items_equal_reference(fixture, name, shuffle, tmp_path):
    """Dataset.__getitem__ (the reference surface: same dict, same shapes, shuffle drawing one
    torch.randperm(horizon) per item) against the reference's items under the same seed."""
    g = fixture
    ds = _our_dataset(g, name, shuffle, tmp_path)
    assert set(ds.dataset) == {"query_states", "optimal_actions", "context_states", "context_actions",
                               "context_next_states", "context_rewards"}
    assert ds.dataset["context_rewards"].dim() == 3
    torch.manual_seed(int(g["item_seed"]))
    for i in range(len(ds)):
        item = ds[i]
        assert set(item) == set(CONTEXT) | {"query_states", "optimal_actions", "zeros"}
        for k, v in item.items():
            ref = g[f"{name}/shuf{int(shuffle)}/item{i}/{k}"]
            assert v.dtype == torch.float32 and np.array_equal(v.numpy(), ref), (i, k)


def test_new_symbols_exported():
    from dpt_hip import _lib
    lib = _lib.load()
    assert lib.dpt_abi_version() == 8 == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


def test_train_step_struct_layouts_match_header(tmp_path):
    """dpt_train_data / dpt_adamw_args: ctypes against the C compiler's layout, field by field."""
    from dpt_hip import _lib
    structs = {"dpt_train_data": _lib.TrainData, "dpt_adamw_args": _lib.AdamWArgs}
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dpt_hip.h"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                              text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[f"{cname} size"]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname} {fname}"]) == getattr(cls, fname).offset, (cname, fname)


def test_host_validation_without_a_device():
    """Every check fails on the host before any launch: the pointers below are host memory that a
    kernel would fault on, and no device is needed to get the reference's exception types."""
    from dpt_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    null = ctypes.c_void_p(None)
    H = 7
    d = _lib.TrainDesc(2, 32, 1, 5, 4 * (1 + H), 8, 1 + H, 0, 0.0, 0, 0)
    data = _lib.TrainData(20, H, 0, *([p.value] * 6))
    opt = _lib.AdamWArgs(1e-3, 0.9, 0.999, 1e-8, 1e-4, 1)
    n = ctypes.c_int64()

    def rc(name, *args):
        return lambda: _lib.check(getattr(lib, name)(*args))

    bad_step = _lib.AdamWArgs(1e-3, 0.9, 0.999, 1e-8, 1e-4, 0)
    wrong_window = _lib.TrainDesc(2, 32, 1, 5, 4 * (1 + H), 8, H, 0, 0.0, 0, 0)
    wide = _lib.TrainDesc(2, 32, 1, 33, 4 * (1 + H), 8, 1 + H, 0, 0.0, 0, 0)
    no_states = _lib.TrainData(20, H, 0, p.value, None, p.value, p.value, p.value, p.value)
    invalid = [
        rc("dpt_adamw_step", null, p, p, p, 16, ctypes.byref(opt), null),                    # null blob
        rc("dpt_adamw_step", p, p, p, p, 16, None, null),                                     # null args
        rc("dpt_adamw_step", p, p, p, p, 16, ctypes.byref(bad_step), null),                   # step < 1
        rc("dpt_adamw_step", p, p, p, p, -1, ctypes.byref(opt), null),                        # numel < 0
        rc("dpt_train_ce_loss", p, null, 2, 3, 5, p, p, p, null),                             # null targets
        rc("dpt_train_ce_loss", p, p, 2, 3, 5, p, p, null, null),                             # null accumulator
        rc("dpt_train_pack_batch", ctypes.byref(d), ctypes.byref(data), null, null, 4, p, p, null),
        rc("dpt_train_pack_batch", ctypes.byref(d), ctypes.byref(no_states), p, null, 4, p, p, null),
        rc("dpt_train_pack_batch", ctypes.byref(wrong_window), ctypes.byref(data), p, null, 4, p, p, null),
        rc("dpt_train_step", ctypes.byref(d), ctypes.byref(data), p, null, 4, p, p, p, ctypes.byref(opt), null, p,
           null),                                                                             # null workspace
        rc("dpt_train_step", ctypes.byref(d), ctypes.byref(data), p, null, 4, p, p, p, ctypes.byref(bad_step), p, p,
           null),
        rc("dpt_train_step", ctypes.byref(d), ctypes.byref(data), p, null, 9, p, p, p, ctypes.byref(opt), p, p,
           null),                                                                             # batch > desc.batch
        rc("dpt_train_step", ctypes.byref(wrong_window), ctypes.byref(data), p, null, 4, p, p, p, ctypes.byref(opt),
           p, p, null),
        rc("dpt_train_eval_loss", ctypes.byref(wrong_window), ctypes.byref(data), p, null, 4, p, p, p, null),
        rc("dpt_train_eval_loss", ctypes.byref(d), ctypes.byref(data), p, null, 4, null, p, p, null),
        rc("dpt_train_step_workspace_numel", ctypes.byref(d), None),
    ]
    for i, call in enumerate(invalid):
        with pytest.raises(ValueError):
            call()
        assert lib.dpt_last_error(), i
    with pytest.raises(ValueError, match="step"):
        invalid[2]()
    with pytest.raises(ValueError, match="window"):
        invalid[8]()
    unsupported = [
        rc("dpt_train_ce_loss", p, p, 2, 3, 33, p, p, p, null),
        rc("dpt_train_step", ctypes.byref(wide), ctypes.byref(data), p, null, 4, p, p, p, ctypes.byref(opt), p, p,
           null),
        rc("dpt_train_eval_loss", ctypes.byref(wide), ctypes.byref(data), p, null, 4, p, p, p, null),
    ]
    for call in unsupported:
        with pytest.raises(NotImplementedError, match="action_dim"):
            call()
    # the workspace covers the training workspace plus tokens, targets, preds, dpreds and dblob
    assert lib.dpt_train_step_workspace_numel(ctypes.byref(d), ctypes.byref(n)) == 0
    tw, nb = ctypes.c_int64(), ctypes.c_int64()
    assert lib.dpt_train_workspace_numel(ctypes.byref(d), ctypes.byref(tw)) == 0
    assert lib.dpt_train_blob_numel(ctypes.byref(d), ctypes.byref(nb)) == 0
    B, T, A, F = 8, 1 + H, 5, 8
    assert n.value >= tw.value + B * T * F + B * A + 2 * B * T * A + nb.value
    assert lib.dpt_adamw_step(p, p, p, p, 0, ctypes.byref(opt), null) == 0  # nothing to do, nothing launched


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_trainstep_has_no_short_hazard_paths(tmp_path):
    """scripts/isa_hazard_cfg.py on dpt_trainstep.hip, compiled as tests/test_isa_hazards.py compiles
    the other sources."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_hazard_cfg
    from test_isa_hazards import file_flags
    src = "dpt_trainstep.hip"
    out = tmp_path / (src + ".s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize",
                    "-I" + os.path.join(ROOT, "include"), *file_flags(src), "--cuda-device-only", "-S",
                    os.path.join(CSRC, src), "-o", str(out)], check=True, capture_output=True)
    isa_hazard_cfg.ALL_PRODUCERS = True
    assert isa_hazard_cfg.scan_all([str(out)]) == 0
    assert "dpt_trainstep.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_train_cli_argument_errors(tmp_path, monkeypatch):
    """train.py keeps the reference's guards: shuffling the linear bandit raises its exception and
    miniworld is not implemented; both before any dataset is read."""
    import importlib
    train = importlib.import_module("train")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(Exception, match="shuffle on the linear bandit"):
        train.main(["--env", "linear_bandit", "--shuffle"])
    with pytest.raises(NotImplementedError):
        train.main(["--env", "miniworld"])
