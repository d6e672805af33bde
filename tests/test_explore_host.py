"""CPU checks of the explorer/exploiter training step: the new C ABI entry points (symbols, struct
layout, host-side validation with no device present, the workspace size), the ISA hazard scan of the
new source and train_explorer_exploiter.py's argument errors.  No device work is launched."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "decision-pretrained-transformer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NEW_SYMBOLS = ("dpt_rollout_bandit_generic_env", "dpt_train_ce_rows", "dpt_explore_weights",
               "dpt_explore_workspace_numel", "dpt_explore_grad")


def test_new_symbols_exported():
    from dpt_hip import _lib
    lib = _lib.load()
    assert lib.dpt_abi_version() == 8 == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.STREAM_ENVACT not in (_lib.STREAM_SELECT, _lib.STREAM_REWARD, _lib.STREAM_ROLLIN,
                                      _lib.STREAM_DROPOUT) and _lib.STREAM_ENVACT < _lib.STREAM_POLICY


def test_explore_struct_layout_matches_header(tmp_path):
    """dpt_explore_args: ctypes against the C compiler's layout, field by field; the public rollout
    args keep their layout (the env action travels outside them)."""
    from dpt_hip import _lib
    structs = {"dpt_explore_args": _lib.ExploreArgs, "dpt_bandit_rollout_args": _lib.BanditRolloutArgs}
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
    assert ctypes.sizeof(_lib.BanditRolloutArgs) == 120


def _args(_lib, p, q, **over):
    """dpt_explore_args whose every pointer is a host buffer (a kernel would fault on it)"""
    f = dict(N=4, K=3, type=0, flags=0, first_task=0, var=0.3, beta=1.0, scale_exploiter=1 / 12, scale_explorer=1 / 8,
             seed=1, counter=0, means=p.value, targets=p.value, uniforms=None, noise=None, env_actions=None,
             actions_out=p.value, env_actions_out=p.value, rewards_out=p.value, workspace=p.value,
             dblob_explorer=p.value, dblob_exploiter=q.value, loss_explorer=p.value, loss_exploiter=q.value)
    f.update(over)
    return _lib.ExploreArgs(*(f[name] for name, _ in _lib.ExploreArgs._fields_))


def test_host_validation_without_a_device():
    """Every check of dpt_explore_grad (and of the new kernels' entry points) fails on the host before
    any launch: the pointers are host memory, and no device is needed to get the exception types."""
    from dpt_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    assert base % 16 == 0 or (base + 8) % 16 == 0
    p = ctypes.c_void_p(base if base % 16 == 0 else base + 8)  # 16-byte aligned
    q = ctypes.c_void_p(p.value + 64)
    odd = ctypes.c_void_p(p.value + 4)
    null = ctypes.c_void_p(None)
    H = 7

    def desc(sd=1, A=5, npos=4 * (1 + H), dropout=0.0):
        return _lib.TrainDesc(2, 32, sd, A, npos, 1, 1, 0, dropout, 0, 0)

    def grad(d, a, explorer=p, exploiter=q):
        return lambda: _lib.check(lib.dpt_explore_grad(ctypes.byref(d) if d is not None else None, explorer,
                                                       exploiter, ctypes.byref(a) if a is not None else None, null))

    def A_(**over):
        return _args(_lib, p, q, **over)

    d = desc()
    n = ctypes.c_int64()
    invalid = {
        "null desc": grad(None, A_()),
        "null explorer": grad(d, A_(), explorer=null),
        "null exploiter": grad(d, A_(), exploiter=null),
        "equal blobs": grad(d, A_(), explorer=p, exploiter=p),
        "null args": grad(d, None),
        "null means": grad(d, A_(means=None)),
        "null targets": grad(d, A_(targets=None)),
        "null workspace": grad(d, A_(workspace=None)),
        "null dblob explorer": grad(d, A_(dblob_explorer=None)),
        "null dblob exploiter": grad(d, A_(dblob_exploiter=None)),
        "equal dblobs": grad(d, A_(dblob_exploiter=p.value)),
        "null loss explorer": grad(d, A_(loss_explorer=None)),
        "null loss exploiter": grad(d, A_(loss_exploiter=None)),
        "null actions_out": grad(d, A_(actions_out=None)),
        "null env_actions_out": grad(d, A_(env_actions_out=None)),
        "null rewards_out": grad(d, A_(rewards_out=None)),
        "N < 1": grad(d, A_(N=0)),
        "K = 1": grad(d, A_(K=1)),
        "K = 0": grad(d, A_(K=0)),
        "K > n_positions": grad(desc(npos=5), A_(K=6)),
        "beta 0": grad(d, A_(beta=0.0)),
        "beta negative": grad(d, A_(beta=-1.0)),
        "beta nan": grad(d, A_(beta=float("nan"))),
        "beta inf": grad(d, A_(beta=float("inf"))),
        "state_dim": grad(desc(sd=2), A_()),
        "dropout": grad(desc(dropout=0.1), A_()),
        "misaligned": grad(d, A_(workspace=odd.value)),
        "unknown flags": grad(d, A_(flags=2)),
        "bandit type": grad(d, A_(type=2)),
        "ce no targets": lambda: _lib.check(lib.dpt_train_ce_rows(p, null, null, null, 2, 3, 5, 0.5, p, p, p, null)),
        "ce both targets": lambda: _lib.check(lib.dpt_train_ce_rows(p, p, p, null, 2, 3, 5, 0.5, p, p, p, null)),
        "ce null rowloss": lambda: _lib.check(lib.dpt_train_ce_rows(p, p, null, null, 2, 3, 5, 0.5, null, p, p, null)),
        "ce null accumulator": lambda: _lib.check(lib.dpt_train_ce_rows(p, p, null, null, 2, 3, 5, 0.5, p, p, null,
                                                                        null)),
        "ce batch < 1": lambda: _lib.check(lib.dpt_train_ce_rows(p, p, null, null, 0, 3, 5, 0.5, p, p, p, null)),
        "weights null": lambda: _lib.check(lib.dpt_explore_weights(p, 2, 3, 1.0, null, null)),
        "weights batch < 1": lambda: _lib.check(lib.dpt_explore_weights(p, 0, 3, 1.0, p, null)),
        "weights inv_beta": lambda: _lib.check(lib.dpt_explore_weights(p, 2, 3, float("inf"), p, null)),
        "workspace null numel": lambda: _lib.check(lib.dpt_explore_workspace_numel(ctypes.byref(d), 4, 3, None)),
        "workspace K = 1": lambda: _lib.check(lib.dpt_explore_workspace_numel(ctypes.byref(d), 4, 1, ctypes.byref(n))),
    }
    for name, call in invalid.items():
        with pytest.raises(ValueError):
            call()
        assert lib.dpt_last_error(), name
    for name, word in (("K = 1", "at least 2"),("beta 0", "beta"), ("beta nan", "beta"), ("beta negative", "beta"),
                       ("K > n_positions", "n_positions"), ("state_dim", "state_dim"), ("dropout", "dropout"),
                       ("misaligned", "aligned"), ("equal blobs", "share one blob")):
        with pytest.raises(ValueError, match=word):
            invalid[name]()
    unsupported = [
        grad(desc(A=33), A_()),
        lambda: _lib.check(lib.dpt_train_ce_rows(p, p, null, null, 2, 3, 33, 0.5, p, p, p, null)),
        lambda: _lib.check(lib.dpt_explore_workspace_numel(ctypes.byref(desc(A=33)), 4, 3, ctypes.byref(n))),
    ]
    for call in unsupported:
        with pytest.raises(NotImplementedError, match="action_dim"):
            call()
    # the rollout entry with the env action apart: same host checks as dpt_rollout_bandit_generic
    with pytest.raises(ValueError):
        _lib.check(lib.dpt_rollout_bandit_generic_env(ctypes.byref(d), null, None, null, 1, null, null))
    r = _lib.BanditRolloutArgs(N=4, H=3, A=5)
    with pytest.raises(ValueError, match="random_env"):
        _lib.check(lib.dpt_rollout_bandit_generic_env(ctypes.byref(d), p, ctypes.byref(r), null, 2, null, null))
    with pytest.raises(ValueError):  # null means / kvcache / outputs
        _lib.check(lib.dpt_rollout_bandit_generic_env(ctypes.byref(d), p, ctypes.byref(r), null, 1, null, null))


def test_workspace_grows_and_covers_both_passes():
    from dpt_hip import _lib
    lib = _lib.load()
    H = 11
    d = _lib.TrainDesc(2, 32, 1, 5, 4 * (1 + H), 1, 1, 0, 0.0, 0, 0)

    def numel(N, K):
        n = ctypes.c_int64()
        assert lib.dpt_explore_workspace_numel(ctypes.byref(d), N, K, ctypes.byref(n)) == 0
        return n.value

    assert numel(8, 6) < numel(9, 6) < numel(16, 6)
    assert numel(8, 2) < numel(8, 3) < numel(8, 6) < numel(8, 12)
    for N, K in ((8, 6), (3, 2), (37, 12)):
        run = _lib.TrainDesc(2, 32, 1, 5, 4 * (1 + H), N, K, 0, 0.0, 0, 0)
        tw, nb, roll, ia = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        assert lib.dpt_train_workspace_numel(ctypes.byref(run), ctypes.byref(tw)) == 0
        assert lib.dpt_train_blob_numel(ctypes.byref(run), ctypes.byref(nb)) == 0
        assert lib.dpt_rollout_bandit_generic_workspace_numel(ctypes.byref(run), N, K - 1, ctypes.byref(roll)) == 0
        assert lib.dpt_interactive_workspace_numel(ctypes.byref(d), N, K, ctypes.byref(ia)) == 0
        # the training workspace, tokens, preds, dpreds, a gradient blob, the rollout's workspace and arm values;
        # on top: row losses and weights (doubles) and the row targets
        base = tw.value + N * K * 8 + 2 * N * K * 5 + nb.value + roll.value + 2 * N * (K - 1)
        assert numel(N, K) >= base + 5 * N * K
        # ONE shared training workspace / token buffer / preds pair: far less than two interactive workspaces
        assert numel(N, K) < ia.value + 5 * N * K + 64


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_explore_has_no_short_hazard_paths(tmp_path):
    """scripts/isa_hazard_cfg.py on dpt_explore.hip, compiled as tests/test_isa_hazards.py compiles
    the other sources; the source is in the Makefile's list (so the source hash covers it)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_hazard_cfg
    from test_isa_hazards import file_flags
    src = "dpt_explore.hip"
    out = tmp_path / (src + ".s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize",
                    "-I" + os.path.join(ROOT, "include"), *file_flags(src), "--cuda-device-only", "-S",
                    os.path.join(CSRC, src), "-o", str(out)], check=True, capture_output=True)
    isa_hazard_cfg.ALL_PRODUCERS = True
    assert isa_hazard_cfg.scan_all([str(out)]) == 0
    assert "dpt_explore.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_train_explorer_exploiter_rejects_other_envs_and_k1(tmp_path, monkeypatch):
    """train_explorer_exploiter.py keeps the reference's guard (only the bandit envs) and names the
    reason for K = 1, both before any device work; wandb is never imported."""
    import importlib
    te = importlib.import_module("train_explorer_exploiter")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="bandit envs only"):
        te.main(["--env", "darkroom"])
    with pytest.raises(ValueError, match="Unsupported env"):
        te.build_bandit_env(5, 4, 3, 0.3, "darkroom")
    with pytest.raises(ValueError, match="K - 1 positions"):
        te.main(["--env", "bandit", "--K", "1"])
    assert "wandb" not in sys.modules
    assert "import wandb" not in open(te.__file__).read()
