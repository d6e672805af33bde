"""CPU checks of the interactive training step: the new C ABI entry points (symbols, struct layout,
host-side validation with no device present, the workspace size), the ISA hazard scan of the new
source, the chunk splitter and train_interactive.py's argument errors.  No device work is launched."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "decision-pretrained-transformer_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NEW_SYMBOLS = ("dpt_interactive_pack", "dpt_train_ce_last", "dpt_interactive_workspace_numel",
               "dpt_interactive_grad")


def test_new_symbols_exported():
    from dpt_hip import _lib
    lib = _lib.load()
    assert lib.dpt_abi_version() == 8 == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name


def test_interactive_struct_layout_matches_header(tmp_path):
    """dpt_interactive_args: ctypes against the C compiler's layout, field by field."""
    from dpt_hip import _lib
    structs = {"dpt_interactive_args": _lib.InteractiveArgs}
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


def _args(_lib, p, **over):
    """dpt_interactive_args whose every pointer is the host buffer ``p`` (a kernel would fault on it)"""
    f = dict(N=4, K=3, type=0, flags=0, first_task=0, var=0.3, scale=0.25, seed=1, counter=0, means=p.value,
             targets=p.value, uniforms=None, noise=None, actions_out=p.value, rewards_out=p.value,
             workspace=p.value, dblob=p.value, loss_acc=p.value)
    f.update(over)
    return _lib.InteractiveArgs(*(f[name] for name, _ in _lib.InteractiveArgs._fields_))


def test_host_validation_without_a_device():
    """Every check of dpt_interactive_grad (and of the two kernels' entry points) fails on the host
    before any launch: the pointers are host memory, and no device is needed to get the exception
    types."""
    from dpt_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    assert base % 16 == 0 or (base + 8) % 16 == 0
    p = ctypes.c_void_p(base if base % 16 == 0 else base + 8)  # 16-byte aligned
    odd = ctypes.c_void_p(p.value + 4)
    null = ctypes.c_void_p(None)
    H = 7

    def desc(sd=1, A=5, npos=4 * (1 + H), dropout=0.0):
        return _lib.TrainDesc(2, 32, sd, A, npos, 1, 1, 0, dropout, 0, 0)

    def grad(d, a, blob=p):
        return lambda: _lib.check(lib.dpt_interactive_grad(ctypes.byref(d) if d is not None else None, blob,
                                                           ctypes.byref(a) if a is not None else None, null))

    d = desc()
    invalid = {
        "null desc": grad(None, _args(_lib, p)),
        "null blob": grad(d, _args(_lib, p), blob=null),
        "null args": grad(d, None),
        "null means": grad(d, _args(_lib, p, means=None)),
        "null targets": grad(d, _args(_lib, p, targets=None)),
        "null workspace": grad(d, _args(_lib, p, workspace=None)),
        "null dblob": grad(d, _args(_lib, p, dblob=None)),
        "null loss": grad(d, _args(_lib, p, loss_acc=None)),
        "null actions_out": grad(d, _args(_lib, p, actions_out=None)),
        "null rewards_out": grad(d, _args(_lib, p, rewards_out=None)),
        "N < 1": grad(d, _args(_lib, p, N=0)),
        "K < 1": grad(d, _args(_lib, p, K=0)),
        "K > n_positions": grad(desc(npos=5), _args(_lib, p, K=6)),
        "state_dim": grad(desc(sd=2), _args(_lib, p)),
        "dropout": grad(desc(dropout=0.1), _args(_lib, p)),
        "misaligned": grad(d, _args(_lib, p, workspace=odd.value)),
        "unknown flags": grad(d, _args(_lib, p, flags=4)),
        "pack null tokens": lambda: _lib.check(lib.dpt_interactive_pack(p, p, 3, 2, 5, null, null)),
        "pack null records": lambda: _lib.check(lib.dpt_interactive_pack(null, p, 3, 2, 5, p, null)),
        "pack Hc < 0": lambda: _lib.check(lib.dpt_interactive_pack(p, p, 3, -1, 5, p, null)),
        "ce null targets": lambda: _lib.check(lib.dpt_train_ce_last(p, null, 2, 3, 5, 0.5, p, p, p, null)),
        "ce null accumulator": lambda: _lib.check(lib.dpt_train_ce_last(p, p, 2, 3, 5, 0.5, p, p, null, null)),
        "ce batch < 1": lambda: _lib.check(lib.dpt_train_ce_last(p, p, 0, 3, 5, 0.5, p, p, p, null)),
        "workspace null numel": lambda: _lib.check(lib.dpt_interactive_workspace_numel(ctypes.byref(d), 4, 3, None)),
    }
    for name, call in invalid.items():
        with pytest.raises(ValueError):
            call()
        assert lib.dpt_last_error(), name
    for name, word in (("K > n_positions", "n_positions"), ("state_dim", "state_dim"), ("dropout", "dropout"),
                       ("misaligned", "aligned")):
        with pytest.raises(ValueError, match=word):
            invalid[name]()
    n = ctypes.c_int64()
    unsupported = [
        grad(desc(A=33), _args(_lib, p)),
        lambda: _lib.check(lib.dpt_train_ce_last(p, p, 2, 3, 33, 0.5, p, p, p, null)),
        lambda: _lib.check(lib.dpt_interactive_workspace_numel(ctypes.byref(desc(A=33)), 4, 3, ctypes.byref(n))),
    ]
    for call in unsupported:
        with pytest.raises(NotImplementedError, match="action_dim"):
            call()


def test_workspace_grows_and_covers_the_training_step():
    from dpt_hip import _lib
    lib = _lib.load()
    H = 11
    d = _lib.TrainDesc(2, 32, 1, 5, 4 * (1 + H), 1, 1, 0, 0.0, 0, 0)

    def numel(N, K):
        n = ctypes.c_int64()
        assert lib.dpt_interactive_workspace_numel(ctypes.byref(d), N, K, ctypes.byref(n)) == 0
        return n.value

    assert numel(8, 6) < numel(9, 6) < numel(16, 6)
    assert numel(8, 1) < numel(8, 2) < numel(8, 6) < numel(8, 12)
    for N, K in ((8, 6), (3, 2), (37, 12)):
        run = _lib.TrainDesc(2, 32, 1, 5, 4 * (1 + H), N, K, 0, 0.0, 0, 0)
        step, tw, nb, roll = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        assert lib.dpt_train_step_workspace_numel(ctypes.byref(run), ctypes.byref(step)) == 0
        assert lib.dpt_train_workspace_numel(ctypes.byref(run), ctypes.byref(tw)) == 0
        assert lib.dpt_train_blob_numel(ctypes.byref(run), ctypes.byref(nb)) == 0
        assert lib.dpt_rollout_bandit_generic_workspace_numel(ctypes.byref(run), N, K - 1, ctypes.byref(roll)) == 0
        assert numel(N, K) >= step.value
        # the training workspace, tokens, preds, dpreds, a gradient blob, the rollout's workspace and arm values
        assert numel(N, K) >= tw.value + N * K * 8 + 2 * N * K * 5 + nb.value + roll.value + 2 * N * (K - 1)


def test_chunk_plan():
    from dpt_hip.train import chunk_plan
    assert chunk_plan(8, 3) == [(0, 3), (3, 3), (6, 2)]
    assert chunk_plan(8, 0) == [(0, 8)]
    assert chunk_plan(8, 8) == [(0, 8)] and chunk_plan(8, 100) == [(0, 8)]
    assert chunk_plan(9, 3) == [(0, 3), (3, 3), (6, 3)]
    assert chunk_plan(1, 1) == [(0, 1)]
    with pytest.raises(ValueError):
        chunk_plan(0, 3)
    with pytest.raises(ValueError):
        chunk_plan(8, -1)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_interactive_has_no_short_hazard_paths(tmp_path):
    """scripts/isa_hazard_cfg.py on dpt_interactive.hip, compiled as tests/test_isa_hazards.py
    compiles the other sources; the source is in the Makefile's list."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_hazard_cfg
    from test_isa_hazards import file_flags
    src = "dpt_interactive.hip"
    out = tmp_path / (src + ".s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize",
                    "-I" + os.path.join(ROOT, "include"), *file_flags(src), "--cuda-device-only", "-S",
                    os.path.join(CSRC, src), "-o", str(out)], check=True, capture_output=True)
    isa_hazard_cfg.ALL_PRODUCERS = True
    assert isa_hazard_cfg.scan_all([str(out)]) == 0
    assert "dpt_interactive.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_train_interactive_rejects_other_envs(tmp_path, monkeypatch):
    """train_interactive.py keeps the reference's guard: only the bandit envs, before any device work."""
    import importlib
    ti = importlib.import_module("train_interactive")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="bandit envs only"):
        ti.main(["--env", "darkroom"])
    with pytest.raises(ValueError, match="Unsupported env"):
        ti.build_bandit_env(5, 4, 3, 0.3, "darkroom")
