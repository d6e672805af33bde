"""CPU checks of the interactive DarkRoom training step (csrc/dpt_interactive_mdp.hip,
dpt_hip.train.InteractiveMDPTrainer, train_interactive_darkroom.py): the new C ABI entry points (symbols,
struct layout, host-side validation with no device present, the workspace size and the monotonicity the
one-workspace claim rests on), the float64 helper's env arithmetic against the committed exhaustive table,
the conditions on the records case's inputs, the machine code of the new source, and the script's flags.
No device work is launched."""
import ctypes
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import interactive_mdp_oracle as MO
from conftest import ROOT, golden
from test_isa_hazards import HIPCC, test_no_short_mfma_hazard_paths as hazard_scan
from test_resource_budget import remarks

CSRC = os.path.join(ROOT, "decision-pretrained-transformer_amd", "csrc")
NEW_SYMBOLS = ("dpt_mdp_pack", "dpt_darkroom_act_step", "dpt_interactive_mdp_workspace_numel",
               "dpt_interactive_mdp_grad")


def test_new_symbols_exported():
    from dpt_hip import _lib
    lib = _lib.load()
    assert lib.dpt_abi_version() == 8 == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    from dpt_hip import train as tr
    assert callable(tr.InteractiveMDPTrainer) and callable(tr.rollout_darkroom_interactive)
    assert (_lib.MDP_LOSS_NONE, _lib.MDP_LOSS_LAST, _lib.MDP_LOSS_EVERY) == (0, 1, 2)
    assert "dpt_interactive_mdp.hip" in open(os.path.join(CSRC, "Makefile")).read()
    # darkroom_move / darkroom_opt: one copy, in the shared header
    env, hdr = (open(os.path.join(CSRC, f)).read() for f in ("dpt_env.hip", "dpt_darkroom_env.h"))
    for fn in ("void darkroom_move(", "int darkroom_opt("):
        assert fn in hdr and fn not in env, fn


def test_mdp_struct_layout_matches_header(tmp_path):
    """dpt_interactive_mdp_args: ctypes against the C compiler's layout, field by field, in the issue's order"""
    from dpt_hip import _lib
    cls, cname = _lib.InteractiveMDPArgs, "dpt_interactive_mdp_args"
    assert [f for f, _ in cls._fields_] == [
        "N", "K", "dim", "loss_mode", "flags", "sample", "first_task", "scale", "seed", "counter", "goal", "perm",
        "uniforms", "states_out", "actions_out", "rewards_out", "targets_out", "workspace", "dblob", "loss_acc"]
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dpt_hip.h"', 'int main(void) {',
             f'printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                              text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname


def _args(_lib, p, **over):
    """dpt_interactive_mdp_args whose every pointer is the host buffer ``p`` (a kernel would fault on it)"""
    f = dict(N=4, K=3, dim=3, loss_mode=_lib.MDP_LOSS_EVERY, flags=0, sample=1, first_task=0, scale=0.25, seed=1,
             counter=0, goal=p.value, perm=None, uniforms=None, states_out=p.value, actions_out=p.value,
             rewards_out=p.value, targets_out=p.value, workspace=p.value, dblob=p.value, loss_acc=p.value)
    f.update(over)
    return _lib.InteractiveMDPArgs(*(f[name] for name, _ in _lib.InteractiveMDPArgs._fields_))


def test_host_validation_without_a_device():
    """Every check of dpt_interactive_mdp_grad (and of the two kernels' entry points and the workspace query)
    fails on the host before any launch: the pointers are host memory, and no device is needed to get the
    exception types."""
    from dpt_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base if base % 16 == 0 else base + 8)  # 16-byte aligned
    assert p.value % 16 == 0
    odd = ctypes.c_void_p(p.value + 4)
    null = ctypes.c_void_p(None)

    def desc(sd=2, A=5, npos=32, dropout=0.0):
        return _lib.TrainDesc(2, 32, sd, A, npos, 1, 1, 0, dropout, 0, 0)

    def grad(d, a, blob=p):
        return lambda: _lib.check(lib.dpt_interactive_mdp_grad(ctypes.byref(d) if d is not None else None, blob,
                                                               ctypes.byref(a) if a is not None else None, null))

    def act(**over):
        f = dict(logits=p, N=4, window=2, K=3, t=1, dim=3, sample=1, uniforms=null, seed=1, counter=0, first_task=0,
                 goal=p, perm=null, states=p, actions=p, rewards=p, targets=p, target_next=null)
        f.update(over)
        return lambda: _lib.check(lib.dpt_darkroom_act_step(*f.values(), null))

    d = desc()
    n = ctypes.c_int64()
    invalid = {
        "null desc": grad(None, _args(_lib, p)),
        "null blob": grad(d, _args(_lib, p), blob=null),
        "null args": grad(d, None),
        "null goal": grad(d, _args(_lib, p, goal=None)),
        "null states_out": grad(d, _args(_lib, p, states_out=None)),
        "null actions_out": grad(d, _args(_lib, p, actions_out=None)),
        "null rewards_out": grad(d, _args(_lib, p, rewards_out=None)),
        "null targets_out": grad(d, _args(_lib, p, targets_out=None)),
        "null workspace": grad(d, _args(_lib, p, workspace=None)),
        "null dblob (every)": grad(d, _args(_lib, p, dblob=None)),
        "null loss (last)": grad(d, _args(_lib, p, loss_mode=_lib.MDP_LOSS_LAST, loss_acc=None)),
        "N < 1": grad(d, _args(_lib, p, N=0)),
        "K < 1": grad(d, _args(_lib, p, K=0)),
        "K > n_positions": grad(desc(npos=5), _args(_lib, p, K=6)),
        "row cap": grad(desc(npos=1 << 20), _args(_lib, p, N=1 << 10, K=(1 << 16) + 1)),
        "dim < 1": grad(d, _args(_lib, p, dim=0)),
        "dropout": grad(desc(dropout=0.1), _args(_lib, p)),
        "loss mode": grad(d, _args(_lib, p, loss_mode=3)),
        "negative loss mode": grad(d, _args(_lib, p, loss_mode=-1)),
        "unknown flags": grad(d, _args(_lib, p, flags=2)),
        "misaligned": grad(d, _args(_lib, p, workspace=odd.value)),
        "pack null tokens": lambda: _lib.check(lib.dpt_mdp_pack(p, p, p, 3, 4, 2, null, null)),
        "pack null states": lambda: _lib.check(lib.dpt_mdp_pack(null, p, p, 3, 4, 2, p, null)),
        "pack null records": lambda: _lib.check(lib.dpt_mdp_pack(p, null, p, 3, 4, 2, p, null)),
        "pack t >= K": lambda: _lib.check(lib.dpt_mdp_pack(p, p, p, 3, 4, 4, p, null)),
        "pack t < 0": lambda: _lib.check(lib.dpt_mdp_pack(p, p, p, 3, 4, -1, p, null)),
        "act null logits": act(logits=null),
        "act null goal": act(goal=null),
        "act null targets": act(targets=null),
        "act t = K - 1": act(t=2),
        "act t < 0": act(t=-1),
        "act dim < 1": act(dim=0),
        "act window < 1": act(window=0),
        "act N < 1": act(N=0),
        "workspace null numel": lambda: _lib.check(lib.dpt_interactive_mdp_workspace_numel(ctypes.byref(d), 4, 3, 2,
                                                                                          None)),
        "workspace loss mode": lambda: _lib.check(lib.dpt_interactive_mdp_workspace_numel(ctypes.byref(d), 4, 3, 7,
                                                                                         ctypes.byref(n))),
    }
    for name, call in invalid.items():
        with pytest.raises(ValueError):
            call()
        assert lib.dpt_last_error(), name
    for name, word in (("K > n_positions", "n_positions"), ("dropout", "dropout"), ("misaligned", "aligned"),
                       ("row cap", "smaller chunks"), ("loss mode", "loss mode"), ("unknown flags", "flags"),
                       ("dim < 1", "dim"), ("null dblob (every)", "loss mode")):
        with pytest.raises(ValueError, match=word):
            invalid[name]()
    unsupported = [
        grad(desc(sd=1), _args(_lib, p)),
        grad(desc(A=4), _args(_lib, p)),
        lambda: _lib.check(lib.dpt_interactive_mdp_workspace_numel(ctypes.byref(desc(sd=1)), 4, 3, 2, ctypes.byref(n))),
    ]
    for call in unsupported:
        with pytest.raises(NotImplementedError, match="state_dim"):
            call()
    # the rollout alone needs neither a gradient blob nor a loss accumulator: with both NULL every host check
    # passes up to the first pointer the chain would use, which is never reached here (N = 0 stops it)
    with pytest.raises(ValueError, match="N=0"):
        grad(d, _args(_lib, p, N=0, loss_mode=_lib.MDP_LOSS_NONE, dblob=None, loss_acc=None))()


@pytest.mark.parametrize("E", [32, 18])
def test_workspace_covers_its_parts_and_every_shorter_window(E):
    """The workspace query is at least the sum of its parts in each loss mode, and
    dpt_train_workspace_numel does not decrease with the window over 1..K in either form the chain runs
    (the last-position training forward and the last-position inference forward): one workspace sized for
    window K serves every shorter window."""
    from dpt_hip import _lib
    lib = _lib.load()
    npos = 4 * (1 + 66)
    d = _lib.TrainDesc(2, E, 2, 5, npos, 1, 1, 0, 0.0, 0, 0)

    def numel(N, K, mode):
        n = ctypes.c_int64()
        assert lib.dpt_interactive_mdp_workspace_numel(ctypes.byref(d), N, K, mode, ctypes.byref(n)) == 0
        return n.value

    def train_ws(N, T, flags):
        run = _lib.TrainDesc(2, E, 2, 5, npos, N, T, flags, 0.0, 0, 0)
        n = ctypes.c_int64()
        assert lib.dpt_train_workspace_numel(ctypes.byref(run), ctypes.byref(n)) == 0
        return n.value

    fwd, fit = _lib.TRAIN_FORWARD_ONLY | _lib.TRAIN_LAST_ONLY, _lib.TRAIN_LAST_LOSS
    nb = ctypes.c_int64()
    assert lib.dpt_train_blob_numel(ctypes.byref(d), ctypes.byref(nb)) == 0
    for N, K in ((7, 6), (3, 66), (8, 1), (8, 2), (1024, 25)):
        for flags in (fwd, fit):
            sizes = [train_ws(N, T, flags) for T in range(1, K + 1)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (N, K, flags)
        rows = N * K * 10 + N * K * 5 + 2 * N  # tokens, logits, the int64 targets of the step
        none, last, every = (numel(N, K, m) for m in (_lib.MDP_LOSS_NONE, _lib.MDP_LOSS_LAST, _lib.MDP_LOSS_EVERY))
        assert none >= train_ws(N, K, fwd) + rows
        loss_rows = N * K * 5 + nb.value + 2 * N  # dpreds, the chunk's gradient, the per-env losses
        assert last >= max(train_ws(N, K, fwd), train_ws(N, K, fit)) + rows + loss_rows
        assert every >= max(train_ws(N, K, fwd), train_ws(N, K, fit)) + rows + loss_rows + nb.value
        assert none < last < every
    assert numel(8, 6, 2) < numel(9, 6, 2) < numel(16, 6, 2)
    assert numel(8, 1, 2) < numel(8, 2, 2) < numel(8, 6, 2) < numel(8, 12, 2)


def test_helper_env_arithmetic_reproduces_the_exhaustive_table():
    """interactive_mdp_oracle.transit / opt_action against tests/golden/darkroom_transit.npz: every state x
    action x goal of the 10 x 10 room, and the 120 action permutations with the goal at (9, 9)."""
    g = golden("darkroom_transit.npz")
    st = g["states"]
    for gi in range(100):
        goal = np.broadcast_to(st[gi], st.shape)
        assert np.array_equal(MO.opt_action(st, goal), g["opt_action"][gi])
        for a in range(5):
            ns, r = MO.transit(st, np.full(100, a), goal, 10)
            assert np.array_equal(ns, g["next_state"][gi, a]) and np.array_equal(r, g["reward"][gi, a])
    goal = np.full((100, 2), 9)
    for pi in range(120):
        perm = np.broadcast_to(g["perms"][pi], (100, 5))
        assert np.array_equal(MO.opt_action(st, goal, perm), g["perm_opt_action"][pi])
        for a in range(5):
            ns, r = MO.transit(st, np.full(100, a), goal, 10, perm)
            assert np.array_equal(ns, g["perm_next_state"][pi, a]) and np.array_equal(r, g["perm_reward"][pi, a])


def test_helper_window_and_selection_on_hand_cases():
    states = np.array([[[0, 0], [1, 0], [1, 1]]])
    actions, rewards = np.array([[0, 7]]), np.array([[0, 1]])
    w = MO.window(states, actions, rewards, 2).numpy()
    assert w.tolist() == [[[1, 1, 0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0, 1, 0, 0],
                           [1, 0, 0, 0, 0, 0, 0, 1, 1, 1]]]  # the out-of-range action packs a zero one-hot
    assert MO.window(states, actions, rewards, 0).numpy().tolist() == [[[0] * 10]]
    lg = np.log(np.array([[0.1, 0.2, 0.3, 0.25, 0.15]]))
    for u, want in ((0.05, 0), (0.1 + 1e-9, 1), (0.59, 2), (0.61, 3), (0.999, 4)):
        a, margin = MO.select(lg, True, [u])
        assert a.tolist() == [want] and margin[0] > 0
    a, margin = MO.select(np.array([[1.0, 3.0, 3.0, 0.0, 2.0]]), False, None)
    assert a.tolist() == [1] and margin[0] == 0.0


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("E", [32, 18])
def test_records_case_inputs_are_clear_of_near_ties(E, permuted):
    """The conditions on the inputs of the GPU records test, checked without a GPU: every draw of the float64
    oracle's episode has a cdf margin above 1e-5 (fp32 logits within 1e-5 cannot move a draw), and the
    oracle's records hold at least one reward 1 and at least one clipped move."""
    _, _, u, perm, ep = MO.records_case(E, permuted)
    assert MO.REC_GOALS.tolist()[:3] == [[0, 0], [0, 1], [2, 2]] and MO.REC_GOALS.shape == (MO.REC_N, 2)
    assert ep["margins"].shape == (MO.REC_K - 1, MO.REC_N) and ep["margins"].min() > 1e-5, ep["margins"].min()
    assert (ep["rewards"] == 1).any()
    moved = ep["actions"] if perm is None else perm[np.arange(MO.REC_N)[:, None], ep["actions"]]
    clipped = (moved != 4) & (ep["states"][:, 1:] == ep["states"][:, :-1]).all(-1)
    assert clipped.any()
    assert (ep["targets"] == np.stack([MO.opt_action(ep["states"][:, t], MO.REC_GOALS, perm)
                                       for t in range(MO.REC_K)], 1)).all()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mdp_source_passes_the_hazard_scan(tmp_path):
    hazard_scan("dpt_interactive_mdp.hip", tmp_path)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mdp_kernels_use_no_scratch(tmp_path):
    """the pack, reset and act kernels: element-wise, no scratch"""
    r = remarks("dpt_interactive_mdp.hip", tmp_path)
    names = [n for n in r if "mdp_pack_kernel" in n or "mdp_reset_kernel" in n or "mdp_act_kernel" in n]
    assert len(names) == 3, list(r)
    for n in names:
        assert r[n]["scratch"] == 0 and r[n]["occ"] >= 4, (n, r[n])
    src = open(os.path.join(CSRC, "dpt_interactive_mdp.hip")).read()
    assert "__shared__" not in src and "hipMalloc" not in src and "hipStreamCreate" not in src


def test_script_rejects_other_envs_and_parses_its_flags(tmp_path, monkeypatch):
    """train_interactive_darkroom.py: common_args plus --seed, --K, --episodes_per_epoch, --chunk, --loss and
    --n_eval; only --env darkroom, refused before any device work; the checkpoint name."""
    ti = importlib.import_module("train_interactive_darkroom")
    monkeypatch.chdir(tmp_path)
    for env in ("bandit", "bandit_thompson", "miniworld"):
        with pytest.raises(ValueError, match="darkroom only"):
            ti.main(["--env", env])
    assert not os.path.exists("trained_models")
    a = ti.parse_args(["--env", "darkroom"])
    assert (a["seed"], a["K"], a["episodes_per_epoch"], a["chunk"], a["loss"], a["n_eval"]) == (0, -1, 1000, 0, "every",
                                                                                               100)
    assert (a["H"], a["dim"], a["embd"], a["layer"], a["lr"], a["dropout"]) == (100, 10, 32, 3, 1e-3, 0)
    a = ti.parse_args(["--env", "darkroom", "--seed", "3", "--K", "12", "--episodes_per_epoch", "5", "--chunk", "64",
                       "--loss", "last", "--n_eval", "8", "--envs", "16", "--dim", "4", "--embd", "16"])
    assert (a["seed"], a["K"], a["episodes_per_epoch"], a["chunk"], a["loss"], a["n_eval"]) == (3, 12, 5, 64, "last", 8)
    with pytest.raises(SystemExit):
        ti.parse_args(["--env", "darkroom", "--loss", "sum"])
    text = open(os.path.join(ROOT, "decision-pretrained-transformer_amd", "train_interactive_darkroom.py")).read()
    assert "trained_models/interactive_darkroom.pt" in text
    # the bandit script is untouched and keeps its guard
    with pytest.raises(ValueError, match="bandit envs only"):
        importlib.import_module("train_interactive").main(["--env", "darkroom"])
