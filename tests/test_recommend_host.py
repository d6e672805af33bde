"""CPU checks of the explore-then-exploit evaluation (csrc/dpt_recommend.hip, dpt_hip.recommend_curve /
empirical_recommend, dpt_hip.train.exploit_curve, evals/eval_explore_exploit.py): the new C ABI entry
points (symbols, struct layout, host-side validation with no device present, the workspace size), the
machine code of the new source, the numpy restatements against the committed reference fixture, and the
evaluation script's flags.  No device work is launched."""
import ctypes
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import recommend_oracle as RO
from conftest import ROOT, golden
from test_isa_hazards import HIPCC, test_no_short_mfma_hazard_paths as hazard_scan
from test_resource_budget import remarks

CSRC = os.path.join(ROOT, "decision-pretrained-transformer_amd", "csrc")
NEW_SYMBOLS = ("dpt_recommend_curve", "dpt_empirical_recommend", "dpt_exploit_eval_workspace_numel",
               "dpt_exploit_eval")
EMP_CASES = {"gauss5": (7, 40, 5), "gauss17": (3, 70, 17), "bern3": (7, 40, 3)}


def test_new_symbols_exported():
    from dpt_hip import _lib
    lib = _lib.load()
    assert lib.dpt_abi_version() == 8 == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    import dpt_hip
    from dpt_hip import train as tr
    assert callable(dpt_hip.recommend_curve) and callable(dpt_hip.empirical_recommend)
    assert callable(tr.exploit_curve) and callable(tr.ExploreExploitTrainer.exploit_curve)
    assert "dpt_recommend.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_exploit_eval_struct_layout_matches_header(tmp_path):
    """dpt_exploit_eval_args: ctypes against the C compiler's layout, field by field"""
    from dpt_hip import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    cname, cls = "dpt_exploit_eval_args", _lib.ExploitEvalArgs
    assert [f for f, _ in cls._fields_] == ["N", "H", "flags", "reserved", "actions", "rewards", "means", "targets",
                                           "workspace", "logits_out", "greedy_arm", "greedy_value", "expected_value",
                                           "p_opt"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dpt_hip.h"', 'int main(void) {',
             f'printf("size %zu\\n", sizeof({cname}));']
    lines += [f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));' for fname, _ in cls._fields_]
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                              text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls) == 96
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname


def _args(_lib, p, **over):
    """dpt_exploit_eval_args whose every pointer is a host buffer (a kernel would fault on it)"""
    f = dict(N=4, H=3, flags=0, reserved=0, actions=p.value, rewards=p.value, means=p.value, targets=p.value,
             workspace=p.value, logits_out=None, greedy_arm=p.value, greedy_value=p.value, expected_value=p.value,
             p_opt=p.value)
    f.update(over)
    return _lib.ExploitEvalArgs(*(f[name] for name, _ in _lib.ExploitEvalArgs._fields_))


def test_host_validation_without_a_device():
    """Every check of dpt_exploit_eval and of the two kernels' entry points fails on the host before any
    launch: the pointers are host memory, and no device is needed to get the exception types."""
    from dpt_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base if base % 16 == 0 else base + 8)  # 16-byte aligned
    assert p.value % 16 == 0
    odd = ctypes.c_void_p(p.value + 4)
    null = ctypes.c_void_p(None)

    def desc(sd=1, A=5, npos=32, dropout=0.0):
        return _lib.TrainDesc(2, 32, sd, A, npos, 1, 1, 0, dropout, 0, 0)

    def ev(d, a, blob=p):
        return lambda: _lib.check(lib.dpt_exploit_eval(ctypes.byref(d) if d is not None else None, blob,
                                                       ctypes.byref(a) if a is not None else None, null))

    def A_(**over):
        return _args(_lib, p, **over)

    def curve(logits=p, means=p, targets=p, N=2, T=3, A=5, p_opt=p):
        return lambda: _lib.check(lib.dpt_recommend_curve(logits, means, targets, N, T, A, p, p, p, p_opt, null))

    def emp(actions=p, rewards=p, means=p, N=2, H=3, A=5):
        return lambda: _lib.check(lib.dpt_empirical_recommend(actions, rewards, means, N, H, A, p, p, null))

    d = desc()
    n = ctypes.c_int64()
    invalid = {
        "null desc": ev(None, A_()),
        "null blob": ev(d, A_(), blob=null),
        "null args": ev(d, None),
        "null means": ev(d, A_(means=None)),
        "null workspace": ev(d, A_(workspace=None)),
        "null actions": ev(d, A_(actions=None)),
        "null rewards": ev(d, A_(rewards=None)),
        "null targets with p_opt": ev(d, A_(targets=None)),
        "N < 1": ev(d, A_(N=0)),
        "H < 0": ev(d, A_(H=-1)),
        "1 + H > n_positions": ev(desc(npos=5), A_(H=5)),
        "state_dim": ev(desc(sd=2), A_()),
        "dropout": ev(desc(dropout=0.1), A_()),
        "flags": ev(d, A_(flags=1)),
        "reserved": ev(d, A_(reserved=1)),
        "misaligned": ev(d, A_(workspace=odd.value)),
        "workspace null numel": lambda: _lib.check(lib.dpt_exploit_eval_workspace_numel(ctypes.byref(d), 4, 3, None)),
        "workspace null desc": lambda: _lib.check(lib.dpt_exploit_eval_workspace_numel(None, 4, 3, ctypes.byref(n))),
        "workspace N < 1": lambda: _lib.check(lib.dpt_exploit_eval_workspace_numel(ctypes.byref(d), 0, 3,
                                                                                    ctypes.byref(n))),
        "workspace H < 0": lambda: _lib.check(lib.dpt_exploit_eval_workspace_numel(ctypes.byref(d), 4, -1,
                                                                                    ctypes.byref(n))),
        "workspace H": lambda: _lib.check(lib.dpt_exploit_eval_workspace_numel(ctypes.byref(d), 4, 32,
                                                                                ctypes.byref(n))),
        "curve null logits": curve(logits=null),
        "curve null means": curve(means=null),
        "curve null targets with p_opt": curve(targets=null),
        "curve N < 1": curve(N=0),
        "curve T < 1": curve(T=0),
        "curve A < 1": curve(A=0),
        "emp null means": emp(means=null),
        "emp null actions": emp(actions=null),
        "emp null rewards": emp(rewards=null),
        "emp N < 1": emp(N=0),
        "emp H < 0": emp(H=-1),
        "emp A < 1": emp(A=0),
    }
    for name, call in invalid.items():
        with pytest.raises(ValueError):
            call()
        assert lib.dpt_last_error(), name
    for name, word in (("H < 0", "H=-1"), ("1 + H > n_positions", "n_positions"), ("state_dim", "state_dim"),
                       ("dropout", "dropout"), ("misaligned", "aligned"), ("flags", "flags"),
                       ("reserved", "reserved")):
        with pytest.raises(ValueError, match=word):
            invalid[name]()
    unsupported = [
        ev(desc(A=33), A_()),
        curve(A=33),
        emp(A=33),
        lambda: _lib.check(lib.dpt_exploit_eval_workspace_numel(ctypes.byref(desc(A=33)), 4, 3, ctypes.byref(n))),
    ]
    for call in unsupported:
        with pytest.raises(NotImplementedError, match="action_dim"):
            call()
    # the last legal window is accepted by the size query (no launch)
    assert lib.dpt_exploit_eval_workspace_numel(ctypes.byref(d), 4, 31, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.dpt_exploit_eval_workspace_numel(ctypes.byref(d), 1, 0, ctypes.byref(n)) == 0 and n.value > 0


@pytest.mark.parametrize("E", [32, 18])
def test_workspace_size_matches_its_restatement(E):
    """the forward-only training workspace at window H + 1, the tokens and the logits, each region rounded
    to 16 bytes: no backward scratch, no gradient blob, no rollout workspace"""
    from dpt_hip import _lib
    lib = _lib.load()
    npos = 4 * (1 + 70)
    d = _lib.TrainDesc(2, E, 1, 5, npos, 1, 1, 0, 0.0, 0, 0)

    def round4(x):
        return (x + 3) & ~3

    def numel(N, H):
        n = ctypes.c_int64()
        assert lib.dpt_exploit_eval_workspace_numel(ctypes.byref(d), N, H, ctypes.byref(n)) == 0
        return n.value

    for N, H in ((5, 0), (5, 1), (5, 6), (5, 70), (3, 70), (37, 11)):
        run = _lib.TrainDesc(2, E, 1, 5, npos, N, H + 1, _lib.TRAIN_FORWARD_ONLY, 0.0, 0, 0)
        tw, full, ex = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        assert lib.dpt_train_workspace_numel(ctypes.byref(run), ctypes.byref(tw)) == 0
        assert numel(N, H) == round4(tw.value) + round4(N * (H + 1) * 8) + round4(N * (H + 1) * 5)
        run.reserved = 0
        assert lib.dpt_train_workspace_numel(ctypes.byref(run), ctypes.byref(full)) == 0
        assert numel(N, H) < full.value + round4(N * (H + 1) * 8) + round4(N * (H + 1) * 5)
        if H >= 1:
            assert lib.dpt_explore_workspace_numel(ctypes.byref(d), N, H + 1, ctypes.byref(ex)) == 0
            assert numel(N, H) < ex.value
    assert numel(5, 6) < numel(6, 6) and numel(5, 6) < numel(5, 7)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_recommend_source_passes_the_hazard_scan(tmp_path):
    hazard_scan("dpt_recommend.hip", tmp_path)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_recommend_kernels_use_no_scratch(tmp_path):
    """the six row widths of the curve kernel and the empirical kernel: no scratch, no LDS pressure"""
    r = remarks("dpt_recommend.hip", tmp_path)
    names = [n for n in r if "rc_curve_kernel" in n or "rc_empirical_kernel" in n]
    assert len(names) == 7, list(r)
    for n in names:
        assert r[n]["scratch"] == 0 and r[n]["occ"] >= 4, (n, r[n])


def test_fixture_is_what_the_generator_describes():
    """tests/golden/recommend_emp.npz: the issue's three cases, arm 0 at budget 0, and the sequential numpy
    restatement (pull order) names the reference's arm (pairwise sums) at every prefix -- the fixture's
    seeds keep every prefix clear of near-ties."""
    g = golden("recommend_emp.npz")
    for name, (N, H, A) in EMP_CASES.items():
        means, acts, rews, arms = (g[f"{name}/{k}"] for k in ("means", "actions", "rewards", "emp_arm"))
        assert means.shape == (N, A) and acts.shape == rews.shape == (N, H) and arms.shape == (N, H + 1)
        assert acts.dtype == np.int32 and rews.dtype == np.float64 and arms.dtype == np.int32
        assert (arms[:, 0] == 0).all() and arms.min() >= 0 and arms.max() < A
        ref = RO.empirical_recommend(acts, rews, means)
        assert np.array_equal(ref["emp_arm"], arms), name
    assert set(np.unique(g["bern3/rewards"])) <= {0.0, 1.0}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "recommend_emp.npz")) < 64 << 10


def test_oracle_restatements_on_hand_cases():
    """the numpy restatements themselves on cases worked by hand"""
    lg = np.array([[[0.0, np.log(3.0)], [2.0, 2.0]]], np.float32)
    means = np.array([[0.25, 0.75]])
    out = RO.recommend_curve(lg, means)
    assert out["greedy_arm"].tolist() == [[1, 0]] and out["greedy_value"].tolist() == [[0.75, 0.25]]
    p1 = np.exp(np.float64(np.float32(np.log(3.0)))) / (1 + np.exp(np.float64(np.float32(np.log(3.0)))))
    assert np.abs(out["expected_value"] - [[0.25 * (1 - p1) + 0.75 * p1, 0.5]]).max() <= 1e-15
    assert np.abs(out["p_opt"] - [[p1, 0.5]]).max() <= 1e-15
    assert (RO.recommend_curve(lg, means, targets=[2])["p_opt"] == 0).all()
    assert (RO.recommend_curve(lg, means, targets=[-1])["p_opt"] == 0).all()
    emp = RO.empirical_recommend([[1, 0, 7, 1]], [[0.5, 0.75, 100.0, -1.0]], means)
    assert emp["emp_arm"].tolist() == [[0, 1, 0, 0, 0]]  # the out-of-range pull adds to no arm
    assert emp["emp_value"].tolist() == [[0.25, 0.75, 0.25, 0.25, 0.25]]
    commit = RO.commit_regret(np.array([[1, 0]]), means, np.array([[0.25, 0.75, 0.75]]))
    assert commit.tolist() == [[2 * 0.5, 0.0 + 1 * 0.0, 0.5]]


def test_eval_script_imports_and_parses_its_flags():
    """evals/eval_explore_exploit.py without a device: eval_interactive_bandit.py's flags plus the four new
    ones, the two checkpoint names train_explorer_exploiter.py writes, twelve result keys"""
    ev = importlib.import_module("evals.eval_explore_exploit")
    sib = importlib.import_module("evals.eval_interactive_bandit")
    assert ev.generate_eval_trajs is sib.generate_eval_trajs
    a = ev.parse_args([])
    assert a["explorer_path"] == "trained_models/explorer_bandit.pt"
    assert a["exploiter_path"] == "trained_models/exploiter_bandit.pt"
    assert a["chunk"] == 0 and a["random_env"] is False and a["n_eval"] == 100 and a["var"] == 0.3
    assert a["save"] == "figs/eval_explore_exploit" and a["bandit_type"] == "uniform"
    a = ev.parse_args(["--n_eval", "8", "--H", "6", "--dim", "5", "--layer", "2", "--chunk", "3", "--random_env",
                       "--explorer_path", "a.pt", "--exploiter_path", "b.pt", "--bandit_type", "bernoulli",
                       "--env", "bandit", "--sample", "--seed", "3", "--save", "x.png", "--embd", "16"])
    assert (a["n_eval"], a["H"], a["dim"], a["layer"], a["chunk"], a["random_env"]) == (8, 6, 5, 2, 3, True)
    assert (a["explorer_path"], a["exploiter_path"], a["bandit_type"]) == ("a.pt", "b.pt", "bernoulli")
    with pytest.raises(SystemExit):
        ev.parse_args(["--bandit_type", "linear"])
    assert len({f"{c}/{r}" for c in ev.COLLECTORS for r in ev.RECOMMENDERS}) == 12
    text = open(os.path.join(ROOT, "decision-pretrained-transformer_amd", "train_explorer_exploiter.py")).read()
    assert "explorer_bandit.pt" in text and "exploiter_bandit.pt" in text
