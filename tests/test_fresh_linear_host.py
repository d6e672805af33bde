"""CPU checks of the linear bandit's fresh-task generator and training step (csrc/dpt_fresh_linear.hip,
dpt_fresh_linear_batch / dpt_fresh_linear_step / dpt_fresh_linear_eval_loss, dpt_hip.FreshEnv.linear_bandit,
train_fresh.py --data_type): the new C ABI entry points (symbols, struct layout, every host-side check with no
device present, each message naming its cause), the numpy restatement (tests/fresh_linear_oracle.py) against
facts, the GPU cases' minimum arg-max gap, the machine code of the new source, and the CLI's refusals.  No
device work is launched."""
import ctypes
import importlib
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fresh_linear_oracle as LO
import fresh_oracle as FO
from conftest import ROOT
from test_isa_hazards import HIPCC, test_no_short_mfma_hazard_paths as hazard_scan
from test_resource_budget import remarks

CSRC = os.path.join(ROOT, "decision-pretrained-transformer_amd", "csrc")
NEW_SYMBOLS = ("dpt_fresh_linear_batch", "dpt_fresh_linear_step", "dpt_fresh_linear_eval_loss")
ALL_CASES = LO.CASES + LO.H_CASES


def test_new_symbols_exported_and_bound():
    import dpt_hip
    from dpt_hip import _lib
    lib = _lib.load()
    assert lib.dpt_abi_version() == _lib.ABI_VERSION == 8
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert (_lib.FRESH_LINEAR_THOMPSON, _lib.FRESH_LINEAR_UNIFORM) == (LO.THOMPSON, LO.UNIFORM) == (0, 1)
    assert callable(dpt_hip.FreshEnv.linear_bandit)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "dpt_fresh_linear.hip" in mk and "dpt_fresh.h " in mk
    # the kernel's chunk and table lengths, as the GPU cases and the binding assume them
    src = open(os.path.join(CSRC, "dpt_fresh_linear.hip")).read()
    assert int(re.search(r"kLinChunk = (\d+);", src).group(1)) == LO.CHUNK == _lib.FRESH_LINEAR_CHUNK
    assert int(re.search(r"kLinTable = (\d+);", src).group(1)) == LO.TABLE
    assert {c[5] for c in LO.H_CASES} >= {0, 1, LO.CHUNK - 1, LO.CHUNK, LO.CHUNK + 1, 2 * LO.CHUNK + 1, LO.TABLE + 6}
    # the bandit's behaviour policy and rows: one copy, in the shared header, called by both generators
    fresh, hdr = (open(os.path.join(CSRC, f)).read() for f in ("dpt_fresh.hip", "dpt_fresh.h"))
    for fn in ("void fresh_bandit_policy(", "void fresh_bandit_rows(", "void fresh_store_rows("):
        assert fn in hdr and fn not in fresh and fn not in src, fn
    for fn in ("fresh_bandit_policy(", "fresh_bandit_rows("):
        assert fn in fresh and fn in src, fn


def test_struct_layout_matches_header(tmp_path):
    """dpt_fresh_linear_args: ctypes against the C compiler's layout, field by field; dpt_fresh_args unchanged"""
    from dpt_hip import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    cname, cls = "dpt_fresh_linear_args", _lib.FreshLinearArgs
    assert [f for f, _ in cls._fields_] == ["rollin", "dim", "lin_d", "H", "var", "seed", "first_task", "arms",
                                           "theta_out", "means_out", "probs_out", "opt_action_out"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dpt_hip.h"', 'int main(void) {',
             f'printf("size %zu\\n", sizeof({cname}));', 'printf("old %zu\\n", sizeof(dpt_fresh_args));']
    lines += [f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));' for fname, _ in cls._fields_]
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                              text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls) == 80
    assert int(got["old"]) == ctypes.sizeof(_lib.FreshArgs) == 112
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname


def test_host_validation_without_a_device():
    """Every check fails on the host before any launch: the pointers are host memory a kernel would fault on.
    Each message names its cause."""
    from dpt_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    pv, null = p.value, ctypes.c_void_p(None)
    H = 7

    def desc(sd=1, A=5, batch=8, window=1 + H, flags=0):
        return _lib.TrainDesc(2, 32, sd, A, 4 * (1 + H), batch, window, flags, 0.0, 0, 0)

    def lin(rollin=0, A=5, d=2, H=H, var=0.3, arms=pv):
        return _lib.FreshLinearArgs(rollin, A, d, H, var, 1, 0, arms, None, None, None, None)

    opt = _lib.AdamWArgs(1e-3, 0.9, 0.999, 1e-8, 1e-4, 1)
    bad_step = _lib.AdamWArgs(1e-3, 0.9, 0.999, 1e-8, 1e-4, 0)
    ref = ctypes.byref

    def batch_call(d, a, n=4, tokens=p, targets=p):
        return lambda: _lib.check(lib.dpt_fresh_linear_batch(ref(d) if d else None, ref(a) if a else None, n, tokens,
                                                             targets, null))

    def step_call(d, a, n=4, blob=p, m=p, v=p, o=opt, ws=p, loss=p):
        return lambda: _lib.check(lib.dpt_fresh_linear_step(ref(d) if d else None, ref(a) if a else None, n, blob, m,
                                                            v, ref(o) if o else None, ws, loss, null))

    def eval_call(d, a, n=4, blob=p, ws=p, loss=p):
        return lambda: _lib.check(lib.dpt_fresh_linear_eval_loss(ref(d) if d else None, ref(a) if a else None, n,
                                                                 blob, ws, loss, null))

    def every(d, a, **kw):  # the generator's own checks hold through all three entry points
        return [batch_call(d, a, **kw), step_call(d, a, **kw), eval_call(d, a, **kw)]

    invalid = [  # (calls, what the message names)
        ([batch_call(None, lin()), step_call(None, lin()), eval_call(None, lin())], "null"),
        ([batch_call(desc(), None), step_call(desc(), None), eval_call(desc(), None)], "null"),
        ([batch_call(desc(), lin(), tokens=null), batch_call(desc(), lin(), targets=null)], "null"),
        (every(desc(), lin(arms=None)), "arms"),
        (every(desc(), lin(), n=0) + every(desc(), lin(), n=9), "batch"),
        (every(desc(window=H), lin()), "window"),
        (every(desc(window=0), lin(H=-1)), "H=-1"),
        (every(desc(sd=2), lin()), "state_dim"),
        (every(desc(A=4), lin()), "action_dim"),
        (every(desc(A=0), lin(A=0)), "dim=0"),
        (every(desc(), lin(d=0)), "lin_d=0"),
        (every(desc(), lin(rollin=2)) + every(desc(), lin(rollin=-1)), "rollin"),
        (every(desc(), lin(var=-0.1)) + every(desc(), lin(var=math.inf)) + every(desc(), lin(var=math.nan)) +
         every(desc(), lin(rollin=1, var=-1.0)), "var"),
        (every(desc(), lin(var=0.0)), "var=0 with the Thompson"),
        ([step_call(desc(flags=1), lin()), eval_call(desc(flags=1), lin())], "flags"),
        ([step_call(desc(), lin(), o=bad_step)], "step=0"),
        ([step_call(desc(), lin(), blob=null), step_call(desc(), lin(), m=null), step_call(desc(), lin(), v=null),
          step_call(desc(), lin(), o=None), step_call(desc(), lin(), ws=null), step_call(desc(), lin(), loss=null),
          eval_call(desc(), lin(), blob=null), eval_call(desc(), lin(), ws=null),
          eval_call(desc(), lin(), loss=null)], "null"),
    ]
    for calls, cause in invalid:
        for i, call in enumerate(calls):
            with pytest.raises(ValueError, match=re.escape(cause)):
                call()
            assert "linear" in lib.dpt_last_error().decode(), (cause, i)
    unsupported = [(every(desc(A=33), lin(A=33)), "action_dim=33"), (every(desc(), lin(d=9)), "lin_d=9")]
    for calls, cause in unsupported:
        for call in calls:
            with pytest.raises(NotImplementedError, match=cause):
                call()


def test_oracle_against_facts():
    seed, ft, n, A, d, H, var = 41, 5, 16, 6, 3, 120, 0.3
    arms = LO.arms_of(A, d)
    t = LO.task(seed, ft, n, arms)
    # theta ~ N(0, 1 / d) per coordinate; means = arms @ theta up to the summation order
    big = LO.task(seed, 0, 20000, arms)
    assert abs(big["theta"].var() - 1 / d) < 0.02 / d and abs(big["theta"].mean()) < 0.02
    assert np.abs(t["means"] - t["theta"] @ arms.T).max() < 1e-15
    # the label is the first argmax, also among equal means
    assert np.array_equal(t["opt_action"], t["means"].argmax(1))
    assert FO.first_argmax(np.array([[0.3, 0.7, 0.7], [0.5, 0.5, 0.1]])).tolist() == [1, 0]
    # a sample is a function of (seed, its global index)
    part = LO.task(seed, ft + 3, 4, arms)
    assert np.array_equal(part["means"], t["means"][3:7])
    r = LO.thompson(t["means"], var, *LO.chain_normals(seed, ft, n, A, H))
    # counts sum to h, and follow the actions
    assert np.array_equal(r["counts"].sum(-1), np.tile(np.arange(H + 1), (n, 1)))
    assert np.array_equal(r["counts"][:, -1], np.stack([np.bincount(a, minlength=A) for a in r["actions"]]))
    # s_k is a function of n_k alone
    assert np.array_equal(r["stds"], LO.posterior_std(r["counts"][:, :-1], var))
    # the rewards are the chosen arm's mean plus var times the step's reward normal
    _, gr = LO.chain_normals(seed, ft, n, A, H)
    assert np.array_equal(r["rewards"], np.take_along_axis(t["means"], r["actions"], 1) + (0.0 + var * gr))
    # Thompson sampling finds the best arm: it is the most pulled one in most tasks ...
    assert (r["counts"][:, -1].argmax(1) == t["opt_action"]).mean() >= 0.75
    # ... and with huge noise the posterior stays wide: the pulls spread over all arms
    wide = LO.thompson(t["means"], 1e3, *LO.chain_normals(seed, ft, n, A, H))
    assert (wide["counts"][:, -1] >= H / A / 4).all()
    assert wide["counts"][:, -1].max() < 2.5 * H / A
    # the uniform rollin's behaviour policy: distributions, over the whole grid, on counters behind theta
    u = LO.uniform_policy(seed, 0, 5000, A, d)
    assert np.abs(u["probs"].sum(1) - 1).max() <= 1e-15 and (u["probs"] >= 0).all()
    assert set(u["cov_index"].tolist()) == set(range(11)) and set(u["rand_index"].tolist()) == set(range(A))
    assert not np.array_equal(u["p"][:16], FO.bandit_task(seed, 0, 16, A)["p"])  # other counters, other draws


@pytest.mark.parametrize("case", ALL_CASES + [LO.SPLIT[:1] + (0, 64) + LO.SPLIT[1:]], ids=LO.case_id)
def test_the_gpu_cases_have_no_near_ties(case):
    """the minimum gap between the largest and second-largest v_k over all tasks and steps is above 1e-9: the
    device's normals lie within 1e-12 of numpy's and its running-sum means orders closer to the pairwise ones,
    so device, oracle and dpt_rollout_policy choose the same arm at every step; and no rollin uniform lies
    within 1e-12 of a cdf step of the uniform rollin's policy"""
    gap = LO.min_gap(case)
    print(f"{LO.case_id(case)}: minimum gap {gap:.3g}")
    assert gap > 1e-9
    assert LO.uniform_near_ties(case) == 0


def test_the_issues_gaps_are_reproduced():
    got = [LO.min_gap(c) for c in LO.CASES]
    assert [float(f"{g:.2g}") for g in got] == [2.0e-4, 3.3e-5, 3.8e-3], got


def test_a_constructed_near_tie_is_reported():
    """the gap function itself: two arms whose values differ by 1e-13 at one step"""
    means = np.array([[0.25, 0.5, 0.125]])
    g = np.zeros((1, 3, 3))
    gr = np.zeros((1, 3))
    # step 0: v = g (m = 0, s = 1): arms 0 and 2 lead, 1e-13 apart
    g[0, 0] = [0.75, -1.0, 0.75 - 1e-13]
    g[0, 1:] = [[5.0, 0.0, -5.0], [0.0, 5.0, -5.0]]
    r = LO.thompson(means, 0.3, g, gr)
    assert 0 < r["gap"] < 2e-13 and r["actions"][0].tolist() == [0, 0, 1]
    g[0, 0, 2] = 0.75  # an exact tie: the first index wins
    r = LO.thompson(means, 0.3, g, gr)
    assert r["gap"] == 0.0 and r["actions"][0, 0] == 0
    assert LO.gaps(np.array([[1.0, 3.0, 2.5]])).tolist() == [0.5] and np.isinf(LO.gaps(np.zeros((2, 1)))).all()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_fresh_linear_source_passes_the_hazard_scan(tmp_path):
    hazard_scan("dpt_fresh_linear.hip", tmp_path)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_fresh_linear_kernels_use_no_scratch(tmp_path):
    r = remarks("dpt_fresh_linear.hip", tmp_path)
    names = [n for n in r if "fresh_linear_thompson_kernel" in n or "fresh_linear_uniform_kernel" in n]
    assert len(names) == 2, list(r)
    for n in names:
        assert r[n]["scratch"] == 0 and r[n]["occ"] >= 4, (n, r[n])


def test_train_fresh_linear_bandit_refusals(tmp_path, monkeypatch):
    """each before anything is created"""
    train_fresh = importlib.import_module("train_fresh")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match="adaptive Thompson.*--data_type"):
        train_fresh.main(["--env", "linear_bandit"])
    with pytest.raises(ValueError, match="--data_type uniform belongs to --env linear_bandit"):
        train_fresh.main(["--env", "bandit", "--data_type", "uniform"])
    with pytest.raises(ValueError, match="--data_type thompson"):
        train_fresh.main(["--env", "darkroom_heldout", "--data_type", "thompson"])
    for data_type in ("thompson", "uniform"):
        with pytest.raises(Exception, match="Are you sure you want to shuffle on the linear bandit"):
            train_fresh.main(["--env", "linear_bandit", "--data_type", data_type, "--shuffle"])
    with pytest.raises(SystemExit):  # argparse: not one of the two
        train_fresh.main(["--env", "linear_bandit", "--data_type", "ucb"])
    assert not os.listdir(tmp_path)
