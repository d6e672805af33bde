"""The linear bandit's Bayes posterior of the optimal arm at lin_d = 2 on the CPU (include/dpt_hip.h, "Linear
bandit, lin_d = 2"): the numpy restatement tests/linear_posterior_oracle.py -- which the GPU tests hold the
kernel to -- is itself held to computations that do not depend on it, and the host side of the new entry points
(symbols, struct layout, every host check, the Python-layer rules, the CLI's refusal) runs with no device work.

- Monte Carlo: on six tasks (the reference's arms at A in {5, 10, 20}, std 0.3 and 1.0) the oracle at rows 1, 5
  and H agrees with the frequency of every arm being optimal under 400,000 draws of theta from the posterior,
  within 5 binomial standard errors sqrt(p (1 - p) / n) at the oracle's p (an arm the oracle gives 0 -- it is
  strictly inside the hull -- must never win a draw).
- The prior row against a count over 2^20 directions, to 1e-5, summing to 1 within 1e-12.
- Convergence: at the default G the rows t >= 1 stay within 1e-6 of G = 65,536 (measured 1.9e-7).
- The rounding floor eps0 of the float64 definition against the same definition in long double on the GPU
  test's own inputs: measured 2.3e-10 (worst at A = 32, std 0.05, G = 256), asserted <= 1e-9, which is what the
  GPU test's relative bar of 1e-7 = 100 eps0 rounded up to a power of ten rests on.
- The kernels use no scratch."""
import ctypes
import importlib
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import linear_posterior_oracle as LO
from conftest import ROOT
from test_isa_hazards import HIPCC
from test_resource_budget import remarks

NEW_SYMBOLS = ("dpt_linear_posterior_workspace_numel", "dpt_linear_posterior")
DEFAULT_GRID = 8192


# ----------------------------------------------------------------------------- the definition is a posterior
@pytest.mark.parametrize("var", [0.3, 1.0])
@pytest.mark.parametrize("A", [5, 10, 20])
def test_the_oracle_matches_monte_carlo(A, var):
    H, draws = 20, 400_000
    arms = LO.reference_arms(A)
    acts, rews, _ = LO.sample_records(arms, 1, H, var, 7 + A)
    post = LO.linear_posterior(arms, acts, rews, var, DEFAULT_GRID)[0]
    _, m, L = LO.moments(arms, acts, rews, var)
    for t in (1, 5, H):
        f, _ = LO.monte_carlo(arms, m[0, t], L[0, t], draws, 3 + t)
        p = post[t]
        se = np.sqrt(p * (1 - p) / draws)
        z = np.abs(p - f) / np.where(se > 0, se, 1.0)
        print(f"A={A} var={var} t={t}: worst |z| {z[se > 0].max():.2f}, arms at 0: {(p == 0).sum()}")
        assert (np.abs(p - f) <= 5 * se).all(), (t, p, f, se)


@pytest.mark.parametrize("arms", [LO.reference_arms(5), LO.reference_arms(10), LO.reference_arms(20), LO.gpu_arms(5),
                                  LO.gpu_arms(20), LO.gpu_arms(32)], ids=["ref5", "ref10", "ref20", "gpu5", "gpu20", "gpu32"])
def test_the_prior_row_is_the_share_of_directions(arms):
    pr = LO.prior(arms)
    brute = LO.prior_brute(arms)
    print(f"max |prior - count| {np.abs(pr - brute).max():.3e}, sum - 1 {pr.sum() - 1:.3e}")
    assert np.abs(pr - brute).max() <= 1e-5 and abs(pr.sum() - 1) <= 1e-12
    assert ((pr == 0) == (brute == 0)).all()  # an arm is dropped iff no direction picks it


def test_the_prior_of_special_arms():
    assert LO.prior(np.array([[0.3, -0.2]])).tolist() == [1.0]
    assert LO.prior(np.array([[1.0, 0.0], [-1.0, 0.0]])).tolist() == [0.5, 0.5]
    sq = LO.prior(np.array([[1.0, 1.0], [-1.0, 1.0], [-1.0, -1.0], [1.0, -1.0], [0.0, 0.0], [1.0, 1.0], [1.0, 0.0]]))
    # a square's corners, the origin inside it, a copy of corner 0, the middle of an edge
    assert np.abs(sq[:4] - 0.25).max() <= 1e-15 and sq[4:].tolist() == [0.0, 0.0, 0.0]
    post = LO.linear_posterior(LO.gpu_arms(20), *LO.gpu_records(20, 0.3), 0.3, 64)
    assert not post[:, :, [3, 5, 8]].any()  # the copy, the arm inside an edge, the arm inside the hull
    assert np.array_equal(post[1, :5], np.broadcast_to(LO.prior(LO.gpu_arms(20)), (5, 20)))  # four invalid actions
    assert np.array_equal(post[0, 1], post[0, 0]) and np.array_equal(post[0, 6], post[0, 5])


def convergence_records():
    arms = LO.reference_arms(10)
    acts, rews, _ = LO.sample_records(arms, 6, 20, 0.3, 11)
    return arms, acts, rews


def test_the_default_grid_has_converged():
    import dpt_hip
    assert dpt_hip.linear_posterior_grid() == DEFAULT_GRID
    arms, acts, rews = convergence_records()
    ref = LO.linear_posterior(arms, acts, rews, 0.3, 65536)
    err = {G: np.abs(LO.linear_posterior(arms, acts, rews, 0.3, G) - ref)[:, 1:].max() for G in (DEFAULT_GRID // 2, DEFAULT_GRID)}
    print(f"max |post(G) - post(65536)| over rows t >= 1: {err}")
    assert err[DEFAULT_GRID] <= 1e-6 < err[DEFAULT_GRID // 2]  # the smallest power of two that meets 1e-6


def test_rounding_floor_on_the_gpu_cases():
    worst = 0.0
    for A in LO.GPU_AS:
        arms = LO.gpu_arms(A)
        for var in LO.GPU_VARS:
            acts, rews = LO.gpu_records(A, var)
            for G in LO.GPU_GS:
                p64 = LO.linear_posterior(arms, acts, rews, var, G)
                pld = LO.linear_posterior(arms, acts, rews, var, G, np.longdouble)
                big = np.abs(pld) >= 1e-100
                rel = float((np.abs(p64 - pld)[big] / np.abs(pld[big])).max())
                assert (np.abs(p64 - pld)[~big] <= 1e-100).all()
                print(f"A={A} var={var} G={G}: eps0 {rel:.3e} on {big.sum()} entries >= 1e-100")
                worst = max(worst, rel)
    print(f"eps0 = {worst:.3e}")
    assert worst <= 1e-9  # 100 eps0 <= 1e-7, the GPU test's relative bar


# ----------------------------------------------------------------------------- the host side of the library
def test_new_symbols_exported_and_bound():
    import dpt_hip
    from dpt_hip import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert callable(dpt_hip.linear_posterior) and callable(dpt_hip.linear_posterior_grid)


def test_struct_layout_matches_the_header(tmp_path):
    from dpt_hip import _lib
    cname, cls = "dpt_linear_posterior_args", _lib.LinearPosteriorArgs
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
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
    assert int(got["size"]) == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname


FAKE = 0x1000  # a non-null pointer no check dereferences: every case below fails before any launch


def test_host_checks_fail_before_any_launch():
    from dpt_hip import _lib
    lib = _lib.load()
    EINVAL, EUNSUP = _lib.DPT_EINVAL, _lib.DPT_EUNSUPPORTED

    def call(**kw):
        f = dict(N=3, H=4, A=5, lin_d=2, G=256, flags=0, var=0.3, arms=FAKE, actions=FAKE, rewards=FAKE,
                 workspace=FAKE, post=FAKE)
        f.update(kw)
        return lib.dpt_linear_posterior(ctypes.byref(_lib.LinearPosteriorArgs(**f)), None)
    assert lib.dpt_linear_posterior(None, None) == EINVAL
    for kw in (dict(arms=None), dict(post=None), dict(workspace=None), dict(actions=None), dict(rewards=None),
               dict(N=0), dict(H=-1), dict(A=0), dict(lin_d=0), dict(G=0), dict(G=-64), dict(var=0.0), dict(var=-0.3),
               dict(var=float("nan")), dict(flags=1), dict(workspace=FAKE + 4)):
        assert call(**kw) == EINVAL, kw
    assert call(var=0.0) == EINVAL and b"std" in lib.dpt_last_error()  # the message says what `var` is
    for kw in (dict(lin_d=3), dict(lin_d=1), dict(A=33), dict(G=32), dict(G=100), dict(G=65536 + 64), dict(G=1 << 17)):
        assert call(**kw) == EUNSUP, kw
    assert call(lin_d=3) == EUNSUP and b"lin_d-dimensional integral" in lib.dpt_last_error()
    with pytest.raises(NotImplementedError, match="lin_d=3"):
        _lib.check(call(lin_d=3))

    n = ctypes.c_int64()
    numel = lib.dpt_linear_posterior_workspace_numel
    assert numel(3, 5, 2, 1024, None) == EINVAL
    assert numel(0, 5, 2, 1024, ctypes.byref(n)) == EINVAL
    assert numel(3, 5, 3, 1024, ctypes.byref(n)) == EUNSUP
    assert numel(3, 33, 2, 1024, ctypes.byref(n)) == EUNSUP
    assert numel(3, 5, 2, 1000, ctypes.byref(n)) == EUNSUP
    # the cos | sin tables and 104 doubles of prior, count and index lists, whatever N and A
    for N, A, G in ((1, 1, 64), (70, 5, 1024), (100000, 32, 65536)):
        assert numel(N, A, 2, G, ctypes.byref(n)) == 0 and n.value == 2 * G + 104, (N, A, G)


def test_python_layer_refusals(tmp_path, monkeypatch):
    import dpt_hip
    assert dpt_hip.linear_posterior_supported(2, 0.3) is None
    for lin_d, var in ((3, 0.3), (1, 0.3), (2, 0.0), (2, -1.0)):
        assert "lin_d-dimensional integral" in dpt_hip.linear_posterior_supported(lin_d, var)
        env = types.SimpleNamespace(kind=dpt_hip.FreshEnv.LINEAR, lin_d=lin_d, var=var)  # read before any device work
        with pytest.raises(NotImplementedError, match="lin_d-dimensional integral"):
            dpt_hip.fresh_posterior(env, {})
    train_fresh = importlib.import_module("train_fresh")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(NotImplementedError, match="lin_d-dimensional integral.*supported: lin_d = 2"):
        train_fresh.main(["--env", "linear_bandit", "--data_type", "thompson", "--lin_d", "3", "--var", "0.3",
                          "--bayes_floor"])
    with pytest.raises(NotImplementedError, match="lin_d-dimensional integral"):
        train_fresh.main(["--env", "linear_bandit", "--data_type", "uniform", "--lin_d", "2", "--var", "0.0",
                          "--bayes_floor"])
    ev = importlib.import_module("evals.eval_posterior")
    with pytest.raises(NotImplementedError, match="lin_d-dimensional integral"):
        ev.run(None, "linear_bandit", "fresh", 4, 5, 6, 0.3, "uniform", 0, lin_d=3)
    assert not os.listdir(tmp_path)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_linear_posterior_kernels_use_no_scratch(tmp_path):
    r = remarks("dpt_posterior_linear.hip", tmp_path)
    names = [n for n in r if "lp_kernel" in n or "lp_setup_kernel" in n]
    assert len(names) == 2, list(r)
    for n in names:
        assert r[n]["scratch"] == 0, (n, r[n])
