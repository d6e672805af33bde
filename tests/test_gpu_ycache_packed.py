"""The bandit rollout's packed 24-bit y cache (DPT_TUNE_YCACHE_BITS = 24, the default;
csrc/dpt_ycache.h) against the float64 C oracle fed the same draws, against the fp32 form
(DPT_TUNE_YCACHE_BITS = 32) of the same build, and its bit-identities.

Shapes are the smallest at which each path of the stream can go wrong: a partial last tile
(N = 11 at tile 8, N = 19 at tile 16); H = 1 (no cached row), 9 (one whole 8-position group and
a partial one), 70 (one whole 64-position chunk and a 6-row tail), 130 (two whole chunks and a
tail); a cache budget that puts the default/non-temporal split at position 64 inside H = 130
(a pinned chunk, a non-temporal chunk, a partial chunk), budget 0 and the default; 1, 2 and 4
layers (1 layer has no y cache: the two forms must be equal there); 5 and 20 arms; sampled and
greedy selection.

Bar (the project's, tests/test_gpu_kernels.py): logits within 1e-5 max(1, |x|) at every step up
to and including a task's first differing action, which must sit on a draw within 1e-5 of a cdf
edge; actions, rewards and arm values exact on the compared steps; at least 0.9 of all task-steps
compared.  The measured errors are printed (pytest -s) and recorded in profiles/ycache24/errors.txt:
the largest logit error against the oracle over all these shapes is 3.6e-7 relative for either form,
the largest 24-against-32 logit difference 3.6e-7, and no run had a near-tie flip."""
import functools

import numpy as np
import pytest

import philox_np
from test_gpu_kernels import compared_steps

pytestmark = pytest.mark.gpu

HS = (1, 9, 70, 130)
HMAX = max(HS)
SEED = 20240


def _setup(L, A):
    """One model per (L, A), n_positions for the longest horizon, shared by every H."""
    import bench
    import dpt_hip
    dpt_hip.device()
    sd, _ = bench.synthetic_state_dict(L, 1, A, HMAX)
    return sd, dpt_hip.DeviceModel(sd, L, 1, A, 4 * (1 + HMAX)), dpt_hip.pack_weights(sd, L).numpy()


def _means(N, A):
    if A == 5:
        return np.random.RandomState(1).uniform(0, 1, (N, A))
    arms = np.random.RandomState(1234).normal(size=(A, 2)) / np.sqrt(2)
    return np.random.RandomState(2).normal(0, 1, (N, 2)) / np.sqrt(2) @ arms.T


@functools.lru_cache(maxsize=None)
def _draws(N, H):
    import dpt_hip
    tasks = np.arange(N)
    u = np.stack([philox_np.uniform(SEED, h, tasks, dpt_hip.STREAM_SELECT) for h in range(H)])
    # the device's own normals (its fp64 Box-Muller may differ from numpy's in the last place; the
    # rewards are compared exactly)
    g = np.stack([dpt_hip.draw(1, SEED, h, 0, N, dpt_hip.STREAM_REWARD).cpu().numpy() for h in range(H)])
    return u, g


def _oracle(blob, L, A, means, H, sample):
    from oracle import c_oracle
    u, g = _draws(len(means), H)
    return c_oracle.bandit_rollout_f64(blob, L, A, 4 * (1 + HMAX), means, H, 0.3, u, g, sample, False, 1,
                                       want_logits=True)


def _run(m, means, H, sample, **kw):
    o = m.rollout_bandit(means, H, 0.3, sample, seed=SEED, want_logits=True, **kw)
    return {k: o[k].cpu().numpy() for k in ("actions", "rewards", "arm_value", "logits")}


def _check(out, ref, margin, bar=1e-5):
    """The bar of the module docstring for one run against a reference run (the oracle, or the
    other form with the oracle's margins); returns the largest relative logit error and the
    compared steps per task.  ``bar``: the logit bar, for callers whose models have one of their own
    (tests/sharp_models.py); every test of this module keeps 1e-5."""
    H = out["actions"].shape[1]
    n_cmp = compared_steps(out["actions"], ref["actions"], margin)
    step = np.arange(H)[:, None]
    sel = step <= np.minimum(n_cmp, H - 1)[None, :]
    got, want = out["logits"][sel].astype(np.float64), ref["logits"][sel].astype(np.float64)
    rel = np.abs(got - want) / np.maximum(1, np.abs(want))
    ok = (step < n_cmp[None, :]).T
    frac = float(ok.mean())
    print(f"  max rel logit err {rel.max():.3e}, compared {frac:.4f}")
    assert rel.max() <= bar, float(rel.max())
    for k in ("actions", "rewards", "arm_value"):
        assert np.array_equal(out[k][ok], ref[k][ok]), k
    assert frac >= 0.9, frac
    return float(rel.max()), n_cmp


def _logit_diff(a, b, n_cmp):
    """Largest relative logit difference of two runs over the steps both computed on the oracle's
    trajectory (n_cmp: per task, the smaller of their compared steps)."""
    H = a["actions"].shape[1]
    sel = np.arange(H)[:, None] <= np.minimum(n_cmp, H - 1)[None, :]
    x, y = a["logits"][sel].astype(np.float64), b["logits"][sel].astype(np.float64)
    return float((np.abs(x - y) / np.maximum(1, np.abs(y))).max())


def _equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


@pytest.fixture(autouse=True)
def _defaults():
    import dpt_hip
    yield
    dpt_hip.set_decode_tile(8)
    dpt_hip.set_cache_budget(224 << 20)
    dpt_hip.set_ycache_bits(24)


@pytest.mark.parametrize("A", [5, 20])
@pytest.mark.parametrize("L", [1, 2, 4])
@pytest.mark.parametrize("tile,N", [(8, 11), (16, 19)])
def test_packed_and_fp32_forms_match_oracle(tile, N, L, A):
    """Both forms against the oracle and against each other at every H, sampled and greedy, with
    the budget that splits the stream at position 64, budget 0 and the default."""
    import dpt_hip
    sd, m, blob = _setup(L, A)
    means = _means(N, A)
    dpt_hip.set_decode_tile(tile)
    split = max(L - 1, 1) * N * 128 * 64  # `pin` = 64 for every block in both forms
    worst = {24: 0.0, 32: 0.0, "24v32": 0.0}
    for H in HS:
        for sample in (True, False):
            ref = _oracle(blob, L, A, means, H, sample)
            outs, n_cmp = {}, {}
            for bits in (24, 32):
                dpt_hip.set_ycache_bits(bits)
                dpt_hip.set_cache_budget(split)
                print(f"tile {tile} N {N} L {L} A {A} H {H} sample {sample} bits {bits}:")
                outs[bits] = _run(m, means, H, sample)
                err, n_cmp[bits] = _check(outs[bits], ref, ref["margin"])
                worst[bits] = max(worst[bits], err)
                for budget in (0, 224 << 20):  # cache policy only: bit-identical
                    dpt_hip.set_cache_budget(budget)
                    assert _equal(outs[bits], _run(m, means, H, sample)), (bits, budget)
            if L == 1:  # no y cache: the same arithmetic
                assert _equal(outs[24], outs[32])
            # both follow the oracle up to their compared steps (same rule, checked above): there the
            # two forms saw identical contexts
            d = _logit_diff(outs[24], outs[32], np.minimum(n_cmp[24], n_cmp[32]))
            print(f"  24 vs 32: max rel logit diff {d:.3e}")
            assert d <= 1e-5, d
            worst["24v32"] = max(worst["24v32"], d)
    print(f"YCACHE-ERR tile={tile} N={N} L={L} A={A}: vs oracle 24-bit {worst[24]:.3e}, 32-bit {worst[32]:.3e}; "
          f"24 vs 32 {worst['24v32']:.3e}")


def test_spike_model_top_of_range():
    """One wpe column raised by 1e3: block 1's normalised rows have an element near sqrt(31) =
    5.57, the top of the range a LayerNorm output can reach (the format holds +-8)."""
    import bench
    import dpt_hip
    dpt_hip.device()
    N, H, L, A = 8, 20, 2, 5
    sd, _ = bench.synthetic_state_dict(L, 1, A, H)
    sd = dict(sd)
    wpe = sd["transformer.wpe.weight"].clone()
    wpe[:, 0] += 1e3
    sd["transformer.wpe.weight"] = wpe
    m = dpt_hip.DeviceModel(sd, L, 1, A, 4 * (1 + H))
    blob = dpt_hip.pack_weights(sd, L).numpy()
    means = _means(N, A)
    from oracle import c_oracle
    u, g = _draws(N, H)
    ref = c_oracle.bandit_rollout_f64(blob, L, A, 4 * (1 + H), means, H, 0.3, u, g, True, False, 1, want_logits=True)
    errs = {}
    for bits in (24, 32):
        dpt_hip.set_ycache_bits(bits)
        print(f"spike bits {bits}:")
        errs[bits] = _check(_run(m, means, H, True), ref, ref["margin"])[0]
    print(f"YCACHE-ERR spike N={N} H={H} L={L}: vs oracle 24-bit {errs[24]:.3e}, 32-bit {errs[32]:.3e}")


@pytest.mark.parametrize("H", [9, 130])
def test_packed_bit_identities(H):
    """In packed form: tile 8 = tile 16, budget 0 = default, two runs equal, and a run split into
    two first_task shards equals the whole (N = 27: partial last tiles at both tile sizes)."""
    import dpt_hip
    N, L, A = 27, 4, 5
    sd, m, _ = _setup(L, A)
    means = _means(N, A)
    dpt_hip.set_ycache_bits(24)
    base = _run(m, means, H, True)
    assert _equal(base, _run(m, means, H, True))
    dpt_hip.set_cache_budget(0)
    assert _equal(base, _run(m, means, H, True))
    dpt_hip.set_cache_budget(224 << 20)
    dpt_hip.set_decode_tile(16)
    assert _equal(base, _run(m, means, H, True))
    dpt_hip.set_decode_tile(8)
    a = _run(m, means[:10], H, True, first_task=0)
    b = _run(m, means[10:], H, True, first_task=10)
    for k in ("actions", "rewards", "arm_value"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), base[k]), k
    assert np.array_equal(np.concatenate([a["logits"], b["logits"]], 1), base["logits"])
