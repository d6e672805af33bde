"""The compared cases of the episode rollout (dpt_rollout_darkroom_episode), shared by the CPU file that
asserts their oracle margins and the GPU file that compares the device against them (a test helper, not a
conftest).  Every case is one float64 oracle episode (tests/interactive_mdp_oracle.py), computed once per
process and never modified.

A float64 forward cannot tell which way a draw at a cdf edge falls, so a case is compared only where every
oracle margin exceeds MARGIN = 1e-5, the bar on the device's fp32 logits; the CPU file asserts it."""
import functools

import numpy as np

import interactive_mdp_oracle as MO

MARGIN = 1e-5
LAYERS = 4

# name -> (K, N, dim, sampled): the window crosses 16 -> 17 (a second block; waves with 0, 1 and 2 blocks),
# 32 -> 33, 128 -> 129 (the 8-wave geometry) and 256 -> 257 (16 waves); K = 1 and 2 have no and one transition
TABLE = {"K17": (17, 5, 4, True), "K33": (33, 4, 5, True), "K129": (129, 3, 10, True), "K257": (257, 2, 10, True),
         "K129_greedy": (129, 3, 10, False), "K1": (1, 4, 3, True), "K2": (2, 4, 3, True)}
SHARP_LEVEL, SHARP_SEED = "medium", 0


@functools.lru_cache(maxsize=None)
def table_case(name):
    """(model, goals (N, 2), uniforms (K - 1, N), sampled, dim, n_layer, the oracle's episode)"""
    K, N, dim, sample = TABLE[name]
    m, w64 = MO.model(32, LAYERS, K, 2000 + K)
    rs = np.random.RandomState(0)
    goals = rs.randint(0, dim, (N, 2)).astype(np.int32)
    u = rs.uniform(size=(K - 1, N))
    ep = MO.episode(w64, LAYERS, goals, K, dim, sample, u if sample else None)
    return m, goals, u, sample, dim, LAYERS, ep


@functools.lru_cache(maxsize=None)
def records_case(permuted):
    """the records case of interactive_mdp_oracle (dim 3, 7 envs, 6 steps, 2 layers) in the same shape"""
    m, _, u, perm, ep = MO.records_case(32, permuted)
    return m, MO.REC_GOALS, u, True, MO.REC_DIM, MO.REC_L, ep, perm


@functools.lru_cache(maxsize=None)
def sharp_case():
    """K = 17 on a model with peaked attention (sharp_models level ``medium``: the project's bars hold)"""
    K, N, dim = 17, 5, 4
    m, w64 = MO.model(32, 2, K, SHARP_SEED, sharp=SHARP_LEVEL)
    rs = np.random.RandomState(0)
    goals = rs.randint(0, dim, (N, 2)).astype(np.int32)
    u = rs.uniform(size=(K - 1, N))
    return m, w64, goals, u, True, dim, 2, MO.episode(w64, 2, goals, K, dim, True, u)


@functools.lru_cache(maxsize=None)
def unpermuted_control():
    """the permuted records case's inputs run through the oracle WITHOUT the permutation: what the permuted
    device records must differ from"""
    _, w64, u, _, _ = MO.records_case(32, True)
    return MO.episode(w64, MO.REC_L, MO.REC_GOALS, MO.REC_K, MO.REC_DIM, True, u, None)
