"""Draws placed at the cdf edges of a rollout's own logits, and the check that every action a rollout
took is the action the selection rule gives for the logits it reported (a test helper, not a conftest;
shared by tests/test_selection_edges_host.py and tests/test_gpu_selection_edges.py).

The rule (include/dpt_hip.h, dpt_select_action): greedy = the first argmax of the fp32 logits; sampled =
scipy's fp32 softmax of logits / temp, numpy's fp64 cdf, searchsorted(cdf, u, 'right').  A rollout is a
callable ``rollout(u) -> dict(logits (steps, N, A) fp32, actions (steps, N)[, forwards])`` on injected
uniforms ``u`` (steps, N); a definition is a callable ``select(logits, u, sample, temp) -> (steps, N)``.

``run_case`` runs the rollout on seeded uniforms u0 (run 1), then per delta on u1 = the chosen arm's cdf
interval edge moved ``delta`` inwards (``place``).  On every run each action must equal the definition's on
the run's own logits and draws, no step left out; at least 0.9 of the task-steps are placed, both sides of
an edge occur, and with the memo on it serves at least 1/4 of the steps.

Steady deltas (1e-6 .. 1e-4): logits and actions bit-identical to run 1's; the definition on draws moved
2 delta across the edge (``control``) disagrees with the rollout at every placed step; at delta <= 2.9e-5
at least 0.9 of the placed steps lie within 2^-15 of an edge of the run's own logits.  The cdf the draws
are placed on is numpy's (oracle/dpt_oracle.softmax_f32), whose expf is not the device's: 1e-6 exceeds
what the two cdfs can differ by (a few fp32 ulp of a value <= 1, about 2e-7).  2.9e-5 and 3.2e-5 sit
1.5e-6 either side of kCdfMargin = 2^-15, cdf_fast is itself only within about 1e-6 of the exact cdf, and
nothing here observes which branch of select_fast ran: 2.5e-5 and 3.6e-5 stand beside them, further from
the band's edge than that error, so that one delta surely takes the fp64 fallback and one surely does not.

Razor deltas (1e-9, 1e-8, 1e-7) are below that distance: the side is the rollout's to decide and only the
definition check is made on the actions.  Where it decides the other side than numpy, the run leaves the
trajectory its draws were placed on, and its later draws are at no edge of its own logits.  So a razor run
is repeated (``razor_runs``): each round keeps every task's draws up to and including its first departure,
re-places the later ones on the latest run's own logits and actions, and runs again, until no task departs
or the round limit is reached.  A kept step repeats (same draws, same windows), so every round moves each
task's first departure at least one step on, and as many runs as the rollout has steps surely end with no
departure: that is the limit for rollouts of up to RAZOR_FULL = 256 steps.  A longer rollout gets
RAZOR_ROUNDS = 64 runs, to keep its test to a few seconds.  Asserted on the last run: at 1e-7, and at 1e-9
and 1e-8 on every rollout of up to 256 steps, the in-band share of the issue, >= 0.9 of the placed steps; on
longer rollouts at 1e-9 and 1e-8, where the device falls the other way too often for 64 rounds to reach the
end (a round moves a task on by two to seven steps; the shares reached are printed), the bound the
construction does guarantee: every placed task-step up to and including each task's first departure
is within 2^-15 of an edge of the run's own logits, and each task has at least as many such steps as
runs were made (or all its steps)."""
import collections

import numpy as np

from oracle import dpt_oracle as O

STEADY = (1e-6, 1e-5, 2.5e-5, 2.9e-5, 3.2e-5, 3.6e-5, 1e-4)
RAZOR = (1e-9, 1e-8, 1e-7)
BAND = 2.0 ** -15  # kCdfMargin (csrc/dpt_common.h): nearer than this to an edge the exact fp64 cdf decides
U_MAX = 1.0 - 2.0 ** -53
MIN_SHARE = 0.9
MIN_MEMO = 0.25
RAZOR_FULL = 256  # rollouts of up to this many steps get as many razor runs as steps: they end with no departure
RAZOR_ROUNDS = 64  # runs of one razor delta on a longer rollout (each costs a whole rollout)

Placement = collections.namedtuple("Placement", "u placed upper")


def cdf(logits, temp):
    """numpy's fp64 cdf of the fp32 softmax of logits / temp (oracle choice_from_uniform's)"""
    c = np.cumsum(O.softmax_f32(logits, temp).astype(np.float64), axis=-1)
    return c / c[..., -1:]


def place(logits, actions, u0, temp, delta, seed):
    """u1 (steps, N): inside the interval [lo, hi) of the arm ``actions`` chose, ``delta`` from its upper
    edge or its lower one by a seeded coin (arm 0: always the upper, arm A - 1: always the lower, so
    only interior edges); a step whose interval is no wider than 4 delta keeps u0 and is not placed."""
    c = cdf(logits, temp)
    A = c.shape[-1]
    a = np.asarray(actions, np.int64)
    hi = np.take_along_axis(c, a[..., None], -1)[..., 0]
    lo = np.where(a > 0, np.take_along_axis(c, np.maximum(a - 1, 0)[..., None], -1)[..., 0], 0.0)
    coin = np.random.RandomState(seed).randint(0, 2, a.shape).astype(bool)
    upper = np.where(a == 0, True, np.where(a == A - 1, False, coin))
    placed = hi - lo > 4 * delta
    u1 = np.where(placed, np.where(upper, hi - delta, lo + delta), u0)
    return Placement(np.clip(u1, 0.0, U_MAX), placed, upper)


def control(pl, delta):
    """the draws of ``pl`` with every placed one moved 2 delta across its edge"""
    moved = np.where(pl.upper, pl.u + 2 * delta, pl.u - 2 * delta)
    return np.clip(np.where(pl.placed, moved, pl.u), 0.0, U_MAX)


def in_band(logits, u, temp):
    """(steps, N) bool: the draw lies within 2^-15 of an interior edge of these logits' cdf"""
    return O.boundary_margin(O.softmax_f32(logits, temp), u) <= BAND


def oracle_select(logits, u, sample, temp):
    """the definition in numpy (the host file's; the GPU file uses the per-step kernel's fp64 path)"""
    return O.select_actions(logits, u, sample, temp=temp if sample else None)


def memo_share(run):
    """share of the steps that needed no forward (``forwards``: window forwards per task and episode)"""
    steps = run["actions"].size
    return 1.0 - float(np.asarray(run["forwards"]).sum()) / steps


def definition_mismatches(run, u, select, sample, temp):
    """item 1: the (step, task) pairs whose action is not the definition's for the run's own logits and draws"""
    want = np.asarray(select(run["logits"], u, sample, temp))
    return np.argwhere(want != np.asarray(run["actions"]))


def _same(a, b):
    return (np.array_equal(a["actions"], b["actions"])
            and np.array_equal(a["logits"].view(np.int32), b["logits"].view(np.int32)))


def razor_runs(rollout, select, run1, u0, temp, delta, seed, problems, tag, rounds=RAZOR_ROUNDS):
    """The razor rounds of the module docstring.  Returns (last run, its draws, placed, upper, prefix: the
    task-steps up to and including each task's first departure from the run its draws were placed on, the
    runs made, whether the last one departed nowhere, the definition mismatches over all runs, whether any
    run departed)."""
    steps, N = u0.shape
    step = np.arange(steps)[:, None]
    base, u_base, frozen = run1, u0, np.zeros(N, np.int64)
    placed = upper = None
    mismatches, departed = 0, False
    for made in range(1, rounds + 1):
        pl = place(base["logits"], base["actions"], u_base, temp, delta, seed)  # one coin per (step, task)
        keep = step < frozen[None, :]
        u = np.where(keep, u_base, pl.u)
        placed = pl.placed if placed is None else np.where(keep, placed, pl.placed)
        upper = pl.upper if upper is None else np.where(keep, upper, pl.upper)
        run = rollout(u)
        bad = definition_mismatches(run, u, select, True, temp)
        mismatches += len(bad)
        if len(bad):
            problems.append((tag, f"run {made}: selection differs from its definition at (step, task)",
                             bad[:8].tolist()))
        moved = np.asarray(run["actions"]) != np.asarray(base["actions"])
        depart = np.where(moved.any(0), moved.argmax(0), steps)
        if not (depart >= frozen).all():
            problems.append((tag, f"run {made}: a kept step did not repeat",
                             np.nonzero(depart < frozen)[0][:8].tolist()))
        prefix = step <= depart[None, :]
        converged = bool((depart == steps).all())
        departed = departed or not converged
        if converged:
            break
        base, u_base, frozen = run, u, np.minimum(depart + 1, steps)
    return run, u, placed, upper, prefix, made, converged, mismatches, departed


def run_case(label, rollout, select, u0, temp=1.0, seed=0, memo=False, deltas=STEADY + RAZOR, rounds=None):
    """Run 1 on u0 and the runs of every delta with the assertions of the module docstring, all collected and
    raised after the last line is printed.  Returns the record lines of the case
    (profiles/selection_edges/summary.txt), which it also prints."""
    problems, lines = [], []

    def need(ok, *what):
        if not ok:
            problems.append(what)

    run1 = rollout(u0)
    bad = definition_mismatches(run1, u0, select, True, temp)
    need(not len(bad), f"{label} run 1", "selection differs from its definition at (step, task)", bad[:8].tolist())
    steps = u0.shape[0]
    if rounds is None:
        rounds = steps if steps <= RAZOR_FULL else RAZOR_ROUNDS
    differs_at = None  # the steady delta at which run 2 first left run 1's trajectory
    flipped = 0.0  # the largest razor delta at which a step fell the other way on the logits its draw was placed on
    for i, delta in enumerate(deltas):
        steady = delta in STEADY
        tag = f"{label} delta {delta:g}"
        if steady:
            pl = place(run1["logits"], run1["actions"], u0, temp, delta, seed + 101 * i)
            run2, u, placed_at, upper = rollout(pl.u), pl.u, pl.placed, pl.upper
            bad = definition_mismatches(run2, u, select, True, temp)
            need(not len(bad), tag, "selection differs from its definition at (step, task)", bad[:8].tolist())
            mismatches, extra = len(bad), ""
        else:
            run2, u, placed_at, upper, prefix, made, converged, mismatches, departed = razor_runs(
                rollout, select, run1, u0, temp, delta, seed + 101 * i, problems, tag, rounds)
            if departed:
                flipped = max(flipped, delta)
        placed = float(placed_at.mean())
        band_at = in_band(run2["logits"], u, temp)
        band = float(band_at[placed_at].mean()) if placed_at.any() else 0.0
        same = _same(run2, run1)
        served = memo_share(run2) if run2.get("forwards") is not None else float("nan")
        need(placed >= MIN_SHARE, tag, "placed share", placed)
        need((upper & placed_at).any() and (~upper & placed_at).any(), tag, "one side of the edges only")
        if memo:
            need(served >= MIN_MEMO, tag, "memo-served share", served)
        if steady:
            if delta <= 2.9e-5:
                need(band >= MIN_SHARE, tag, "in-band share of the placed steps", band)
            if not same and differs_at is None:
                differs_at = delta
            need(same, tag, "run 2 left run 1's trajectory: the numpy cdf is further from the rollout's decision "
                            "boundary than this delta")
            ctl = np.asarray(select(run2["logits"], control(pl, delta), True, temp))
            agree = (ctl == np.asarray(run2["actions"])) & placed_at
            need(not agree.any(), tag, "the control agrees at placed (step, task)", np.argwhere(agree)[:8].tolist())
        else:
            on_prefix = prefix & placed_at
            extra = f" runs={made} departs_nowhere={int(converged)} prefix_share={float(prefix.mean()):.4f}"
            if delta >= 1e-7 or steps <= rounds:
                need(band >= MIN_SHARE, tag, "in-band share of the placed steps", band)
            else:
                need(band_at[on_prefix].all(), tag, "a step up to a task's first departure is not in band")
                short = np.nonzero(prefix.sum(0) < min(steps, made))[0]
                need(not short.size, tag, "tasks with fewer steps up to their first departure than runs made",
                     short[:8].tolist())
        line = (f"SELECTION-EDGES {label} delta={delta:g} placed={placed:.4f} in_band={band:.4f} "
                f"memo_served={served:.4f} mismatches={mismatches}{extra} same_as_run1={int(same)}")
        print(line)
        lines.append(line)
    bound = (f"SELECTION-EDGES {label} boundary: |numpy cdf - decision boundary| "
             + (f">= {flipped:g}" if flipped else "showed at no razor delta")
             + (f", >= {differs_at:g} (steady run differs)" if differs_at else f", < {min(STEADY):g}"))
    print(bound)
    lines.append(bound)
    assert not problems, problems[:6]
    return lines


def run_greedy(label, rollout, select, u0):
    """one greedy run: every action is the first argmax of the run's own logits (the draws are not read)"""
    run = rollout(u0)
    bad = definition_mismatches(run, u0, select, False, 1.0)
    line = f"SELECTION-EDGES {label} greedy mismatches={len(bad)}"
    print(line)
    assert not len(bad), (label, "greedy selection differs from the first argmax at (step, task)", bad[:8].tolist())
    return [line]
