"""The fresh-task entry points (dpt_fresh_batch, dpt_fresh_step, dpt_fresh_eval_loss) under the regime of
tests/test_gpu_dirty_buffers.py and tests/test_gpu_side_stream.py: the three fill patterns of
tests/buffer_poison.py (every ``torch.empty`` of the bindings and the trainer's persistent ``_ws``), and a
side stream behind a delay with decoy inputs.  Identical bytes are required; the runners are those modules'."""
import functools

import numpy as np
import pytest
import torch

import entry_point_cases as EC
from test_gpu_dirty_buffers import run_case
from test_gpu_side_stream import on_side_stream, reference

pytestmark = pytest.mark.gpu

DIM, H_ROOM, H_BANDIT, A = 6, 40, 300, 5  # H 300: the lanes take a second chunk of steps


def room_inputs(seed):
    rs = EC.rs_of(seed, 41)
    return dict(goals=EC.i32(rs.randint(0, DIM, (7, 2))), perms=EC.i32(np.stack([rs.permutation(5) for _ in range(6)])))


def room_env(inp, H):
    import dpt_hip
    env = dpt_hip.FreshEnv.darkroom(DIM, H, inp["goals"], inp["perms"])
    assert env.goals.data_ptr() == inp["goals"].data_ptr() and env.perms.data_ptr() == inp["perms"].data_ptr()
    return env


def batch_room_call(obj, inp, dirty):
    import dpt_hip
    return dpt_hip.fresh_batch(room_env(inp, H_ROOM), 31, 2 ** 33 + 5, 5)


def batch_bandit_call(obj, inp, dirty):
    import dpt_hip
    return dpt_hip.fresh_batch(dpt_hip.FreshEnv.bandit(A, H_BANDIT, 0.3, "uniform"), 32, 3, 3)


def trainer_case(kind):
    from dpt_hip import train as tr
    Hm = 12 if kind == "bandit" else 9
    sd = 1 if kind == "bandit" else 2
    model = functools.partial(EC.transformer, 32, 2, Hm, sd, A, 130 + sd)

    def inputs(seed):
        inp = dict(blob=EC.blob_of(model(), seed))
        if kind == "darkroom":
            inp.update(room_inputs(seed))
        return inp

    def prepare(inp):
        import dpt_hip
        env = dpt_hip.FreshEnv.bandit(A, Hm, 0.3, "bernoulli") if kind == "bandit" else room_env(inp, Hm)
        t = tr.FreshTrainer(model(), env, lr=1e-3, seed=33, first_task=7)
        t.state.blob = inp["blob"]
        return t

    def call(t, inp, dirty):
        t.step(8)
        dirty(t._ws)
        t.step(5)
        dirty(t._ws)
        t.eval_loss(100, 11, seed=34, batch=8)
        return dict(blob=t.blob, m=t.m, v=t.v, loss=t.loss)
    return EC.Case(f"fresh_trainer-{kind}", inputs, call, prepare)


CASES = [EC.Case("fresh_batch-darkroom", room_inputs, batch_room_call),
         EC.Case("fresh_batch-bandit", lambda seed: dict(unused=EC.i32(np.arange(4) + seed)), batch_bandit_call,
                 side=False),  # a bandit batch reads no device input: nothing a decoy could stand in for
         trainer_case("bandit"), trainer_case("darkroom")]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_results_do_not_depend_on_what_the_buffers_held(case):
    clean, log = run_case(case, 0x00)
    again, _ = run_case(case, 0x00)
    assert not EC.same_bytes(clean, again), f"not reproducible on clean buffers: {EC.same_bytes(clean, again)}"
    assert len(log) >= 1, "nothing allocated through torch.empty: the poison reached no buffer"
    for pattern in (0xFF, 0x7F):
        got, _ = run_case(case, pattern)
        diff = EC.same_bytes(clean, got)
        assert not diff, f"pattern {pattern:#04x}: {diff} differ from the run on zeroed buffers"


@pytest.mark.parametrize("case", [c for c in CASES if c.side], ids=[c.name for c in CASES if c.side])
def test_side_stream_behind_a_delay(case):
    ref, run_ms = reference(case)
    got, busy = on_side_stream(case, run_ms)
    assert busy, (f"the stream was idle when the binding returned (run time {run_ms:.2f} ms): the call blocked "
                  f"the host, or the delay was too short to prove anything")
    diff = EC.same_bytes(ref, got)
    assert not diff, f"{diff} differ from the default-stream reference: a launch, memset or copy off the given stream"
