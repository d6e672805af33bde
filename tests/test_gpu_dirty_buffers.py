"""Workspaces and outputs need no initialisation (include/dpt_hip.h, Conventions): every entry point of the
case table (tests/entry_point_cases.py) gives the same bytes whatever its buffers held before the call.

Each case runs under tests/buffer_poison.py with every ``torch.empty`` / ``empty_like`` / ``new_empty``
of the bindings filled with 0x00 (twice: the path must first be reproducible on clean buffers), 0xFF (NaN,
int32 -1) and 0x7F (3.39e38, int32 2139062143); workspaces the caller owns (the rollout's kvcache, the
ctypes-level training forward, the regret statistics) and the trainers' persistent ``_ws`` (before the
second, smaller step and again before the test loss) are filled directly as well.  Every returned tensor
must be identical byte for byte (compared as uint8: NaN != NaN), which also proves that every documented
output element is written.  No tolerance: a difference names a load of a word the call did not write.

Integer words: the workspace words a kernel turns into an address were read in the kernels before they
were poisoned -- the bandit rollout's token records (arm index: written for every live task before the
position is attended, partial tiles masked; the table it indexes lives in LDS), the explorer's per-row
targets and the DarkRoom trainer's int64 targets (written for all rows by the launch before the
cross-entropy, which ignores a target outside [0, A)).  The classical policies' counters and the episode
rollout's records live in LDS, not in a workspace.  So no region is left unpoisoned."""
import ctypes

import pytest
import torch

import buffer_poison as BP
import entry_point_cases as EC

pytestmark = pytest.mark.gpu

CASES = EC.build()


def run_case(case, pattern):
    """(the outputs' bytes, the helper's log) of one run with every buffer holding ``pattern``"""
    with case.tuning():
        inp = case.inputs(0)
        torch.cuda.synchronize()
        with BP.poisoned_empty(pattern) as log:
            obj = case.prepare(inp) if case.prepare else None
            out = case.call(obj, inp, lambda t: BP.fill_bytes(t, pattern))
            assert isinstance(out, dict) and out
        torch.cuda.synchronize()
        return EC.as_bytes(out), log


@pytest.mark.parametrize("case", CASES, ids=EC.ids())
def test_results_do_not_depend_on_what_the_buffers_held(case):
    clean, log = run_case(case, 0x00)
    again, _ = run_case(case, 0x00)
    assert not EC.same_bytes(clean, again), f"not reproducible on clean buffers: {EC.same_bytes(clean, again)}"
    # dpt_adamw_step updates its three arrays in place: no workspace, no output buffer
    assert len(log) >= 1 or case.name == "adamw_step", "nothing allocated through torch.empty: the poison reached no buffer"
    for pattern in (0xFF, 0x7F):
        got, _ = run_case(case, pattern)
        diff = EC.same_bytes(clean, got)
        assert not diff, f"pattern {pattern:#04x}: {diff} differ from the run on zeroed buffers"


def test_the_case_table_can_fail():
    """an output element the 'binding' leaves unwritten, and a workspace word read before it is written,
    both show up as differing bytes"""
    def call(obj, inp, dirty):
        out = torch.empty(8, dtype=torch.float32, device="cuda")
        out[:7] = inp["x"][:7]  # the last element is never written
        ws = torch.empty(8, dtype=torch.float32, device="cuda")  # never written: 0 * sum is 0, NaN or 0 * inf
        return dict(unwritten=out, stale_read=inp["x"] + 0 * ws.sum())
    case = EC.Case("control", lambda seed: dict(x=torch.arange(8, dtype=torch.float32, device="cuda")), call)
    clean, _ = run_case(case, 0x00)
    assert not EC.same_bytes(clean, run_case(case, 0x00)[0])
    assert EC.same_bytes(clean, run_case(case, 0xFF)[0]) == ["stale_read", "unwritten"]
    assert EC.same_bytes(clean, run_case(case, 0x7F)[0]) == ["stale_read", "unwritten"]


@pytest.mark.parametrize("pattern", [0xFF, 0x7F])
def test_the_bindings_really_receive_poisoned_workspaces(pattern):
    """the control of the issue: the workspace handed to rollout_bandit and to dpt_train_forward held the
    pattern before the call (read back, and listed in the helper's log), and the results are those of
    zeroed workspaces"""
    from dpt_hip import _lib
    from dpt_hip import train as tr
    m = EC.golden_model("bandit5")[0]
    N, H = 9, 70
    inp = EC._bandit_inputs(N, H, 5, 3)(0)
    outs = []
    for pat in (0x00, pattern):
        with BP.poisoned_empty(pat) as log:
            kv = torch.empty(m.kv_numel(N, H), dtype=torch.float32, device="cuda")
            assert BP.holds_pattern(kv, pat)
            o = m.rollout_bandit(inp["means"], H, 0.3, True, uniforms=inp["uniforms"], noise=inp["noise"],
                                 want_logits=True, kvcache=kv)
        hit = log.find(kv.data_ptr())
        assert hit and hit[0].nbytes == 4 * m.kv_numel(N, H) and hit[0].dtype == torch.float32
        # the outputs went through the helper too
        assert all(log.find(o[k].data_ptr()) for k in EC.BANDIT_OUT)
        torch.cuda.synchronize()
        assert not BP.holds_pattern(kv, pat) or pat == 0  # the rollout wrote its cache
        outs.append(EC.as_bytes({k: o[k] for k in EC.BANDIT_OUT}))
    assert not EC.same_bytes(*outs)

    E, T, B = 32, 17, 3
    model = EC.transformer(E, EC.L_TR, T - 1, EC.SD, EC.A_TR, 50 + E, 0.0)
    blob = EC.blob_of(model, 0)
    tokens = EC.f32(EC._tokens(EC.rs_of(0, 19), B, T))
    d = tr.desc(EC.L_TR, E, EC.SD, EC.A_TR, 4 * T, B, T)
    outs = []
    for pat in (0x00, pattern):
        with BP.poisoned_empty(pat) as log:
            ws = torch.empty(tr._numel("dpt_train_workspace_numel", d), dtype=torch.float32, device="cuda")
            preds = torch.empty((B, T, EC.A_TR), dtype=torch.float32, device="cuda")
        assert BP.holds_pattern(ws, pat) and BP.holds_pattern(preds, pat)
        assert log.find(ws.data_ptr()) and log.find(preds.data_ptr())
        _lib.call("dpt_train_forward", ctypes.byref(d), EC._p(blob), EC._p(tokens), EC._p(ws), EC._p(preds),
                  EC._stream())
        torch.cuda.synchronize()
        outs.append(EC.as_bytes(dict(preds=preds)))
    assert not EC.same_bytes(*outs)
