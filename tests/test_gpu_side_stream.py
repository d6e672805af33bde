"""'All launches are asynchronous on the given stream', 'no host synchronisation' (include/dpt_hip.h):
every entry point of the case table (tests/entry_point_cases.py) on a side stream, behind a delay.

Per case: the reference on the default stream, synchronised.  Then every device input is replaced by a
decoy (another valid input set of the same shapes and ranges; a second valid weight blob), and on a side
stream are enqueued, in this order: a delay, copies of the real inputs over the decoys, the binding under
the 0xFF poison of tests/buffer_poison.py, copies of the outputs.  Right after the binding returns the
stream must still be busy: the call did not block the host and the delay was still running, so a launch,
memset or copy issued on any other stream would have read decoys or poison.  (The only other stream the
library can name is NULL; ``side_stream`` picks a stream that is proven to run beside it.)  After the stream is
synchronised the results must equal the reference byte for byte.

The delay is calibrated in this module with events on the default stream: at least 20 ms and at least ten
times the case's own measured run time.  That is a premise which the busy-stream assert checks, not a
performance bar.  The control passes NULL as the stream of one call in the same setup and must NOT
reproduce the reference."""
import functools

import pytest
import torch

import buffer_poison as BP
import entry_point_cases as EC

pytestmark = pytest.mark.gpu

CASES = [c for c in EC.build() if c.side]
MIN_DELAY_MS, DELAY_FACTOR = 20.0, 10.0


@functools.lru_cache(maxsize=None)
def cycles_per_ms():
    """torch.cuda._sleep's cycle count per millisecond, measured with events on the default stream"""
    torch.cuda._sleep(1_000_000)  # warm-up
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20_000_000
    a.record()
    torch.cuda._sleep(n)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    assert ms > 0.5, f"torch.cuda._sleep({n}) took {ms} ms: no usable delay"
    return n / ms


def delay(ms):
    """enqueue ``ms`` milliseconds of spinning on the current stream (chunks below 2^31 cycles)"""
    left = int(ms * cycles_per_ms())
    while left > 0:
        step = min(left, 1_000_000_000)
        torch.cuda._sleep(step)
        left -= step


@functools.lru_cache(maxsize=None)
def side_stream():
    """A stream that provably runs beside the default (NULL) stream.  The runtime multiplexes its streams
    onto a few hardware queues (four by default), and a stream that shares the NULL stream's queue would
    run a wrongly NULL-streamed launch in submission order, i.e. correctly, and hide it.  So each candidate
    is probed: with a delay pending on it, a small operation on the default stream must complete while the
    candidate is still busy."""
    x = torch.zeros(64, device="cuda")
    for _ in range(8):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            delay(MIN_DELAY_MS)
        x.add_(1)
        done = torch.cuda.Event()
        done.record()
        beside = False
        while not s.query():  # at most the delay
            if done.query():
                beside = True
                break
        torch.cuda.synchronize()
        if beside:
            return s
    pytest.fail("no side stream runs beside the default stream: a launch on the NULL stream could not be told apart")


def reference(case):
    """(the outputs' bytes, the run time in ms) on the default stream; the first run warms up"""
    def once():
        inp = case.inputs(0)
        obj = case.prepare(inp) if case.prepare else None
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = case.call(obj, inp, lambda t: None)
        b.record()
        torch.cuda.synchronize()
        return EC.as_bytes(out), a.elapsed_time(b)
    once()
    return once()


def on_side_stream(case, run_ms, call=None):
    """the four steps of the module docstring; returns (the results' bytes, whether the stream was still busy
    when the binding returned)"""
    real, buf = case.inputs(0), case.inputs(1)
    assert set(real) == set(buf) and all(real[k].shape == buf[k].shape and real[k].dtype == buf[k].dtype for k in real)
    assert any(not torch.equal(real[k], buf[k]) for k in real), "the decoys equal the real inputs"
    obj = case.prepare(buf) if case.prepare else None
    torch.cuda.synchronize()
    s = side_stream()
    with torch.cuda.stream(s):
        delay(max(MIN_DELAY_MS, DELAY_FACTOR * run_ms))
        for k in real:
            buf[k].copy_(real[k])
        with BP.poisoned_empty(0xFF):
            out = (call or case.call)(obj, buf, lambda t: BP.fill_bytes(t, 0xFF))
        busy = not s.query()
        res = {k: v.clone() for k, v in out.items() if v is not None}
    s.synchronize()
    torch.cuda.synchronize()
    return EC.as_bytes(res), busy


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_side_stream_behind_a_delay(case):
    with case.tuning():
        ref, run_ms = reference(case)
        got, busy = on_side_stream(case, run_ms)
    assert busy, (f"the stream was idle when the binding returned (run time {run_ms:.2f} ms): the call blocked "
                  f"the host, or the delay was too short to prove anything")
    diff = EC.same_bytes(ref, got)
    assert not diff, f"{diff} differ from the default-stream reference: a launch, memset or copy off the given stream"


def _select_case(stream_arg):
    """dpt_select_action through ctypes; ``stream_arg()`` gives the stream argument at call time"""
    from dpt_hip import _lib
    N, A = 70, 5

    def inputs(seed):
        rs = EC.rs_of(seed, 9)
        return dict(logits=EC.f32(rs.normal(size=(N, A))), uniforms=EC.f64(rs.uniform(size=N)))

    def call(obj, inp, dirty):
        out = torch.empty(N, dtype=torch.int32, device="cuda")
        _lib.call("dpt_select_action", EC._p(inp["logits"]), N, A, 1, 1.0, EC._p(inp["uniforms"]), 0, 0,
                  0, EC._p(out), stream_arg())
        return dict(actions=out)
    return EC.Case("select_action-ctypes", inputs, call)


def test_a_call_on_the_null_stream_is_caught():
    """the control: the same setup with the stream argument NULL (the launch runs at once on the default
    stream, on the decoy logits, and the poison fill of its output lands afterwards) does not reproduce the
    reference; with the current stream it does"""
    good = _select_case(EC._stream)
    ref, run_ms = reference(good)
    got, busy = on_side_stream(good, run_ms)
    assert busy and not EC.same_bytes(ref, got)
    bad = _select_case(lambda: None)
    got, busy = on_side_stream(bad, run_ms)
    assert busy
    assert EC.same_bytes(ref, got) == ["actions"], "a launch on the wrong stream went unnoticed"
