"""tests/buffer_poison.py on the CPU: the replaced allocators hand out the pattern for every dtype the
bindings allocate, the originals come back (also after an exception), and the log lists what went out."""
import numpy as np
import pytest
import torch

import buffer_poison as BP

DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8)
ORIG = (torch.empty, torch.empty_like, torch.Tensor.new_empty)


def _restored():
    return (torch.empty, torch.empty_like, torch.Tensor.new_empty) == ORIG


@pytest.mark.parametrize("pattern", BP.PATTERNS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_every_allocator_hands_out_the_pattern(pattern, dtype):
    like = torch.zeros((3, 5), dtype=dtype)
    with BP.poisoned_empty(pattern) as log:
        got = [torch.empty((4, 7), dtype=dtype), torch.empty(11, dtype=dtype, device="cpu"),
               torch.empty_like(like), like.new_empty((2, 3)), torch.empty_like(like.t())]
        assert torch.empty is not ORIG[0]
    assert _restored()
    for t in got:
        assert t.dtype == dtype
        assert (t.contiguous().view(torch.uint8).numpy() == pattern).all()
        assert BP.holds_pattern(t, pattern)
    assert [a.data_ptr for a in log] == [t.data_ptr() for t in got]
    assert [a.shape for a in log] == [tuple(t.shape) for t in got]
    assert all(a.dtype == dtype for a in log)


def test_the_patterns_are_the_values_the_kernels_would_read():
    with BP.poisoned_empty(0xFF):
        f, d, i = (torch.empty(3, dtype=t) for t in (torch.float32, torch.float64, torch.int32))
    assert torch.isnan(f).all() and torch.isnan(d).all() and (i == -1).all()
    with BP.poisoned_empty(0x7F):
        f, d, i = (torch.empty(3, dtype=t) for t in (torch.float32, torch.float64, torch.int32))
    assert torch.isfinite(f).all() and (f > 3.3e38).all()
    assert torch.isfinite(d).all() and (d > 1.3e306).all()
    assert (i == 2139062143).all()
    with BP.poisoned_empty(0x00):
        f, i = torch.empty(3, dtype=torch.float32), torch.empty(3, dtype=torch.int64)
    assert not f.any() and not i.any()


def test_zero_element_and_meta_tensors_are_left_alone():
    with BP.poisoned_empty(0xFF) as log:
        z = torch.empty((0, 4), dtype=torch.float32)
        m = torch.empty((3, 4), device="meta")
        k = torch.empty(2, dtype=torch.float32)
    assert z.numel() == 0 and m.device.type == "meta" and tuple(m.shape) == (3, 4)
    assert len(log) == 1 and log[0].data_ptr == k.data_ptr() and log[0].nbytes == 8


def test_an_exception_inside_restores_the_originals():
    with pytest.raises(KeyError):
        with BP.poisoned_empty(0x7F):
            assert not _restored()
            raise KeyError("boom")
    assert _restored()
    # nested contexts unwind in order; the inner pattern wins while it is active
    with BP.poisoned_empty(0x00):
        with BP.poisoned_empty(0xFF):
            assert torch.isnan(torch.empty(2)).all()
        assert not torch.empty(2).any()
    assert _restored()


def test_with_monkeypatch(monkeypatch):
    with BP.poisoned_empty(0xFF, monkeypatch) as log:
        assert torch.isnan(torch.empty(5)).all()
    assert _restored() and len(log) == 1


def test_the_log_lists_the_allocations(capsys):
    with BP.poisoned_empty(0x7F) as log:
        torch.empty((2, 3), dtype=torch.float64)
        torch.empty(4, dtype=torch.int32)
    text = str(log)
    print(text)
    assert len(log) == 2 and len(log.find(log[1].data_ptr)) >= 1
    assert "(2, 3) torch.float64" in text and "(4,) torch.int32" in text and "(48 B)" in text
    assert "torch.int32" in capsys.readouterr().out


def test_fill_bytes_and_pattern_check():
    t = torch.arange(6, dtype=torch.float32)
    BP.fill_bytes(t, 0x7F)
    assert BP.holds_pattern(t, 0x7F) and not BP.holds_pattern(t, 0xFF)
    assert np.frombuffer(t.numpy().tobytes(), np.uint8).tolist() == [0x7F] * 24
    with pytest.raises(ValueError):
        with BP.poisoned_empty(256):
            pass
