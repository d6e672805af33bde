"""Poisoned ``torch.empty``: a test helper (not a conftest, no fixtures) for the promise of
include/dpt_hip.h that workspaces and outputs need no initialisation.

``poisoned_empty(pattern)`` replaces ``torch.empty``, ``torch.empty_like`` and ``Tensor.new_empty`` while
it is active: each allocates as before and then fills the tensor's bytes with ``pattern``, so every
workspace and output the bindings allocate starts from known dirt instead of whatever the allocator
handed back.  The log of what was handed out lets a test assert that a binding really got dirty memory.

Patterns: 0x00 (what a fresh process mostly sees), 0xFF (fp32 / fp64 NaN, int32 -1) and 0x7F (fp32
3.39e38, fp64 1.4e306, int32 2139062143: finite, so sums overflow where a product with 0 would hide)."""
import contextlib
from collections import namedtuple

import torch

PATTERNS = (0x00, 0xFF, 0x7F)

Allocation = namedtuple("Allocation", "shape dtype device data_ptr nbytes")


def fill_bytes(t, pattern):
    """Every byte of ``t`` becomes ``pattern``; zero-element and meta tensors are left alone."""
    if isinstance(t, torch.Tensor) and t.numel() and t.device.type != "meta":
        try:
            t.view(torch.uint8).fill_(pattern)
        except RuntimeError:  # strides that a byte view cannot express (empty_like of a transposed tensor)
            torch.tensor([], dtype=torch.uint8, device=t.device).set_(t.untyped_storage()).fill_(pattern)
    return t


def holds_pattern(t, pattern):
    """Whether every byte of ``t`` is ``pattern`` (one device synchronisation on a device tensor)."""
    return bool((t.contiguous().view(torch.uint8) == pattern).all().item())


class PoisonLog(list):
    """The tensors handed out while the context was active, in order."""

    def find(self, data_ptr):
        return [a for a in self if a.data_ptr == data_ptr]

    def __str__(self):
        return "\n".join(f"{tuple(a.shape)} {a.dtype} {a.device} @{a.data_ptr:#x} ({a.nbytes} B)" for a in self)


@contextlib.contextmanager
def poisoned_empty(pattern, monkeypatch=None):
    """Within the block ``torch.empty`` / ``torch.empty_like`` / ``Tensor.new_empty`` return memory whose
    bytes are all ``pattern``.  Yields the PoisonLog.  With pytest's ``monkeypatch`` the replacements are
    registered there as well (undone at the latest with the test); either way the originals are back when
    the block ends, also after an exception."""
    pattern = int(pattern)
    if not 0 <= pattern <= 0xFF:
        raise ValueError(f"pattern {pattern} is not a byte")
    log = PoisonLog()
    empty, empty_like, new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def dirty(t):
        if isinstance(t, torch.Tensor) and t.numel() and t.device.type != "meta":
            fill_bytes(t, pattern)
            log.append(Allocation(tuple(t.shape), t.dtype, t.device, t.data_ptr(), t.numel() * t.element_size()))
        return t

    def p_empty(*args, **kw):
        return dirty(empty(*args, **kw))

    def p_empty_like(*args, **kw):
        return dirty(empty_like(*args, **kw))

    def p_new_empty(self, *args, **kw):
        return dirty(new_empty(self, *args, **kw))

    def install(a, b, c):
        if monkeypatch is not None:
            monkeypatch.setattr(torch, "empty", a)
            monkeypatch.setattr(torch, "empty_like", b)
            monkeypatch.setattr(torch.Tensor, "new_empty", c)
        else:
            torch.empty, torch.empty_like, torch.Tensor.new_empty = a, b, c

    install(p_empty, p_empty_like, p_new_empty)
    try:
        yield log
    finally:
        install(empty, empty_like, new_empty)
