"""Poisoned, guard-banded allocations for the GPU tests: what a kernel did not write in THIS launch, or wrote beside its
buffer, becomes visible.

The Python entry points (quantization/mxnet_amd/ops.py) take every output, statistic target and workspace from
`torch.empty` / `torch.empty_like`, and torch's caching allocator hands a freed block straight back to the next request of
the same size - so the memory a launch writes into usually still holds the right answer of the launch before it.  `Proxy`
stands in for the `torch` module inside `ops` for one test:

    proxy = poison.Proxy(0xFF)
    monkeypatch.setattr(ops, "torch", proxy)
    ops._WS.clear()
    ... run the case, compare with the reference as always ...
    torch.cuda.synchronize()
    proxy.guards_intact()

Everything but `empty` and `empty_like` is forwarded.  Those two allocate one flat uint8 buffer laid out as
guard | body | guard, fill ALL of it with the byte pattern and return the body as a contiguous view of the requested
dtype and shape.  Guards are a multiple of 256 bytes (every alignment-based kernel choice stays the one the plain call
makes), at least the tensor's own size (a ragged channel tile overruns by whole planes), at least 4 KiB, at most 4 MiB.

Two patterns, every case runs under both (`PATTERNS`):
    0xFF  fp32 NaN, int32 -1, int8 -1, the largest value under an unsigned-bit maximum;
    0x7F  fp32 3.39e38 (finite), int8 127 (a legal code), int32 2139062143 - `fmax`-style statistics swallow a NaN.

`guarded(array, device)` places a test INPUT in such a buffer: a read past either end returns poison, not a neighbour.
"""
import numpy as np
import torch as _torch

PATTERNS = (0xFF, 0x7F)
GUARD_ALIGN = 256
GUARD_MIN = 4 << 10
GUARD_MAX = 4 << 20


class GuardError(AssertionError):
    pass


def guard_bytes(nbytes):
    """Size of each guard band of a body of `nbytes`."""
    g = min(max(int(nbytes), GUARD_MIN), GUARD_MAX)
    return (g + GUARD_ALIGN - 1) // GUARD_ALIGN * GUARD_ALIGN


def _shape_of(size):
    if len(size) == 1 and isinstance(size[0], (tuple, list, _torch.Size)):
        size = tuple(size[0])
    return tuple(int(d) for d in size)


class Proxy(object):
    """The `torch` module with poisoned, guard-banded `empty` / `empty_like` (module docstring)."""

    def __init__(self, pattern):
        if not 0 <= int(pattern) <= 0xFF:
            raise ValueError("the pattern is one byte")
        self.pattern = int(pattern)
        self.records = []            # (raw uint8 buffer, guard bytes, body bytes, dtype, shape, what)

    def __getattr__(self, name):     # only reached for what the instance does not define itself
        return getattr(_torch, name)

    # ---- allocation --------------------------------------------------------------------------------------------------------
    def _alloc(self, shape, dtype, device, what):
        dtype = _torch.get_default_dtype() if dtype is None else dtype
        item = _torch.empty(0, dtype=dtype).element_size()
        numel = 1
        for d in shape:
            numel *= d
        body = numel * item
        g = guard_bytes(body)
        # the body's size rounded up so that the trailing guard starts on an element boundary of every dtype
        span = (body + 15) // 16 * 16
        raw = _torch.full((g + span + g,), self.pattern, dtype=_torch.uint8, device=device)
        view = raw[g:g + body].view(dtype).view(shape)
        assert view.is_contiguous() and view.data_ptr() % 16 == 0
        self.records.append((raw, g, body, dtype, shape, what))
        return view

    def empty(self, *size, dtype=None, device=None):
        return self._alloc(_shape_of(size), dtype, device, "empty")

    def empty_like(self, t, dtype=None, device=None):
        return self._alloc(tuple(t.shape), t.dtype if dtype is None else dtype, t.device if device is None else device,
                           "empty_like")

    def guarded(self, array, device):
        """A test input in a guard-banded buffer of its own: the array's values between two bands of poison."""
        src = array if isinstance(array, _torch.Tensor) else _torch.from_numpy(np.ascontiguousarray(array))
        view = self._alloc(tuple(src.shape), src.dtype, device, "input")
        view.copy_(src)
        return view

    # ---- checks ------------------------------------------------------------------------------------------------------------
    def first_broken_guard(self):
        """None, or a description of the first buffer (in allocation order) one of whose guard bytes changed."""
        for order, (raw, g, body, dtype, shape, what) in enumerate(self.records):
            host = raw.cpu().numpy()
            for name, lo, hi in (("before", 0, g), ("after", g + body, host.size)):
                bad = np.flatnonzero(host[lo:hi] != self.pattern)
                if bad.size:
                    at = int(bad[0]) + lo - g                     # relative to the body's first byte
                    return ("allocation #%d (%s, %s, shape %s, %d bytes): guard %s the body changed, first at byte offset %d "
                            "of the body (%d bytes %s), 0x%02X -> 0x%02X, %d guard bytes changed in all"
                            % (order, what, str(dtype).replace("torch.", ""), shape, body, name, at,
                               -at if at < 0 else at - body + 1, "before its start" if at < 0 else "past its end",
                               self.pattern, int(host[lo:hi][bad[0]]), int(bad.size)))
        return None

    def guards_intact(self):
        """True when no guard byte of any allocation changed; raises GuardError naming the first buffer otherwise.
        Synchronise the device first."""
        msg = self.first_broken_guard()
        if msg is not None:
            raise GuardError(msg)
        return True

    def release(self):
        """Forget the buffers (after the check): the next case starts from fresh, freshly poisoned memory."""
        del self.records[:]
