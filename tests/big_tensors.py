"""Helpers of tests/test_gpu_big_tensors.py: tensors past the 2 GiB and 4 GiB limits of 32-bit byte offsets, buffer resources and
element indices ("Large tensors").

What a case is made of:

* Inputs drawn ON THE DEVICE from a seeded `torch.Generator`, piece by piece (`PIECE` bytes at most, whole samples): a wrapped
  offset reads or writes another sample of the same tensor, so every sample differs from every other, and `Drawn.replay()` draws
  the same pieces again one at a time - the sub-batch launches of an in-place call need the input the large launch overwrote.
* Outputs, statistic targets and workspaces of the large launch from tests/poison.py's proxy (0xFF): a store that was skipped
  reads back as NaN / -1 and fails the comparison, a store outside the tensor changes a guard band.  The bands are checked on the
  device here (`guards_intact`): the proxy's own check copies whole buffers to the host.
* Reference 1, independent of the library: the host twin or the numpy oracle on `picks()` - sample 0, sample n - 1 and, for every
  tensor of the case that contains byte 2^31 or 2^32, the sample holding that byte and both its neighbours.
* Reference 2, the whole tensor: the same entry point on `pieces()` - consecutive sub-batches of at most 256 MB, sizes the rest of
  the suite holds against the oracle - each into a small output of its own, compared on the device with `torch.equal`.
* `bounded()`: the case's peak of allocated device memory stays at or below 16 GiB - a condition on the shapes chosen, not a
  measurement - and the case starts only with 24 GiB free.
"""
import contextlib

import numpy as np
import pytest
import torch

GIB = 1 << 30
BOUNDARIES = (1 << 31, 1 << 32)
PIECE = 256 << 20
PEAK_MAX = 16 * GIB
FREE_MIN = 24 * GIB


def need_free_memory():
    """Skip - before anything else of a case runs - below 24 GiB of free device memory."""
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < FREE_MIN:
        pytest.skip("%.1f GiB of device memory free, the large-tensor cases want 24" % (free / GIB))


class Sink(object):
    """A histogram sink as distribution_calibrate keeps one per collected block: range, counts, negatives."""

    def __init__(self, bins, mx_, dev):
        self.fm_max = torch.tensor([mx_], dtype=torch.float32, device=dev)
        self.hist = torch.zeros(bins, dtype=torch.int64, device=dev)
        self.neg = torch.zeros(1, dtype=torch.int32, device=dev)


def pieces(n, sample_bytes, limit=PIECE):
    """[(lo, hi)]: consecutive runs of whole samples, each at most `limit` bytes of a tensor with `sample_bytes` per sample
    (`sample_bytes`: a number or several - the largest decides)."""
    per = max(sample_bytes) if isinstance(sample_bytes, (tuple, list)) else sample_bytes
    step = max(1, int(limit // per))
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


def picks(n, sample_bytes):
    """Sorted samples for reference 1.  `sample_bytes`: bytes per sample of every tensor of the case (input, residual, workspace,
    output)."""
    sel = {0, n - 1}
    for b in sample_bytes:
        for edge in BOUNDARIES:
            if edge < n * b:
                s = edge // b
                sel.update(t for t in (s - 1, s, s + 1) if 0 <= t < n)
    return sorted(sel)


def crossed(n, sample_bytes):
    """The boundaries some tensor of the case contains: a case that names a boundary asserts it is really there."""
    return sorted({edge for b in sample_bytes for edge in BOUNDARIES if edge < n * b})


class Drawn(object):
    """A (n, ...) fp32 tensor of standard normals times `scale` (post-ReLU unless `signed`), drawn piece by piece."""

    def __init__(self, shape, dev, seed, signed=False, scale=2.0):
        self.shape, self.dev, self.seed, self.signed, self.scale = tuple(shape), dev, seed, signed, scale
        self.sample_bytes = 4 * int(np.prod(self.shape[1:]))
        self.t = torch.empty(self.shape, dtype=torch.float32, device=dev)
        for lo, hi, piece in self.replay():
            self.t[lo:hi] = piece

    def replay(self):
        """(lo, hi, values of samples lo .. hi - 1), in order, freshly drawn into a tensor of their own."""
        g = torch.Generator(device=self.dev)
        g.manual_seed(self.seed)
        for lo, hi in pieces(self.shape[0], self.sample_bytes):
            p = torch.empty((hi - lo,) + self.shape[1:], dtype=torch.float32, device=self.dev)
            p.normal_(generator=g)
            p.mul_(self.scale)
            if not self.signed:
                p.relu_()
            yield lo, hi, p


def assert_distinct(t, sel):
    """The selected samples differ pairwise: a wrapped offset that lands in another of them cannot hide."""
    for i, a in enumerate(sel):
        for b in sel[i + 1:]:
            assert not torch.equal(t[a], t[b]), "samples %d and %d hold the same values" % (a, b)


def guards_intact(proxy, first=0):
    """The guard bands of the proxy's allocations `first` .. on the device (synchronises)."""
    torch.cuda.synchronize()
    for order in range(first, len(proxy.records)):
        raw, g, body, dtype, shape, what = proxy.records[order]
        for name, band in (("before", raw[:g]), ("after", raw[g + body:])):
            bad = int((band != proxy.pattern).sum())
            assert bad == 0, ("allocation #%d (%s, %s, shape %s, %d bytes): %d bytes of the guard %s the body changed"
                              % (order, what, str(dtype).replace("torch.", ""), shape, body, bad, name))


def drop(proxy, first):
    """Check and forget the proxy's allocations from `first` on (a sub-batch launch's): their memory goes back to the pool."""
    guards_intact(proxy, first)
    del proxy.records[first:]


@contextlib.contextmanager
def bounded(monkeypatch, ops, poison):
    """One case: skipped below 24 GiB of free memory; `ops` allocates from a 0xFF proxy (yielded); at the end the guard bands of
    what is still recorded are checked, everything is released and the peak of allocated memory is held against 16 GiB."""
    need_free_memory()
    torch.cuda.reset_peak_memory_stats()
    proxy = poison.Proxy(0xFF)
    monkeypatch.setattr(ops, "torch", proxy)
    ops._WS.clear()
    try:
        yield proxy
        guards_intact(proxy)
    finally:
        proxy.release()
        ops._WS.clear()
        peak = torch.cuda.max_memory_allocated()
        torch.cuda.empty_cache()
    assert peak <= PEAK_MAX, "the case held %.2f GiB at its peak, the bound is 16" % (peak / GIB)


def host(t, sel=None):
    """Samples `sel` (all when None) of a device tensor as a numpy array."""
    return (t if sel is None else t[torch.as_tensor(sel, device=t.device)]).cpu().numpy()
