"""The poison harness itself (tests/poison.py), on CPU tensors: what it must let pass, what it must catch - and that the
table of tests/test_gpu_poison.py names every entry point of ops.py that allocates."""
import inspect
import re

import numpy as np
import pytest
import torch

import poison


def _expected(x):
    return np.abs(x).astype(np.float32) * np.float32(2), np.abs(x).reshape(x.shape[0], -1).max(axis=1)


def _launch(proxy, x, fake):
    """What an entry point of ops.py does: outputs and statistic target from `empty`, then the "kernel" `fake` fills them."""
    xt = proxy.guarded(x, "cpu")
    y = proxy.empty_like(xt)
    stat = proxy.empty(x.shape[0], dtype=torch.float32, device="cpu")
    fake(xt, y, stat)
    return y.numpy(), stat.numpy()


def _writes_everything(x, y, stat):
    y.copy_(x.abs() * 2)
    stat.copy_(x.abs().reshape(x.shape[0], -1).amax(dim=1))


def _skips_one_element(x, y, stat):
    _writes_everything(x, y, stat)
    y.reshape(-1)[-1] = STALE[0]              # the last element of a ragged tile: never stored by this launch


def _overruns_by_one_element(x, y, stat):
    _writes_everything(x, y, stat)
    flat = y.reshape(-1)
    beyond = torch.as_strided(flat, (flat.numel() + 1,), (1,), flat.storage_offset())
    beyond[-1] = 1.0


def _maximum_over_an_uninitialised_slot(x, y, stat):
    y.copy_(x.abs() * 2)
    stat.copy_(torch.fmax(stat, x.abs().reshape(x.shape[0], -1).amax(dim=1)))      # atomic-max style, slot never zeroed


STALE = [None]


def _x():
    return np.random.default_rng(1).standard_normal((3, 5, 7)).astype(np.float32)


@pytest.mark.parametrize("pattern", poison.PATTERNS)
def test_a_kernel_that_writes_everything_passes(pattern):
    x = _x()
    proxy = poison.Proxy(pattern)
    y, stat = _launch(proxy, x, _writes_everything)
    want_y, want_stat = _expected(x)
    assert np.array_equal(y, want_y) and np.array_equal(stat, want_stat)
    assert proxy.guards_intact() is True
    assert len(proxy.records) == 3
    proxy.release()
    assert proxy.records == [] and proxy.guards_intact() is True


@pytest.mark.parametrize("pattern", poison.PATTERNS)
def test_an_unwritten_element_is_caught(pattern):
    """The skipped element keeps whatever the memory held.  From a plain allocator that is, as a rule, the previous launch's
    right answer and the comparison passes; from the proxy it is the pattern, which no reference value equals."""
    x = _x()
    want_y, want_stat = _expected(x)
    STALE[0] = float(want_y.reshape(-1)[-1])                  # a reused block: the previous launch's right answer
    plain, _ = _launch(poison.Proxy(pattern), x, _skips_one_element)
    assert np.array_equal(plain, want_y), "(the skip is invisible when the stale value is the right one)"
    proxy = poison.Proxy(pattern)
    fresh = proxy.empty_like(torch.from_numpy(x))
    STALE[0] = float(fresh.reshape(-1)[-1])                   # ... under the proxy: the poison
    y, stat = _launch(proxy, x, _skips_one_element)
    assert not np.array_equal(y, want_y, equal_nan=True)
    bad = np.flatnonzero(~(y.reshape(-1) == want_y.reshape(-1)))
    assert list(bad) == [y.size - 1]
    assert proxy.guards_intact() is True                      # nothing was overrun: the comparison is what catches it


@pytest.mark.parametrize("pattern", poison.PATTERNS)
def test_a_store_past_the_body_is_caught_and_named(pattern):
    x = _x()
    proxy = poison.Proxy(pattern)
    y, stat = _launch(proxy, x, _overruns_by_one_element)
    want_y, want_stat = _expected(x)
    assert np.array_equal(y, want_y) and np.array_equal(stat, want_stat)       # the values give nothing away
    with pytest.raises(poison.GuardError) as e:
        proxy.guards_intact()
    msg = str(e.value)
    assert "allocation #1 " in msg and "empty_like" in msg and "float32" in msg and "(3, 5, 7)" in msg, msg
    assert "byte offset %d " % (4 * x.size) in msg and "past its end" in msg, msg


@pytest.mark.parametrize("where", ["before", "after"])
def test_one_byte_beside_either_end_is_caught(where):
    proxy = poison.Proxy(0xFF)
    t = proxy.empty((4, 3), dtype=torch.int8, device="cpu")
    raw, g, body = proxy.records[0][:3]
    raw[g - 1 if where == "before" else g + body] = 0
    with pytest.raises(poison.GuardError, match="before its start" if where == "before" else "past its end"):
        proxy.guards_intact()
    assert t.shape == (4, 3)


def test_a_maximum_over_an_uninitialised_slot_is_caught_under_the_finite_pattern():
    """`fmax` swallows a NaN: under 0xFF the uninitialised slot goes unnoticed, under 0x7F (3.39e38) it wins."""
    x = _x()
    want_y, want_stat = _expected(x)
    caught = []
    for pattern in poison.PATTERNS:
        proxy = poison.Proxy(pattern)
        y, stat = _launch(proxy, x, _maximum_over_an_uninitialised_slot)
        assert np.array_equal(y, want_y) and proxy.guards_intact() is True
        if not np.array_equal(stat, want_stat):
            caught.append(pattern)
    assert caught == [0x7F]


def test_views_layout_and_call_shapes():
    proxy = poison.Proxy(0x7F)
    like = torch.zeros(2, 3, 5, dtype=torch.int32)
    views = [proxy.empty((2, 3), dtype=torch.float32, device="cpu"), proxy.empty(7, dtype=torch.int8, device="cpu"),
             proxy.empty(2, 3, dtype=torch.float64, device="cpu"), proxy.empty_like(like),
             proxy.empty(torch.Size((4, 1, 2)), dtype=torch.int64, device="cpu"), proxy.empty((3,), device="cpu"),
             proxy.empty(1 << 16, dtype=torch.uint8, device="cpu"), proxy.empty((5 << 20,), dtype=torch.uint8, device="cpu")]
    shapes = [(2, 3), (7,), (2, 3), (2, 3, 5), (4, 1, 2), (3,), (1 << 16,), (5 << 20,)]
    dtypes = [torch.float32, torch.int8, torch.float64, torch.int32, torch.int64, torch.float32, torch.uint8, torch.uint8]
    for v, shape, dtype, rec in zip(views, shapes, dtypes, proxy.records):
        raw, g, body = rec[:3]
        assert tuple(v.shape) == shape and v.dtype == dtype and v.is_contiguous() and v.data_ptr() % 16 == 0
        assert body == v.numel() * v.element_size() and v.data_ptr() == raw.data_ptr() + g
        assert g % 256 == 0 and g >= max(body, 4 << 10) or g == 4 << 20
        assert 4 << 10 <= g <= 4 << 20 and raw.numel() >= g + body + g
        assert bool((raw == 0x7F).all())                                       # body and both guards: all poison
    assert views[0].view(torch.int32)[0, 0].item() == 2139062143 and views[1][0].item() == 127
    assert float(views[0][0, 0]) == pytest.approx(3.39e38, rel=1e-2)
    nan = poison.Proxy(0xFF)
    assert bool(torch.isnan(nan.empty(3, device="cpu")).all()) and nan.empty(2, dtype=torch.int32, device="cpu")[0].item() == -1
    # everything else is torch's own
    assert proxy.zeros is torch.zeros and proxy.float32 is torch.float32 and proxy.Tensor is torch.Tensor
    assert proxy.cuda is torch.cuda and not proxy.zeros(3).any()
    with pytest.raises(TypeError):
        proxy.empty(3, pin_memory=True)                                         # nothing is quietly left unpoisoned
    x = np.arange(6, dtype=np.int64).reshape(2, 3)
    gx = proxy.guarded(x, "cpu")
    assert gx.dtype == torch.int64 and np.array_equal(gx.numpy(), x) and proxy.guards_intact() is True


# ---- coverage: every allocating entry point of ops.py is run by the poisoned GPU tests -------------------------------------
EXEMPT_PREFIXES = ("comm_", "profile_")
EXEMPT_NAMES = ("device_info",)
EXEMPT = {}          # name -> one-line reason; starts empty


def _allocating_entry_points(ops):
    pat = re.compile(r"\btorch\.empty(_like)?\(|\b_workspace\(|\b_stat_ws\(|\b_stat_target\(|\bCodes16\.empty\(")
    names = []
    for name, fn in vars(ops).items():
        if name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != ops.__name__:
            continue
        if fn.__name__ != name:                  # an alias (stem_conv3x3s2): listed under its own name
            continue
        if pat.search(inspect.getsource(fn)):
            names.append(name)
    return sorted(names)


def test_every_allocating_entry_point_is_in_the_case_table():
    from quantization.mxnet_amd import ops
    import test_gpu_poison as G
    names = _allocating_entry_points(ops)
    assert len(names) >= 35 and "pwdw_fused" in names and "qconv_workspace" in names and "add_act_stat" in names, names
    covered = G.covered_entry_points()
    unknown = sorted(e for e in covered if not callable(getattr(ops, e, None)))
    assert not unknown, "the case table names what ops.py does not have: %s" % unknown
    missing = [n for n in names if n not in covered and n not in EXEMPT and n not in EXEMPT_NAMES
               and not n.startswith(EXEMPT_PREFIXES)]
    assert not missing, "entry points of ops.py that allocate and that no poisoned case runs: %s" % missing
    assert not EXEMPT or all(isinstance(r, str) and r.strip() for r in EXEMPT.values())
    stale = [n for n in EXEMPT if n in covered or n not in names]
    assert not stale, "exemptions that are not needed: %s" % stale
    for family, cases in G.CASES.items():
        assert cases, family
        for c in cases:
            assert callable(c.driver) and c.entries, (family, c)
            params = inspect.signature(c.driver).parameters
            assert set(c.kwargs) <= set(params) and {"dev", "ops"} <= set(params), (family, c.driver.__name__, c.kwargs)
