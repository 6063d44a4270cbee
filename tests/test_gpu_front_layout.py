"""GPU parity of the front-layer statistic pass (fq_pwconv_i8_stat with a front layer) on the shapes at which its band buffer
(csrc/fq_front_layout.h) and its rows per band can go wrong, against the two storing launches it replaces: both per-sample
statistics, both `current_input_max` and every byte of the code buffer bit for bit, inputs and outputs in poisoned, guard-banded
memory (tests/poison.py) under both patterns.  The drivers are tests/test_gpu_front_dw.py's."""
import pytest
import torch

import poison
from test_gpu_front_dw import _compare, _eq, _front, _input_codes, _make, _two_launches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    from quantization.mxnet_amd import ops as _ops
    return _ops


# ((n, cin, cout, h, w), rows per band forced through FQ_PWSTAT_FRONT_ROWS or None)
CASES = [
    ((2, 32, 64, 3, 256), None),      # Q = 64: one segment fills the wavefront, the widest row admitted
    ((2, 32, 64, 5, 80), None),       # Q = 20: three segments, 60 lanes, 12.5 tiles per plane
    ((2, 16, 32, 9, 16), None),       # Q = 4: sixteen segments, half-slab past Cin
] + [((3, 32, 64, 17, 112), r) for r in (1, 3, 7, 8)] + [((2, 16, 96, 9, 32), r) for r in (2, 5)]
# short last bands (17 = 2 * 8 + 1 = 2 * 7 + 3 = 5 * 3 + 2; 9 = 4 * 2 + 1 = 5 + 4), partial last tiles (7 and 3 rows of 112: 24.5
# and 10.5 tiles; 5 rows of 32: 5 tiles; 1 row of 112: 3.5), the second on a three-tile Cout
MODES = ["u8_bn_relu", "s8_both"]     # the unsigned fast path, the signed general path


def _id(v):
    if isinstance(v, str):
        return v
    (n, cin, cout, h, w), r = v
    return "%dx%d->%d@%dx%d%s" % (n, cin, cout, h, w, "" if r is None else "-rows%d" % r)


_REFERENCE = {}


def _reference(shape, mode, dev, ops):
    """(inputs, results of the two storing launches): once per shape and mode, shared, never changed."""
    key = (shape, mode)
    if key not in _REFERENCE:
        k = _make(shape, mode)
        _REFERENCE[key] = (k, _two_launches(k, dev, ops))
    return _REFERENCE[key]


@pytest.mark.parametrize("pattern", poison.PATTERNS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_front_pass_equals_the_two_storing_launches(dev, ops, monkeypatch, case, mode, pattern):
    shape, rows = case
    n, cin, cout, h, w = shape
    if rows is None:
        monkeypatch.delenv("FQ_PWSTAT_FRONT_ROWS", raising=False)
    else:
        monkeypatch.setenv("FQ_PWSTAT_FRONT_ROWS", str(rows))      # (the library reads it at every call)
    assert ops.pwconv_front_supported((n, cin, h, w), cout), "shape refused: %s" % (shape,)
    k, want = _reference(shape, mode, dev, ops)
    proxy = poison.Proxy(pattern)
    monkeypatch.setattr(ops, "torch", proxy)
    ops._WS.clear()
    try:
        got = _front(k, dev, ops, put=lambda a: proxy.guarded(a, dev),
                     empty=lambda s, dtype: proxy.empty(s, dtype=dtype, device=dev))
        torch.cuda.synchronize()
        proxy.guards_intact()
        _compare(got, want, k)
        _eq(got["y0"], k["y0"], "the depthwise input after both passes")
        _eq(got["ycodes"], _input_codes(k), "codes of the depthwise input")
    finally:
        proxy.release()
        ops._WS.clear()
