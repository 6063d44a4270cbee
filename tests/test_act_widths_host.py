"""The width table of tests/test_gpu_act_widths.py without a GPU: every (family, width setting, regime) triple with the numpy
oracle (oracle/patch.py) in the place of the HIP entry points, for the drivers whose every launch both references implement -
the drivers then compare the numpy oracle with the host twin (oracle/fq_host.cpp) bit for bit at that width and assert the
regime's condition from the oracle's codes.  For the recompute pair, the folded front layer and the chain: the data they make
meets the regime's condition.  Then the two references directly, at every width setting, on every rounding boundary."""
import numpy as np
import pytest
import torch

import regimes as R
import test_gpu_act_widths as W
import test_gpu_front_dw as FRONT
import test_gpu_pair_chain as CHAIN
import test_gpu_parity as P
import test_gpu_pwdw as PWDW
import test_gpu_shortcut as SC
import test_gpu_value_regimes as V
from oracle import fq_oracle as O
from oracle import host as H
from oracle import patch
from test_value_regimes_host import HOST_DRIVERS, MAX_MACS, _macs

# (signed, lo_neg_max, width): unsigned; signed with lo = -max; the Dense quirk (signed levels, clip at 0)
SETTINGS = [(False, None, 2), (False, None, 3), (False, None, 4), (False, None, 7), (True, None, 2), (True, None, 4), (True, None, 5),
            (True, False, 2), (True, False, 4)]


def _macs_of(c):
    """(the folded shortcut's case names two input channel counts: its multiply-adds are their sum's, not their product's)"""
    if c.driver is SC.test_folded_shortcut_equals_the_two_launches_and_the_host_twin:
        n, cin, cin2, cout, h, w = c.kwargs["case"]
        return float(n * (cin + cin2) * cout * h * w)
    return _macs(c)


def test_the_table_covers_the_width_settings():
    families = {f for f, _ in W.CASES}
    assert families == {"pointwise1x1", "dense3x3", "depthwise3x3", "codes", "recompute_pair", "head"}
    for family in ("pointwise1x1", "dense3x3", "depthwise3x3"):
        assert {"u2", "u4", "u7", "s2", "s4"} <= {s for f, s in W.CASES if f == family}, family
    assert ("pointwise1x1", "quirk4") in W.CASES
    assert {s for f, s in W.CASES if f == "codes"} == set(W.IN_OUT) and {s for f, s in W.CASES if f == "recompute_pair"} == set(W.IN_MID)
    assert set(W.OPERANDS) <= {s for f, s in W.CASES if f == "pointwise1x1"}
    # every case names a width other than 8, and every triple has a case
    for cs in W.CASES.values():
        for c in cs:
            assert any(c.kwargs.get(k, 8) != 8 for k in ("width", "out_width", "mid_width", "front_width", "width2")), V._describe(c)
    assert len(set(W.TRIPLES)) == len(W.TRIPLES) and all(r in W.REGIMES for _, _, r in W.TRIPLES)
    forms = {c.kwargs["form"] for c in W.CASES[("pointwise1x1", "u4")] if c.driver is P._pwconv_case}
    assert forms == {"two_kernels", "stream", "split", "sample", "rows", None}


@pytest.mark.parametrize("family,setting,regime", W.TRIPLES, ids=[W._id(t) for t in W.TRIPLES])
def test_family_at_width_under_regime_on_the_references(family, setting, regime):
    from quantization.mxnet_amd import ops
    dev = torch.device("cpu")
    ran = 0
    with patch.oracle_ops():
        for c in W.CASES[(family, setting)]:
            if regime not in c.regimes:
                continue
            kw = c.kwargs
            # the drivers that need a device: at least the data they make meets the regime's condition
            if c.driver is V._pair:
                PWDW._make(kw["case"], kw["mode"], None, None, regime=regime, width=kw["width"], mid_width=kw["mid_width"])
            elif c.driver is V._front:
                FRONT._make(kw["case"], kw["mode"], regime=regime, front_width=kw["front_width"], width=kw["width"])
            elif c.driver is V._chain:
                CHAIN._make(kw["case"], kw["signed"], regime=regime, width=kw["width"], mid_width=kw["mid_width"])
            elif c.driver in HOST_DRIVERS and _macs_of(c) <= MAX_MACS:
                try:
                    c.driver(dev=dev, ops=ops, regime=regime, **kw)
                except AssertionError as e:
                    raise AssertionError("%s, regime %s, %s: %s" % (setting, regime, V._describe(c), e)) from e
            else:
                continue
            ran += 1
    # (the launches that read or write code tensors are not restated on the references: they run on the GPU only)
    assert ran > 0 or family == "codes"


@pytest.mark.parametrize("signed,lo_neg_max,width", SETTINGS,
                         ids=["%s%d" % ("quirk" if lo is False else ("s" if sg else "u"), wd) for sg, lo, wd in SETTINGS])
@pytest.mark.parametrize("stored", [False, True], ids=["online", "stored"])
@pytest.mark.parametrize("regime", [None, "boundaries"], ids=["gaussian", "boundaries"])
def test_oracle_equals_host_twin_at_width(regime, stored, signed, lo_neg_max, width):
    """pwconv_i8, conv3x3_i8 and dwconv3x3 (strides 1 and 2) directly: the numpy oracle and the host twin agree bit for bit at
    every width setting, under an online and under a stored threshold, on Gaussian data and on every rounding boundary - whose
    condition (both codes of every tie present) the oracle's codes meet first."""
    rng = np.random.default_rng(7 + width)
    nonneg = not signed or lo_neg_max is False
    kw = dict(signed=signed, width=width, lo_neg_max=lo_neg_max)

    def draw(shape):
        x = (rng.standard_normal(shape) * 2).astype(np.float32)
        x = np.maximum(x, 0) if nonneg else x
        x, _, thr = R.apply(regime, x, signed, thr=np.float32(2.3) if stored else None, width=width, lo_neg_max=lo_neg_max)
        if regime is None and stored:
            thr = np.float32(2.3)
        in_max = R.stored_threshold(x) if thr is None else thr
        R.check(regime, x, in_max, signed, width=width, lo_neg_max=lo_neg_max)
        # (online: the host twin takes the per-sample maxima and forms the batch mean itself)
        return x, in_max, (dict(in_max=in_max) if stored else dict(in_stat=H.absmax_per_sample(x)))

    for taps, (n, cin, cout, h, w) in ((1, (2, 32, 40, 5, 7)), (9, (2, 64, 32, 5, 6))):
        x, in_max, hin = draw((n, cin, h, w))
        wt = (rng.standard_normal((cout, cin) + ((1, 1) if taps == 1 else (3, 3))) * 0.1).astype(np.float32)
        fo, fh = (O.pwconv_i8, H.pwconv_i8) if taps == 1 else (O.conv3x3_i8, H.conv3x3_i8)
        want = fo(x, wt, cout, 8, in_max, **kw)
        assert np.isfinite(want).all()
        P._eq(fh(x, wt, cout, 8, **hin, **kw), want, "host twin vs numpy oracle, %d taps" % taps)
    x, in_max, hin = draw((2, 8, 7, 7))
    wt = (rng.standard_normal((8, 1, 3, 3)) * 0.5).astype(np.float32)
    for stride in (1, 2):
        want = O.dwconv3x3(x, wt, stride=stride, in_max=in_max, **kw)
        assert np.isfinite(want).all()
        got = H.dwconv3x3(x, wt, stride=stride, **hin, **kw)
        if regime is None:
            # (Gaussian data: numpy's emulation of fmaf may differ at double-rounding ties)
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)
            assert (got != want).mean() < 1e-3
        else:
            P._eq(got, want, "depthwise: host twin vs numpy oracle")
