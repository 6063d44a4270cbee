"""The recompute pair alone on the GPU (round 6): fq_pwconv_i8 + fq_dwconv3x3 (two launches, the tensor between them written and
read) against fq_pwconv_i8_stat + fq_pwdw_fused, on MobileNet1.0's pointwise -> depthwise pairs at batch 128.

    python tools/pwdwbench.py [--batch 128] [--reps 30] [--pairs 1,2,3,4,5] [--codes 0] [--front 1] [--chain 1] [--sweep 1]
                              [--front-store 1]

--codes 1 (default): the statistic pass keeps the int8 codes of x and the fused launch loads them; 0: both read the fp32 x.
--front 1: ONLY the table of the depthwise layer in front of the first pair - fq_dwconv3x3 (storing) + fq_pwconv_i8_stat against
fq_dwconv3x3 without y (statistic pass, input codes kept) + fq_pwconv_i8_stat with that layer recomputed in front - on
MobileNet1.0's and MobileNet0.5's dw1 -> pw1 at the batch size.
--chain 1: ONLY the link between two pairs, pair 2 -> pair 3 - fq_pwdw_fused (storing z) + fq_pwconv_i8_stat reading it against
fq_pwdw_fused in statistic mode (mid_codes_out: the codes of its depthwise input kept, no z) + fq_pwconv_i8_stat with the depthwise
layer recomputed in front - on MobileNet1.0's and MobileNet0.5's shapes, the four launches alternating repetition by repetition.
Under a library without the statistic mode (FQ_LIB_PATH = the parent's) the stored pair alone is timed.
--front-store 1: ONLY the storing 1x1 behind a stand-alone depthwise layer, dw5 -> pw5 (256 channels at 28 x 28; MobileNet0.5's 128
channels where the library takes them) - fq_dwconv3x3 (storing) + fq_pwconv_i8 against fq_dwconv3x3 without y + fq_pwconv_i8_front,
the four launches alternating repetition by repetition.
--sweep 1: with --front 1 or --chain 1, ONLY the statistic pass with the front layer, under FQ_PWSTAT_FRONT_ROWS = 1 .. 8 and
FQ_PWSTAT_FRONT_WAVES = 4 and 8 (the library reads both at every call) and under the launch's own choice, all configurations
alternating repetition by repetition in this one process; median +- standard deviation, every configuration's values compared
with the first one's (the forced-rows blocks of profiles/front_waves_sweep.txt).

Per pair: time of each launch (HIP events on the launch stream, median over reps, all launches back to back), bytes each form
moves, and the resulting TB/s.  Values are checked bit-equal before timing."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantization.mxnet_amd import ops  # noqa: E402

PAIRS = {1: (32, 64, 112, 2), 2: (64, 128, 56, 1), 3: (128, 128, 56, 2), 4: (128, 256, 28, 1), 5: (256, 256, 28, 2),
         6: (256, 512, 14, 1), 7: (512, 512, 14, 1)}


def timed(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    timed.sd = float(np.std(ts))                       # (of the call just made: front_table prints it beside the medians)
    return float(np.median(ts))


def sweep_front_stat(label, cin, run, result, reps):
    """`run()`: the statistic pass with the front layer; `result()`: its outputs, to be compared.  One block of the table."""
    waves = (4, 8) if cin >= 64 else (4,)
    cfgs = [(w, r) for w in waves for r in range(1, 9)] + [(0, 0)]
    ts, same, first = {c: [] for c in cfgs}, True, None

    def under(c):
        for name, v in (("FQ_PWSTAT_FRONT_WAVES", c[0]), ("FQ_PWSTAT_FRONT_ROWS", c[1])):
            if v:
                os.environ[name] = str(v)
            else:
                os.environ.pop(name, None)
    for c in cfgs:                                         # warm-up, and the values of every configuration
        under(c)
        run()
        run()
        torch.cuda.synchronize()
        got = [t.clone() for t in result()]
        first = first or got
        same = same and all(torch.equal(a, b) for a, b in zip(got, first))
    for _ in range(reps):
        for c in cfgs:
            under(c)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            ts[c].append(a.elapsed_time(b) * 1e3)
    under((0, 0))
    cell = lambda c: "%6.1f±%-4.1f" % (float(np.median(ts[c])), float(np.std(ts[c])))      # noqa: E731
    print("== %s, %d alternating repetitions, values %s" % (label, reps, "bit-equal" if same else "DIFFER"))
    print("   rows:     " + " ".join("%11d" % r for r in range(1, 9)))
    for w in waves:
        print("   %d waves:   " % w + " ".join(cell((w, r)) for r in range(1, 9)))
    print("   the launch's own choice: " + cell((0, 0)))


FRONTS = {"mobilenet1.0": (32, 64, 112), "mobilenet0.5": (16, 32, 112)}


def front_table(n, reps, dev, sweep=False):
    if sweep:
        print("statistic pass with the front layer, forced rows per band and wavefronts per workgroup (us)")
    else:
        print("front          shape              stored: dw + stat = total (us)        recomputed: dw-stat + stat = total (us)   "
              "MB moved stored / recomputed   speed-up")
    for name, (cin, cout, hw) in FRONTS.items():
        y0 = torch.relu(torch.randn(n, cin, hw, hw, device=dev)) * 1.7
        dww = ops.weight_fake_quant(torch.randn(cin, 1, 3, 3, device=dev) * 0.3, cin, 8)
        codes, scales, rowsum = ops.weight_codes(torch.randn(cout, cin, device=dev) * 0.2, cout, 8)
        scA, shA = torch.rand(cin, device=dev) + 0.5, torch.randn(cin, device=dev) * 0.3
        scB, shB = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev) * 0.3
        s0 = ops.absmax_per_sample(y0)
        curA, curB = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        if not ops.pwconv_front_supported(y0.shape, cout):
            print("%-14s %s: shape not taken" % (name, (n, cin, cout, hw)))
            continue
        st = {}
        zc = [torch.empty(ops.pair_codes_shape(y0.shape), dtype=torch.int8, device=dev) for _ in range(2)]
        yc = torch.empty(ops.front_codes_shape(y0.shape), dtype=torch.int8, device=dev)
        dwk = dict(stride=1, in_stat=s0, cur_out=curA, bn_scale=scA, bn_shift=shA, act="relu")
        pwk = dict(cur_out=curB, bn_scale=scB, bn_shift=shB, act="relu")

        def dw():
            st["z"], st["zs"] = ops.dwconv3x3(y0, dww, None, **dwk)

        def sa():
            st["ps"] = ops.pwconv_i8_stat(st["z"], codes, scales, rowsum, None, in_stat=st["zs"], x_codes_out=zc[0], **pwk)

        def ds():
            st["zs1"] = ops.dwconv3x3(y0, dww, None, store=False, x_codes_out=yc, **dwk)[1]

        def sf():
            st["ps1"] = ops.pwconv_i8_stat(st["z"], codes, scales, rowsum, None, in_stat=st["zs1"], x_codes_out=zc[1],
                                           front=dict(x_codes=yc, w=dww, bn_scale=scA, bn_shift=shA, act="relu", in_stat=s0), **pwk)
        dw(); sa(); ds(); sf()
        torch.cuda.synchronize()
        ok = torch.equal(st["zs"], st["zs1"]) and torch.equal(st["ps"], st["ps1"]) and torch.equal(zc[0], zc[1])
        if sweep:
            sweep_front_stat("%s %d->%d @%d, batch %d%s" % (name, cin, cout, hw, n, "" if ok else ", VALUES DIFFER from the stored pair"),
                             cin, sf, lambda: (st["ps1"], zc[1]), reps)
            continue
        ts, sds = [], []
        for fn in (dw, sa, ds, sf):
            ts.append(timed(fn, reps))
            sds.append(timed.sd)
        t_dw, t_sa, t_ds, t_sf = ts
        yb = 4e-6 * n * cin * hw * hw                                    # the depthwise input = its output, fp32
        zcb = 32e-6 * n * ((cin + 31) // 32) * hw * hw                    # the pair's code buffer
        mb2, mb1 = 2 * yb + yb + zcb, yb + yb / 4 + yb / 4 + zcb
        print("%-14s %3d->%3d @%3dx%-3d   %6.1f + %6.1f = %6.1f (%4.2f TB/s)        %6.1f + %6.1f = %6.1f (%4.2f TB/s)          "
              "%6.0f / %5.0f            %5.2fx  %s" % (name, cin, cout, hw, hw, t_dw, t_sa, t_dw + t_sa, mb2 / (t_dw + t_sa), t_ds,
                                                    t_sf, t_ds + t_sf, mb1 / (t_ds + t_sf), mb2, mb1,
                                                    (t_dw + t_sa) / (t_ds + t_sf), "bit-equal" if ok else "VALUES DIFFER"))
        print("%-14s sd over the %d repetitions (us): dw %.2f  stat %.2f  dw-stat %.2f  stat with the front layer %.2f"
              % ("", reps, sds[0], sds[1], sds[2], sds[3]))


CHAINS = {"mobilenet1.0": (64, 128, 128, 56), "mobilenet0.5": (32, 64, 64, 56)}


def chain_table(n, reps, dev, sweep=False):
    has_new = ops.pwdw_chain_supported((n, 64, 56, 56), 128)
    print("chain          shape                   stored: fused + stat = total (us)        chained: fused-stat + stat = total (us)   "
          "MB moved stored / chained   speed-up")
    for name, (cin, cmid, cout, hw) in CHAINS.items():
        x = torch.relu(torch.randn(n, cin, hw, hw, device=dev)) * 1.7
        w1 = ops.weight_codes(torch.randn(cmid, cin, device=dev) * 0.2, cmid, 8)
        w2 = ops.weight_codes(torch.randn(cout, cmid, device=dev) * 0.2, cout, 8)
        dww = ops.weight_fake_quant(torch.randn(cmid, 1, 3, 3, device=dev) * 0.3, cmid, 8)
        bn = [(torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev) * 0.3) for c in (cmid, cmid, cout)]
        xstat = ops.absmax_per_sample(x)
        cur = [torch.zeros(1, device=dev) for _ in range(3)]
        xc = torch.empty(ops.pair_codes_shape(x.shape), dtype=torch.int8, device=dev)
        ystat = ops.pwconv_i8_stat(x, *w1, None, in_stat=xstat, cur_out=cur[0], bn_scale=bn[0][0], bn_shift=bn[0][1], act="relu",
                                   x_codes_out=xc)
        zshape = (n, cmid, hw, hw)
        zc = [torch.empty(ops.pair_codes_shape(zshape), dtype=torch.int8, device=dev) for _ in range(2)]
        yc = torch.empty(ops.front_codes_shape(zshape), dtype=torch.int8, device=dev)
        fk = dict(in_stat=xstat, pw_bn_scale=bn[0][0], pw_bn_shift=bn[0][1], pw_act="relu", mid_stat=ystat, mid_cur_out=cur[1],
                  stride=1, dw_bn_scale=bn[1][0], dw_bn_shift=bn[1][1], dw_act="relu", x_codes=xc)
        pk = dict(cur_out=cur[2], bn_scale=bn[2][0], bn_shift=bn[2][1], act="relu")
        st = {}

        def fs():
            st["z"], st["zs"] = ops.pwdw_fused(x, *w1, dww, **fk)

        def sa():
            st["ps"] = ops.pwconv_i8_stat(st["z"], *w2, None, in_stat=st["zs"], x_codes_out=zc[0], **pk)

        def fn():
            st["zs1"] = ops.pwdw_fused(x, *w1, dww, store=False, mid_codes_out=yc, **fk)[1]

        def sf():
            st["ps1"] = ops.pwconv_i8_stat(st["z"], *w2, None, in_stat=st["zs1"], x_codes_out=zc[1],
                                           front=dict(x_codes=yc, w=dww, bn_scale=bn[1][0], bn_shift=bn[1][1], act="relu",
                                                      in_stat=ystat), **pk)
        fns = [fs, sa] + ([fn, sf] if has_new else [])
        for f in fns:
            f()
        torch.cuda.synchronize()
        ok = not has_new or (torch.equal(st["zs"], st["zs1"]) and torch.equal(st["ps"], st["ps1"]) and torch.equal(zc[0], zc[1]))
        if sweep and has_new:
            sweep_front_stat("%s %d->%d @%d, batch %d%s" % (name, cmid, cout, hw, n, "" if ok else ", VALUES DIFFER from the stored pair"),
                             cmid, sf, lambda: (st["ps1"], zc[1]), reps)
            continue
        for _ in range(3):
            for f in fns:
                f()
        ts = [[] for _ in fns]
        for _ in range(reps):                              # alternating: every repetition times each launch once
            for i, f in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ts[i].append(a.elapsed_time(b) * 1e3)
        med = [float(np.median(t)) for t in ts]
        sds = [float(np.std(t)) for t in ts]
        zb = 4e-6 * n * cmid * hw * hw                                    # z in fp32
        xcb = 32e-6 * n * ((cin + 31) // 32) * hw * hw                    # the first pair's code buffer (read, with halo rows)
        zcb = 32e-6 * n * ((cmid + 31) // 32) * hw * hw                   # the second pair's code buffer (written)
        mb2, mb1 = xcb + zb + zb + zcb, xcb + zb / 4 + zb / 4 + zcb
        if not has_new:
            print("%-14s %3d->%3d->%3d @%3dx%-3d   %6.1f + %6.1f = %6.1f (%4.2f TB/s)        (this library has no statistic mode)"
                  % (name, cin, cmid, cout, hw, hw, med[0], med[1], med[0] + med[1], mb2 / (med[0] + med[1])))
            continue
        print("%-14s %3d->%3d->%3d @%3dx%-3d   %6.1f + %6.1f = %6.1f (%4.2f TB/s)        %6.1f + %6.1f = %6.1f (%4.2f TB/s)          "
              "%6.0f / %5.0f            %5.2fx  %s" % (name, cin, cmid, cout, hw, hw, med[0], med[1], med[0] + med[1],
                                                    mb2 / (med[0] + med[1]), med[2], med[3], med[2] + med[3],
                                                    mb1 / (med[2] + med[3]), mb2, mb1, (med[0] + med[1]) / (med[2] + med[3]),
                                                    "bit-equal" if ok else "VALUES DIFFER"))
        print("%-14s sd over the %d repetitions (us): fused %.2f  stat %.2f  fused-stat %.2f  stat with the front layer %.2f"
              % ("", reps, sds[0], sds[1], sds[2], sds[3]))


FRONT_STORES = {"mobilenet1.0": (256, 256, 28), "mobilenet0.5": (128, 128, 28)}


def front_store_table(n, reps, dev):
    """--front-store 1: the storing 1x1 behind a stand-alone depthwise layer, MobileNet's dw5 -> pw5 - fq_dwconv3x3 (storing) +
    fq_pwconv_i8 against fq_dwconv3x3 without y (statistic pass, input codes kept) + fq_pwconv_i8_front; the four launches
    alternating repetition by repetition."""
    print("front-store    shape              stored: dw + pw = total (us)          folded: dw-stat + pw-front = total (us)   "
          "MB moved stored / folded   speed-up")
    for name, (cin, cout, hw) in FRONT_STORES.items():
        shape = (n, cin, hw, hw)
        if not ops.pwconv_front_store_supported(shape, cout):
            print("%-14s %s: shape not taken" % (name, (n, cin, cout, hw)))
            continue
        y0 = torch.relu(torch.randn(*shape, device=dev)) * 1.7
        dww = ops.weight_fake_quant(torch.randn(cin, 1, 3, 3, device=dev) * 0.3, cin, 8)
        codes, scales, rowsum = ops.weight_codes(torch.randn(cout, cin, device=dev) * 0.2, cout, 8)
        scA, shA = torch.rand(cin, device=dev) + 0.5, torch.randn(cin, device=dev) * 0.3
        scB, shB = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev) * 0.3
        s0 = ops.absmax_per_sample(y0)
        curA, curB = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        yc = torch.empty(ops.front_codes_shape(shape), dtype=torch.int8, device=dev)
        dwk = dict(stride=1, in_stat=s0, cur_out=curA, bn_scale=scA, bn_shift=shA, act="relu")
        pwk = dict(cur_out=curB, bn_scale=scB, bn_shift=shB, act="relu")
        st = {}

        def dw():
            st["z"], st["zs"] = ops.dwconv3x3(y0, dww, None, **dwk)

        def pw():
            st["y"], st["ys"] = ops.pwconv_i8(st["z"], codes, scales, rowsum, None, in_stat=st["zs"], **pwk)

        def ds():
            st["zs1"] = ops.dwconv3x3(y0, dww, None, store=False, x_codes_out=yc, **dwk)[1]

        def pf():
            st["y1"], st["ys1"] = ops.pwconv_i8(shape, codes, scales, rowsum, None, in_stat=st["zs1"],
                                                front=dict(x_codes=yc, w=dww, bn_scale=scA, bn_shift=shA, act="relu", in_stat=s0), **pwk)
        fns = [dw, pw, ds, pf]
        for _ in range(3):
            for f in fns:
                f()
        torch.cuda.synchronize()
        ok = torch.equal(st["zs"], st["zs1"]) and torch.equal(st["ys"], st["ys1"]) and torch.equal(st["y"], st["y1"])
        ts = [[] for _ in fns]
        for _ in range(reps):                              # alternating: every repetition times each launch once
            for i, f in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ts[i].append(a.elapsed_time(b) * 1e3)
        med = [float(np.median(t)) for t in ts]
        sds = [float(np.std(t)) for t in ts]
        zb, yb = 4e-6 * n * cin * hw * hw, 4e-6 * n * cout * hw * hw        # the depthwise input = its output, the 1x1 output, fp32
        mb2, mb1 = 3 * zb + yb, zb + zb / 4 + zb / 4 + yb                  # (folded: without the halo rows of the bands)
        print("%-14s %3d->%3d @%3dx%-3d   %6.1f + %6.1f = %6.1f (%4.2f TB/s)        %6.1f + %6.1f = %6.1f (%4.2f TB/s)          "
              "%6.0f / %5.0f            %5.2fx  %s" % (name, cin, cout, hw, hw, med[0], med[1], med[0] + med[1],
                                                    mb2 / (med[0] + med[1]), med[2], med[3], med[2] + med[3],
                                                    mb1 / (med[2] + med[3]), mb2, mb1, (med[0] + med[1]) / (med[2] + med[3]),
                                                    "bit-equal" if ok else "VALUES DIFFER"))
        print("%-14s sd over the %d repetitions (us): dw %.2f  pw %.2f  dw-stat %.2f  pw with the front layer %.2f"
              % ("", reps, sds[0], sds[1], sds[2], sds[3]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--pairs", default="1,2,3,4,5")
    ap.add_argument("--codes", type=int, default=1)
    ap.add_argument("--front", type=int, default=0)
    ap.add_argument("--chain", type=int, default=0)
    ap.add_argument("--sweep", type=int, default=0)
    ap.add_argument("--front-store", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    n = a.batch
    if a.front_store:
        front_store_table(n, a.reps, dev)
        return
    if a.front:
        front_table(n, a.reps, dev, bool(a.sweep))
        return
    if a.chain:
        chain_table(n, a.reps, dev, bool(a.sweep))
        return
    print("pair  shape                          two launches: pw + dw = total (us)   recompute: stat + fused = total (us)   "
          "MB moved two / fused   speed-up")
    tot2 = tot1 = 0.0
    for p in [int(v) for v in a.pairs.split(",")]:
        cin, cout, hw, stride = PAIRS[p]
        x = torch.relu(torch.randn(n, cin, hw, hw, device=dev)) * 1.7
        w1 = torch.randn(cout, cin, device=dev) * 0.2
        w2 = ops.weight_fake_quant(torch.randn(cout, 1, 3, 3, device=dev) * 0.3, cout, 8)
        codes, scales, rowsum = ops.weight_codes(w1, cout, 8)
        sc1, sh1 = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev) * 0.3
        sc2, sh2 = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev) * 0.3
        xstat = ops.absmax_per_sample(x)
        cur1, cur2 = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        if not ops.pwdw_supported(x.shape, cout, stride):
            print("%4d  %s: shape not taken" % (p, (n, cin, cout, hw, stride)))
            continue
        st = {}
        xc = torch.empty(ops.pair_codes_shape(x.shape), dtype=torch.int8, device=dev) if a.codes else None

        def pw():
            st["y"], st["ys"] = ops.pwconv_i8(x, codes, scales, rowsum, None, in_stat=xstat, cur_out=cur1, bn_scale=sc1,
                                              bn_shift=sh1, act="relu")

        def dw():
            st["z"], st["zs"] = ops.dwconv3x3(st["y"], w2, None, stride=stride, in_stat=st["ys"], cur_out=cur2, bn_scale=sc2,
                                              bn_shift=sh2, act="relu")

        def sa():
            st["ys1"] = ops.pwconv_i8_stat(x, codes, scales, rowsum, None, in_stat=xstat, cur_out=cur1, bn_scale=sc1,
                                           bn_shift=sh1, act="relu", x_codes_out=xc)

        def fb():
            st["z1"], st["zs1"] = ops.pwdw_fused(x, codes, scales, rowsum, w2, in_stat=xstat, pw_bn_scale=sc1, pw_bn_shift=sh1,
                                                 pw_act="relu", mid_stat=st["ys1"], mid_cur_out=cur2, stride=stride,
                                                 dw_bn_scale=sc2, dw_bn_shift=sh2, dw_act="relu", x_codes=xc)
        pw(); dw(); sa(); fb()
        torch.cuda.synchronize()
        ok = torch.equal(st["z"], st["z1"]) and torch.equal(st["zs"], st["zs1"]) and torch.equal(st["ys"], st["ys1"])
        t_pw, t_dw, t_sa, t_fb = timed(pw, a.reps), timed(dw, a.reps), timed(sa, a.reps), timed(fb, a.reps)
        ho = (hw - 1) // stride + 1
        xb, yb, zb = 4e-6 * n * cin * hw * hw, 4e-6 * n * cout * hw * hw, 4e-6 * n * cout * ho * ho
        cb = 32e-6 * n * ((cin + 31) // 32) * hw * hw if a.codes else 0.0      # the code buffer: written once, read once
        mb2, mb1 = xb + 2 * yb + zb, (xb + 2 * cb + zb if a.codes else 2 * xb + zb)
        tot2 += t_pw + t_dw
        tot1 += t_sa + t_fb
        print("%4d  %3d->%3d @%3dx%-3d dw stride %d   %7.1f + %6.1f = %7.1f (%4.2f TB/s)   %6.1f + %6.1f = %7.1f (%4.2f TB/s)   "
              "%6.0f / %5.0f   %5.2fx  %s" % (p, cin, cout, hw, hw, stride, t_pw, t_dw, t_pw + t_dw, mb2 / (t_pw + t_dw),
                                            t_sa, t_fb, t_sa + t_fb, mb1 / (t_sa + t_fb), mb2, mb1,
                                            (t_pw + t_dw) / (t_sa + t_fb), "bit-equal" if ok else "VALUES DIFFER"))
    print("sum of the listed pairs: two launches %.1f us, recompute %.1f us" % (tot2, tot1))


if __name__ == "__main__":
    main()
