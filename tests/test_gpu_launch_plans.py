"""Every launch configuration of the int8 MFMA families at the smallest ragged shapes where it can go wrong.

The host rules that pick a template instantiation (wavefronts per workgroup, tiles per wavefront, statistic path, store policy)
compare the amount of work with the number of compute units, so every small shape of the other tables lands on ONE side of each
rule: the side a full-size layer takes is seen at batch 128 only, on Gaussian data whose pixel counts are multiples of 64.  Here
the tuning variables that select an instantiation - read at every call - steer the small shapes to the other side, the drivers of
the other files run there with their own bit-for-bit assertions, and `ops.last_launch()` (fq_debug_last_launch: written at the
launch from the kernel's template arguments) must say that the instantiation a case names is the one that ran.

`ROWS`: row -> (environment, [case]); a case is (driver, arguments, the notes its launches must leave, ...).  Each row runs
  (a) the drivers as they are, every case;
  (b) its `small` cases under both poison patterns (tests/poison.py: fresh poisoned outputs, statistic targets and workspaces
      between guard bands, the scratch cache cleared per case, guards compared after a synchronise);
  (c) its `small` cases under the value regimes `boundaries`, `saturated`, `zero_sample` - and `out_saturated` where the launch
      writes codes -, each with the regime's own condition check (tests/regimes.py);
  (d) its `small` cases at the activation widths (4, 4) and (2, 2), on Gaussian data and on `boundaries`.
A last test compares the notes the whole file has confirmed with `INSTANTIATIONS`, the hand-written list to hold against the
launch macros.  No tolerance is added anywhere: a driver asserts what its own test asserts."""
import collections

import pytest
import torch

import poison
import test_gpu_c16 as C16
import test_gpu_front_dw as FRONT
import test_gpu_gap as GAP
import test_gpu_parity as P
import test_gpu_poison as POISON
import test_gpu_shortcut as SC
import test_gpu_value_regimes as V

pytestmark = pytest.mark.gpu

ANY = None                                           # a value of a note that the case does not pin (it follows the CU count)


# ---- notes (ops.LAUNCH_FAMILIES: the order of the values) --------------------------------------------------------------------
def c3(kt, ptw, wc, nw, nsl=1, in16=0, out16=0):
    return ("conv3x3", kt, ptw, wc, nw, nsl, in16, out16)


def split(kt, cw, lb, nw, bits=0):                   # bits: 1 IN16 | 2 OUT16 | 4 second output | 8 subsampled
    return ("split", kt, cw, lb, nw, bits)


def sample(kt, ctw, pt, res=0, gap=0):
    return ("sample", kt, ctw, pt, res, gap)


def short(kt, kt2, nw, bits=0, nts=0):               # bits: 1 A16 | 2 B16 | 4 second output
    return ("short", kt, kt2, nw, bits, nts)


def stream(kt, thin, res=0, o16=0, i16=0, nt=1, dual=0):
    return ("stream", kt, thin, res, o16, i16, nt, dual)


def stat(kt, waves, front, table):
    return ("stat", kt, waves, front, table)


def _matches(note, seen):
    return any(len(s) == len(note) and all(a is ANY or a == b for a, b in zip(note, s)) for s in seen)


Case = collections.namedtuple("Case", "driver kwargs notes small regimes widths refused")
Row = collections.namedtuple("Row", "env cases")

REGIMES = ("boundaries", "saturated", "zero_sample")
CODES = REGIMES + ("out_saturated",)                 # a launch that writes codes


def case(driver, notes, regimes=REGIMES, widths=None, refused=None, **kwargs):
    """notes: what the driver's launches must leave (every one of them); widths: the keywords of the driver that carry the
    activation width(s); refused: the text of the error the call must end in instead - nothing of `notes`' family may then have
    been launched.  Whether the case also runs under (b) - (d) (`small`) is derived from the notes: `_derive_small` below."""
    return Case(driver, kwargs, tuple(notes), False, tuple(regimes), widths, refused)


ROWS = collections.OrderedDict()

# ---- dense 3x3 ---------------------------------------------------------------------------------------------------------------
# (added: 35 pixels: a block whose 2nd .. 4th pixel tiles are empty; 63 pixels in seven samples: one block's statistic flush spans them)
# (512 -> 64: the one K / 32 x arrangement the other tables have no shape for)
# (128 -> 64 on 5 x 6: beside the 1 x 50 plane, a shape of that arrangement on which `saturated` can meet its condition)
C3_EXTRA = [(1, 64, 64, 5, 7), (7, 128, 128, 3, 3), (1, 512, 64, 3, 3), (2, 128, 64, 5, 6)]
C3_MODES = ("online_u8_bn_relu", "offline_s8_channel_w4")
C3S_MODES = ("online_u8_bn_relu_wino", "offline_s8_bias")


def _wc(cout):
    return 4 if cout >= 128 else 2


def _c3_regimes(c, base=REGIMES):
    """A plane of one row has three valid taps: below 173 channels 3 * Cin * 255 * 127 < 2^24 and `saturated` cannot meet its
    own condition (tests/regimes.py: `check` asks for a sum past 2^24 of every 3x3 with 9 * Cin >= 519)."""
    return base if c[3] > 1 or c[1] >= 173 else tuple(r for r in base if r != "saturated")


for ptw in (2, 4):
    ROWS["c3-ptw%d" % ptw] = Row({"FQ_C3_PTW": ptw}, [
        case(P.test_conv3x3_i8_vs_oracle, [c3(c[1] // 32, ptw, _wc(c[2]), 4)], regimes=_c3_regimes(c), widths=("width",), case=c, mode=m)
        for c in P.C3_CASES + C3_EXTRA for m in C3_MODES])
# (288 channels: a partial ninth channel tile in the second group of 256)
C3_NW8 = [(2, 256, 256, 5, 6), (1, 512, 512, 7, 7), (3, 256, 288, 3, 3), (1, 256, 256, 1, 50)]
for ptw in (1, 2):
    ROWS["c3-nw8-ptw%d" % ptw] = Row({"FQ_C3_NW": 8, "FQ_C3_PTW": ptw}, [
        case(P.test_conv3x3_i8_vs_oracle, [c3(c[1] // 32, ptw, 8, 8)], widths=("width",), case=c, mode=m)
        for c in C3_NW8 for m in C3_MODES])
ROWS["c3s-ptw2"] = Row({"FQ_C3_PTW": 2}, [
    case(P.test_conv3x3_i8_sliced_vs_oracle, [c3(c[1] // 32, 2, _wc(c[2]), 4, 3)],
         widths=("width",), case=c, mode=m)
    for c in P.C3S_CASES + C3_EXTRA for m in C3S_MODES])
for ptw in (1, 2):
    ROWS["c3s-nw8-ptw%d" % ptw] = Row({"FQ_C3_NW": 8, "FQ_C3_PTW": ptw}, [
        case(P.test_conv3x3_i8_sliced_vs_oracle, [c3(8, ptw, 8, 8, 3)], widths=("width",), case=c, mode=m)
        for c in ((2, 256, 256, 5, 6), (3, 256, 288, 3, 3)) for m in C3S_MODES])
# codes on one side and on both: the driver launches fp32 -> fp32, codes -> fp32, fp32 -> codes and codes -> codes
C316_SHAPES = POISON.C3_SHAPES + [(2, 256, 256, 5, 6)]
ROWS["c316-ptw2"] = Row({"FQ_C3_PTW": 2}, [
    case(C16.test_dense3x3_with_codes_on_both_sides,
         [c3(c[1] // 32, 2, _wc(c[2]), 4, 1, i, o) for i, o in ((0, 0), (1, 0), (0, 1), (1, 1))],
         regimes=_c3_regimes(c, CODES), widths=("width", "out_width"), case=c, signed=sg)
    for c in C316_SHAPES for sg in (False, True)])
# (eight wavefronts are built for fp32 on both sides and for codes on both sides: the one-sided launches stay on four)
for ptw in (1, 2):
    ROWS["c316-nw8-ptw%d" % ptw] = Row({"FQ_C3_NW": 8, "FQ_C3_PTW": ptw}, [
        case(C16.test_dense3x3_with_codes_on_both_sides,
             [c3(8, ptw, 8, 8, 1, 1, 1), c3(8, ptw, 8, 8), c3(8, ptw, 4, 4, 1, 1, 0), c3(8, ptw, 4, 4, 1, 0, 1)],
             regimes=CODES, widths=("width", "out_width"), case=(2, 256, 256, 5, 6), signed=sg)
        for sg in (False, True)])

# ---- split form --------------------------------------------------------------------------------------------------------------
PW_MODES = ("online_u8_bn_relu", "offline_s8_channel_w4")
RES_MODES = ("online_u8_bn_relu", "offline_s8_channel_w4_bn_none")


def _kt(cin):
    return (cin + 63) // 64 * 2                      # padded row length of fq_weight_codes / 32


PWS_WIDE = [(3, 1024, 1024, 7, 7), (3, 256, 512, 5, 6), (5, 512, 1024, 7, 7), (2, 2048, 512, 7, 7), (2, 320, 1280, 7, 7),
            (4, 1024, 1000, 1, 1)]
# Cout >= 512 on four wavefronts (twice the channel groups): what every layer above 16 tiles per CU runs
ROWS["pws-nw4"] = Row({"FQ_PWS_NW": 4}, [
    case(P._pwconv_case, [split(_kt(c[1]), 2, 4, 4)], widths=("width",), case=c, mode=m,
         form="split") for c in PWS_WIDE for m in PW_MODES] + [
    case(P.test_pwconv_i8_residual_vs_oracle, [split(16, 2, 4, 4)], widths=("width",), form="split",
         case=(3, 512, 2048, 7, 7), mode=m) for m in RES_MODES])
# eight wavefronts where half of them have no channel tile
ROWS["pws-nw8"] = Row({"FQ_PWS_NW": 8}, [
    case(P._pwconv_case, [split(_kt(c[1]), 2, 4, 8)], widths=("width",), case=c, mode=m, form="split")
    for c in ((2, 512, 256, 7, 7), (2, 256, 160, 9, 7)) for m in PW_MODES])
# the instantiations only FQ_PWS_CFG reaches: three wavefronts per SIMD with one, two and four channel tiles per wavefront
for cfg in (31, 32, 34):
    ROWS["pws-cfg%d" % cfg] = Row({"FQ_PWS_CFG": cfg}, [
        case(P._pwconv_case, [split(_kt(c[1]), cfg % 10, 3, 4)], widths=("width",), case=c,
             mode=m, form="split")
        for c in ((3, 256, 512, 5, 6), (2, 512, 512, 14, 14), (3, 1024, 1024, 7, 7), (2, 2048, 512, 7, 7)) for m in PW_MODES])
# the closing 1x1 with its code copy on four and on eight wavefronts (the one-output launch of the driver: codes in, four)
DUAL_WIDE = [(3, 256, 1024, 9, 11), (3, 512, 2048, 5, 5)]
for on, nw in ((0, 4), (1, 8)):
    ROWS["pws-dual-nw%d" % nw] = Row({"FQ_PWS16_DUAL_NW8": on}, [
        case(C16.test_closing_pointwise_stores_the_trunk_twice, [split(c[1] // 32, 2, 4, nw, 1 | 4), split(c[1] // 32, 2, 4, 4, 1)],
             regimes=CODES, widths=("width", "out_width"), case=c) for c in DUAL_WIDE])

# what the full-size layers of tests/test_gpu_resnet_full_batch.py run by the default rules and nothing above forces: the streaming
# form's plain K = 256 with nontemporal loads only, one channel tile per wavefront (Cout <= 128) at K = 256 and 512, two at K = 64,
# 256 channels per workgroup at K = 1024 on blocked planes.  Named forms at shapes too small for any rule to turn
ROWS["full-size-defaults"] = Row({}, [
    case(P._pwconv_case, [n], widths=("width",), case=c, mode=m, form=f)
    for f, c, n in (("stream", (3, 256, 256, 9, 7), stream(8, 0, nt=1)), ("split", (2, 256, 128, 9, 7), split(8, 1, 4, 4)),
                    ("split", (2, 512, 128, 5, 6), split(16, 1, 4, 4)), ("split", (2, 64, 256, 5, 6), split(2, 2, 4, 4)),
                    ("sample", (3, 1024, 256, 14, 14), sample(32, 1, 4))) for m in PW_MODES])

# ---- sample form -------------------------------------------------------------------------------------------------------------
# two channel tiles per wavefront (512 channels per workgroup) without a residual operand: blocked planes (PT = 4) and whole
# small planes (PT = 2)
SMP_CASES = [c for f, c in P.FORM_CASES if f == "sample" and c[2] % 512 == 0] + [
    (2, 128, 512, 14, 14), (2, 256, 512, 28, 28), (2, 2048, 512, 7, 7), (3, 1024, 1024, 8, 8), (2, 1024, 512, 14, 14)]


def _pt(c):
    return 2 if c[3] * c[4] <= 64 else 4


ROWS["smp-ctw2"] = Row({"FQ_PWSMP_CTW": 2}, [
    case(P._pwconv_case, [sample(c[1] // 32, 2, _pt(c))], widths=("width",), case=c,
         mode=m, form="sample") for c in SMP_CASES for m in PW_MODES] + [
    case(P.test_pwconv_i8_residual_vs_oracle, [sample(c[1] // 32, 2, _pt(c), 1)],
         widths=("width",), form="sample", case=c, mode=m)
    for f, c in P.PW_RES_CASES if f == "sample" for m in RES_MODES] + [
    case(GAP.test_gap_producer_equals_the_two_launches_and_the_host_twin, [sample(c[1] // 32, 2, 2, 0, 1)],
         widths=("width",), case=c, mode=m)
    for c in ((5, 512, 1024, 7, 7, False), (3, 2048, 512, 7, 7, False)) for m in GAP.MODES[:2]])
# 256 channels per workgroup with a residual operand is not built: the named form refuses, the pooled producer refuses
ROWS["smp-ctw1"] = Row({"FQ_PWSMP_CTW": 1}, [
    case(P.test_pwconv_i8_residual_vs_oracle, [sample(ANY, ANY, ANY, ANY, ANY)], refused="sample form is not built", form="sample",
         case=(2, 512, 1024, 8, 8), mode=RES_MODES[0]),
    case(GAP.test_gap_producer_equals_the_two_launches_and_the_host_twin, [sample(ANY, ANY, ANY, ANY, 1)], refused="shape not taken",
         case=(4, 512, 2048, 7, 7, True), mode=GAP.MODES[0]),
    case(P._pwconv_case, [sample(16, 1, 2)], widths=("width",), case=(5, 512, 1024, 7, 7), mode=PW_MODES[0], form="sample")])

# ---- folded shortcut ---------------------------------------------------------------------------------------------------------
SH_CASES = [(3, 128, 256, 512, 9, 11), (9, 256, 512, 1024, 7, 7), (2, 64, 64, 256, 5, 3), (4, 512, 1024, 2048, 7, 7)]
SH_MODES = ("online_u8_relu", "mixed_relu6_bias")
SH_DRIVER = SC.test_folded_shortcut_equals_the_two_launches_and_the_host_twin
SH16_DRIVER = SC.test_folded_shortcut_under_stored_thresholds_equals_the_two_launches
SH16_CASES = [(9, 256, 512, 1024, 7, 7, False), (5, 256, 512, 1024, 14, 14, True)]


def _sh_nw(c, nw):
    return nw if c[3] % 512 == 0 else 4              # (64 / 64 -> 256: four wavefronts whatever is asked)


for nts in (None, 0):
    for nw in (4, 8):
        env = {"FQ_PWSH_NW": nw}
        if nts is not None:
            env["FQ_PWSH_NTS_MB"] = nts
        flag = 0 if nts is None else 1
        built = [c for c in SH_CASES if not (nw == 4 and c[1] == 512)]
        ROWS["psh-nw%d%s" % (nw, "" if nts is None else "-nts")] = Row(env, [
            case(SH_DRIVER, [short(c[1] // 32, c[2] // 32, _sh_nw(c, nw), 0, flag)],
                 widths=("width", "width2"), case=c, mode=m)
            for c in built for m in SH_MODES] + ([
                # the widest pair and the stored-threshold variants are built for eight wavefronts only
                case(SH_DRIVER, [short(ANY, ANY, ANY, ANY, ANY)], refused="no instantiation", case=SH_CASES[3], mode=SH_MODES[0])] + [
                case(SH16_DRIVER, [short(ANY, ANY, ANY, ANY, ANY)], refused="no instantiation", case=c) for c in SH16_CASES]
            if nw == 4 else [
                case(SH16_DRIVER, [short(8, 16, 8, 1 | 4 | (2 if c[6] else 0), flag)], case=c) for c in SH16_CASES]))

# ---- streaming form ----------------------------------------------------------------------------------------------------------
# the thin instantiations (ragged Cin / Cout, codes in) on few tiles: 3 tiles - fewer than one workgroup's four -, 13 tiles
ROWS["pwst-thin"] = Row({"FQ_PWS_THIN_MIN_TILES": 0}, [
    case(P._pwconv_case, [stream((c[1] + 31) // 32, 1, nt=0)], widths=("width",), case=c, mode=m, form=f)
    for c in ((2, 24, 40, 5, 7), (2, 144, 24, 14, 14)) for f in ("stream", None) for m in PW_MODES] + [
    case(P.test_pwconv_i8_residual_vs_oracle, [stream(5, 1, 1, nt=0)], widths=("width",), form="stream",
         case=(2, 144, 24, 14, 14), mode=m) for m in RES_MODES] + [
    # codes in (with and without a residual operand), codes out of a ragged layer (48 channels: a block of 16 past them does
    # not exist), codes on both sides (K = 32 and the wide K = 256 / 512), the closing 1x1 with its code copy (K = 64 / 128)
    case(C16.test_pointwise_consumer_of_codes_equals_consumer_of_fp32, [stream((c[1] + 31) // 32, 1, int("res" in m), 0, 1, 0)],
         widths=("width",), case=c, mode=m)
    for c in ((3, 16, 96, 9, 11, 1), (2, 144, 24, 7, 7, 1)) for m in ("u8_bn_relu", "s8_res")] + [
    case(C16.test_pointwise_producer_writes_the_consumers_codes, [stream(1, 1, 0, 1, 0, 0)], regimes=CODES,
         widths=("width", "out_width"), case=(2, 24, 48, 5, 7, 1), mode=m) for m in ("u8-out", "s8-out-relu")] + [
    case(C16.test_pointwise_between_two_code_tensors, [stream(c[1] // 32, 1, 0, 1, 1, 0)], regimes=CODES,
         widths=("width", "out_width"), case=c) for c in ((2, 32, 16, 9, 11, 1), (2, 256, 64, 9, 11, 1), (2, 512, 64, 5, 6, 1))] + [
    case(C16.test_closing_pointwise_stores_the_trunk_twice, [stream(c[1] // 32, 1, 1, 0, 1, 0, 1), stream(c[1] // 32, 1, 1, 0, 1, 0)],
         regimes=CODES, widths=("width", "out_width"), case=c) for c in ((3, 64, 256, 9, 11), (3, 128, 256, 5, 5))])
# nontemporal stores beside the nontemporal loads every plain launch has, without and with a residual operand
ROWS["pwst-nt3"] = Row({"FQ_PWS_NTS_MB": 0}, [
    case(P._pwconv_case, [stream(c[1] // 32, 0, nt=3)], widths=("width",), case=c, mode=m,
         form="stream") for f, c in P.FORM_CASES if f == "stream" for m in PW_MODES] + [
    case(P.test_pwconv_i8_residual_vs_oracle, [stream(2, 0, 1, nt=3)], widths=("width",), form="stream",
         case=(2, 64, 256, 28, 28), mode=m) for m in RES_MODES])

# ---- statistic pass and fused pair -------------------------------------------------------------------------------------------
# maxima straight to memory (table = 0: what a layer of more than about 30 000 tiles runs) and through the LDS table on small
# planes; 40 samples of 84 pixels: many samples per tile, more than the table has slots for one workgroup.  (The statistic pass
# itself takes the (40, 32, 32, 4, 8) of the request - fq_pwconv_i8_stat_supported says yes to 32 pixels -, but the driver runs the
# fused launch behind it, and `pwdw_plan` refuses rows of 8: a plane of one strip is built for 28 or 30 columns.  3 x 28 is the
# smallest plane BOTH launches take.)
PAIR_SHAPES = POISON.PAIR_CASES + [(40, 32, 32, 3, 28, 1)]
PAIR_MODES = ("online_u8_bn_relu", "offline_u8_bn_relu")
for table in (0, 1):
    ROWS["stat-table%d" % table] = Row({"FQ_PWSTAT_TABLE": table}, [
        case(V._pair, [stat((c[1] + 31) // 32, 4, -1, table), ("pair", (c[1] + 31) // 32, ANY, c[5], ANY, ANY, ANY, 0, ANY)],
             regimes=REGIMES, widths=("width", "mid_width"), case=c, mode=m,
             regime=None) for c in PAIR_SHAPES for m in PAIR_MODES] + [
        # (front mode, BatchNorm + ReLU epilogue; 16 and 32 front channels: four wavefronts whatever the CU count)
        case(V._front, [stat((c[1] + 31) // 32, 4, 1, table)], regimes=("boundaries", "zero_sample"), widths=("front_width", "width"),
             case=c, mode="u8_bn_relu", regime=None)
        for c in (FRONT.TAKEN[0], FRONT.TAKEN[4])])

# ---- which cases run under (b) - (d) --------------------------------------------------------------------------------------------
def _size(c):
    n = 1
    for v in c.kwargs["case"]:
        n *= 1 if isinstance(v, bool) else v
    return n


def _derive_small():
    """For EVERY note a row's cases name - every instantiation - the two smallest shapes that leave it, each in its first-listed
    mode, also run from poisoned memory, under the regimes and at the widths: no instantiation is seen as it is only."""
    for name, row in ROWS.items():
        by_note = collections.defaultdict(list)
        for i, c in enumerate(row.cases):
            if c.refused is None:
                for n in c.notes:
                    by_note[n].append(i)
        picked = set()
        for idx in by_note.values():
            shapes = []
            for i in sorted(idx, key=lambda i: (_size(row.cases[i]), i)):
                if row.cases[i].kwargs["case"] not in shapes:
                    shapes.append(row.cases[i].kwargs["case"])
                    picked.add(i)
                if len(shapes) == 2:
                    break
        row.cases[:] = [c._replace(small=i in picked) for i, c in enumerate(row.cases)]


_derive_small()

# ---- what the whole file must have confirmed ---------------------------------------------------------------------------------
# Hand-written, to be held against the launch macros (FQ_C3_CASE_NS / FQ_C316_CASE* of fq_conv3x3*.hip, FQ_PWS_CASE_NW / fq_pw_split16
# / _sub of the split form, FQ_PWSMP_CASE_R / FQ_PWSMP_GAP, FQ_PWSH_CASE_C, FQ_PWS_LAUNCH* / FQ_PWS_THIN*, pw_stat_go): the
# instantiations that only a tuning variable or a full-size layer reaches.  The default instantiations of the small shapes are the
# other tables' (they appear here only where a driver of this file launches them beside the one it is about).
# Shipped and NOT reached by any driver even with the variables ("Launch configurations"):
#   * 3x3 on codes with one slice at PTW = 4, sliced at PTW = 4: not built (FQ_C3_PTW=4 is ignored there) - nothing to run;
#   * split form FQ_PWS_KT_TUNE at cw = 4 for Cout < 128 shapes and the K / 32 = 2 ... 30 defaults: the other tables' (default rule);
#   * sample form (32, 1, 4), (4, 1, 4), (8, 1, 4), (16, 1, 4), (64, 1, 2), (32, 1, 2): 256 channels per workgroup is what the small
#     shapes of the other tables take by default; GAP (10, 1), (16, 1), (32, *), (64, 1) and (16, 2) with a residual operand:
#     tests/test_gpu_gap.py at their default; GAP (10, 2) is dead code: its one layer has 1280 channels, no multiple of 512;
#   * split form storing subsampled (`pw_split_sub`, `FQ_PWS16_DUAL_SUB`): always four wavefronts and two channel tiles, no rule
#     compares with the CU count and no variable reaches in (FQ_PWS_CFG is ignored there): tests/test_gpu_sub2.py as they are;
#   * shortcut (16, 32, 8) on codes: tests/test_gpu_shortcut.py's (4, 512, 1024, 2048, 7, 7, True) at its default;
#   * streaming form NT = 0 / 2 (FQ_PWS_NTL_MB, read once per process), the thin K / 32 = 2, 3, 4, 6 fp32 instantiations beyond
#     those below, thin codes-out at K / 32 > 1;
#   * statistic pass with eight wavefronts and the front epilogues other than BatchNorm + ReLU: tests/test_gpu_front_*.py;
#   * fused pair: its instantiations follow the shape alone (no rule compares with the CU count); FQ_PWDW_NO_FAST stays open.
INSTANTIATIONS = {
    "conv3x3": (
        # FQ_C3_KT at PTW = 2 and 4, both wavefront arrangements
        {c3(kt, ptw, wc, 4) for kt in (2, 4, 8, 16) for ptw in (2, 4) for wc in (2, 4)} |
        # FQ_C3_CASE_NW(., ., 8, ., ., 8)
        {c3(kt, ptw, 8, 8) for kt in (8, 16) for ptw in (1, 2)} |
        # FQ_C3_SLICED at PTW = 2 and FQ_C3_CASE_NS(8, ., 8, ., ., 8, 3)
        {c3(kt, 2, wc, 4, 3) for kt in (2, 4, 8, 16) for wc in (2, 4)} |
        {c3(8, ptw, 8, 8, 3) for ptw in (1, 2)} |
        # FQ_C316_IO at PTW = 2 (the shapes of the poison table: K / 32 = 2 with two channel tiles, 4 with two, 8 with two and four)
        {c3(kt, 2, wc, 4, 1, i, o) for kt, wc in ((2, 2), (4, 2), (8, 2), (8, 4)) for i, o in ((1, 0), (0, 1), (1, 1))} |
        # FQ_C316_CASE8, and the one-sided launches beside it
        {c3(8, ptw, 8, 8, 1, 1, 1) for ptw in (1, 2)} | {c3(8, 1, 4, 4, 1, 1, 0), c3(8, 1, 4, 4, 1, 0, 1)}),
    "split": (
        {split(kt, 2, 4, 4) for kt in (2, 8, 10, 16, 32, 64)} | {split(kt, 1, 4, 4) for kt in (8, 16)} | {split(kt, 2, 4, 8) for kt in (8, 16)} |
        {split(kt, cw, 3, 4) for kt in (8, 16, 32, 64) for cw in (1, 2, 4)} |
        {split(kt, 2, 4, nw, 1 | 4) for kt in (8, 16) for nw in (4, 8)} | {split(kt, 2, 4, 4, 1) for kt in (8, 16)}),
    "sample": (
        {sample(kt, 2, 4) for kt in (4, 8, 16, 32)} | {sample(kt, 2, 2) for kt in (16, 32, 64)} |
        {sample(kt, 2, 4, 1) for kt in (4, 8, 16)} | {sample(16, 2, 2, 1), sample(16, 2, 2, 0, 1), sample(64, 2, 2, 0, 1), sample(16, 1, 2), sample(32, 1, 4)}),
    "short": (
        {short(2, 2, 4, 0, f) for f in (0, 1)} | {short(kt, 2 * kt, nw, 0, f) for kt in (4, 8) for nw in (4, 8) for f in (0, 1)} |
        {short(16, 32, 8, 0, f) for f in (0, 1)} | {short(8, 16, 8, b, f) for b in (1 | 4, 1 | 2 | 4) for f in (0, 1)}),
    "stream": (
        {stream(1, 1, nt=0), stream(5, 1, nt=0), stream(5, 1, 1, nt=0)} |
        {stream(1, 1, r, 0, 1, 0) for r in (0, 1)} | {stream(5, 1, r, 0, 1, 0) for r in (0, 1)} | {stream(1, 1, 0, 1, 0, 0)} |
        {stream(kt, 1, 0, 1, 1, 0) for kt in (1, 8, 16)} |
        {stream(kt, 1, 1, 0, 1, 0, d) for kt in (2, 4) for d in (0, 1)} |
        {stream(kt, 0, nt=3) for kt in (1, 4, 8)} | {stream(2, 0, 1, nt=3), stream(8, 0, nt=1)}),
    "stat": (
        {stat(kt, 4, -1, t) for kt in (1, 2, 4) for t in (0, 1)} | {stat(1, 4, 1, t) for t in (0, 1)}),
}

# The folded shortcut under stored thresholds has one driver, without a `regime` or a width keyword: as it is and under poison only
NO_REGIME_NO_WIDTH = {short(8, 16, 8, b, f) for b in (1 | 4, 1 | 2 | 4) for f in (0, 1)}
# What the drivers launch BESIDE the instantiation a case is about, in the same family: the reference launches they compare with
# (fp32 in and out, named "split") and the consumers they feed - the default instantiations of these small shapes
ALSO_LAUNCHED = {
    "conv3x3": set(),
    # the closing 1x1's driver feeds a consumer of a quarter of the channels from the fp32 trunk and from its code copy: 1024 -> 256
    # (fp32: split(32, 2, 4, 4), listed above) and 2048 -> 512, which 3 tiles put on eight wavefronts
    "split": {split(32, 2, 4, 4, 1), split(64, 2, 4, 4, 1), split(64, 2, 4, 8)},
    "sample": set(),
    "short": set(),
    "stream": set(),
    "stat": set(),
}

WAYS = ("as it is", "poison", "regimes", "widths")
CONFIRMED = {w: collections.defaultdict(set) for w in WAYS}    # way -> family -> the expected notes that a launch left
SEEN = collections.defaultdict(set)                  # family -> every note seen in a case about that family
RAN = set()                                          # the parametrised runs of the four ways that completed

# the entry points whose launches leave a note
SPIED = ("pwconv_i8", "conv3x3_i8", "pwconv_i8_shortcut", "pwconv_i8_gap", "pwconv_i8_stat", "pwdw_fused")


# ---- the runs ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    from quantization.mxnet_amd import ops as _ops
    return _ops


def _describe(c):
    return "%s(%s)" % (c.driver.__name__, ", ".join("%s=%r" % kv for kv in sorted(c.kwargs.items())))


def _spy(ops, monkeypatch, seen):
    """After every call of an entry point that launches one of the families: what it left."""
    for name in SPIED:
        real = getattr(ops, name)

        def wrapped(*a, _real=real, **kw):
            try:
                return _real(*a, **kw)
            finally:
                seen.append(ops.last_launch())
        monkeypatch.setattr(ops, name, wrapped)


def _run_case(c, row, dev, ops, monkeypatch, way, extra=None, after=None):
    """One driver call under the row's environment: its own assertions, then the notes."""
    from quantization.mxnet_amd._lib import FakeQuantError
    kw = dict(c.kwargs)
    kw.update(extra or {})
    if c.driver is not V._pair and c.driver is not V._front and "regime" in kw and kw["regime"] is None:
        del kw["regime"]
    seen = []
    with monkeypatch.context() as mp:
        for k, v in row.env.items():
            mp.setenv(k, str(v))
        _spy(ops, mp, seen)
        before = ops.last_launch()
        try:
            if c.refused is not None:
                with pytest.raises(FakeQuantError, match=c.refused):
                    c.driver(dev=dev, ops=ops, **kw)
                # the refused call - the driver's last - launched nothing: the note is the one the call before it left
                assert seen and seen[-1] == ops.last_launch() == (seen[-2] if len(seen) > 1 else before), \
                    "a refused call left a note: %s" % (seen[-1:],)
                return
            c.driver(dev=dev, ops=ops, **kw)
            if after is not None:
                after()
        except AssertionError as e:
            raise AssertionError("%s, %s: %s" % (dict(row.env), _describe(c), e)) from e
    for note in c.notes:
        assert _matches(note, seen), "%s, %s: no launch left the note %s; seen: %s" % (
            dict(row.env), _describe(c), note, sorted(set(s for s in seen if s is not None), key=str))
        if ANY not in note:
            CONFIRMED[way][note[0]].add(note)
    families = {n[0] for n in c.notes} - {"pair"}        # (the fused pair's rows per band follow the CU count)
    for s in seen:
        if s is not None and s[0] in families:
            SEEN[s[0]].add(s)


def test_last_launch_is_a_note_of_the_thread_and_costs_no_device_work(dev, ops, monkeypatch):
    """`ops.last_launch()` names the family and the values in the order of `ops.LAUNCH_FAMILIES`; a launch of another family
    replaces it, a refused call leaves it, the tuning variable is read at every call."""
    x = torch.relu(torch.randn(2, 64, 5, 7, device=dev))
    w3 = ops.weight_codes_3x3(torch.randn(64, 64, 3, 3, device=dev) * 0.1, 64, 8)
    thr = torch.full((1,), 2.0, device=dev)
    want = None
    for ptw in (1, 2, 4, 1):
        monkeypatch.setenv("FQ_C3_PTW", str(ptw))
        y, _ = ops.conv3x3_i8(x, *w3, in_thr=thr)
        assert ops.last_launch() == c3(2, ptw, 2, 4), ops.last_launch()
        want = y if want is None else want
        assert torch.equal(y, want), "PTW = %d computes other values" % ptw
    assert len(ops.LAUNCH_FAMILIES[1][1]) == len(ops.last_launch()) - 1
    from quantization.mxnet_amd._lib import FakeQuantError
    w192 = ops.weight_codes_3x3(torch.randn(64, 192, 3, 3, device=dev) * 0.1, 64, 8)
    with pytest.raises(FakeQuantError, match="Cin must be 64, 128, 256 or 512"):
        ops.conv3x3_i8(torch.relu(torch.randn(2, 192, 5, 7, device=dev)), *w192, in_thr=thr)
    assert ops.last_launch() == c3(2, 1, 2, 4)
    w1 = ops.weight_codes(torch.randn(32, 64, 1, 1, device=dev) * 0.1, 32, 8)
    ops.pwconv_i8(x, *w1, in_thr=thr, form="split")
    assert ops.last_launch() == split(2, 1, 4, 4)


EVERY_CASE = [(r, i) for r in ROWS for i in range(len(ROWS[r].cases))]


@pytest.mark.parametrize("row,i", EVERY_CASE, ids=["%s-%d" % ri for ri in EVERY_CASE])
def test_case_as_it_is(dev, ops, monkeypatch, row, i):
    _run_case(ROWS[row].cases[i], ROWS[row], dev, ops, monkeypatch, WAYS[0])
    RAN.add((WAYS[0], row, i))


def _small(row):
    return [c for c in ROWS[row].cases if c.small and c.refused is None]


POISONED = [r for r in ROWS if _small(r)]


@pytest.mark.parametrize("pattern", poison.PATTERNS, ids=["0x%02X" % p for p in poison.PATTERNS])
@pytest.mark.parametrize("row", POISONED)
def test_row_under_poison(dev, ops, monkeypatch, row, pattern):
    proxy = poison.Proxy(pattern)
    monkeypatch.setattr(ops, "torch", proxy)
    for mod in POISON.DRIVER_MODULES:
        for name in ("T", "_t"):
            if hasattr(mod, name):
                monkeypatch.setattr(mod, name, lambda a, d, _p=proxy: None if a is None else _p.guarded(a, d))

    def guards():
        torch.cuda.synchronize()
        proxy.guards_intact()
        assert proxy.records, "the case took neither an input nor an allocation from the proxy: it checks nothing here"
    for c in _small(row):
        ops._WS.clear()                                  # the scratch cache is taken anew, poisoned, in every case
        try:
            _run_case(c, ROWS[row], dev, ops, monkeypatch, WAYS[1], after=guards)
        except AssertionError as e:
            raise AssertionError("pattern 0x%02X: %s" % (pattern, e)) from e
        proxy.release()
    ops._WS.clear()
    RAN.add((WAYS[1], row, pattern))


REGIME_PAIRS = [(r, g) for r in POISONED for g in CODES if any(g in c.regimes and c.driver is not SH16_DRIVER for c in _small(r))]


@pytest.mark.parametrize("row,regime", REGIME_PAIRS, ids=["%s-%s" % p for p in REGIME_PAIRS])
def test_row_under_regime(dev, ops, monkeypatch, row, regime):
    ran = 0
    for c in _small(row):
        if regime in c.regimes and c.driver is not SH16_DRIVER:
            _run_case(c, ROWS[row], dev, ops, monkeypatch, WAYS[2], extra={"regime": regime})
            ran += 1
    assert ran > 0
    RAN.add((WAYS[2], row, regime))


# (the width table of tests/test_gpu_act_widths.py takes the recompute pair, the front layer and the folded shortcut down to four bits)
FOUR_BITS_ONLY = (V._pair, V._front, SH_DRIVER)


def _at_width(row, width):
    return [c for c in _small(row) if c.widths and not (width == 2 and c.driver in FOUR_BITS_ONLY)]


WIDTH_TRIPLES = [(r, wd, g) for r in POISONED for wd in (4, 2) if _at_width(r, wd) for g in (None, "boundaries")]


@pytest.mark.parametrize("row,width,regime", WIDTH_TRIPLES, ids=["%s-w%d-%s" % (r, wd, g or "gaussian") for r, wd, g in WIDTH_TRIPLES])
def test_row_at_width(dev, ops, monkeypatch, row, width, regime):
    for c in _at_width(row, width):
        extra = {k: width for k in c.widths}
        extra["regime"] = regime
        _run_case(c, ROWS[row], dev, ops, monkeypatch, WAYS[3], extra=extra)
    RAN.add((WAYS[3], row, width, regime))


def test_the_file_confirmed_every_listed_instantiation_in_each_way_and_launched_no_other():
    """Each of the four ways confirmed - from the note of the launch itself - exactly the hand-written list (less what a way cannot
    run: the one driver without the keywords), and every note SEEN in the cases of a family is on that list or on the list of the
    drivers' own reference launches: an instantiation added to a launch macro without a case here is noticed by whoever edits
    its neighbour, and a launch nobody listed is noticed here."""
    total = len(EVERY_CASE) + len(POISONED) * len(poison.PATTERNS) + len(REGIME_PAIRS) + len(WIDTH_TRIPLES)
    if len(RAN) != total:
        pytest.skip("only with the whole file: %d of %d runs completed" % (len(RAN), total))
    for way in WAYS:
        for family, listed in INSTANTIATIONS.items():
            want = listed if way in WAYS[:2] else listed - NO_REGIME_NO_WIDTH
            got = CONFIRMED[way][family]
            assert got == want, "%s, %s: confirmed but not listed %s; listed but not confirmed %s" % (
                way, family, sorted(got - want, key=str), sorted(want - got, key=str))
        assert set(CONFIRMED[way]) <= set(INSTANTIATIONS)
    wrong = []
    for family, listed in INSTANTIATIONS.items():
        assert not listed & ALSO_LAUNCHED[family], "listed twice: %s" % sorted(listed & ALSO_LAUNCHED[family], key=str)
        want = listed | ALSO_LAUNCHED[family]
        if SEEN[family] != want:
            wrong.append("%s: seen but on neither list %s; listed but never seen %s" % (
                family, sorted(SEEN[family] - want, key=str), sorted(want - SEEN[family], key=str)))
    assert not wrong, "\n".join(wrong)
